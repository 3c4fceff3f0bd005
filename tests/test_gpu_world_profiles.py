"""GPU: push-broom profiles of a synthetic world (world.render_profiles / TraversalPlan, di2p_world_render_profiles in csrc/world.hip)
against tests/world_profiles_oracle.py -- the noise-free render bit for bit (rows, offsets, counts), the noisy one with the oracle's keep mask
and within one float32 ulp (the device's log and cos are not numpy's), the edges of the kernel's prefix, the status of bad offsets,
TraversalPlan + OxfordRawPlan replayed from one graph, and the camera / laser consistency property through submap.build_raw and the device's
own trace.  Small shapes: 37 beams, 65 profiles in three sub-maps (one empty); the prefix cases have up to 262 145 rays of a four-primitive
scene.  Every test runs in well under a second of device time."""
import numpy as np
import pytest
import torch

from deepi2p_amd import submap, synthetic, world
from tests import submap_oracle as smo
from tests import world_profiles_oracle as wpo

pytestmark = pytest.mark.gpu
B, COUNTS, BEAMS = 3, [40, 0, 25], 37
OFFSETS = np.array([0, 40, 40, 65], np.int32)
UP = 47                                                   # a profile of sub-map 2 turned to the sky
CAL = synthetic.make_lms_traversal(np.random.default_rng(0), 1, 1, 1)
G_LASER, G_CAM = CAL["G_posesource_laser"], CAL["G_cam"]
QUIET = dict(dropout=0.0, range_sigma=0.0, reflectance_sigma=0.0)


def _np(t):
    return t.cpu().numpy()


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _low_scene():
    """the ground, a box lower than the laser and a short pole: nothing above the horizon of a laser 1.4 m up"""
    table = np.zeros((world.MAX_PRIMS, world.SLOTS))
    table[0] = world._row(world.GROUND, [0.0], np.full(3, 0.25), 0.7)
    table[1] = world._row(world.BOX, [-30.0, 5.0, 0.0, 30.0, 9.0, 1.0], np.array([0.6, 0.4, 0.3]), 0.5)
    table[2] = world._row(world.BOX, [-30.0, -8.0, 0.0, 30.0, -4.5, 1.2], np.array([0.2, 0.5, 0.7]), 0.9)
    table[3] = world._row(world.CYLINDER, [3.0, 4.2, 0.15, 0.0, 1.3], np.array([0.9, 0.9, 0.8]), 0.4)
    return table, 4


@pytest.fixture(scope="module")
def drive(dev):
    """three sub-maps of 40, 0 and 25 profiles: a street, any scene for the empty one, the low scene; profile UP looks at open sky"""
    rng = np.random.default_rng(17)
    table, count = world.make_street(rng, B, 40.0)
    table[2], count[2] = _low_scene()
    T = world.make_trajectory(rng, B, 40)
    L = np.concatenate([world.traversal_inputs(T, 20, 20, G_LASER, G_CAM)[0][b, :n] for b, n in enumerate(COUNTS)])
    L[UP] = L[UP] @ np.diag([-1.0, 1.0, -1.0, 1.0])          # half a turn about laser y: x, the middle of the fan, points up
    beam = world.lms_pattern(BEAMS, 160.0)                   # +-80 degrees: every beam of the turned profile is above the horizon
    return dict(world=(table, count), dev=(torch.from_numpy(table).to(dev), torch.from_numpy(count).to(dev)), L=L, beam=beam)


def test_profiles_without_noise_equal_the_oracle(dev, drive):
    """2405 rays in ten workgroups: workgroup boundaries fall inside profiles (256 is no multiple of 37), and workgroup 5 holds the end of
    sub-map 0 and the start of sub-map 2 (ray 1480), whose tables it stages one after the other"""
    xyr, off, cnt, status = (_np(a) for a in world.render_profiles(drive["dev"], OFFSETS, drive["L"], drive["beam"], 5, device=dev, **QUIET))
    rows, want_off, subs = wpo.render_batch(drive["world"], OFFSETS, drive["L"], drive["beam"], 5, **QUIET)
    assert (40 * BEAMS) % 256 and (40 * BEAMS) // 256 == 5
    assert list(status) == [0, 0, 0] and np.array_equal(off, want_off) and np.array_equal(cnt, np.diff(want_off))
    total = int(off[-1])
    assert total == len(rows) > 1500 and xyr.shape == (65 * BEAMS, 3) and _bits(xyr[:total], rows)
    assert np.all(xyr[total:] == 0)                                                        # nothing written past the batch
    assert cnt[UP] == 0 and off[UP] == off[UP + 1] and cnt[UP - 1] > 0 and cnt[UP + 1] > 0  # open sky: offsets, no rows
    assert subs[1]["rows"].shape == (0, 3) and min(cnt[:40].max(), cnt[40:].max()) == BEAMS
    # a host world and device offsets give the same result
    again = world.render_profiles(drive["world"], torch.from_numpy(OFFSETS), drive["L"], drive["beam"], 5, device=dev, **QUIET)
    assert _bits(_np(again[0]), xyr) and _bits(_np(again[1]), off)


def test_profiles_with_noise(dev, drive):
    """keep mask, order, offsets and counts exact; the values, rounded to float32 as di2p_submap_build rounds them, within one float32 ulp of
    the oracle's (the bound tests/test_gpu_world.py has for the noisy scan, for the same Box-Muller)"""
    run = lambda seed, frame0=0: [_np(a) for a in world.render_profiles(drive["dev"], OFFSETS, drive["L"], drive["beam"], seed, frame0=frame0, device=dev)]
    xyr, off, cnt, status = run(5)
    rows, want_off, subs = wpo.render_batch(drive["world"], OFFSETS, drive["L"], drive["beam"], 5)
    assert list(status) == [0, 0, 0] and np.array_equal(off, want_off) and np.array_equal(cnt, np.diff(want_off))
    assert 0 < int(off[-1]) < sum(int((s["t"] < world.LMS_MAX_RANGE).sum()) for s in subs)          # the dropout removed some
    got, want = xyr[:off[-1]].astype(np.float32), rows.astype(np.float32)
    worst = np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
    print("profiles with noise: largest difference %.2f float32 ulp over %d values" % (worst.max(), worst.size))
    assert worst.max() <= 1.0
    assert xyr[:off[-1], 2].min() >= 0.0 and xyr[:off[-1], 2].max() <= 255.0 and not np.array_equal(xyr[:off[-1], 2], np.rint(xyr[:off[-1], 2]))
    again, other, later = run(5), run(6), run(5, 3)
    assert _bits(again[0], xyr) and _bits(again[1], off)
    assert not np.array_equal(other[0], xyr) and not np.array_equal(later[0], xyr)
    shifted = wpo.render_batch(drive["world"], OFFSETS, drive["L"], drive["beam"], 5, frame0=3)
    assert np.array_equal(later[1], shifted[1])                                            # the counter's second word is frame0 + s


@pytest.mark.parametrize("S,beams", [(3, 5375), (3, 5461), (3, 5463), (4, 65471), (4, 65535), (5, 52429)])
def test_profiles_at_the_edges_of_the_prefix(dev, S, beams):
    """The kernel's prefix runs over the counts of its 256-ray workgroups, not over profiles: wave_prefix in chunks of 64 workgroups inside
    groups of 1024, then over the groups.  63, 64 and 65 workgroups (one below, at and one above a chunk) and 1023, 1024 and 1025 (a group);
    two sub-maps of 1 and S - 1 profiles of the four-primitive scene, no noise but a dropout of 0.3 (an exact comparison of integers), so the
    counts are irregular.  Rows, offsets and counts bit for bit."""
    parts = -(-S * beams // 256)
    assert parts in (63, 64, 65, 1023, 1024, 1025) and beams % 64
    table, count = _low_scene()
    w = (np.stack([table, table]), np.array([count, count - 1], np.int32))
    rng = np.random.default_rng(S * beams)
    L = world.traversal_inputs(world.make_trajectory(rng, 1, S), 0, 0, G_LASER, G_CAM)[0][0]
    beam = world.lms_pattern(beams, 200.0)
    off = np.array([0, 1, S], np.int32)
    kw = dict(dropout=0.3, range_sigma=0.0, reflectance_sigma=0.0)
    xyr, scan_off, cnt, status = (_np(a) for a in world.render_profiles(w, off, L, beam, 11, device=dev, **kw))
    rows, want_off, _ = wpo.render_batch(w, off, L, beam, 11, **kw)
    assert list(status) == [0, 0] and np.array_equal(scan_off, want_off) and np.array_equal(cnt, np.diff(want_off))
    assert 0.3 * S * beams < len(rows) < 0.7 * S * beams and _bits(xyr[:len(rows)], rows) and np.all(xyr[len(rows):] == 0)


def test_bad_offsets_give_a_status_and_leave_the_submaps_before_them_alone(dev, drive):
    full = [_np(a) for a in world.render_profiles(drive["dev"], OFFSETS, drive["L"], drive["beam"], 5, device=dev, **QUIET)]
    n0 = int(full[1][40])
    for bad, status, ok in (([0, 40, 30, 65], [0, 3, 3], 40), ([0, 40, 40, 66], [0, 0, 3], 40), ([1, 40, 40, 65], [3, 3, 3], 0),
                            ([0, -1, 40, 65], [3, 3, 3], 0)):
        got = [_np(a) for a in world.render_profiles(drive["dev"], np.array(bad, np.int32), drive["L"], drive["beam"], 5, device=dev, **QUIET)]
        rows = n0 if ok else 0
        assert list(got[3]) == status, bad
        assert _bits(got[0][:rows], full[0][:rows]) and np.all(got[0][rows:] == 0), bad          # a rejected sub-map has no rows
        assert np.array_equal(got[1][:ok + 1], full[1][:ok + 1]) and np.all(got[1][ok:] == rows) and np.all(got[2][ok:] == 0), bad


def test_returns_are_seen_or_occluded_from_the_camera(dev):
    """Consistency on the device: noise-free profiles -> submap.build_raw without the skip rule and the ground filter.  Its float32 rows are
    first tied to fp64 returns -- tests/submap_oracle.py's fp64 points of the device's own scan_xyr, rounded once, bit for bit (the float32
    rounding alone moves a point 60 times the bound off its surface) -- and every one of those returns p, taken to the world, then has
    trace(o_cam, (p - o_cam) / |p - o_cam|).t <= |p - o_cam| (1 + 1e-9) through the device's own trace."""
    S, beams, origin = 30, 181, 15
    rng = np.random.default_rng(23)
    w = world.make_street(rng, 1, 40.0)
    wd = (torch.from_numpy(w[0]).to(dev), torch.from_numpy(w[1]).to(dev))
    T = world.make_trajectory(rng, 1, S)
    L, poses, c2w, _ = world.traversal_inputs(T, origin, origin, G_LASER, G_CAM)
    off = np.array([0, S], np.int32)
    xyr, scan_off, cnt, status = world.render_profiles(wd, off, L[0], world.lms_pattern(beams), 0, device=dev, **QUIET)
    d_poses = torch.from_numpy(poses[0]).to(dev)
    pts, out_off, kept, _, st = (_np(a) for a in submap.build_raw(xyr, scan_off, off, d_poses, None, G_LASER))
    h_xyr, h_off = _np(xyr), _np(scan_off)
    want = smo.build_raw(h_xyr, h_off, off, poses[0], None, G_LASER)
    total = int(h_off[-1])
    assert list(st) == [0] and np.all(kept == 1) and out_off[1] == total > 3000
    assert _bits(pts[:total], want["points"]) and _bits(pts[:total, :3], want["points64"].astype(np.float32))
    p = want["points64"] @ T[0, origin, :3, :3].T + T[0, origin, :3, 3]          # from the origin's vehicle frame to the world
    o = c2w[0, :3, 3]
    v = p - o[None]
    dist = np.sqrt((v * v).sum(1))
    tc = _np(world.trace(wd, o[None], (v / dist[:, None])[None], device=dev)[0])[0]
    print("camera / laser consistency: %d returns, worst t / dist - 1 = %.2e" % (len(p), float((tc / dist).max() - 1.0)))
    assert np.all(tc <= dist * (1 + 1e-9))


def test_traversal_and_oxford_plans_replay_from_one_graph(dev):
    Bg, N, H, W, raw_hw, S, beams = 2, 2048, 64, 128, (128, 256), 60, 181
    rng = np.random.default_rng(13)
    opt = synthetic.OptLike(N, H, W, False)
    tp_caps = (Bg * S, Bg * S * beams)
    ox = submap.OxfordRawPlan(opt, Bg, tp_caps[0], tp_caps[1], tp_caps[1], S * beams, raw_hw, "train", skip_threshold=0.1 / 16, device=dev)
    tp = world.TraversalPlan(Bg, S, beams, raw_hw[0], raw_hw[1], dev, seed_slot=ox.seed)
    assert (tp.S_cap, tp.P_cap) == tp_caps and tp.seed is ox.seed
    w = world.make_street(rng, Bg, 40.0)
    T = world.make_trajectory(rng, Bg, S)
    inputs = world.traversal_inputs(T, S // 2, S // 2, G_LASER, G_CAM)
    tp.set_world(w)
    tp.set_calibration(G_LASER, G_CAM)
    tp.set_camera(np.tile(np.array([[200.0, 0, 128.3], [0, 200.0, 63.3], [0, 0, 1]]), (Bg, 1, 1)))
    tp.set_traversal(*inputs)

    def both(seed):
        outs = tp.run(seed=seed)
        return outs[:2] + (outs[7],) + tuple(ox.run(*outs, seed=None))

    def frozen(out):
        total = int(out[1][-1])
        return [out[0][:total].clone()] + [t.clone() for t in out[1:]]

    eager = {s: frozen(both(s)) for s in (11, 12)}
    assert not torch.equal(eager[11][0][:1000], eager[12][0][:1000]) and torch.equal(eager[11][2], eager[12][2])       # the image has no noise
    assert not torch.equal(eager[11][3], eager[12][3])
    for s in (11, 12):
        want = wpo.render_batch(w, _np(tp.submap_offsets), inputs[0].reshape(-1, 4, 4), _np(tp.beam), s)
        assert np.array_equal(_np(eager[s][1]), want[1])
        assert np.all(_np(eager[s][12]) == 0) and np.all(_np(tp.status) == 0), _np(eager[s][12])          # status 0 for every sub-map
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        both(None)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = both(None)
    for s in (12, 11):
        ox.seed.fill_(s)
        for t in out[3:8]:
            t.zero_()
        out[2].zero_()
        g.replay()
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(eager[s], frozen(out))):
            assert a.dtype == b.dtype and a.shape == b.shape and _np(a).tobytes() == _np(b).tobytes(), (s, i)
