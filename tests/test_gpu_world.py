"""GPU: synthetic worlds (deepi2p_amd.world, csrc/world.hip) against tests/world_oracle.py -- trace, the camera render and the scan bit for
bit (the noisy scan within one float32 ulp: the device's log and cos are not numpy's), the camera / LiDAR consistency property through the
device's own trace, and WorldPlan + RawFramePlan replayed from one graph.  Small shapes: 257 rays, 37 x 61 and 8 x 64 images, 5 x 67 scans;
one 64 x 1800 scan and one pair of 370 x 1226 frames.  Every test runs in well under a second of device time."""
import math

import numpy as np
import pytest
import torch

from deepi2p_amd import raw_prep, synthetic, world
from tests import world_oracle as wo

pytestmark = pytest.mark.gpu
B = 3
Z0 = -1.73
EYE = np.array([0.0, 2.0, 0.5])          # frame 0's sensor / ray origin: on the plane y = 2 that two boxes share, above a low box
P_BASE = np.array([[0.0, -1, 0, 0.06], [0, 0, -1, -0.08], [1, 0, 0, -0.27], [0, 0, 0, 1]])          # sensor (x fwd, y left, z up) -> camera
CAM_OFFSET = np.array([0.27, 0.06, -0.08])


def _np(t):
    return t.cpu().numpy()


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _tri_world():
    """frame 0: 32 primitives of all three types (two abutting boxes 1, 2 sharing the face y = 2, a low box 3 under EYE, a pole 4 that the
    ray EYE + t (-1, 0, 0) touches in one point), frame 1: the ground alone, frame 2: nothing"""
    rng = np.random.default_rng(42)
    table, count = np.zeros((B, world.MAX_PRIMS, world.SLOTS)), np.array([world.MAX_PRIMS, 1, 0], np.int32)
    rows = [(world.GROUND, [Z0]), (world.BOX, [10.0, 0.0, Z0, 12.0, 2.0, 1.0]), (world.BOX, [10.0, 2.0, Z0, 12.0, 4.0, 1.0]),
            (world.BOX, [-1.0, 1.0, Z0, 1.0, 3.0, 0.2]), (world.CYLINDER, [-5.0, 2.25, 0.25, Z0, 3.0])]
    while len(rows) < world.MAX_PRIMS:
        r, a = rng.uniform(15, 45), rng.uniform(-np.pi, np.pi)
        c = np.array([r * np.cos(a), r * np.sin(a)])
        if len(rows) % 2:
            h = rng.uniform(0.8, 5.0, 2)
            rows.append((world.BOX, [c[0] - h[0], c[1] - h[1], Z0, c[0] + h[0], c[1] + h[1], Z0 + rng.uniform(1.2, 8.0)]))
        else:
            rows.append((world.CYLINDER, [c[0], c[1], rng.uniform(0.1, 0.6), Z0, rng.uniform(2.0, 6.0)]))
    for i, (kind, g) in enumerate(rows):
        table[0, i] = world._row(kind, g, world._albedo(rng.uniform(0.1, 0.9), rng.uniform(0.35, 1.0, 3)), rng.uniform(0.3, 1.5))
    table[1, 0] = world._row(world.GROUND, [Z0], np.full(3, 0.25), 0.7)
    return table, count


def _rays():
    """257 directions: the special ones first, then seeded random ones (not normalised)"""
    special = [[1.0, 0, 0],          # two zero components, horizontal: along the shared face y = 2 (a tie: box 1), inside box 3's y slab, outside its z slab
               [-1.0, 0, 0],         # tangent to the pole (disc = 0 exactly)
               [0.0, 1, 0], [0.0, -1, 0],          # two zero components, outside the x slab of boxes 1 and 2
               [0.0, 0, -1],         # from above box 3, looking down
               [0.0, 0, 1],          # up: nothing
               [1.0, 0.05, 0], [1.0, -0.05, 0], [1.0, 0, -0.04], [1.0, 0, 0.04], [0.0, 1, -0.2], [0.3, 0, -1],          # one zero component
               [-1.0, 0.01, 0], [-1.0, -0.01, 0], [2.0, 0, 0], [1.0, 1, 0]]
    rng = np.random.default_rng(7)
    rest = rng.standard_normal((257 - len(special), 3)) * np.array([1.0, 1.0, 0.3])
    return np.concatenate([np.array(special), rest])


@pytest.fixture(scope="module")
def tri(dev):
    table, count = _tri_world()
    return dict(table=table, count=count, dev=(torch.from_numpy(table).to(dev), torch.from_numpy(count).to(dev)))


def test_trace_equals_the_oracle(dev, tri):
    d = np.tile(_rays()[None], (B, 1, 1))
    o = np.array([EYE, [0.0, 0.0, 0.0], [1.0, 2.0, 3.0]])
    t, prim = (_np(a) for a in world.trace(tri["dev"], o, d, device=dev))
    for b in range(B):
        wt, wp = wo.trace(tri["table"][b], int(tri["count"][b]), o[b], d[b])
        assert _bits(t[b], wt) and _bits(prim[b], wp), b
    # the cases the rays were made for
    assert prim[0, 0] == 1 and t[0, 0] == 10.0                      # the tie goes to the lower index
    assert prim[0, 1] == 4 and t[0, 1] == 5.0                       # tangent
    assert prim[0, 4] == 3 and t[0, 4] == 0.5 - 0.2                 # down onto the box
    assert prim[0, 5] == -1 and np.isinf(t[0, 5])
    assert len(set(prim[0].tolist())) >= 8 and np.all(prim[1][d[1, :, 2] >= 0] == -1) and np.all(prim[1][d[1, :, 2] < 0] == 0)
    assert np.all(prim[2] == -1) and np.all(np.isinf(t[2]))
    # a host world gives the same result
    t2, prim2 = world.trace((tri["table"], tri["count"]), o, d, device=dev)
    assert _bits(_np(t2), t) and _bits(_np(prim2), prim)


def _cameras(H0, W0):
    f = 0.7 * W0
    K = np.tile(np.array([[f, 0, (W0 - 1) / 2.0], [0, f, (H0 - 1) / 2.0], [0, 0, 1.0]]), (B, 1, 1))
    up = np.eye(4)
    c, s = math.cos(-1.2), math.sin(-1.2)
    up[1:3, 1:3] = [[c, -s], [s, c]]          # about the camera's x axis: frame 1 looks at the sky only
    Pc = np.stack([P_BASE, up @ P_BASE, P_BASE])
    T = np.tile(np.eye(4), (B, 1, 1))
    cy, sy = math.cos(0.07), math.sin(0.07)
    T[0, :2, :2] = [[cy, -sy], [sy, cy]]
    T[0, :3, 3] = EYE
    return K, Pc, T


@pytest.mark.parametrize("H0,W0", [(37, 61), (8, 64)])
def test_camera_equals_the_oracle(dev, tri, H0, W0):
    """(37, 61): rows of 183 bytes, frames of 6771: frames 1 and 2 start off a dword; the centre column has d.x = 0 in the camera frame"""
    K, Pc, T = _cameras(H0, W0)
    img, depth, prim = (_np(a) for a in world.render_camera(tri["dev"], K, Pc, H0, W0, T=T, depth=True, prim=True, device=dev))
    M = world.camera_pose(Pc, T)
    for b in range(B):
        want = wo.render_camera(tri["table"][b], int(tri["count"][b]), K[b], M[b], H0, W0)
        assert _bits(prim[b], want["prim"]), b
        assert _bits(depth[b], want["depth"]), b
        assert _bits(img[b], want["image"]), (b, int(np.sum(img[b] != want["image"])))
    assert len(set(prim[0].ravel().tolist())) >= 4 and np.all(prim[1] == -1) and np.all(prim[2] == -1)
    assert np.all(img[1] == img[2]) and img[2, 0, 0, 2] > img[2, 0, 0, 0]          # sky
    only = world.render_camera(tri["dev"], K, Pc, H0, W0, T=T, device=dev)            # without the optional outputs
    assert _bits(_np(only), img)


PATTERN = world.hdl64_pattern(np.random.default_rng(3), B, 5, 67)
POSE = np.tile(np.eye(4), (B, 1, 1))
POSE[0, :3, 3] = EYE


def _scan_oracle(tri, seed, **kw):
    return [wo.render_scan(tri["table"][b], int(tri["count"][b]), PATTERN[0], PATTERN[1][b], seed, b, pose=POSE[b], **kw) for b in range(B)]


def test_scan_without_noise_equals_the_oracle(dev, tri):
    quiet = dict(dropout=0.0, range_sigma=0.0, intensity_sigma=0.0)
    pts, off, cnt = (_np(a) for a in world.render_scan(tri["dev"], PATTERN, 5, T=POSE, device=dev, **quiet))
    want = _scan_oracle(tri, 5, **quiet)
    counts = [len(w["rows"]) for w in want]
    assert counts[0] > 100 and counts[1] > 100 and counts[2] == 0
    assert list(off) == [0, counts[0], counts[0] + counts[1], counts[0] + counts[1]] and list(cnt) == counts          # the empty frame repeats
    assert pts.shape == (B * 5 * 67, 4) and _bits(pts[:off[-1]], np.concatenate([w["rows"] for w in want]))
    assert np.all(pts[off[-1]:] == 0)                                                                                 # nothing written past the batch


def test_scan_with_noise(dev, tri):
    """keep mask, order, offsets and count exact; coordinates and intensity within one float32 ulp of the oracle's value (the rule
    tests/test_gpu_sample_prep.py::test_jitter applies to this Box-Muller)"""
    run = lambda seed: [_np(a) for a in world.render_scan(tri["dev"], PATTERN, seed, T=POSE, device=dev)]
    pts, off, cnt = run(5)
    want = _scan_oracle(tri, 5)
    counts = [len(w["rows"]) for w in want]
    assert list(cnt) == counts and list(off) == [0] + list(np.cumsum(counts))
    assert 0 < counts[0] < int(np.sum(want[0]["t"] < world.MAX_RANGE))          # the dropout removed some
    rows = np.concatenate([w["rows"] for w in want])
    got = pts[:off[-1]]
    worst = np.abs(got.astype(np.float64) - rows.astype(np.float64)) / np.spacing(np.abs(rows)).astype(np.float64)
    print("scan with noise: largest difference %.2f float32 ulp over %d values" % (worst.max(), worst.size))
    assert worst.max() <= 1.0
    assert got[:, 3].min() >= 0.0 and got[:, 3].max() <= 1.0
    again, other = run(5), run(6)
    assert _bits(again[0], pts) and _bits(again[1], off)
    assert not np.array_equal(other[0], pts)


def test_full_size_scan_offsets(dev):
    rng = np.random.default_rng(8)
    pattern = world.hdl64_pattern(rng, 2, 64, 1800)
    w = world.make_world(rng, 2)
    pts, off, cnt = (_np(a) for a in world.render_scan(w, pattern, 77, device=dev))
    want = [wo.render_scan(w[0][b], int(w[1][b]), pattern[0], pattern[1][b], 77, b) for b in range(2)]
    counts = [int(x["keep"].sum()) for x in want]
    assert list(cnt) == counts and list(off) == [0, counts[0], counts[0] + counts[1]] and min(counts) > 90000
    assert np.all(pts[off[-1]:] == 0)


def test_returns_are_seen_or_occluded_from_the_camera(dev):
    """Consistency on the device: every return p of a noise-free scan, seen from the camera origin, has trace(o, (p - o) / |p - o|).t <=
    |p - o| (1 + 1e-9).  The property is one of the fp64 returns d * t: the float32 rounding of a stored row moves a point by up to 2^-24
    relative (60 times the bound) off its surface, so the rows are first tied to the fp64 returns -- the device's own trace of the scan's
    rays, rounded once, bit for bit -- and the property is then checked on those."""
    rng = np.random.default_rng(21)
    pattern = world.hdl64_pattern(rng, 1, 16, 450)
    w = world.make_world(rng, 1)
    wd = (torch.from_numpy(w[0]).to(dev), torch.from_numpy(w[1]).to(dev))
    pts, off, _ = (_np(a) for a in world.render_scan(wd, pattern, 0, dropout=0.0, range_sigma=0.0, intensity_sigma=0.0, device=dev))
    s = wo.scan_dirs(pattern[0], pattern[1][0])
    t = _np(world.trace(wd, np.zeros((1, 3)), s[None], device=dev)[0])[0]
    keep = t < world.MAX_RANGE
    p = s[keep] * t[keep, None]
    assert off[1] == keep.sum() > 4000 and _bits(pts[:off[1], :3], p.astype(np.float32))
    v = p - CAM_OFFSET[None]
    dist = np.sqrt((v * v).sum(1))
    tc = _np(world.trace(wd, CAM_OFFSET[None], (v / dist[:, None])[None], device=dev)[0])[0]
    print("camera / LiDAR consistency: %d returns, worst t / dist - 1 = %.2e" % (len(p), float((tc / dist).max() - 1.0)))
    assert np.all(tc <= dist * (1 + 1e-9))


def test_world_and_raw_frame_plans_replay_from_one_graph(dev):
    Bg, N, H, W, raw_hw, beams, azimuths = 2, 2048, 64, 128, (370, 1226), 64, 300
    rng = np.random.default_rng(13)
    opt = synthetic.OptLike(N, H, W, False)
    cap = Bg * beams * azimuths
    raw = raw_prep.RawFramePlan(opt, Bg, cap, beams * azimuths, raw_hw, "train", "kitti", "cells", dev)
    wp = world.WorldPlan(Bg, raw_hw[0], raw_hw[1], beams, azimuths, dev, seed_slot=raw.seed)
    pattern = world.hdl64_pattern(rng, Bg, beams, azimuths)
    w = world.make_world(rng, Bg)
    K = np.tile(np.array([[720.0, 0, 612.5], [0, 720.0, 184.5], [0, 0, 1]]), (Bg, 1, 1))
    Pc = np.tile(P_BASE, (Bg, 1, 1))
    wp.set_pattern(pattern)
    assert wp.cap == cap and wp.seed is raw.seed

    def both(seed):
        points, offsets, images = wp.run(seed=seed)
        return (points, offsets, images) + tuple(raw.run(points, offsets, images, wp.K_raw, wp.Pc, seed=None))

    def frozen(out):
        total = int(out[1][-1])
        return [out[0][:total].clone()] + [t.clone() for t in out[1:]]

    first = wp.run(w, K, Pc, seed=11)          # host arrays: checked and uploaded here, outside the capture
    want = wo.render_camera(w[0][1], int(w[1][1]), K[1], world.camera_pose(Pc)[1], *raw_hw)
    assert _bits(_np(first[2][1]), want["image"])                                  # the plan renders what the oracle renders
    eager = {s: frozen(both(s)) for s in (11, 12)}
    assert not torch.equal(eager[11][3], eager[12][3]) and torch.equal(eager[11][2], eager[12][2])
    for s in (11, 12):
        ora = [wo.render_scan(w[0][b], int(w[1][b]), pattern[0], pattern[1][b], s, b) for b in range(Bg)]
        assert list(_np(eager[s][1])) == [0] + list(np.cumsum([int(o["keep"].sum()) for o in ora]))
        assert np.all(_np(eager[s][12]) == 0), _np(eager[s][12])                  # status 0 for every frame
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        both(None)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = both(None)
    for s in (12, 11):
        raw.seed.fill_(s)
        for t in out[3:8]:
            t.zero_()
        out[2].zero_()
        g.replay()
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(eager[s], frozen(out))):
            assert a.dtype == b.dtype and a.shape == b.shape and _np(a).tobytes() == _np(b).tobytes(), (s, i)
