"""GPU: Oxford sub-maps from LMS profiles (deepi2p_amd.submap, csrc/submap.hip) at the shapes of tests/golden/submap_golden.npz: stages A-C
against tests/submap_oracle.py bit for bit and against the reference's fp64 cloud within one float32 ulp, the record against the voxel pass +
the oracle's camera transform and against the reference's record, the three statuses, and the two plans (eager and replayed from a graph)
against the eager composition.  108 profiles, 2254 rows, 24 x 32 images: every test runs in well under a second of device time."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from deepi2p_amd import sample_prep, scan_prep, submap, synthetic
from tests import submap_oracle as smo
from tests.test_submap_host import CASES, G, GROUNDS, SKIPS, U24, golden_case

pytestmark = pytest.mark.gpu
KEYS = ("scan_xyr", "scan_offsets", "submap_offsets", "poses", "present")
N, NODES, HW = 256, 16, (72, 96)
OX = SimpleNamespace(crop_original_bottom_rows=8, img_H=24, img_W=32, input_pt_num=N, node_a_num=NODES, node_b_num=NODES, pc_max_range=50.0,
                     P_tx_amplitude=10.0, P_ty_amplitude=5.0, P_tz_amplitude=10.0, P_Rx_amplitude=0.1, P_Ry_amplitude=2.0 * math.pi, P_Rz_amplitude=0.2)
NINE = ("pc", "intensity", "sn", "node_a", "node_b", "P", "img", "K", "t_ij")
B = 4


def _np(t):
    return t.cpu().numpy()


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and _np(a).tobytes() == _np(b).tobytes()


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def batches(dev):
    """the golden batch and a second, synthetic one of the same B (host arrays; never modified)"""
    first = {k: G[k] for k in KEYS}
    trav = synthetic.make_lms_traversal(np.random.default_rng(11), B, [50, 9, 70, 30], 40)
    second = dict(zip(KEYS, (_np(t) for t in submap.pack_scans(trav["submaps"], device="cpu"))))
    return first, second


@pytest.fixture(scope="module")
def on_device(dev, batches):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in batches[0].items()}


@pytest.fixture(scope="module")
def camera(dev):
    rng = np.random.default_rng(5)
    raw = np.stack([synthetic.make_camera_image(np.random.default_rng(300 + b), HW[0], HW[1]) for b in range(B)])
    K = np.tile(np.array([[120.0, 0, HW[1] / 2 + 0.3], [0, 120.0, HW[0] / 2 - 0.7], [0, 0, 1]]), (B, 1, 1))
    Pcp = np.tile(np.eye(4), (B, 1, 1))
    Pcp[:, :3, 3] = rng.uniform(-2, 2, (B, 3))
    return dict(raw=raw, img=torch.from_numpy(raw).to(dev), K=K, dK=torch.from_numpy(K).to(dev), P=Pcp, dP=torch.from_numpy(Pcp).to(dev))


def _raw(d, g, s, **kw):
    return submap.build_raw(d["scan_xyr"], d["scan_offsets"], d["submap_offsets"], d["poses"], d["present"], G["G_posesource_laser"], SKIPS[s], GROUNDS[g],
                            **kw)


@pytest.mark.parametrize("g,s", CASES)
def test_build_raw_equals_the_oracle_and_meets_the_reference(dev, on_device, g, s):
    pts, off, kept, skip_count, status = (_np(t) for t in _raw(on_device, g, s))
    want = smo.build_raw(G["scan_xyr"], G["scan_offsets"], G["submap_offsets"], G["poses"], G["present"], G["G_posesource_laser"], SKIPS[s], GROUNDS[g])
    total = int(off[-1])
    assert np.array_equal(off, want["offsets"]) and np.array_equal(kept, want["kept"]) and np.array_equal(skip_count, want["skip_count"])
    assert np.array_equal(status, want["status"]) and list(status) == [0, 0, 0, 4]          # the all-missing sub-map
    assert _bits(pts[:total], want["points"])                                               # coordinates and reflectance, bit for bit
    assert np.all(pts[total:] == 0)                                                         # nothing written past the batch
    ref = golden_case(g, s)
    assert np.array_equal(off, ref["raw_offsets"]) and np.array_equal(kept, ref["kept"]) and np.array_equal(skip_count, ref["skip_count"])
    assert np.array_equal(status, 4 * ref["raised"].astype(np.int32))
    assert np.array_equal(pts[:total, 3], ref["raw_refl"].astype(np.float32))
    ulp = np.spacing(np.abs(ref["raw64"]).astype(np.float32)).astype(np.float64)
    err = np.abs(pts[:total, :3].astype(np.float64) - ref["raw64"])
    print("%s %s: largest error %.3f ulp" % (g, s, (err / ulp).max()))
    assert np.all(err <= ulp)


@pytest.mark.parametrize("g,s", CASES)
def test_build_submaps(dev, on_device, g, s):
    d = on_device
    rec, off, status = submap.build_submaps(d["scan_xyr"], d["scan_offsets"], d["submap_offsets"], d["poses"], d["present"], G["G_posesource_laser"],
                                            SKIPS[s], GROUNDS[g], voxel=float(G["voxel"]), G_cam=G["G_cam"])
    rec, off, status = _np(rec), _np(off), _np(status)
    # the voxel pass on build_raw's rows, then the oracle's camera transform on its fp64 means
    pts, roff, _, _, _ = _raw(d, g, s)
    st = scan_prep.voxel_down_sample(pts, roff, float(G["voxel"]))
    cen, inten, voff = _np(submap.voxel_centroids(st)).copy(), _np(st.intensity), _np(st.offsets)
    assert np.array_equal(off, voff) and list(status) == [0, 0, 0, 4]
    total = int(off[-1])
    assert _bits(rec[:total], smo.to_camera(cen[:total], inten[:total], G["G_cam"]))
    assert _bits(cen[:total].astype(np.float32), _np(st.points)[:total])          # the means the voxel pass rounds into its own output
    assert np.all(rec[total:] == 0)
    # and the reference's record, within the bounds of tests/test_submap_host.py
    ref = golden_case(g, s)
    assert np.array_equal(off, ref["record_offsets"])
    R = max(np.linalg.norm(ref["raw64"], axis=1).max(), np.linalg.norm(ref["record"][:, :3].astype(np.float64), axis=1).max())
    dc = np.abs(rec[:total, :3].astype(np.float64) - ref["record"][:, :3].astype(np.float64)).max()
    di = np.abs(rec[:total, 3].astype(np.float64) - ref["record"][:, 3].astype(np.float64)).max()
    print("%s %s: coordinates %.3e (bound %.3e), intensity %.3e (bound %.3e)" % (g, s, dc, (3 ** 0.5 + 1) * U24 * R, di, 2 * U24 * ref["raw_refl"].max()))
    assert dc <= (3 ** 0.5 + 1) * U24 * R and di <= 2 * U24 * ref["raw_refl"].max()


def test_build_raw_at_the_chunk_edges_of_the_prefix(dev):
    """The per-sub-map prefix over the profile counts runs in chunks of 64 profiles: sub-maps of exactly 64, 65 (one profile in the second
    chunk), 128 (two full chunks) and 1 profile, 258 profiles and 1705 rows in all, without the skip rule, with it, and with the ground filter.
    Offsets, kept, skip_count, status and every row against the numpy restatement, bit for bit."""
    trav = synthetic.make_lms_traversal(np.random.default_rng(23), 4, [64, 65, 128, 1], 8)
    h = dict(zip(KEYS, (_np(t) for t in submap.pack_scans(trav["submaps"], device="cpu"))))
    assert list(h["submap_offsets"]) == [0, 64, 129, 257, 258] and len(h["scan_xyr"]) == 1705
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in h.items()}
    Gl = trav["G_posesource_laser"]
    for (skip, ground), offsets in zip(((None, None), (0.1 / 16, None), (0.1 / 16, 0.5)),
                                       ([0, 443, 862, 1697, 1705], [0, 404, 752, 1473, 1481], [0, 106, 205, 407, 409])):
        want = smo.build_raw(h["scan_xyr"], h["scan_offsets"], h["submap_offsets"], h["poses"], h["present"], Gl, skip, ground)
        assert list(want["status"]) == [0, 0, 0, 0] and list(want["offsets"]) == offsets, (skip, ground)
        pts, off, kept, skip_count, status = (_np(t) for t in submap.build_raw(d["scan_xyr"], d["scan_offsets"], d["submap_offsets"], d["poses"],
                                                                                d["present"], Gl, skip, ground))
        total = int(off[-1])
        assert np.array_equal(off, want["offsets"]) and np.array_equal(kept, want["kept"]) and np.array_equal(skip_count, want["skip_count"]), (skip, ground)
        assert np.array_equal(status, want["status"]) and list(status) == [0, 0, 0, 0], (skip, ground)
        assert _bits(pts[:total], want["points"]), (skip, ground)
        assert np.all(pts[total:] == 0), (skip, ground)


def test_status_1_leaves_the_other_submaps_alone(dev, on_device):
    full = [_np(t) for t in _raw(on_device, "gnone", "s16")]
    counts = np.diff(full[1])
    assert counts[1] > counts[0] > counts[2] > 0
    got = [_np(t) for t in _raw(on_device, "gnone", "s16", max_frame_points=int(counts[1]) - 1)]
    assert list(got[4]) == [0, 1, 0, 4]
    assert np.array_equal(got[1], [0, counts[0], counts[0], counts[0] + counts[2], counts[0] + counts[2]])
    assert np.array_equal(got[2], full[2]) and np.array_equal(got[3], full[3])          # the keep rule is reported for the rejected sub-map too
    for b in (0, 2):
        assert _bits(got[0][got[1][b]:got[1][b + 1]], full[0][full[1][b]:full[1][b + 1]]), b
    assert np.all(got[0][got[1][-1]:] == 0)
    # exactly at the limit the sub-map passes; a capacity the rows would pass rejects it the same way
    assert list(_np(_raw(on_device, "gnone", "s16", max_frame_points=int(counts[1]))[4])) == [0, 0, 0, 4]
    tight = [_np(t) for t in _raw(on_device, "gnone", "s16", cap=int(counts[0] + counts[1]) - 1)]
    assert list(tight[4]) == [0, 1, 0, 4] and _bits(tight[0][:tight[1][-1]], got[0][:got[1][-1]])


def test_status_3_for_a_decreasing_offset(dev, on_device, batches):
    first = batches[0]
    full = [_np(t) for t in _raw(on_device, "gnone", "s16")]
    # a scan offset that decreases inside sub-map 1: that sub-map alone
    so = first["scan_offsets"].copy()
    so[50] = so[49] - 1
    d = dict(on_device, scan_offsets=torch.from_numpy(so).to(dev))
    got = [_np(t) for t in _raw(d, "gnone", "s16")]
    assert list(got[4]) == [0, 3, 0, 4] and np.all(got[2][37:103] == -1) and got[3][1] == 0
    assert _bits(got[0][:got[1][1]], full[0][:full[1][1]]) and got[1][2] == got[1][1]
    assert _bits(got[0][got[1][2]:got[1][3]], full[0][full[1][2]:full[1][3]])
    # a scan offset past the row buffer
    so = first["scan_offsets"].copy()
    so[-1] = len(first["scan_xyr"]) + 1
    got = [_np(t) for t in _raw(dict(on_device, scan_offsets=torch.from_numpy(so).to(dev)), "gnone", "s16")]
    assert list(got[4]) == [0, 0, 0, 3]
    # a sub-map offset that decreases: that sub-map and every one after it (their profiles can no longer be told apart)
    mo = first["submap_offsets"].copy()
    mo[2] = mo[1] - 1
    got = [_np(t) for t in _raw(dict(on_device, submap_offsets=torch.from_numpy(mo).to(dev)), "gnone", "s16")]
    assert list(got[4]) == [0, 3, 3, 3] and got[1][-1] == got[1][1] and _bits(got[0][:got[1][1]], full[0][:full[1][1]])
    assert np.all(got[2][37:] == -1)
    mo = first["submap_offsets"].copy()
    mo[0] = 1
    got = [_np(t) for t in _raw(dict(on_device, submap_offsets=torch.from_numpy(mo).to(dev)), "gnone", "s16")]
    assert list(got[4]) == [3, 3, 3, 3] and got[1][-1] == 0


def test_status_4_and_present_none(dev, on_device):
    """the all-missing sub-map; a sub-map without profiles; a sub-map whose only kept profile the ground filter empties; present=None"""
    d = on_device
    mo = torch.tensor([0, 37, 37, 103, 108], dtype=torch.int32, device=dev)
    got = [_np(t) for t in _raw(dict(d, submap_offsets=mo), "gnone", "s16")]
    assert list(got[4]) == [0, 4, 0, 0] and got[1][2] == got[1][1] and np.all(got[2][108:] == -1)
    one = torch.tensor([0, 20, 21, 37, 108], dtype=torch.int32, device=dev)          # sub-map 1 = the emptied profile alone
    got = [_np(t) for t in _raw(dict(d, submap_offsets=one), "g0p1", "s16")]
    assert got[4][1] == 4 and got[2][20] == 1 and got[1][2] == got[1][1]
    none = [_np(t) for t in _raw(dict(d, present=None), "gnone", "snone")]
    want = smo.build_raw(G["scan_xyr"], G["scan_offsets"], G["submap_offsets"], G["poses"], None, G["G_posesource_laser"], None, None)
    assert list(none[4]) == [0, 0, 0, 0] and np.all(none[2] == 1) and _bits(none[0][:none[1][-1]], want["points"])


def _padded(batch, S_cap, P_cap, dev):
    """the batch in buffers of the plan's capacities; the tails hold values that would show if they were read"""
    S, P = len(batch["poses"]), len(batch["scan_xyr"])
    xyr = np.full((P_cap, 3), np.nan)
    xyr[:P] = batch["scan_xyr"]
    so = np.full(S_cap + 1, -7, np.int32)
    so[:S + 1] = batch["scan_offsets"]
    poses = np.full((S_cap, 4, 4), np.nan)
    poses[:S] = batch["poses"]
    present = np.ones(S_cap, np.uint8)
    present[:S] = batch["present"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return dict(scan_xyr=t(xyr), scan_offsets=t(so), submap_offsets=t(batch["submap_offsets"].astype(np.int32)), poses=t(poses), present=t(present))


def _caps(batches):
    return max(len(b["poses"]) for b in batches) + 5, max(len(b["scan_xyr"]) for b in batches) + 7


def _eager(batch, camera, dev, mode, seed, ground=None):
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in batch.items()}
    rec, off, st = submap.build_submaps(d["scan_xyr"], d["scan_offsets"], d["submap_offsets"], d["poses"], d["present"], G["G_posesource_laser"],
                                        float(G["skip"]), ground, G_cam=G["G_cam"])
    nine = sample_prep.prepare_samples((rec, None), camera["raw"], camera["K"], camera["P"], OX, mode, seed, offsets=off, dataset="oxford")
    return rec, off, st, nine


@pytest.mark.parametrize("mode", ["val", "train"])
def test_plans_equal_the_eager_composition(dev, batches, camera, mode):
    S_cap, P_cap = _caps(batches)
    Gl = torch.from_numpy(G["G_posesource_laser"]).to(dev)
    Gc = torch.from_numpy(np.tile(G["G_cam"], (B, 1, 1))).to(dev)
    for i, (batch, ground) in enumerate(zip(batches, (0.1, None))):
        rec, off, st, nine = _eager(batch, camera, dev, mode, 21 + i, ground)
        total = int(_np(off)[-1])
        assert i or 2 * N < np.diff(_np(off)).max()                     # the loader's 0.2 m pass runs for a sub-map of the golden batch
        p = _padded(batch, S_cap, P_cap, dev)
        sp = submap.SubmapPlan(B, S_cap, P_cap, P_cap, 4000, skip_threshold=float(G["skip"]), ground_threshold=ground, device=dev)
        got = sp.run(p["scan_xyr"], p["scan_offsets"], p["submap_offsets"], p["poses"], p["present"], Gl, Gc)
        assert _same(got[1], off) and _same(got[2], st) and _same(got[0][:total], rec[:total])
        op = submap.OxfordRawPlan(OX, B, S_cap, P_cap, P_cap, 4000, HW, mode, skip_threshold=float(G["skip"]), ground_threshold=ground, device=dev)
        out = op.run(p["scan_xyr"], p["scan_offsets"], p["submap_offsets"], p["poses"], p["present"], Gl, Gc, camera["img"], camera["dK"], camera["dP"],
                     seed=21 + i)
        assert len(out) == 10 and _same(out[9], st)
        for name, a, b in zip(NINE, out, nine):
            assert _same(a, b), (i, name)
        assert _same(op.submap.record[:total], rec[:total]) and op.submap.ws.data_ptr() == op.sample.points.ws.data_ptr()
    # the convenience form is the same run (a batch without a rejected sub-map: it checks the status)
    trav = synthetic.make_lms_traversal(np.random.default_rng(12), 2, [40, 25], 60)
    conv = submap.prepare_oxford_raw(trav["submaps"], trav["G_posesource_laser"], trav["G_cam"], camera["raw"][:2], camera["K"][:2], camera["P"][:2], OX,
                                     mode, seed=3, skip_threshold=0.1 / 16)
    t = submap.pack_scans(trav["submaps"], dev)
    rec, off, st = submap.build_submaps(t[0], t[1], t[2], t[3], t[4], trav["G_posesource_laser"], 0.1 / 16, None, G_cam=trav["G_cam"])
    want = sample_prep.prepare_samples((rec, None), camera["raw"][:2], camera["K"][:2], camera["P"][:2], OX, mode, 3, offsets=off, dataset="oxford")
    for name, a, b in zip(NINE, conv, want):
        assert _same(a, b), name
    assert np.all(_np(conv[9]) == 0)
    with pytest.raises(submap.DeepI2PHipError, match="no profile or no surviving row"):
        submap.prepare_oxford_raw([([None], np.eye(4)[None])], np.eye(4), np.eye(4), camera["raw"][:1], camera["K"][:1], camera["P"][:1], OX)


@pytest.mark.parametrize("mode", ["val", "train"])
def test_graph_replay_equals_eager(dev, batches, camera, mode):
    S_cap, P_cap = _caps(batches)
    Gl = torch.from_numpy(G["G_posesource_laser"]).to(dev)
    Gc = torch.from_numpy(np.tile(G["G_cam"], (B, 1, 1))).to(dev)
    want = [_eager(batch, camera, dev, mode, 31 + i) for i, batch in enumerate(batches)]
    buf = _padded(batches[0], S_cap, P_cap, dev)
    sp = submap.SubmapPlan(B, S_cap, P_cap, P_cap, 4000, skip_threshold=float(G["skip"]), device=dev)
    op = submap.OxfordRawPlan(OX, B, S_cap, P_cap, P_cap, 4000, HW, mode, skip_threshold=float(G["skip"]), device=dev)

    def run_both():
        a = sp.run(buf["scan_xyr"], buf["scan_offsets"], buf["submap_offsets"], buf["poses"], buf["present"], Gl, Gc)
        b = op.run(buf["scan_xyr"], buf["scan_offsets"], buf["submap_offsets"], buf["poses"], buf["present"], Gl, Gc, camera["img"], camera["dK"],
                   camera["dP"], seed=None)
        return a, b

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run_both()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        a, b = run_both()
    for i in (1, 0):          # the second batch first: every input buffer and the seed slot overwritten since the capture
        for k, v in _padded(batches[i], S_cap, P_cap, dev).items():
            buf[k].copy_(v)
        op.seed.fill_(31 + i)
        for t in (a[0], op.submap.record) + tuple(b[:5]):
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        rec, off, st, nine = want[i]
        total = int(_np(off)[-1])
        assert _same(a[1], off) and _same(a[2], st) and _same(a[0][:total], rec[:total]), i
        assert _same(b[9], st) and _same(op.submap.record[:total], rec[:total]), i
        for name, x, y in zip(NINE, b, nine):
            assert _same(x, y), (i, name)
