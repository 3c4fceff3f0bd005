"""GPU: nuScenes sweep accumulation (deepi2p_amd.sweeps, csrc/sweeps.hip) at the shapes of tests/golden/sweeps_golden.npz: the pose matrices
against the scipy-based float32 matrices, the transform chain against the reference's matrices within the fp64 bound of
tests/sweeps_oracle.chain_bounds, the accumulation against tests/sweeps_oracle.py bit for bit and against the reference's fp64 cloud within
one float32 ulp, the statuses, and the two plans (eager and replayed from a graph) against the eager composition.  13 sweeps of at most
300 rows (1101 rows in the golden batch, 1267 in the second) and 24 x 32 images; one case with sweeps of 34 720, 8 203 and 9 001 rows, where
a workgroup's tile loop runs five and two times.  Every test runs in well under a second of device time."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from deepi2p_amd import sample_prep, sweeps, synthetic
from tests import sweeps_oracle as swo
from tests.test_sweeps_host import G, MATRIX_KEYS, RECORD_KEYS, f32_ulp, scipy_matrices

pytestmark = pytest.mark.gpu
KEYS = ("rows", "sweep_offsets", "frame_offsets") + RECORD_KEYS
N, NODES, HW = 256, 16, (140, 170)
NU = SimpleNamespace(crop_original_top_rows=10, img_scale=0.2, img_H=24, img_W=32, input_pt_num=N, node_a_num=NODES, node_b_num=NODES,
                     P_tx_amplitude=1.0, P_ty_amplitude=0.5, P_tz_amplitude=0.2, P_Rx_amplitude=0.05, P_Ry_amplitude=0.1, P_Rz_amplitude=2.0 * math.pi)
NINE = ("pc", "intensity", "sn", "node_a", "node_b", "P", "img", "K", "t_ij")
B = 4


def _np(t):
    return t.cpu().numpy()


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and _np(a).tobytes() == _np(b).tobytes()


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.fixture(scope="module")
def batches(dev):
    """the golden batch and a second, synthetic one of the same frame and sweep counts (host arrays; never modified)"""
    first = {k: G[k] for k in KEYS}
    s = synthetic.make_nuscenes_sweeps(np.random.default_rng(11), B, [7, 1, 3, 2], [300, 0, 90, 64, 257, 31, 130, 200, 1, 65, 40, 12, 77])
    rows, so, fo = (_np(t) for t in sweeps.pack_sweeps(s["frames"], device="cpu"))
    second = dict(rows=rows, sweep_offsets=so, frame_offsets=fo, ego=np.concatenate(s["ego"]), lidar_calib=s["lidar_calib"], cam_pose=s["cam_pose"],
                  cam_calib=s["cam_calib"])
    return first, second


@pytest.fixture(scope="module")
def on_device(dev, batches):
    return {k: _t(v, dev) for k, v in batches[0].items()}


@pytest.fixture(scope="module")
def oracle():
    """the numpy restatement of the golden batch, computed once"""
    return swo.accumulate(G["rows"], G["sweep_offsets"], G["frame_offsets"], G["T"])


@pytest.fixture(scope="module")
def camera(dev):
    raw = np.stack([synthetic.make_camera_image(np.random.default_rng(300 + b), HW[0], HW[1]) for b in range(B)])
    K = np.tile(np.array([[120.0, 0, HW[1] / 2 + 0.3], [0, 120.0, HW[0] / 2 - 0.7], [0, 0, 1]]), (B, 1, 1))
    return dict(raw=raw, img=torch.from_numpy(raw).to(dev), K=K, dK=torch.from_numpy(K).to(dev))


def test_pose_matrices(dev):
    rec = np.concatenate([G[k] for k in RECORD_KEYS])
    got = _np(sweeps.pose_matrices(_t(rec, dev)))
    want = scipy_matrices(rec)
    assert np.array_equal(want, np.concatenate([G[k] for k in MATRIX_KEYS]))          # the reference's matrices of the golden file
    assert _bits(got[:, :, 3], want[:, :, 3]) and _bits(got[:, 3], want[:, 3])          # translation and last row: bit for bit
    err = np.abs(got - want)
    print("pose_matrices: %d of %d rotation entries differ from the scipy-based float32 matrix, largest %.3f ulp"
          % (np.count_nonzero(err), 9 * len(got), (err / f32_ulp(want)).max()))
    assert np.all(err <= f32_ulp(want))
    assert _bits(got, swo.pose_matrices(rec))                                            # and the restatement, bit for bit
    assert _bits(_np(sweeps.pose_matrices(rec)), got)                                    # host records are uploaded as they are


def test_sweep_transforms(dev):
    """fed the REFERENCE's P matrices: the quaternion step does not enter.  Against the reference within chain_bounds (gamma_38 times the
    product of the absolute matrices); against the restatement bit for bit."""
    fo = G["frame_offsets"]
    P = [_t(G[k], dev) for k in MATRIX_KEYS]
    T, Pcp = (_np(t) for t in sweeps.sweep_transforms(P[0], fo, P[1], P[2], P[3]))
    k, bT, bP = swo.chain_bounds(G["P_ego"], fo, G["P_vehicle_lidar"], G["P_ego_cam"], G["P_vehicle_cam"])
    eT, eP = np.abs(T - G["T"]), np.abs(Pcp - G["P_cam_pc"])
    ratio = lambda e, b: (e[b > 0] / b[b > 0]).max()
    print("sweep_transforms: T largest |difference| %.3e, largest ratio to gamma_%d . product %.4f; P_cam_pc %.3e, %.4f"
          % (eT.max(), k, ratio(eT, bT), eP.max(), ratio(eP, bP)))
    assert np.all(eT <= bT) and np.all(eP <= bP)
    for b in range(B):
        assert _bits(T[fo[b]], np.eye(4))
    wT, wP = swo.sweep_transforms(G["P_ego"], fo, G["P_vehicle_lidar"], G["P_ego_cam"], G["P_vehicle_cam"])
    assert _bits(T, wT) and _bits(Pcp, wP)
    # a frame without a sweep: a zero P_cam_pc, the others as before; device offsets are taken as they are
    fo2 = torch.tensor([0, 7, 7, 11, 13], dtype=torch.int32, device=dev)
    T2, P2 = (_np(t) for t in sweeps.sweep_transforms(P[0], fo2, P[1], P[2], P[3]))
    assert np.all(P2[1] == 0) and _bits(P2[0], Pcp[0]) and _bits(T2[:7], T[:7]) and _bits(T2[7], np.eye(4))


def _acc(d, T, **kw):
    return [_np(t) for t in sweeps.accumulate_sweeps(d["rows"], d["sweep_offsets"], d["frame_offsets"], T, **kw)]


def test_accumulate_equals_the_oracle_and_meets_the_reference(dev, on_device, oracle):
    T = _t(G["T"], dev)
    pts, off, kept, status = _acc(on_device, T)
    total = int(off[-1])
    assert np.array_equal(off, oracle["offsets"]) and np.array_equal(kept, oracle["kept"]) and np.array_equal(status, oracle["status"])
    assert np.array_equal(off, G["offsets"]) and np.array_equal(kept, G["kept"]) and list(status) == [0, 0, 0, 4]
    assert _bits(pts[:total], oracle["points"])                                          # coordinates and intensity, bit for bit
    assert np.all(pts[total:] == 0)                                                      # nothing written past the batch
    err = np.abs(pts[:total, :3].astype(np.float64) - G["cloud64"])
    print("accumulate: largest error %.3f float32 ulp of the reference's fp64 cloud" % (err / f32_ulp(G["cloud64"])).max())
    assert np.all(err <= f32_ulp(G["cloud64"]))
    # intensities and the key sweeps' rows: the input's bits
    so, fo = G["sweep_offsets"], G["frame_offsets"]
    src = np.concatenate([G["rows"][so[s]:so[s + 1]][swo.keep_mask(G["rows"][so[s]:so[s + 1]])] for s in range(fo[3])])
    assert _bits(pts[:total, 3], src[:, 3])
    for b in range(3):
        n = kept[fo[b]]
        assert _bits(pts[off[b]:off[b] + n], src[off[b]:off[b] + n, :4]), b
    # the same rows without the ring column: the same bytes
    four = dict(on_device, rows=on_device["rows"][:, :4].contiguous())
    again = _acc(four, T)
    assert all(_bits(a, b) for a, b in zip(again, (pts, off, kept, status)))
    # another box
    wide = _acc(on_device, T, box=(3.0, 5.0))
    want = swo.accumulate(G["rows"], so, fo, G["T"], box=(3.0, 5.0))
    assert np.array_equal(wide[1], want["offsets"]) and _bits(wide[0][:wide[1][-1]], want["points"]) and wide[1][-1] < total


def test_accumulate_with_several_tiles_per_part(dev):
    """A sweep is cut into 32 parts of ceil(ceil(n / 32) / 256) * 256 rows, and a workgroup takes 256 rows per iteration: up to 8192 rows a part
    is one iteration.  Here the key sweep of frame 0 has 34 720 rows (the reference's size: 1280-row parts, five iterations, the last part
    short), its transformed sweep 8 203 (512-row parts, two iterations, a last part of 11 rows and 15 empty parts), frame 1 a key sweep of
    9 001 rows and a transformed one of 300; about 4 % of the rows lie inside the box.  Offsets, kept counts and every row against the numpy
    restatement, bit for bit, with 5 and with 4 columns."""
    counts = [34720, 8203, 9001, 300]
    s = synthetic.make_nuscenes_sweeps(np.random.default_rng(21), 2, [2, 2], counts)
    rows, so, fo = (_np(t) for t in sweeps.pack_sweeps(s["frames"], device="cpu"))
    P = [swo.pose_matrices(r) for r in (np.concatenate(s["ego"]), s["lidar_calib"], s["cam_pose"], s["cam_calib"])]
    T, _ = swo.sweep_transforms(P[0], fo, P[1], P[2], P[3])
    want = swo.accumulate(rows, so, fo, T)
    assert all(0 < k < n for k, n in zip(want["kept"], counts)) and any(k % 256 for k in want["kept"])          # rows removed inside every sweep
    for cols in (5, 4):
        d = dict(rows=_t(rows[:, :cols], dev), sweep_offsets=so, frame_offsets=fo)
        pts, off, kept, status = _acc(d, _t(T, dev))
        total = int(off[-1])
        assert np.array_equal(off, want["offsets"]) and np.array_equal(kept, want["kept"]) and list(status) == [0, 0], cols
        assert _bits(pts[:total], want["points"]), cols
        assert np.all(pts[total:] == 0), cols


def test_accumulate_at_the_chunk_edges_of_the_prefix(dev):
    """The per-frame prefix over the part counts runs in chunks of 64 parts, 32 parts to a sweep: frames of 2, 4, 3 and 1 sweeps are 64 (exactly
    one chunk), 128 (two), 96 (one and a half) and 32 (half a chunk) parts.  Sweeps of 300 rows: 256-row parts, two of them filled.  Offsets,
    kept counts, status and every row against the numpy restatement, bit for bit."""
    s = synthetic.make_nuscenes_sweeps(np.random.default_rng(29), 4, [2, 4, 3, 1], 300)
    rows, so, fo = (_np(t) for t in sweeps.pack_sweeps(s["frames"], device="cpu"))
    P = [swo.pose_matrices(r) for r in (np.concatenate(s["ego"]), s["lidar_calib"], s["cam_pose"], s["cam_calib"])]
    T, _ = swo.sweep_transforms(P[0], fo, P[1], P[2], P[3])
    want = swo.accumulate(rows, so, fo, T)
    assert list(want["status"]) == [0, 0, 0, 0] and list(want["offsets"]) == [0, 576, 1728, 2592, 2880] and list(want["kept"]) == [288] * 10
    pts, off, kept, status = _acc(dict(rows=_t(rows, dev), sweep_offsets=so, frame_offsets=fo), _t(T, dev))
    total = int(off[-1])
    assert np.array_equal(off, want["offsets"]) and np.array_equal(kept, want["kept"])
    assert np.array_equal(status, want["status"]) and list(status) == [0, 0, 0, 0]
    assert _bits(pts[:total], want["points"])
    assert np.all(pts[total:] == 0)


def test_status_1_leaves_the_other_frames_alone(dev, on_device):
    T = _t(G["T"], dev)
    full = _acc(on_device, T)
    counts = np.diff(full[1])
    assert counts[0] > counts[1] > counts[2] > 0 == counts[3]
    got = _acc(on_device, T, max_frame_points=int(counts[0]) - 1)
    assert list(got[3]) == [1, 0, 0, 4]
    assert np.array_equal(got[1], [0, 0, counts[1], counts[1] + counts[2], counts[1] + counts[2]])
    assert np.array_equal(got[2], full[2])                                               # the kept counts are reported for the rejected frame too
    for b in (1, 2):
        assert _bits(got[0][got[1][b]:got[1][b + 1]], full[0][full[1][b]:full[1][b + 1]]), b
    assert np.all(got[0][got[1][-1]:] == 0)
    # exactly at the limit the frame passes; a capacity the rows would pass rejects a frame the same way
    assert list(_acc(on_device, T, max_frame_points=int(counts[0]))[3]) == [0, 0, 0, 4]
    tight = _acc(on_device, T, cap=int(counts[0] + counts[1]) - 1)
    assert list(tight[3]) == [0, 1, 0, 4] and tight[1][-1] == counts[0] + counts[2]
    assert _bits(tight[0][:counts[0]], full[0][:counts[0]]) and _bits(tight[0][counts[0]:tight[1][-1]], full[0][full[1][2]:full[1][3]])


def test_status_3_for_offsets_the_kernel_rejects(dev, on_device, batches):
    first = batches[0]
    T = _t(G["T"], dev)
    full = _acc(on_device, T)
    # a sweep offset that decreases inside frame 0: that frame alone
    so = first["sweep_offsets"].copy()
    so[3] = so[2] - 1
    got = _acc(dict(on_device, sweep_offsets=_t(so, dev)), T)
    assert list(got[3]) == [3, 0, 0, 4] and np.all(got[2][:7] == 0) and got[1][1] == 0
    for b in (1, 2):
        assert _bits(got[0][got[1][b]:got[1][b + 1]], full[0][full[1][b]:full[1][b + 1]]), b
    assert np.all(got[0][got[1][-1]:] == 0)
    # a sweep offset past the row buffer
    so = first["sweep_offsets"].copy()
    so[-1] = len(first["rows"]) + 1
    got = _acc(dict(on_device, sweep_offsets=_t(so, dev)), T)
    assert list(got[3]) == [0, 0, 0, 3] and _bits(got[0][:got[1][-1]], full[0][:full[1][-1]])
    # a frame offset that decreases: that frame and every one after it (their sweeps can no longer be told apart)
    fo = first["frame_offsets"].copy()
    fo[2] = fo[1] - 1
    got = _acc(dict(on_device, frame_offsets=_t(fo, dev)), T)
    assert list(got[3]) == [0, 3, 3, 3] and got[1][-1] == got[1][1] and _bits(got[0][:got[1][1]], full[0][:full[1][1]]) and np.all(got[2][7:] == 0)
    fo = first["frame_offsets"].copy()
    fo[0] = 1
    got = _acc(dict(on_device, frame_offsets=_t(fo, dev)), T)
    assert list(got[3]) == [3, 3, 3, 3] and got[1][-1] == 0 and np.all(got[0] == 0)
    # a frame offset past the sweeps
    fo = first["frame_offsets"].copy()
    fo[-1] = len(first["sweep_offsets"])
    got = _acc(dict(on_device, frame_offsets=_t(fo, dev)), T)
    assert list(got[3]) == [0, 0, 0, 3]
    # a frame without a sweep: status 4
    got = _acc(dict(on_device, frame_offsets=torch.tensor([0, 7, 7, 11, 13], dtype=torch.int32, device=dev)), T)
    assert list(got[3]) == [0, 4, 0, 4]


def _padded(batch, S_cap, P_cap, dev):
    """the batch in buffers of the plan's capacities; the tails hold values that would show if they were read"""
    S, P = len(batch["ego"]), len(batch["rows"])
    rows = np.full((P_cap, batch["rows"].shape[1]), np.nan, np.float32)
    rows[:P] = batch["rows"]
    so = np.full(S_cap + 1, -7, np.int32)
    so[:S + 1] = batch["sweep_offsets"]
    ego = np.full((S_cap, 7), np.nan)
    ego[:S] = batch["ego"]
    out = dict(rows=rows, sweep_offsets=so, frame_offsets=batch["frame_offsets"].astype(np.int32), ego=ego)
    out.update({k: batch[k] for k in RECORD_KEYS[1:]})
    return {k: _t(v, dev) for k, v in out.items()}


def _caps(batches):
    return max(len(b["ego"]) for b in batches) + 3, max(len(b["rows"]) for b in batches) + 7


def _eager(batch, camera, dev, mode, seed):
    """the eager stages one after the other, then the loader's sample preparation"""
    P = [sweeps.pose_matrices(_t(batch[k], dev)) for k in RECORD_KEYS]
    T, Pcp = sweeps.sweep_transforms(P[0], batch["frame_offsets"], P[1], P[2], P[3])
    pts, off, kept, st = sweeps.accumulate_sweeps(_t(batch["rows"], dev), batch["sweep_offsets"], batch["frame_offsets"], T)
    nine = sample_prep.prepare_samples((pts, None), camera["raw"], camera["K"], Pcp, NU, mode, seed, offsets=off, dataset="nuscenes")
    return dict(pts=pts, off=off, kept=kept, st=st, Pcp=Pcp, nine=nine)


def _run(plan, p, *more, **kw):
    return plan.run(p["rows"], p["sweep_offsets"], p["frame_offsets"], p["ego"], p["lidar_calib"], p["cam_pose"], p["cam_calib"], *more, **kw)


@pytest.mark.parametrize("mode", ["val", "train"])
def test_plans_equal_the_eager_composition(dev, batches, camera, mode):
    S_cap, P_cap = _caps(batches)
    for i, batch in enumerate(batches):
        want = _eager(batch, camera, dev, mode, 21 + i)
        total, S = int(_np(want["off"])[-1]), len(batch["ego"])
        counts = np.diff(_np(want["off"]))
        assert i or (counts[0] > 2 * N > counts[1] > 0)                   # the loader's 0.2 m pass runs for one frame of the golden batch and not for another
        p = _padded(batch, S_cap, P_cap, dev)
        sp = sweeps.SweepPlan(B, S_cap, P_cap, P_cap, 4000, cols=5, device=dev)
        got = _run(sp, p)
        assert _same(got[1], want["off"]) and _same(got[2][:S], want["kept"]) and _same(got[3], want["st"]) and _same(got[4], want["Pcp"])
        assert _same(got[0][:total], want["pts"][:total]) and np.all(_np(got[0][total:]) == 0) and np.all(_np(got[2][S:]) == 0)
        rp = sweeps.NuScenesRawPlan(NU, B, S_cap, P_cap, P_cap, 4000, HW, mode, cols=5, device=dev)
        out = _run(rp, p, camera["img"], camera["dK"], seed=21 + i)
        assert len(out) == 11 and _same(out[9], want["st"]) and tuple(out[10].shape) == (B, 4, 4) and out[10].dtype == torch.float64
        for name, a, b in zip(NINE, out, want["nine"]):
            assert _same(a, b), (i, name)
        assert _same(rp.sweeps.points[:total], want["pts"][:total]) and _same(rp.P_cam_pc, want["Pcp"])
        assert rp.sweeps.ws.data_ptr() == rp.sample.points.ws.data_ptr()          # one workspace
        assert list(_np(out[9])) == ([0, 0, 0, 4] if i == 0 else [0, 0, 0, 0])
        # T_scan is the Pr of the draw: P = P_cam_pc . Pr^-1
        Pr, Pgt = _np(out[10]), _np(out[5]).astype(np.float64)
        for b in range(B):
            assert np.allclose(Pgt[b] @ Pr[b], _np(want["Pcp"])[b, :3], rtol=0, atol=2e-5 * max(1.0, np.abs(Pgt[b]).max()))
        if mode == "val":
            assert _bits(Pr, np.tile(np.eye(4), (B, 1, 1)))
    # the convenience form is the same run (a batch without a rejected frame: it checks the status)
    s = synthetic.make_nuscenes_sweeps(np.random.default_rng(12), 2, [3, 2], 150)
    conv = sweeps.prepare_nuscenes_raw(s["frames"], s["ego"], s["lidar_calib"], s["cam_pose"], s["cam_calib"], camera["raw"][:2], camera["K"][:2], NU,
                                       mode, seed=3)
    rows, so, fo = (_np(t) for t in sweeps.pack_sweeps(s["frames"], device="cpu"))
    want = _eager(dict(rows=rows, sweep_offsets=so, frame_offsets=fo, ego=np.concatenate(s["ego"]), lidar_calib=s["lidar_calib"],
                       cam_pose=s["cam_pose"], cam_calib=s["cam_calib"]), {k: v[:2] for k, v in camera.items()}, dev, mode, 3)
    for name, a, b in zip(NINE, conv, want["nine"]):
        assert _same(a, b), name
    assert np.all(_np(conv[9]) == 0)
    inside = [[np.array([[0.1, 0.2, -1.0, 5.0, 0.0]], np.float32)]]
    one = np.array([[1.0, 0, 0, 0, 0, 0, 0]])
    with pytest.raises(sweeps.DeepI2PHipError, match="no sweep or no surviving row"):
        sweeps.prepare_nuscenes_raw(inside, [one], one, one, one, camera["raw"][:1], camera["K"][:1], NU)


@pytest.mark.parametrize("mode", ["val", "train"])
def test_graph_replay_equals_eager(dev, batches, camera, mode):
    S_cap, P_cap = _caps(batches)
    want = [_eager(batch, camera, dev, mode, 31 + i) for i, batch in enumerate(batches)]
    buf = _padded(batches[0], S_cap, P_cap, dev)
    sp = sweeps.SweepPlan(B, S_cap, P_cap, P_cap, 4000, cols=5, device=dev)
    rp = sweeps.NuScenesRawPlan(NU, B, S_cap, P_cap, P_cap, 4000, HW, mode, cols=5, device=dev)

    def run_both():
        return _run(sp, buf), _run(rp, buf, camera["img"], camera["dK"], seed=None)

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
        rp.seed.fill_(31 + i)
        for t in (a[0], rp.sweeps.points) + tuple(b[:5]):
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        w = want[i]
        total, S = int(_np(w["off"])[-1]), len(batches[i]["ego"])
        assert _same(a[1], w["off"]) and _same(a[2][:S], w["kept"]) and _same(a[3], w["st"]) and _same(a[4], w["Pcp"]), i
        assert _same(a[0][:total], w["pts"][:total]) and _same(rp.sweeps.points[:total], w["pts"][:total]), i
        assert _same(b[9], w["st"]), i
        for name, x, y in zip(NINE, b, w["nine"]):
            assert _same(x, y), (i, name)
