"""GPU: raw frames in one call -- raw_prep.RawFramePlan against the eager chain it replaces (scan_prep.preprocess_velodyne followed by
sample_prep.prepare_samples), its graph replay, the exposed transform T_scan, and raw_pipeline.RawFrameExecutor against
pipeline.RegistrationExecutor fed the tensors the plan produced.  Small shapes: 2048 points, 64 x 128 images, scans of about 20 k points."""
import os

import numpy as np
import pytest
import torch

from deepi2p_amd import raw_prep, sample_prep, scan_prep, synthetic

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "sample_prep_golden.npz"))
K_RAW, PC = G["K_raw"], G["item_Pc"]
N, H, W = 2048, 64, 128
RAW_HW = (370, 1226)
NAMES = ("pc", "intensity", "sn", "node_a", "node_b", "img")
NINE = ("pc", "intensity", "sn", "node_a", "node_b", "P", "img", "K", "t_ji")


def _np(t):
    return t.cpu().numpy()


def _same(a, b):
    """bit for bit (NaN payloads included)"""
    return a.dtype == b.dtype and a.shape == b.shape and _np(a).tobytes() == _np(b).tobytes()


@pytest.fixture(scope="module")
def data(dev):
    scans = [synthetic.make_velodyne_scan(np.random.default_rng(60 + i), azimuths=300) for i in range(3)]
    raw = np.stack([synthetic.make_camera_image(np.random.default_rng(100 + i)) for i in range(3)])
    return dict(scans=scans, raw=raw, dimg=torch.from_numpy(raw).to(dev), empty=np.zeros((0, 4), np.float32))


def _opt(fine=False):
    return synthetic.OptLike(N, H, W, fine)


def _KP(B, dev=None):
    K, Pc = np.tile(K_RAW, (B, 1, 1)), np.tile(PC, (B, 1, 1))
    return (K, Pc) if dev is None else tuple(torch.from_numpy(a).to(dev) for a in (K, Pc))


def _plan(scans, dev, max_frame_points=None, method="cells", cap=None):
    points, offsets, host = scan_prep.pack(scans, dev)
    mfp = int(np.diff(host).max()) if max_frame_points is None else max_frame_points
    plan = raw_prep.RawFramePlan(_opt(), len(scans), points.shape[0] if cap is None else cap, mfp, RAW_HW, "val", "kitti", method, dev)
    return plan, points, offsets


@pytest.mark.parametrize("method", ["cells", "query"])
def test_plan_equals_the_eager_chain(dev, data, method):
    scans = [data["scans"][0], data["empty"], data["scans"][1]]
    B = 3
    K, Pc = _KP(B)
    recs = scan_prep.preprocess_velodyne(scans, device=dev)
    assert recs[1].shape == (7, 0) and recs[0].shape[1] > 2 * N          # the 0.3 m pass of the loader runs
    want = sample_prep.prepare_samples(recs, data["raw"][:B], K, Pc, _opt(), "val", seed=5)
    plan, points, offsets = _plan(scans, dev, method=method)
    Kd, Pd = _KP(B, dev)
    got = plan.run(points, offsets, data["dimg"][:B], Kd, Pd, seed=5)
    assert len(got) == 11
    for name, a, b in zip(NINE, got, want):
        assert _same(a, b), name
    assert np.all(_np(got[9]) == 0) and tuple(got[10].shape) == (B, 4, 4) and got[10].dtype == torch.float64
    assert np.all(_np(got[0][1]) == 0)                                     # the empty frame gives zeros
    # the convenience wrapper is the same run
    conv = raw_prep.prepare_raw(scans, data["raw"][:B], K, Pc, _opt(), "val", 5, normals_method=method)
    for name, a, b in zip(NINE, conv, want):
        assert _same(a, b), name


def test_graph_replay_equals_eager(dev, data):
    scans = data["scans"][:2]
    B = 2
    plan, points, offsets = _plan(scans, dev)
    Kd, Pd = _KP(B, dev)
    img = data["dimg"][:B]
    eager = {s: [t.clone() for t in plan.run(points, offsets, img, Kd, Pd, seed=s)] for s in (11, 12)}
    assert not torch.equal(eager[11][0], eager[12][0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        plan.run(points, offsets, img, Kd, Pd, seed=None)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = plan.run(points, offsets, img, Kd, Pd, seed=None)
    for s in (12, 11):
        plan.seed.fill_(s)
        for t in out[:5]:
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager[s], out):
            assert _same(a, b), s


def test_T_scan_is_the_transform_of_the_gather(dev, data):
    scans = data["scans"][:2]
    plan, points, offsets = _plan(scans, dev)
    Kd, Pd = _KP(2, dev)
    out = plan.run(points, offsets, data["dimg"][:2], Kd, Pd, seed=3)
    pc, T = _np(out[0]), _np(out[10])
    bp = plan.sample.points
    idx, v_off, v_pts = _np(bp.idx), _np(bp.v_off), _np(bp.v_pts).astype(np.float64)
    for b in range(2):
        assert np.allclose(T[b, 3], [0, 0, 0, 1]) and abs(np.linalg.det(T[b, :3, :3]) - 1) < 1e-12
        g = v_off[b] + idx[b]
        want = T[b, :3, :3] @ v_pts[g].T + T[b, :3, 3:4]
        assert np.allclose(pc[b], want, rtol=2e-7, atol=1e-6)


def test_rejected_frame_leaves_the_others_alone(dev, data):
    """a frame above max_frame_points: status 1 for it alone, zeros for it, and the other frames as in the batch that has an empty frame in
    its place (the draws are a function of the frame's index, so the place is kept)"""
    s = data["scans"]
    long = np.concatenate([s[2], s[2]])
    mfp = max(len(s[0]), len(s[1]))
    assert len(long) > mfp
    Kd, Pd = _KP(3, dev)
    cap = len(s[0]) + len(s[1]) + len(long)
    outs = []
    for mid in (long, data["empty"]):
        plan, points, offsets = _plan([s[0], mid, s[1]], dev, max_frame_points=mfp, cap=cap)
        outs.append([t.clone() for t in plan.run(points, offsets, data["dimg"][:3], Kd, Pd, seed=9)])
    assert list(_np(outs[0][9])) == [0, 1, 0] and list(_np(outs[1][9])) == [0, 0, 0]
    for name, a, b in zip(NINE, outs[0], outs[1]):
        for f in (0, 2):
            assert _same(a[f], b[f]), (name, f)
    assert np.all(_np(outs[0][0][1]) == 0)


def test_voxel_stage_keeps_a_rejected_frame_out_of_its_neighbours(dev, data):
    """the voxel grid of the good frames around (and before) a rejected one against the numpy restatement, bit for bit: the rejected
    frame's points start no voxel and belong to no voxel of the frame before them"""
    from tests import scan_prep_oracle as spo
    s = data["scans"]
    long = np.concatenate([s[2], s[2]])
    mfp = max(len(s[0]), len(s[1]))
    for frames, status in (([s[0], long, s[1]], [0, 1, 0]), ([s[0], long], [0, 1]), ([long, s[1]], [1, 0])):
        points, offsets, _ = scan_prep.pack(frames, dev)
        for voxel in (0.1, 0.3):
            st = scan_prep.voxel_down_sample(points, offsets, voxel, want_keys=True, max_frame_points=mfp)
            assert list(_np(st.status)) == status
            vo = _np(st.offsets)
            for b, f in enumerate(frames):
                sl = slice(vo[b], vo[b + 1])
                if status[b]:
                    assert vo[b + 1] == vo[b]
                    continue
                ref = spo.voxel_down_sample(f, voxel)
                assert np.array_equal(_np(st.keys)[sl], ref["keys"]), (status, voxel, b)
                assert np.array_equal(_np(st.points)[sl], ref["points"]), (status, voxel, b)
                assert np.array_equal(_np(st.intensity)[sl], ref["intensity"]), (status, voxel, b)


def _mm(dev, fine):
    from deepi2p_amd.networks import MMClassifer, MMClassiferCoarse
    opt = _opt(fine)
    opt.device = dev
    mm = (MMClassifer if fine else MMClassiferCoarse)(opt)
    mm.detector.load_state_dict(synthetic.synthetic_state_dict(opt))
    return mm


def _host_batches(data, B):
    """four batches of B frames over the three scans, ragged, with their own seeds; batch 2 in the flat form"""
    s, out = data["scans"], []
    K, Pc = _KP(B)
    for i in range(4):
        frames = [s[(i + b) % 3][: len(s[(i + b) % 3]) - 1000 * ((i + b) % 4)] for b in range(B)]
        image = torch.from_numpy(np.stack([data["raw"][(i + 2 * b) % 3] for b in range(B)]))
        hb = dict(scans=frames, image=image, K_raw=torch.from_numpy(K), Pc=torch.from_numpy(Pc), seed=20 + i)
        if i == 2:
            hb["offsets"] = np.concatenate([[0], np.cumsum([len(f) for f in frames])])
            hb["scans"] = np.concatenate(frames + [np.full((7, 4), np.nan, np.float32)])      # host rows past offsets[B] are ignored
        out.append((frames, hb))
    return out


def _p_scan_bound(P, T):
    """Both sides are fp64 sums of four products; each differs from the exact entry by at most gamma_4 sum_k |P_ik| |T_kj| with
    gamma_4 = 4u / (1 - 4u), u = 2^-53 (any summation order, fused or not), so the two differ by at most twice that."""
    u = 2.0 ** -53
    return 2.0 * (4 * u / (1 - 4 * u)) * (np.abs(P) @ np.abs(T))


@pytest.mark.parametrize("pnp", [False, True])
def test_raw_executor_equals_prepared_executor(dev, data, pnp):
    """RawFrameExecutor against RegistrationExecutor fed the tensors RawFramePlan produced for the same frames: two submits per slot on
    two streams, every staged row a step does not copy itself holding NaN.  P_scan against P @ T_scan in numpy fp64, entry by entry
    within _p_scan_bound.  di2p_compose_poses is IEEE arithmetic (rounded products summed in ascending k), so its results are reproduced
    exactly on the host: over 13,200 random pairs of rigid transforms with |t| <= 50 m the largest difference between that arithmetic and
    numpy's product was 3.90e-16 sum_k |P_ik| |T_kj| (2.8e-14 absolute); four times that is 1.56e-15, and the bound asserted here,
    2 gamma_4 = 8.9e-16 of the same sum, is below it.  The largest absolute difference of each batch is printed."""
    from deepi2p_amd.pipeline import RegistrationExecutor
    from deepi2p_amd.raw_pipeline import RawFrameExecutor
    from deepi2p_amd.registration import RegistrationPipeline
    from deepi2p_amd.registration_pnp import PnPPipeline
    B = 2
    mm = _mm(dev, pnp)
    pipe = PnPPipeline(H, W, iterations=64, seed=5) if pnp else RegistrationPipeline(H, W, R=6, seed=3)
    draws = pipe.draw(B, dev)
    kw = dict(samples=draws) if pnp else dict(restarts=draws)
    keys = ("pred", "P", "best") + (("fine_pred", "n_inliers") if pnp else ("cost",))
    batches = _host_batches(data, B)
    cap = max(sum(len(f) for f in frames) for frames, _ in batches) + 100
    mfp = max(len(f) for frames, _ in batches for f in frames)
    ex = RawFrameExecutor(mm, pipe, _opt(pnp), batches[0][1], cap, mfp, n_streams=2, normals_method="cells", **kw)
    ex.warm_up(True)
    for slot in ex.slots:          # every staged row is NaN from here on: a step may read only the rows its own submit copies
        slot.host["points"].fill_(float("nan"))
        slot.devs[0]["points"].fill_(float("nan"))
    torch.cuda.synchronize()
    got = []
    for _, hb in batches:
        out = ex.result(ex.submit(hb))
        got.append({k: out[k].clone() for k in keys + ("status", "T_scan", "P_scan")})
    assert ex.use_graph, ex.graph_error
    # the same frames through the plan, eagerly, and the prepared tensors through the existing executor
    plan = raw_prep.RawFramePlan(_opt(pnp), B, cap, mfp, RAW_HW, "val", "kitti", "cells", dev)
    Kd, Pd = _KP(B, dev)
    ref_ex = None
    for i, (frames, hb) in enumerate(batches):
        points, offsets, _ = scan_prep.pack(frames, dev)
        prepared = [t.clone() for t in plan.run(points, offsets, hb["image"].to(dev), Kd, Pd, seed=hb["seed"])]
        host = {k: prepared[j].cpu() for j, k in enumerate(NAMES[:5])}
        host["img"], host["K"] = prepared[6].cpu(), prepared[7].cpu()
        if ref_ex is None:
            ref_ex = RegistrationExecutor(mm, pipe, host["K"], host, n_streams=2, **kw)
        ref = ref_ex.result(ref_ex.submit(host))
        for k in keys:
            assert _same(got[i][k], ref[k]), (i, k)
        assert np.all(_np(got[i]["status"]) == 0)
        assert _same(got[i]["T_scan"], prepared[10]), i
        want = _np(got[i]["P"]) @ _np(got[i]["T_scan"])
        diff = np.abs(_np(got[i]["P_scan"]) - want)
        print("P_scan: batch %d largest |P_scan - P @ T_scan| = %.3e (largest |entry| %.3e)" % (i, diff.max(), np.abs(want).max()))
        assert np.all(diff <= _p_scan_bound(_np(got[i]["P"]), _np(got[i]["T_scan"]))), (i, diff.max())


def test_raw_executor_rejects_on_the_host(dev, data):
    from deepi2p_amd.raw_pipeline import RawFrameExecutor
    from deepi2p_amd.registration import RegistrationPipeline
    B = 2
    mm = _mm(dev, False)
    pipe = RegistrationPipeline(H, W, R=4, seed=3)
    frames, hb = _host_batches(data, B)[0]
    cap = sum(len(f) for f in frames)
    ex = RawFrameExecutor(mm, pipe, _opt(), hb, cap, max(len(f) for f in frames), n_streams=1, use_graph=False)
    with pytest.raises(ValueError, match="cap_raw"):
        ex.submit(dict(hb, scans=[frames[0], np.concatenate([frames[1], frames[1][:5]])]))
    with pytest.raises(ValueError, match="B = 2"):
        ex.submit(dict(hb, scans=frames[:1]))
    with pytest.raises(ValueError, match="image"):
        ex.submit(dict(hb, image=hb["image"][:, :100]))
    assert ex._next == 0                                                    # a rejected submit consumed nothing
    out = ex.result(ex.submit(hb))
    assert np.all(_np(out["status"]) == 0) and torch.isfinite(out["P_scan"]).all()
