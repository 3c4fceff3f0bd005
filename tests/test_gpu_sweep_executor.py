"""GPU: sweep_pipeline.SweepFrameExecutor with the tiny model configuration of tests/test_gpu_raw_frames.py (2048 points, 64 x 128 images), the
Gauss-Newton back end and a frame="enu" pipeline (nuScenes clouds are z-up): two submits against sweeps.NuScenesRawPlan followed by the
pipeline called directly, with and without graphs; evaluation mode with a rejected frame; P_scan = P . T_scan."""
import numpy as np
import pytest
import torch

from deepi2p_amd import evaluation, ops, sweeps, synthetic
from tests.test_gpu_raw_frames import H, W, _mm, _opt, _p_scan_bound

pytestmark = pytest.mark.gpu
B, RAW_HW, MODE = 2, (450, 650), "val_random_Ry"          # top crop 100, scale 1/5: 70 x 130 before the 64 x 128 window


def _np(t):
    return t.cpu().numpy()


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and _np(a).tobytes() == _np(b).tobytes()


@pytest.fixture(scope="module")
def host_batches():
    """two batches of B frames (3 + 2 and 2 + 3 sweeps, ragged), the second in the flat form, and a third whose frame 1 lies inside the ego box"""
    out = []
    for i, counts in enumerate(([3, 2], [2, 3], [3, 2])):
        rng = np.random.default_rng(40 + i)
        s = synthetic.make_nuscenes_sweeps(rng, B, counts, [int(n) for n in rng.integers(2500, 3500, sum(counts))])
        raw = np.stack([synthetic.make_camera_image(np.random.default_rng(200 + 2 * i + b), RAW_HW[0], RAW_HW[1]) for b in range(B)])
        K = np.tile(np.array([[600.0, 0, RAW_HW[1] / 2 + 0.3], [0, 600.0, RAW_HW[0] / 2 - 0.7], [0, 0, 1]]), (B, 1, 1))
        hb = dict(sweeps=s["frames"], ego=s["ego"], lidar_calib=s["lidar_calib"], cam_pose=s["cam_pose"], cam_calib=s["cam_calib"],
                  image=torch.from_numpy(raw), K_raw=torch.from_numpy(K), seed=50 + i)
        if i == 1:
            flat = [x for f in s["frames"] for x in f]
            hb.update(sweeps=np.concatenate(flat + [np.full((5, 5), np.nan, np.float32)]), ego=np.concatenate(s["ego"]),
                      sweep_offsets=np.concatenate([[0], np.cumsum([len(x) for x in flat])]), frame_offsets=np.concatenate([[0], np.cumsum(counts)]))
        if i == 2:
            for x in hb["sweeps"][1]:
                x[:, :2] *= np.float32(0.7) / np.abs(x[:, :2]).max()          # every return on the ego car: the frame keeps no row
        out.append((s, hb))
    return out


def _caps(host_batches):
    S_cap = max(sum(len(f) for f in s["frames"]) for s, _ in host_batches) + 2
    cap = max(sum(len(x) for f in s["frames"] for x in f) for s, _ in host_batches) + 100
    mfp = max(sum(len(x) for x in f) for s, _ in host_batches for f in s["frames"])
    return S_cap, cap, mfp


def _padded(s, S_cap, cap, dev):
    rows, so, fo = sweeps.pack_sweeps(s["frames"], device="cpu")
    S, P = len(so) - 1, int(so[-1])
    r = torch.full((cap, 5), float("nan"))
    r[:P] = rows[:P]
    o = torch.full((S_cap + 1,), P, dtype=torch.int32)
    o[:S + 1] = so
    ego = torch.zeros((S_cap, 7), dtype=torch.float64)
    ego[:, 0] = 1.0
    ego[:S] = torch.from_numpy(np.concatenate(s["ego"]))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return (r.to(dev), o.to(dev), fo.to(dev), ego.to(dev), t(s["lidar_calib"]), t(s["cam_pose"]), t(s["cam_calib"]))


@pytest.mark.parametrize("graph,override", [(True, True), (False, True), (True, False)])
def test_sweep_executor_equals_the_plan_and_the_pipeline(dev, host_batches, graph, override):
    """every staged row a step does not copy itself holds NaN; the pose solve is the pipeline called directly on the plan's tensors.
    override=False is the executor as a user runs it, the solver fed the network's own prediction (as tests/test_gpu_raw_frames.py does)."""
    from deepi2p_amd.registration import RegistrationPipeline
    from deepi2p_amd.sweep_pipeline import SweepFrameExecutor
    mm = _mm(dev, False)
    pipe = RegistrationPipeline(H, W, R=6, seed=3, frame="enu")
    restarts = pipe.draw(B, dev)
    S_cap, cap, mfp = _caps(host_batches)
    # the synthetic weights predict no point inside the image, which leaves the solver nothing to do: with override it gets seeded labels
    # instead, while the network's own prediction is still compared
    labels = torch.from_numpy(np.random.default_rng(9).integers(0, 2, (B, _opt().input_pt_num)).astype(np.int32)).to(dev) if override else None
    ex = SweepFrameExecutor(mm, pipe, _opt(), host_batches[0][1], S_cap, cap, mfp, n_streams=2, use_graph=graph, restarts=restarts, mode=MODE,
                            labels_override=labels)
    ex.warm_up(True)
    for slot in ex.slots:
        slot.host["rows"].fill_(float("nan"))
        slot.devs[0]["rows"].fill_(float("nan"))
    torch.cuda.synchronize()
    keys = ("pred", "P", "best", "cost", "status", "T_scan", "P_cam_pc", "P_scan")
    got = []
    for _, hb in host_batches[:2]:
        out = ex.result(ex.submit(hb))
        got.append({k: out[k].clone() for k in keys})
    assert ex.use_graph == graph, ex.graph_error
    plan = sweeps.NuScenesRawPlan(_opt(), B, S_cap, cap, cap, mfp, RAW_HW, MODE, cols=5, device=dev)
    for i, (s, hb) in enumerate(host_batches[:2]):
        p = _padded(s, S_cap, cap, dev)
        prepared = plan.run(*p, hb["image"].to(dev), hb["K_raw"].to(dev), seed=hb["seed"])
        pc, intensity, sn, node_a, node_b, _, img, K = prepared[:8]
        logits = mm.detector(pc, intensity, sn, node_a, node_b, img)
        pred = ops.argmax_channels(logits[0] if isinstance(logits, tuple) else logits)
        ref = pipe(pc, labels if override else pred, K.double().contiguous(), restarts)
        for k in ("P", "best", "cost"):
            assert _same(got[i][k], ref[k]), (i, k)
        assert _same(got[i]["pred"], pred), i
        assert np.all(_np(got[i]["status"]) == 0)
        assert _same(got[i]["T_scan"], prepared[10]) and _same(got[i]["P_cam_pc"], plan.P_cam_pc), i
        T = _np(got[i]["T_scan"])
        assert not np.array_equal(T[0], np.eye(4)) and np.array_equal(T[:, 2], np.tile([0.0, 0, 1, 0], (B, 1)))      # a rotation about z
        want = _np(got[i]["P"]) @ T
        diff = np.abs(_np(got[i]["P_scan"]) - want)
        print("P_scan: batch %d largest |P_scan - P @ T_scan| = %.3e" % (i, diff.max()))
        assert np.all(diff <= _p_scan_bound(_np(got[i]["P"]), T)), (i, diff.max())
    assert not override or not _same(got[0]["P"], got[1]["P"])


def test_sweep_executor_evaluation_mode(dev, host_batches):
    """the errors are pose_errors of out["P"] against the prepared sample's own P; the summary counts only the frames with status 0"""
    from deepi2p_amd.registration import RegistrationPipeline
    from deepi2p_amd.sweep_pipeline import SweepFrameExecutor
    mm = _mm(dev, False)
    pipe = RegistrationPipeline(H, W, R=4, seed=3, frame="enu")
    S_cap, cap, mfp = _caps(host_batches)
    ex = SweepFrameExecutor(mm, pipe, _opt(), host_batches[0][1], S_cap, cap, mfp, n_streams=1, restarts=pipe.draw(B, dev), mode=MODE, evaluate=True)
    assert ex.eval_state().n == 0
    counts = []
    for i, status in ((0, [0, 0]), (2, [0, 4])):
        ex.eval_reset()
        out = ex.result(ex.submit(host_batches[i][1]))
        assert list(_np(out["status"])) == status
        P_prepared = ex.slots[0].plan.sample.table.P[:B].double()
        rte, rre, flags = evaluation.pose_errors(out["P"], P_prepared, out["cost"], frame="enu")
        for k, t in (("rte", rte), ("rre", rre), ("flags", flags)):
            assert _np(out[k]).tobytes() == _np(t).tobytes(), (i, k)
        counts.append(ex.eval_state().n)
    assert ex.use_graph, ex.graph_error
    assert counts == [2, 1]


def test_sweep_executor_rejects_on_the_host(dev, host_batches):
    from deepi2p_amd.registration import RegistrationPipeline
    from deepi2p_amd.sweep_pipeline import SweepFrameExecutor
    mm = _mm(dev, False)
    pipe = RegistrationPipeline(H, W, R=4, seed=3, frame="enu")
    s, hb = host_batches[0]
    total = sum(len(x) for f in s["frames"] for x in f)
    ex = SweepFrameExecutor(mm, pipe, _opt(), hb, 5, total, total, n_streams=1, use_graph=False, mode=MODE)
    with pytest.raises(ValueError, match="cap_raw"):
        ex.submit(dict(hb, sweeps=[s["frames"][0], s["frames"][1][:1] + [np.concatenate([s["frames"][1][1], s["frames"][1][1][:5]])]]))
    with pytest.raises(ValueError, match="S_cap"):
        ex.submit(dict(hb, sweeps=[s["frames"][0] + s["frames"][0][:1], s["frames"][1]], ego=[np.concatenate([s["ego"][0], s["ego"][0][:1]]), s["ego"][1]]))
    with pytest.raises(ValueError, match="B = 2"):
        ex.submit(dict(hb, sweeps=s["frames"][:1], ego=s["ego"][:1]))
    with pytest.raises(ValueError, match="image"):
        ex.submit(dict(hb, image=hb["image"][:, :100]))
    assert ex._next == 0                                                    # a rejected submit consumed nothing
    out = ex.result(ex.submit(hb))
    assert np.all(_np(out["status"]) == 0) and torch.isfinite(out["P_scan"]).all()
