"""GPU: evaluation mode (csrc/eval.hip, deepi2p_amd/evaluation.py, frame="enu" of both pipelines, evaluate=True of both executors).

Bounds.  pose_errors against the reference's recorded get_P_diff (tests/golden/eval_golden.npz): 1e-9 absolute in metres and degrees --
both sides are fp64, the golden keeps the middle Euler angle of every measured difference within +-80 degrees, where the extraction is
conditioned by at most 1 / cos(80 deg) < 6, and the entries of P_pred^-1 P_gt carry a few ulp of |t| <= 60 m, so the expected agreement
is around 1e-12; flags are exact because the golden keeps every error 1e-6 away from its threshold.  Accumulator sums against numpy:
1e-12 relative (fp64 sums of at most 67 positive terms differ by at most 67 ulp between any two orders); counts, histograms and
overflow exact (no error within 1e-6 of a bin edge).  Everything else here is bit-equality between two runs of the same kernels."""
import numpy as np
import pytest
import torch

from deepi2p_amd import evaluation, prep, synthetic

pytestmark = pytest.mark.gpu
NAMES = ("pc", "intensity", "sn", "node_a", "node_b", "img")
# what an evaluate=False Gauss-Newton executor returns (RegistrationPipeline's dict and the network's prediction): unchanged by this mode
PLAIN_KEYS = {"P", "cost", "best", "yaw0", "costs", "iters", "sweeps", "params", "labels_front", "pred"}
EVAL_KEYS = {"rte", "rre", "flags", "accuracy", "coarse_gt", "fine_gt"}


@pytest.fixture(scope="module")
def G(golden):
    return golden("eval_golden.npz")


def _np(t):
    return t.cpu().numpy()


def _dev64(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)


def _flags(rte, rre, cost):
    valid = np.ones(rte.shape, np.int32) if cost is None else (cost > 1e-6).astype(np.int32)
    return valid | (np.logical_and(rte < 2.0, rre < 5.0).astype(np.int32) << 1)


# ---------------------------------------------------------------------------------------------------------------- 1. pose errors
def test_pose_errors_against_the_golden(dev, G):
    Pp, cost = _dev64(G["P_pred"], dev), _dev64(G["cost"], dev)
    worst = 0.0
    for rows in (3, 4):
        Pg = _dev64(G["P_gt"][:, :rows], dev)
        for frame, s in (("cam", ""), ("enu", "_enu")):
            for c in (cost, None):
                rte, rre, flags = evaluation.pose_errors(Pp, Pg, c, frame=frame)
                dt, dr = np.abs(_np(rte) - G["rte" + s]).max(), np.abs(_np(rre) - G["rre" + s]).max()
                print("pose_errors gt_rows %d frame %s cost %s: largest |rte - golden| %.3e m, |rre - golden| %.3e deg"
                      % (rows, frame, c is not None, dt, dr))
                worst = max(worst, dt, dr)
                assert dt <= 1e-9 and dr <= 1e-9, (rows, frame, dt, dr)
                assert np.array_equal(_np(flags), _flags(G["rte" + s], G["rre" + s], None if c is None else G["cost"])), (rows, frame)
    print("pose_errors: largest difference from the golden over all settings %.3e" % worst)


def test_pose_errors_bits_do_not_depend_on_the_batch(dev, G):
    """F = 1, 64 and 67 (one lane, a full wave, a full wave and a partial one): every frame's bits are the same"""
    Pp, Pg, cost = _dev64(G["P_pred"], dev), _dev64(G["P_gt"], dev), _dev64(G["cost"], dev)
    full = [_np(t) for t in evaluation.pose_errors(Pp, Pg, cost, frame="enu")]
    for F in (1, 64):
        part = [_np(t) for t in evaluation.pose_errors(Pp[:F].contiguous(), Pg[:F].contiguous(), cost[:F].contiguous(), frame="enu")]
        for a, b in zip(part, full):
            assert a.tobytes() == b[:F].tobytes(), F
    one = [_np(t) for t in evaluation.pose_errors(Pp[66:].contiguous(), Pg[66:].contiguous(), cost[66:].contiguous(), frame="enu")]
    for a, b in zip(one, full):
        assert a.tobytes() == b[66:].tobytes()


def test_pose_errors_stay_finite_at_gimbal_lock_and_reject_bad_arguments(dev):
    from scipy.spatial.transform import Rotation
    P = np.tile(np.eye(4), (3, 1, 1))
    for i, z in enumerate((90.0, -90.0, 90.0 - 1e-5)):
        P[i, :3, :3] = Rotation.from_euler("xzy", [20.0, z, -35.0], degrees=True).as_matrix()
    rte, rre, flags = evaluation.pose_errors(_dev64(np.tile(np.eye(4), (3, 1, 1)), dev), _dev64(P, dev))
    assert torch.isfinite(rre).all() and torch.all(rte == 0) and torch.all(rre >= 90.0 - 1e-4)
    with pytest.raises(ValueError):
        evaluation.pose_errors(_dev64(P, dev), _dev64(P[:, :2], dev))
    with pytest.raises(ValueError):
        evaluation.pose_errors(_dev64(P, dev), _dev64(P, dev), frame="sideways")
    with pytest.raises(ValueError):
        evaluation.pose_errors(_dev64(P, dev).float(), _dev64(P, dev))


# ---------------------------------------------------------------------------------------------------------------- 2. accumulator
def _numpy_state(rte, rre, flags, mask, accuracy):
    seen = mask != 0
    valid = seen & ((flags & 1) != 0)
    t, r = rte[valid], rre[valid]
    out = dict(n=int(seen.sum()), n_valid=int(valid.sum()), n_success=int((valid & ((flags & 2) != 0)).sum()),
               rte_sum=t.sum(), rte_sq=(t * t).sum(), rre_sum=r.sum(), rre_sq=(r * r).sum(),
               rte_hist=np.histogram(t, range=[0, 15], bins=60)[0], rre_hist=np.histogram(r, range=[0, 30], bins=60)[0],
               rte_over=int((t > 15).sum()), rre_over=int((r > 30).sum()), n_coarse=0, n_fine=0, coarse_sum=0.0, fine_sum=0.0)
    if accuracy is not None:
        a = accuracy[seen].astype(np.float64)
        out.update(n_coarse=int((~np.isnan(a[:, 0])).sum()), n_fine=int((~np.isnan(a[:, 1])).sum()), coarse_sum=np.nansum(a[:, 0]),
                   fine_sum=np.nansum(a[:, 1]))
    return out


def _assert_state(st, want, scale=1):
    for k in ("n", "n_valid", "n_success", "n_coarse", "n_fine", "rte_over", "rre_over"):
        assert getattr(st, k) == scale * want[k], k
    assert np.array_equal(st.rte_hist, scale * want["rte_hist"]) and np.array_equal(st.rre_hist, scale * want["rre_hist"])
    for k in ("rte_sum", "rte_sq", "rre_sum", "rre_sq", "coarse_sum", "fine_sum"):
        assert abs(getattr(st, k) - scale * want[k]) <= 1e-12 * abs(scale * want[k]), (k, getattr(st, k), scale * want[k])


@pytest.mark.parametrize("with_accuracy", [True, False])
def test_accumulator_equals_numpy(dev, G, with_accuracy):
    """reset, three updates on slices of 1, 64 and 2 frames with masked and invalid frames among them, against numpy on the survivors;
    a second reset gives zeros; one captured update replayed twice adds its batch twice"""
    rte_np, rre_np, cost_np = G["rte_enu"], G["rre_enu"], G["cost"]
    flags_np = _flags(rte_np, rre_np, cost_np)
    mask_np = np.ones(67, np.int32)
    mask_np[[0, 7, 20, 31, 65]] = 0                                        # the whole first slice, an invalid frame (20), the last slice in part
    assert (flags_np[mask_np != 0] & 1).min() == 0                         # invalid frames survive the mask too
    rng = np.random.default_rng(3)
    acc_np = rng.uniform(0, 1, (67, 2)).astype(np.float32)
    acc_np[[5, 40], 1] = np.nan
    acc_np[7] = np.nan                                                     # masked: never looked at
    rte, rre, flags = _dev64(rte_np, dev), _dev64(rre_np, dev), torch.from_numpy(flags_np).to(dev)
    mask = torch.from_numpy(mask_np).to(dev)
    accuracy = torch.from_numpy(acc_np).to(dev) if with_accuracy else None
    acc = evaluation.EvalAccumulator(dev)
    acc.buf.fill_(-1)
    acc.reset()
    assert int(acc.buf.abs().sum()) == 0
    for a, b in ((0, 1), (1, 65), (65, 67)):
        acc.update(rte[a:b], rre[a:b], flags[a:b], mask[a:b], None if accuracy is None else accuracy[a:b])
    want = _numpy_state(rte_np, rre_np, flags_np, mask_np, acc_np if with_accuracy else None)
    st = acc.state()
    _assert_state(st, want)
    assert st.n == 62 and st.n_valid < st.n and st.rte_over > 0 and st.rre_over > 0 and (st.n_fine == 60 if with_accuracy else st.n_fine == 0)
    # frame_mask NULL: every frame
    acc.reset()
    acc.update(rte, rre, flags, None, accuracy)
    _assert_state(acc.state(), _numpy_state(rte_np, rre_np, flags_np, np.ones(67, np.int32), acc_np if with_accuracy else None))
    acc.reset()
    assert int(acc.buf.abs().sum()) == 0 and acc.state().n == 0
    # a captured update replayed twice
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        acc.update(rte, rre, flags, mask, accuracy)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        acc.update(rte, rre, flags, mask, accuracy)
    acc.reset()
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    _assert_state(acc.state(), want, scale=2)


def test_device_summary_equals_the_golden_statistics(dev, G):
    """pose_errors -> accumulate -> summary / line on the device path against the restated registration_result_analysis numbers"""
    for frame in ("cam", "enu"):
        rte, rre, flags = evaluation.pose_errors(_dev64(G["P_pred"], dev), _dev64(G["P_gt"], dev), _dev64(G["cost"], dev), frame=frame)
        acc = evaluation.EvalAccumulator(dev)
        acc.update(rte, rre, flags)
        out = acc.state().summary()
        p = frame + "_"
        assert out["n"] == 67 and out["n_valid"] == int(G[p + "n_valid"])
        assert np.array_equal(out["rte_hist"], G[p + "rte_hist"]) and np.array_equal(out["rre_hist"], G[p + "rre_hist"])
        assert out["rte_overflow"] == int(G[p + "rte_over"]) and out["rre_overflow"] == int(G[p + "rre_over"])
        for k in ("rte_mean", "rte_sigma", "rre_mean", "rre_sigma", "success_rate"):
            assert abs(out[k] - float(G[p + k])) <= 1e-9, (frame, k)              # the 1e-9 of the errors themselves
        assert acc.state().line() == "RTE %.2f +- %.2f, RRE %.2f +- %.2f, success rate %.2f" % (
            G[p + "rte_mean"], G[p + "rte_sigma"], G[p + "rre_mean"], G[p + "rre_sigma"], G[p + "success_rate"] * 100)


# ---------------------------------------------------------------------------------------------------------------- 3. ENU frames
def _to_enu(pc):
    """the inverse of (x, -z, y): (x, y, z) -> (x, z, -y); exact"""
    return np.ascontiguousarray(np.stack([pc[:, 0], pc[:, 2], -pc[:, 1]], axis=1))


def test_enu2cam_points(dev, G):
    pc = torch.from_numpy(np.tile(G["pc"].astype(np.float32), (3, 1, 70)))            # [3,3,1120]: more than one block
    want = np.stack([_np(pc)[:, 0], -_np(pc)[:, 2], _np(pc)[:, 1]], axis=1)
    d = pc.to(dev)
    assert np.array_equal(_np(evaluation.enu2cam_points(d)), want)
    assert np.array_equal(_np(evaluation.enu2cam_points(d, out=d)), want)              # in place
    assert np.array_equal(_np(d)[0, :, :16], G["pc_enu2cam"].astype(np.float32))


def test_enu_frame_gauss_newton(dev):
    """the synthetic labelled scene of test_gpu_solver.py (N = 1000, 2 frames, R = 4, max_iter = 50) as it is through frame="cam" and
    mapped into the z-up frame through frame="enu": the same bits, and P = P_cam P_convert exactly"""
    from deepi2p_amd.registration import RegistrationPipeline
    H, W, F, N = 160, 512, 2, 1000
    rng = np.random.default_rng(21)
    frames = [synthetic.make_frame(rng, N=N, H=H, W=W, flip=0.05, with_image=False) for _ in range(F)]
    pc = np.stack([f["pc"] for f in frames])
    lab = torch.from_numpy(np.stack([f["labels"] for f in frames])).to(dev)
    K = torch.from_numpy(np.stack([f["K"] for f in frames])).to(dev)
    cam = RegistrationPipeline(H, W, R=4, max_iter=50, seed=1)
    restarts = cam.draw(F, dev)
    a = cam(torch.from_numpy(pc).to(dev), lab, K, restarts)
    enu = RegistrationPipeline(H, W, R=4, max_iter=50, seed=1, frame="enu")
    b = enu(torch.from_numpy(_to_enu(pc)).to(dev), lab, K, restarts)
    assert set(b) == set(a) | {"P_cam"} and "P_cam" not in a
    for k in ("params", "cost", "iters"):
        assert _np(a[k]).tobytes() == _np(b[k]).tobytes(), k
    assert _np(a["P"]).tobytes() == _np(b["P_cam"]).tobytes()
    assert torch.all(a["best"] >= 0)
    assert np.array_equal(_np(b["P"]), _np(b["P_cam"]) @ evaluation.P_CONVERT)
    # and the pose of the points as given does what it says: the ENU points through P are the camera points through P_cam
    q = np.concatenate([_to_enu(pc).astype(np.float64), np.ones((F, 1, N))], axis=1)
    p = np.concatenate([pc.astype(np.float64), np.ones((F, 1, N))], axis=1)
    assert np.allclose(_np(b["P"]) @ q, _np(b["P_cam"]) @ p, rtol=0, atol=1e-9)      # the same products summed in another order


def test_enu_frame_pnp(dev):
    """the same for PnPPipeline at the smallest shape of test_gpu_pnp_executor.py"""
    from deepi2p_amd.registration_pnp import PnPPipeline
    B, N, H, W = 2, 1024, 64, 128
    batch = synthetic.make_batch(9, B, N=N, H=H, W=W)
    pc = torch.from_numpy(batch["pc"]).to(dev)
    K = torch.from_numpy(batch["K"]).to(dev)
    coarse, fine = prep.project_labels(pc, torch.from_numpy(batch["P_gt"][:, :3, :]).float().to(dev), K.float(), H, W, 32)
    cam = PnPPipeline(H, W, iterations=64, seed=5)
    samples = cam.draw(B, dev)
    a = cam(pc, coarse, fine, K, samples)
    b = PnPPipeline(H, W, iterations=64, seed=5, frame="enu")(torch.from_numpy(_to_enu(batch["pc"])).to(dev), coarse, fine, K, samples)
    assert set(b) == set(a) | {"P_cam"}
    for k in ("outlier_ratio", "n_inliers", "n_corr", "best"):
        assert _np(a[k]).tobytes() == _np(b[k]).tobytes(), k
    assert _np(a["P"]).tobytes() == _np(b["P_cam"]).tobytes()
    assert int((a["n_corr"] > 0).sum()) == B
    assert np.array_equal(_np(b["P"]), _np(b["P_cam"]) @ evaluation.P_CONVERT)


# ---------------------------------------------------------------------------------------------------------------- 4. executor
def _summary_numpy(rte, rre, flags, accuracy):
    valid = (flags & 1) != 0
    t, r = rte[valid], rre[valid]
    return dict(n=len(rte), n_valid=int(valid.sum()), rte_mean=np.mean(t), rte_sigma=np.sqrt(np.var(t)), rre_mean=np.mean(r),
                rre_sigma=np.sqrt(np.var(r)), success_rate=np.mean(((flags & 2) != 0)[valid].astype(np.float64)),
                coarse_accuracy=np.mean(accuracy[:, 0].astype(np.float64)),
                rte_hist=np.histogram(t, range=[0, 15], bins=60)[0], rre_hist=np.histogram(r, range=[0, 30], bins=60)[0],
                rte_overflow=int((t > 15).sum()), rre_overflow=int((r > 30).sum()))


def _assert_summary(out, want):
    for k, v in want.items():
        if isinstance(v, np.ndarray) or isinstance(v, int):
            assert np.array_equal(out[k], v), k
        else:
            assert abs(out[k] - v) <= 1e-12 * abs(v), (k, out[k], v)


@pytest.mark.parametrize("graph", [True, False])
def test_executor_evaluation_mode(dev, graph):
    """B = 2 on two streams, five batches (each slot accumulates more than once): every result's errors and accuracies are what the
    eager calls give afterwards on the returned tensors, the merged state is numpy's over the ten frames (nine with one masked), and
    an evaluate=False executor is the parent's: the same keys, the same bits."""
    from deepi2p_amd.pipeline import RegistrationExecutor
    from tests.test_gpu_pipeline import _setup
    B, H, W = 2, 64, 128
    mm, pipe, K, restarts, batches, host = _setup(dev, B=B)
    labels = torch.from_numpy(batches[0]["labels"]).to(dev)
    order = (0, 1, 2, 1, 0)
    truth = [torch.from_numpy(batches[i]["P_gt"][:, :3 + (n % 2)].copy()) for n, i in enumerate(order)]      # 3-row and 4-row, f64
    subs = [dict(host[i], P=truth[n]) for n, i in enumerate(order)]
    ex = RegistrationExecutor(mm, pipe, K, subs[0], n_streams=2, use_graph=graph, restarts=restarts, labels_override=labels, evaluate=True)
    ex.warm_up(with_h2d=True)
    assert ex.use_graph == graph, ex.graph_error
    assert ex.eval_state().n == 0                                          # warming up is not a result
    K32 = K.float()

    def run(batches_in):
        got = []
        for hb in batches_in:
            out = ex.result(ex.submit(hb))
            assert set(out) == PLAIN_KEYS | EVAL_KEYS
            got.append({k: out[k].clone() for k in ("P", "cost", "pred", "rte", "rre", "flags", "accuracy", "coarse_gt", "fine_gt")})
        return got

    got = run(subs)
    for n, (i, o) in enumerate(zip(order, got)):
        rte, rre, flags = evaluation.pose_errors(o["P"], truth[n].to(dev), o["cost"])
        for k, t in (("rte", rte), ("rre", rre), ("flags", flags)):
            assert _np(o[k]).tobytes() == _np(t).tobytes(), (n, k)
        P32 = torch.eye(4)[None].repeat(B, 1, 1)
        P32[:, :truth[n].shape[1]] = truth[n].float()
        gt = prep.project_labels(host[i]["pc"].to(dev), P32.to(dev), K32, H, W)
        assert torch.equal(o["coarse_gt"], gt[0]) and torch.equal(o["fine_gt"], gt[1])
        assert _np(o["accuracy"]).tobytes() == _np(prep.label_accuracy(o["pred"], *gt)).tobytes(), n
        assert int(gt[0].sum()) > 0
    cat = lambda k: np.concatenate([_np(o[k]) for o in got])               # noqa: E731
    state = ex.eval_state()
    assert state.n == 10 and state.n_coarse == 10
    _assert_summary(state.summary(), _summary_numpy(cat("rte"), cat("rre"), cat("flags"), cat("accuracy")))
    # one frame masked out: nine frames
    ex.eval_reset()
    assert ex.eval_state().n == 0 and ex.eval_state().rte_sum == 0.0
    masked = [dict(hb) for hb in subs]
    masked[3]["frame_mask"] = torch.tensor([1, 0], dtype=torch.int32)
    got2 = run(masked)
    for a, b in zip(got, got2):
        for k in a:
            assert _np(a[k]).tobytes() == _np(b[k]).tobytes(), k          # the mask only keeps the frame out of the statistics
    keep = np.ones(10, bool)
    keep[7] = False
    state = ex.eval_state()
    assert state.n == 9
    _assert_summary(state.summary(), _summary_numpy(cat("rte")[keep], cat("rre")[keep], cat("flags")[keep], cat("accuracy")[keep]))
    # a batch without its ground truth is refused and consumes nothing
    nxt = ex._next
    with pytest.raises(ValueError, match="ground-truth"):
        ex.submit(host[0])
    with pytest.raises(ValueError, match="frame_mask"):
        ex.submit(dict(subs[0], frame_mask=torch.ones(3, dtype=torch.int32)))
    assert ex._next == nxt and ex.eval_state().n == 9
    # evaluate=False: the parent's executor
    plain = RegistrationExecutor(mm, pipe, K, host[0], n_streams=2, use_graph=graph, restarts=restarts, labels_override=labels)
    assert [k for k, _, _ in plain._staged_inputs(host[0], B)] == list(NAMES) + ["K"]
    for n, i in enumerate(order):
        out = plain.result(plain.submit(host[i]))
        assert set(out) == PLAIN_KEYS
        for k in ("P", "cost", "pred"):
            assert _np(out[k]).tobytes() == _np(got[n][k]).tobytes(), (n, k)
    with pytest.raises(ValueError, match="evaluate=True"):
        plain.eval_state()


def test_executor_evaluation_mode_pnp_in_the_enu_frame(dev):
    """PnP mode (cost is NULL: every frame valid; coarse and fine accuracies from the fine head) with a frame="enu" pipeline: the errors
    are pose_errors(..., frame="enu") of the returned P against the submitted P"""
    from deepi2p_amd.pipeline import RegistrationExecutor
    from deepi2p_amd.registration_pnp import PnPPipeline
    from tests.test_gpu_pnp_executor import _mm
    B, N, H, W = 2, 1024, 64, 128
    mm = _mm(dev, N, H, W)
    b = synthetic.make_batch(9, B, N=N, H=H, W=W)
    hb = {k: torch.from_numpy(b[k]) for k in NAMES}
    hb["pc"] = torch.from_numpy(_to_enu(b["pc"]))
    hb["P"] = torch.from_numpy(b["P_gt"] @ evaluation.P_CONVERT)           # the pose of the z-up points
    K = torch.from_numpy(b["K"])
    pipe = PnPPipeline(H, W, iterations=64, seed=5, frame="enu")
    gt = prep.project_labels(hb["pc"].to(dev), hb["P"].float().to(dev), K.float().to(dev), H, W, 32)
    ex = RegistrationExecutor(mm, pipe, K, hb, n_streams=1, labels_override=gt, evaluate=True)
    out = ex.result(ex.submit(hb))
    assert ex.use_graph, ex.graph_error
    rte, rre, flags = evaluation.pose_errors(out["P"], hb["P"].to(dev), None, frame="enu")
    for k, t in (("rte", rte), ("rre", rre), ("flags", flags)):
        assert _np(out[k]).tobytes() == _np(t).tobytes(), k
    assert torch.all((out["flags"] & 1) == 1)
    assert torch.equal(out["coarse_gt"], gt[0]) and torch.equal(out["fine_gt"], gt[1])
    assert _np(out["accuracy"]).tobytes() == _np(prep.label_accuracy(out["pred"], gt[0], out["fine_pred"], gt[1])).tobytes()
    st = ex.eval_state()
    assert st.n == B and st.n_valid == B and st.n_coarse == B


# ---------------------------------------------------------------------------------------------------------------- 5. raw executor
def test_raw_executor_evaluation_mode(dev):
    """the smallest configuration of test_gpu_raw_frames.py with one over-long frame: the errors are pose_errors of out["P"] against the
    prepared P, the rejected frame is absent from the summary, and the frame beside it is what it is beside an empty frame"""
    from deepi2p_amd.raw_pipeline import RawFrameExecutor
    from deepi2p_amd.registration import RegistrationPipeline
    from tests.test_gpu_raw_frames import H, W, _KP, _mm, _opt
    B = 2
    scans = [synthetic.make_velodyne_scan(np.random.default_rng(60 + i), azimuths=300) for i in range(2)]
    raw = np.stack([synthetic.make_camera_image(np.random.default_rng(100 + i)) for i in range(2)])
    long = np.concatenate([scans[1], scans[1]])
    mfp = max(len(s) for s in scans)
    K, Pc = _KP(B)
    base = dict(image=torch.from_numpy(raw), K_raw=torch.from_numpy(K), Pc=torch.from_numpy(Pc), seed=31)
    mm = _mm(dev, False)
    pipe = RegistrationPipeline(H, W, R=4, seed=3)
    ex = RawFrameExecutor(mm, pipe, _opt(), dict(base, scans=scans), len(scans[0]) + len(long), mfp, n_streams=1,
                          restarts=pipe.draw(B, dev), evaluate=True)
    res = {}
    for name, second in (("long", long), ("empty", np.zeros((0, 4), np.float32)), ("good", scans[1])):
        ex.eval_reset()
        out = ex.result(ex.submit(dict(base, scans=[scans[0], second])))
        P_prepared = ex.slots[0].plan.sample.table.P[:B].double()
        rte, rre, flags = evaluation.pose_errors(out["P"], P_prepared, out["cost"])
        for k, t in (("rte", rte), ("rre", rre), ("flags", flags)):
            assert _np(out[k]).tobytes() == _np(t).tobytes(), (name, k)
        res[name] = ({k: _np(out[k]).copy() for k in ("status", "rte", "rre", "flags", "accuracy")}, ex.eval_state())
    assert ex.use_graph, ex.graph_error
    (o, st), (e, st_e), (g, st_g) = res["long"], res["empty"], res["good"]
    assert list(o["status"]) == [0, 1] and list(e["status"]) == [0, 0] and list(g["status"]) == [0, 0]
    assert st.n == 1 and st_e.n == 2 and st_g.n == 2
    want = _numpy_state(o["rte"], o["rre"], o["flags"], np.array([1, 0]), o["accuracy"])
    _assert_state(st, want)
    for k in ("rte", "rre", "flags", "accuracy"):
        assert o[k][0].tobytes() == e[k][0].tobytes(), k                   # the frame beside the rejected one is unaffected
    _assert_state(st_g, _numpy_state(g["rte"], g["rre"], g["flags"], np.array([1, 1]), g["accuracy"]))
