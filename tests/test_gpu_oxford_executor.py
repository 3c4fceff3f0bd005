"""GPU: submap_pipeline.OxfordFrameExecutor with the tiny model configuration of tests/test_gpu_raw_frames.py (2048 points, 64 x 128 images;
128 x 256 raw frames, the smallest the Oxford option block takes for that image at its scale 1/2): submits against submap.OxfordRawPlan
followed by the classifier and the pipeline called directly, with and without graphs; the PnP back end against RegistrationExecutor fed the
plan's tensors; evaluation mode with a rejected sub-map; T_scan = Pr . G_cam and P_scan = P . T_scan; host rejections; and one end-to-end
case on a rendered traversal (world.TraversalPlan)."""
import numpy as np
import pytest
import torch

from deepi2p_amd import evaluation, ops, prep, submap, synthetic, world
from deepi2p_amd._lib import call, ptr, stream
from tests.test_gpu_raw_frames import H, NAMES, W, _mm, _opt, _p_scan_bound

pytestmark = pytest.mark.gpu
B, RAW_HW, MODE, SKIP = 2, (128, 256), "val_random_Ry", 0.1 / 16.0
K_ONE = np.array([[200.0, 0, RAW_HW[1] / 2 + 0.3], [0, 200.0, RAW_HW[0] / 2 - 0.7], [0, 0, 1]])


def _np(t):
    return t.cpu().numpy()


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and _np(a).tobytes() == _np(b).tobytes()


@pytest.fixture(scope="module")
def host_batches():
    """two batches of B sub-maps (120 + 90 and 80 + 130 profiles, ragged), the second in the flat form with rows past its end, and a third
    whose sub-map 1 has only missing profiles"""
    out = []
    for i, counts in enumerate(([120, 90], [80, 130], [120, 90])):
        rng = np.random.default_rng(70 + i)
        trav = synthetic.make_lms_traversal(rng, B, counts, 60)
        raw = np.stack([synthetic.make_camera_image(np.random.default_rng(400 + 2 * i + b), RAW_HW[0], RAW_HW[1]) for b in range(B)])
        P = np.tile(np.eye(4), (B, 1, 1))
        P[:, :3, 3] = rng.uniform(-0.5, 0.5, (B, 3))
        Gc = trav["G_cam"] if i == 0 else np.tile(trav["G_cam"], (B, 1, 1))
        hb = dict(submaps=trav["submaps"], G_posesource_laser=trav["G_posesource_laser"], G_cam=Gc, image=torch.from_numpy(raw),
                  K_raw=torch.from_numpy(np.tile(K_ONE, (B, 1, 1))), P_cam_pc=torch.from_numpy(P), seed=80 + i)
        if i == 2:
            hb["submaps"] = [trav["submaps"][0], ([None] * counts[1], trav["submaps"][1][1])]
        packed = [_np(t) for t in submap.pack_scans(hb["submaps"], device="cpu")]
        if i == 1:
            del hb["submaps"]
            hb.update(scan_xyr=np.concatenate([packed[0], np.full((5, 3), np.nan)]), scan_offsets=packed[1], submap_offsets=packed[2],
                      poses=packed[3], present=packed[4])
        out.append((packed, hb))
    return out


def _caps(host_batches):
    S_cap = max(len(p[3]) for p, _ in host_batches) + 3
    P_cap = max(int(p[1][-1]) for p, _ in host_batches) + 100
    mfp = max(int(np.diff(p[1][p[2]]).max()) for p, _ in host_batches)
    return S_cap, P_cap, mfp


def _padded(packed, hb, S_cap, P_cap, dev):
    """the batch in buffers of the plan's capacities, as the executor stages it; the row tail holds NaN"""
    xyr, so, mo, poses, present = packed
    S, P = int(mo[-1]), int(so[-1])
    x = np.full((P_cap, 3), np.nan)
    x[:P] = xyr[:P]
    o = np.full(S_cap + 1, P, np.int32)
    o[:S + 1] = so[:S + 1]
    ps = np.tile(np.eye(4), (S_cap, 1, 1))
    ps[:S] = poses[:S]
    pr = np.zeros(S_cap, np.uint8)
    pr[:S] = present[:S]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    Gc = np.asarray(hb["G_cam"], dtype=np.float64)
    Gc = np.tile(Gc, (B, 1, 1)) if Gc.shape == (4, 4) else Gc
    return (t(x), t(o), t(mo.astype(np.int32)), t(ps), t(pr), t(np.asarray(hb["G_posesource_laser"], dtype=np.float64)), t(Gc), hb["image"].to(dev),
            hb["K_raw"].to(dev), hb["P_cam_pc"].to(dev))


def _executor(mm, pipe, hb, caps, fine=False, **kw):
    from deepi2p_amd.submap_pipeline import OxfordFrameExecutor
    S_cap, P_cap, mfp = caps
    return OxfordFrameExecutor(mm, pipe, _opt(fine), hb, S_cap, P_cap, P_cap, mfp, mode=MODE, skip_threshold=SKIP, **kw)


def _plan(caps, dev, fine=False):
    S_cap, P_cap, mfp = caps
    return submap.OxfordRawPlan(_opt(fine), B, S_cap, P_cap, P_cap, mfp, RAW_HW, MODE, skip_threshold=SKIP, device=dev)


def _nan_rows(ex):
    for slot in ex.slots:          # every staged row is NaN from here on: a step may read only the rows its own submit copies
        slot.host["scan_xyr"].fill_(float("nan"))
        slot.devs[0]["scan_xyr"].fill_(float("nan"))
    torch.cuda.synchronize()


def _check_T_scan(got, plan, padded, i):
    """T_scan bit for bit compose(Pr, G_cam), no identity; P_cam_pc the staged one; P_scan against P @ T_scan within _p_scan_bound"""
    Pr, Gc = plan.sample.table.Pr[:B], padded[6]
    want = torch.zeros_like(Pr)
    call("di2p_compose_poses", ptr(Pr), ptr(Gc), B, ptr(want), stream())
    assert _same(got["T_scan"], want), i
    T = _np(got["T_scan"])
    assert not np.allclose(T[0], np.eye(4), atol=0.1) and not np.array_equal(_np(Pr)[0], np.eye(4))
    assert np.all(np.abs(T - _np(Pr) @ _np(Gc)) <= _p_scan_bound(_np(Pr), _np(Gc))), i
    assert got["P_cam_pc"].dtype == torch.float64 and _same(got["P_cam_pc"], padded[9].double()), i
    diff = np.abs(_np(got["P_scan"]) - _np(got["P"]) @ T)
    print("P_scan: batch %d largest |P_scan - P @ T_scan| = %.3e" % (i, diff.max()))
    assert np.all(diff <= _p_scan_bound(_np(got["P"]), T)), (i, diff.max())


@pytest.mark.parametrize("graph,override", [(True, True), (False, True), (True, False)])
def test_oxford_executor_equals_the_plan_and_the_pipeline(dev, host_batches, graph, override):
    """every staged row a step does not copy itself holds NaN; the pose solve is the pipeline called directly on the plan's tensors.
    override=False is the executor as a user runs it, the solver fed the network's own prediction."""
    from deepi2p_amd.registration import RegistrationPipeline
    mm = _mm(dev, False)
    pipe = RegistrationPipeline(H, W, R=6, seed=3)          # frame="cam": the Oxford record is in a camera frame
    restarts = pipe.draw(B, dev)
    caps = _caps(host_batches)
    labels = torch.from_numpy(np.random.default_rng(9).integers(0, 2, (B, _opt().input_pt_num)).astype(np.int32)).to(dev) if override else None
    ex = _executor(mm, pipe, host_batches[0][1], caps, n_streams=2, use_graph=graph, restarts=restarts, labels_override=labels)
    ex.warm_up(True)
    _nan_rows(ex)
    keys = ("pred", "P", "best", "cost", "status", "T_scan", "P_cam_pc", "P_scan")
    got = []
    for _, hb in host_batches[:2]:
        out = ex.result(ex.submit(hb))
        got.append({k: out[k].clone() for k in keys})
    assert ex.use_graph == graph, ex.graph_error
    plan = _plan(caps, dev)
    for i, (packed, hb) in enumerate(host_batches[:2]):
        p = _padded(packed, hb, caps[0], caps[1], dev)
        prepared = plan.run(*p, seed=hb["seed"], with_T_scan=True)
        assert len(prepared) == 11
        pc, intensity, sn, node_a, node_b, _, img, K = prepared[:8]
        logits = mm.detector(pc, intensity, sn, node_a, node_b, img)
        pred = ops.argmax_channels(logits[0] if isinstance(logits, tuple) else logits)
        ref = pipe(pc, labels if override else pred, K.double().contiguous(), restarts)
        for k in ("P", "best", "cost"):
            assert _same(got[i][k], ref[k]), (i, k)
        assert _same(got[i]["pred"], pred), i
        assert np.all(_np(got[i]["status"]) == 0) and np.all(_np(sn) == 0)
        assert _same(got[i]["T_scan"], prepared[10]), i
        _check_T_scan(got[i], plan, p, i)
    assert not override or not _same(got[0]["P"], got[1]["P"])


def test_oxford_executor_with_the_pnp_back_end(dev, host_batches):
    """the fine model and a PnPPipeline, against RegistrationExecutor fed the tensors OxfordRawPlan produced for the same sub-maps"""
    from deepi2p_amd.pipeline import RegistrationExecutor
    from deepi2p_amd.registration_pnp import PnPPipeline
    mm = _mm(dev, True)
    pipe = PnPPipeline(H, W, iterations=64, seed=5)
    samples = pipe.draw(B, dev)
    caps = _caps(host_batches)
    ex = _executor(mm, pipe, host_batches[0][1], caps, fine=True, n_streams=2, samples=samples)
    ex.warm_up(True)
    _nan_rows(ex)
    keys = ("pred", "P", "best", "fine_pred", "n_inliers")
    got = []
    for _, hb in host_batches[:2]:
        out = ex.result(ex.submit(hb))
        got.append({k: out[k].clone() for k in keys + ("status", "T_scan", "P_cam_pc", "P_scan")})
    assert ex.use_graph, ex.graph_error
    plan = _plan(caps, dev, True)
    ref_ex = None
    for i, (packed, hb) in enumerate(host_batches[:2]):
        p = _padded(packed, hb, caps[0], caps[1], dev)
        prepared = [t.clone() for t in plan.run(*p, seed=hb["seed"], with_T_scan=True)]
        host = {k: prepared[j].cpu() for j, k in enumerate(NAMES[:5])}
        host["img"], host["K"] = prepared[6].cpu(), prepared[7].cpu()
        if ref_ex is None:
            ref_ex = RegistrationExecutor(mm, pipe, host["K"], host, n_streams=2, samples=samples)
        ref = ref_ex.result(ref_ex.submit(host))
        for k in keys:
            assert _same(got[i][k], ref[k]), (i, k)
        assert np.all(_np(got[i]["status"]) == 0) and _same(got[i]["T_scan"], prepared[10]), i
        _check_T_scan(got[i], plan, p, i)


def test_oxford_executor_evaluation_mode(dev, host_batches):
    """the errors are pose_errors of out["P"] against the prepared sample's own P; the summary counts only the sub-maps with status 0"""
    from deepi2p_amd.registration import RegistrationPipeline
    mm = _mm(dev, False)
    pipe = RegistrationPipeline(H, W, R=4, seed=3)
    ex = _executor(mm, pipe, host_batches[0][1], _caps(host_batches), n_streams=1, restarts=pipe.draw(B, dev), evaluate=True)
    assert ex.eval_state().n == 0
    counts = []
    for i, status in ((0, [0, 0]), (2, [0, 4])):
        ex.eval_reset()
        out = ex.result(ex.submit(host_batches[i][1]))
        assert list(_np(out["status"])) == status
        P_prepared = ex.slots[0].plan.sample.table.P[:B].double()
        rte, rre, flags = evaluation.pose_errors(out["P"], P_prepared, out["cost"])
        for k, t in (("rte", rte), ("rre", rre), ("flags", flags)):
            assert _np(out[k]).tobytes() == _np(t).tobytes(), (i, k)
        counts.append(ex.eval_state().n)
    assert ex.use_graph, ex.graph_error
    assert counts == [2, 1]


def test_oxford_executor_rejects_on_the_host(dev, host_batches):
    from deepi2p_amd.registration import RegistrationPipeline
    mm = _mm(dev, False)
    pipe = RegistrationPipeline(H, W, R=4, seed=3)
    packed, hb = host_batches[0]
    S, P = len(packed[3]), int(packed[1][-1])
    mfp = int(np.diff(packed[1][packed[2]]).max())
    ex = _executor(mm, pipe, hb, (S, P, mfp), n_streams=1, use_graph=False)
    sm = hb["submaps"]
    longer = list(sm[1][0])
    j = next(i for i, s in enumerate(longer) if s is not None)
    longer[j] = np.concatenate([longer[j], np.zeros((5, 3))])
    with pytest.raises(ValueError, match="P_cap"):
        ex.submit(dict(hb, submaps=[sm[0], (longer, sm[1][1])]))
    with pytest.raises(ValueError, match="S_cap"):
        ex.submit(dict(hb, submaps=[sm[0], (sm[1][0] + [None], np.concatenate([sm[1][1], np.eye(4)[None]]))]))
    with pytest.raises(ValueError, match="B = 2"):
        ex.submit(dict(hb, submaps=sm[:1]))
    with pytest.raises(ValueError, match="image"):
        ex.submit(dict(hb, image=hb["image"][:, :100]))
    with pytest.raises(ValueError, match="float64"):
        ex.submit(dict(hb, submaps=[([None if s is None else s.astype(np.float32) for s in sm[0][0]], sm[0][1]), sm[1]]))
    assert ex._next == 0                                                    # a rejected submit consumed nothing
    out = ex.result(ex.submit(hb))
    assert np.all(_np(out["status"]) == 0) and torch.isfinite(out["P_scan"]).all()


# ---------------------------------------------------------------------------------------------------------------- through world.TraversalPlan
# The one case of this file that needs the push-broom render (di2p_world_render_profiles); every test above runs without it.
def test_oxford_executor_on_a_rendered_traversal(dev):
    """TraversalPlan's outputs copied to the host and submitted; the solver is fed the ground-truth labels of the prepared points.  Status 0,
    a finite P_scan, and the executor's prepared tensors equal OxfordRawPlan.run on the plan's device outputs bit for bit.  No pose accuracy
    is asserted: none has been measured for synthetic labels at this size."""
    from deepi2p_amd.registration import RegistrationPipeline
    S, beams = 60, 181
    rng = np.random.default_rng(31)
    cal = synthetic.make_lms_traversal(rng, 1, 1, 1)
    Gl, Gc = cal["G_posesource_laser"], cal["G_cam"]
    tp = world.TraversalPlan(B, S, beams, RAW_HW[0], RAW_HW[1], dev)
    tp.set_world(world.make_street(rng, B, 40.0))
    tp.set_calibration(Gl, Gc)
    tp.set_camera(np.tile(K_ONE, (B, 1, 1)))
    tp.set_traversal(*world.traversal_inputs(world.make_trajectory(rng, B, S), S // 2, S // 2, Gl, Gc))
    outs = tp.run(seed=17)
    torch.cuda.synchronize()
    assert np.all(_np(tp.status) == 0) and int(outs[1][-1]) > B * 2048
    mfp = int(np.diff(_np(outs[1])[_np(outs[2])]).max())
    plan = submap.OxfordRawPlan(_opt(), B, tp.S_cap, tp.P_cap, tp.P_cap, mfp, RAW_HW, MODE, skip_threshold=SKIP, device=dev)
    want = [t.clone() for t in plan.run(*outs, seed=17, with_T_scan=True)]
    assert np.all(_np(want[9]) == 0)
    labels = prep.project_labels(want[0], want[5], want[7], H, W, 32)[0]
    assert 0 < int(labels.sum()) < labels.numel()                           # some of the street is inside the image, some is not
    names = ("scan_xyr", "scan_offsets", "submap_offsets", "poses", "present", "G_posesource_laser", "G_cam", "image", "K_raw", "P_cam_pc")
    hb = dict(zip(names, (t.cpu() for t in outs)), seed=17)
    hb["scan_xyr"] = hb["scan_xyr"].numpy()
    mm = _mm(dev, False)
    pipe = RegistrationPipeline(H, W, R=6, seed=3)
    ex = _executor(mm, pipe, hb, (tp.S_cap, tp.P_cap, mfp), n_streams=1, restarts=pipe.draw(B, dev), labels_override=labels)
    out = ex.result(ex.submit(hb))
    assert ex.use_graph, ex.graph_error
    assert np.all(_np(out["status"]) == 0) and torch.isfinite(out["P_scan"]).all()
    for j, (a, b) in enumerate(zip(ex.slots[0].prepared, want)):
        assert _same(a, b), j
