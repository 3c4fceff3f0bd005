"""GPU: map_pipeline.MapFrameExecutor with the tiny model configuration of tests/test_gpu_raw_frames.py (2048 points, 64 x 128 images,
128 x 256 raw frames), B = 2, on synthetic.make_map's street of about 40 k rows (tests/map_cases.py): submits against map_index.MapRawPlan
followed by the classifier and the pipeline called directly, with and without graphs and with dirty staging buffers; T_scan, P_scan and
T_map_cam; evaluation mode against get_P_diff on (T_map_cam, T_map_cam_gt) computed on the host, with a frame whose prior lies off the map;
the PnP back end; host rejections."""
import numpy as np
import pytest
import torch

from deepi2p_amd import evaluation, map_index, ops, prep, registration, synthetic
from tests import map_cases as mc
from tests.test_gpu_map_index import _pose_bound, rigid_inverse
from tests.test_gpu_raw_frames import H, NAMES, W, _mm, _opt, _p_scan_bound

pytestmark = pytest.mark.gpu
B, RAW_HW, MODE = mc.STREET_B, (128, 256), "val_random_Ry"
K_ONE = np.array([[200.0, 0, RAW_HW[1] / 2 + 0.3], [0, 200.0, RAW_HW[0] / 2 - 0.7], [0, 0, 1]])


def _np(t):
    return t.cpu().numpy()


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and _np(a).tobytes() == _np(b).tobytes()


@pytest.fixture(scope="module")
def street(dev):
    """the map's index on the device and three host batches; the second variant has frame 1 of batch 0 off the map"""
    world = mc.street()
    index = map_index.MapIndex.build(world["points"], mc.STREET_CELL, up_axis=1, device=dev)

    def complete(batches):
        for i, hb in enumerate(batches):
            raw = np.stack([synthetic.make_camera_image(np.random.default_rng(500 + 2 * i + b), RAW_HW[0], RAW_HW[1]) for b in range(B)])
            hb.update(image=torch.from_numpy(raw), K_raw=torch.from_numpy(np.tile(K_ONE, (B, 1, 1))))
        return batches
    return dict(index=index, batches=complete(mc.street_batches(world)), off=complete(mc.street_batches(world, off_map=[(0, 1)])))


def _executor(mm, pipe, street, hb, fine=False, **kw):
    from deepi2p_amd.map_pipeline import MapFrameExecutor
    return MapFrameExecutor(mm, pipe, _opt(fine), street["index"], hb, mc.STREET_CAP, mc.STREET_MFP, mc.STREET_RADIUS, mode=MODE, **kw)


def _plan(street, fine=False):
    return map_index.MapRawPlan(street["index"], _opt(fine), B, mc.STREET_CAP, mc.STREET_MFP, mc.STREET_RADIUS, RAW_HW, MODE)


def _run_plan(plan, hb, dev):
    """MapRawPlan.run on a host batch as the executor stages it: P_cam_pc = inv(T_map_cam_gt) . T_map_prior in fp64"""
    from deepi2p_amd.map_pipeline import host_map_frames
    T, r, image, K_raw, P_cam_pc, _, seed = host_map_frames(hb, B, RAW_HW)
    return plan.run(T.view(B, 4, 4).to(dev), r.to(dev), image.to(dev), K_raw.to(dev), P_cam_pc.to(dev), seed=seed)


def _dirty(ex):
    for slot in ex.slots:          # every staged value is NaN (or 255) from here on: a step may read only what its own submit copies
        slot.host_flat.fill_(255)
        for d in slot.dev_flats:
            d.fill_(255)
        slot.host["T_map_prior"].fill_(float("nan"))
        slot.devs[0]["T_map_prior"].fill_(float("nan"))
    torch.cuda.synchronize()


def _check_poses(got, hb, T_scan_plan, i):
    """T_scan bit for bit what the sample stage applied; P_scan against P @ T_scan; T_map_cam against T_map_prior @ inv(P_scan)"""
    assert _same(got["T_scan"], T_scan_plan), i
    T = _np(got["T_scan"])
    assert not np.array_equal(T[0], np.eye(4))                               # val_random_Ry: the draw turned the crop
    diff = np.abs(_np(got["P_scan"]) - _np(got["P"]) @ T)
    assert np.all(diff <= _p_scan_bound(_np(got["P"]), T)), (i, diff.max())
    assert _np(got["T_map_prior"]).tobytes() == np.ascontiguousarray(hb["T_map_prior"]).tobytes(), i
    A, P = _np(got["T_map_prior"]), _np(got["P_scan"])
    diff = np.abs(_np(got["T_map_cam"]) - A @ rigid_inverse(P))
    print("T_map_cam: batch %d largest |T_map_cam - T_map_prior @ inv(P_scan)| = %.3e" % (i, diff.max()))
    assert np.all(diff <= _pose_bound(A, P)), (i, diff.max())


@pytest.mark.parametrize("graph", [True, False])
def test_map_executor_equals_the_plan_and_the_pipeline(dev, street, graph):
    """three batches with different priors, radii and seeds through two slots, the staging buffers dirtied between the warm-up and the
    submits; the pose solve is the pipeline called directly on the plan's tensors"""
    from deepi2p_amd.registration import RegistrationPipeline
    mm = _mm(dev, False)
    pipe = RegistrationPipeline(H, W, R=6, seed=3)
    restarts = pipe.draw(B, dev)
    labels = torch.from_numpy(np.random.default_rng(9).integers(0, 2, (B, _opt().input_pt_num)).astype(np.int32)).to(dev)
    ex = _executor(mm, pipe, street, street["batches"][0], n_streams=2, use_graph=graph, restarts=restarts, labels_override=labels)
    ex.warm_up(True)
    _dirty(ex)
    keys = ("pred", "P", "best", "cost", "status", "T_scan", "P_scan", "T_map_prior", "T_map_cam")
    got = []
    for hb in street["batches"]:
        out = ex.result(ex.submit(hb))
        got.append({k: out[k].clone() for k in keys})
        _dirty(ex)
    assert ex.use_graph == graph, ex.graph_error
    plan = _plan(street)
    for i, hb in enumerate(street["batches"]):
        prepared = _run_plan(plan, hb, dev)
        assert len(prepared) == 11
        pc, intensity, sn, node_a, node_b, _, img, K = prepared[:8]
        logits = mm.detector(pc, intensity, sn, node_a, node_b, img)
        pred = ops.argmax_channels(logits[0] if isinstance(logits, tuple) else logits)
        ref = pipe(pc, labels, K.double().contiguous(), restarts)
        for k in ("P", "best", "cost"):
            assert _same(got[i][k], ref[k]), (i, k)
        assert _same(got[i]["pred"], pred), i
        assert np.all(_np(got[i]["status"]) == 0) and np.all(_np(sn) == 0)
        _check_poses(got[i], hb, prepared[10], i)
    assert not _same(got[0]["P"], got[1]["P"]) and not _same(got[1]["P"], got[2]["P"])


def test_map_executor_evaluation_pins_the_frames(dev, street):
    """labels from the true pose; the reported RTE / RRE are get_P_diff's of (T_map_cam, T_map_cam_gt) computed on the host, whatever the
    solver found; a frame whose prior lies off the map is absent from the statistics and leaves the other frame's outputs as they were"""
    from deepi2p_amd.registration import RegistrationPipeline
    mm = _mm(dev, False)
    pipe = RegistrationPipeline(H, W, R=6, seed=3)
    restarts = pipe.draw(B, dev)
    hb, hb_off = street["batches"][0], street["off"][0]
    plan = _plan(street)
    prepared = _run_plan(plan, hb, dev)
    labels = prep.project_labels(prepared[0], prepared[5], prepared[7], H, W, 32)[0].clone()
    assert 0 < int(labels.sum()) < labels.numel()
    ex = _executor(mm, pipe, street, hb, n_streams=1, restarts=restarts, labels_override=labels, evaluate=True)
    assert ex.eval_state().n == 0
    keys = ("P", "cost", "status", "T_map_cam", "rte", "rre", "flags", "P_scan")
    outs = []
    for batch, n, status in ((hb, 2, [0, 0]), (hb_off, 1, [0, 4])):
        ex.eval_reset()
        out = ex.result(ex.submit(batch))
        out = {k: out[k].clone() for k in keys}
        assert list(_np(out["status"])) == status and ex.eval_state().n == n
        T_cam, gt = _np(out["T_map_cam"]), batch["T_map_cam_gt"]
        for f in range(B):
            if status[f] == 0:
                rte, rre = registration.get_P_diff(T_cam[f], gt[f])
                print("frame %d: RTE %.4f m, RRE %.4f deg" % (f, rte, rre))
                assert abs(float(out["rte"][f]) - rte) <= 1e-6 and abs(float(out["rre"][f]) - rre) <= 1e-6, (f, rte, rre)
                assert abs(rte - np.linalg.norm(T_cam[f, :3, 3] - gt[f, :3, 3])) <= 1e-9      # the camera's position error in the map
        dev_err = evaluation.pose_errors(out["T_map_cam"], torch.from_numpy(gt).to(dev), out["cost"])
        assert _same(out["rte"], dev_err[0]) and _same(out["rre"], dev_err[1])
        outs.append(out)
    assert ex.use_graph, ex.graph_error
    for k in ("P", "cost", "T_map_cam", "P_scan", "rte", "rre"):
        assert _np(outs[0][k])[0].tobytes() == _np(outs[1][k])[0].tobytes(), k
    with pytest.raises(ValueError, match="T_map_cam_gt"):
        ex.submit({k: v for k, v in hb.items() if k != "T_map_cam_gt"})


def test_map_executor_with_the_pnp_back_end(dev, street):
    """the fine model and a PnPPipeline, against RegistrationExecutor fed the tensors MapRawPlan produced for the same priors"""
    from deepi2p_amd.pipeline import RegistrationExecutor
    from deepi2p_amd.registration_pnp import PnPPipeline
    mm = _mm(dev, True)
    pipe = PnPPipeline(H, W, iterations=64, seed=5)
    samples = pipe.draw(B, dev)
    hb = street["batches"][1]
    ex = _executor(mm, pipe, street, hb, fine=True, n_streams=1, samples=samples)
    keys = ("pred", "P", "best", "fine_pred", "n_inliers")
    out = ex.result(ex.submit(hb))
    got = {k: out[k].clone() for k in keys + ("status", "T_scan", "P_scan", "T_map_prior", "T_map_cam")}
    assert ex.use_graph, ex.graph_error
    prepared = [t.clone() for t in _run_plan(_plan(street, True), hb, dev)]
    host = {k: prepared[j].cpu() for j, k in enumerate(NAMES[:5])}
    host["img"], host["K"] = prepared[6].cpu(), prepared[7].cpu()
    ref_ex = RegistrationExecutor(mm, pipe, host["K"], host, n_streams=1, samples=samples)
    ref = ref_ex.result(ref_ex.submit(host))
    for k in keys:
        assert _same(got[k], ref[k]), k
    assert np.all(_np(got["status"]) == 0)
    _check_poses(got, hb, prepared[10], 1)


def test_map_executor_rejects_on_the_host(dev, street):
    from deepi2p_amd.map_pipeline import MapFrameExecutor
    from deepi2p_amd.registration import RegistrationPipeline
    mm = _mm(dev, False)
    pipe = RegistrationPipeline(H, W, R=4, seed=3)
    hb = street["batches"][0]
    no_gt = {k: v for k, v in hb.items() if k != "T_map_cam_gt"}
    args = (mm, pipe, _opt(), street["index"], no_gt, mc.STREET_CAP, mc.STREET_MFP, mc.STREET_RADIUS)
    for kw, match in ((dict(dataset="kitti"), "kitti"), (dict(evaluate=True), "T_map_cam_gt"), (dict(h2d_mode="graph"), "h2d_mode")):
        with pytest.raises(ValueError, match=match):
            MapFrameExecutor(*args, mode=MODE, **kw)
    with pytest.raises(ValueError, match="MapIndex"):
        MapFrameExecutor(mm, pipe, _opt(), None, no_gt, mc.STREET_CAP, mc.STREET_MFP, mc.STREET_RADIUS)
    ex = MapFrameExecutor(*args, mode=MODE, n_streams=1, use_graph=False)          # without ground truth: P_cam_pc is the identity
    skew = hb["T_map_prior"].copy()
    skew[0, :3, :3] *= 1.01
    for bad, match in ((dict(T_map_prior=skew), "rigid"), (dict(T_map_prior=hb["T_map_prior"][:1]), "T_map_prior"),
                       (dict(radius=mc.STREET_RADIUS * 2), "max_radius"), (dict(radius=np.ones(3)), "radius"),
                       (dict(image=hb["image"][:, :100]), "image"), (dict(K_raw=hb["K_raw"][:1]), "K_raw"), (dict(radius=None), "no 'radius'")):
        with pytest.raises(ValueError, match=match):
            ex.submit(dict(no_gt, **bad))
    assert ex._next == 0                                                    # a rejected submit consumed nothing
    out = ex.result(ex.submit(no_gt))
    assert np.all(_np(out["status"]) == 0) and torch.isfinite(out["T_map_cam"]).all()
    assert np.array_equal(_np(ex.slots[0].dev["P_cam_pc"]), np.tile(np.eye(4), (B, 1, 1)))
