"""GPU: map_pipeline.MapFrameExecutor(dataset="kitti") with the tiny model of tests/test_gpu_raw_frames.py (2048 points, 64 x 128 images),
B = 2, on the street of tests/map_cases.py with normals computed by MapIndex.build(normals=True): submits against
map_index.MapRawPlan(dataset="kitti") followed by the classifier and the pipeline called directly, with and without graphs, through dirty
staging buffers; the `sn` the classifier reads is the plan's; T_map_cam within the bound of tests/test_gpu_map_index.py."""
import numpy as np
import pytest
import torch

from deepi2p_amd import map_index, ops, synthetic
from tests import map_cases as mc
from tests.test_gpu_map_executor import MODE, _check_poses, _dirty, _np, _same
from tests.test_gpu_raw_frames import H, W, _mm, _opt

pytestmark = pytest.mark.gpu
B = mc.STREET_B
RAW_HW = (180, 256)          # the KITTI loader cuts 50 rows off the top and halves: 65 x 128 for the 64 x 128 window
K_ONE = np.array([[200.0, 0, RAW_HW[1] / 2 + 0.3], [0, 200.0, RAW_HW[0] / 2 - 0.7], [0, 0, 1]])


@pytest.fixture(scope="module")
def street(dev):
    world = mc.street()
    index = map_index.MapIndex.build(world["points"], mc.STREET_CELL, up_axis=1, device=dev, normals=True)
    batches = mc.street_batches(world)
    for i, hb in enumerate(batches):
        raw = np.stack([synthetic.make_camera_image(np.random.default_rng(700 + 2 * i + b), RAW_HW[0], RAW_HW[1]) for b in range(B)])
        hb.update(image=torch.from_numpy(raw), K_raw=torch.from_numpy(np.tile(K_ONE, (B, 1, 1))))
    return dict(index=index, batches=batches)


def _run_plan(plan, hb, dev):
    from deepi2p_amd.map_pipeline import host_map_frames
    T, r, image, K_raw, P_cam_pc, _, seed = host_map_frames(hb, B, RAW_HW)
    return plan.run(T.view(B, 4, 4).to(dev), r.to(dev), image.to(dev), K_raw.to(dev), P_cam_pc.to(dev), seed=seed)


@pytest.mark.parametrize("graph", [True, False])
def test_kitti_map_executor_equals_the_plan_and_the_pipeline(dev, street, graph):
    from deepi2p_amd.map_pipeline import MapFrameExecutor
    from deepi2p_amd.registration import RegistrationPipeline
    mm = _mm(dev, False)
    pipe = RegistrationPipeline(H, W, R=6, seed=3)
    restarts = pipe.draw(B, dev)
    labels = torch.from_numpy(np.random.default_rng(9).integers(0, 2, (B, _opt().input_pt_num)).astype(np.int32)).to(dev)
    ex = MapFrameExecutor(mm, pipe, _opt(), street["index"], street["batches"][0], mc.STREET_CAP, mc.STREET_MFP, mc.STREET_RADIUS, mode=MODE,
                          dataset="kitti", n_streams=2, use_graph=graph, restarts=restarts, labels_override=labels)
    ex.warm_up(True)
    for slot in ex.slots:          # the classifier's sn input IS the KITTI plan's buffer
        assert slot.plan.sample.sn is None and slot.devs[0]["sn"].data_ptr() == slot.plan.sample.points.sn.data_ptr()
    _dirty(ex)
    keys = ("pred", "P", "best", "cost", "status", "T_scan", "P_scan", "T_map_prior", "T_map_cam")
    got = []
    for hb in street["batches"]:
        out = ex.result(ex.submit(hb))
        got.append({k: out[k].clone() for k in keys})
        _dirty(ex)
    assert ex.use_graph == graph, ex.graph_error
    plan = map_index.MapRawPlan(street["index"], _opt(), B, mc.STREET_CAP, mc.STREET_MFP, mc.STREET_RADIUS, RAW_HW, MODE, dataset="kitti")
    for i, hb in enumerate(street["batches"]):
        prepared = _run_plan(plan, hb, dev)
        assert len(prepared) == 11
        pc, intensity, sn, node_a, node_b, _, img, K = prepared[:8]
        assert sn.data_ptr() == plan.sample.points.sn.data_ptr() and float(sn.abs().sum()) > 0
        logits = mm.detector(pc, intensity, sn, node_a, node_b, img)
        pred = ops.argmax_channels(logits[0] if isinstance(logits, tuple) else logits)
        ref = pipe(pc, labels, K.double().contiguous(), restarts)
        for k in ("P", "best", "cost"):
            assert _same(got[i][k], ref[k]), (i, k)
        assert _same(got[i]["pred"], pred), i
        first = lambda x: (x[0] if isinstance(x, tuple) else x).clone()
        scores = first(logits)
        assert not _same(scores, first(mm.detector(pc, intensity, torch.zeros_like(sn), node_a, node_b, img))), i          # this model reads sn
        assert np.all(_np(got[i]["status"]) == 0)
        _check_poses(got[i], hb, prepared[10], i)
    assert not _same(got[0]["P"], got[1]["P"]) and not _same(got[1]["P"], got[2]["P"])
