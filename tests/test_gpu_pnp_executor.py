"""The stream / graph executor in PnP mode (deepi2p_amd/pipeline.py with a registration_pnp.PnPPipeline): the network part of a step is
KeypointDetector.predict_labels (the fine head's layers 1-2 and both argmaxes in one launch), the solve part PnP-RANSAC.  A graph-replayed step
is BIT-identical to eager launches and to the plain calls; at BASELINE configs[2] (B = 64, 20480 points, 160 x 512, 500 EPnP samples) with GT
labels the poses meet the bound of test_gpu_fullsize.py's config-2 test."""
import numpy as np
import pytest
import torch

from deepi2p_amd import synthetic

pytestmark = pytest.mark.gpu
NAMES = ("pc", "intensity", "sn", "node_a", "node_b", "img")
KEYS = ("pred", "fine_pred", "P", "outlier_ratio", "n_inliers", "n_corr", "best")


def _mm(dev, N, H, W, fine=True):
    from deepi2p_amd.networks import MMClassifer, MMClassiferCoarse
    opt = synthetic.OptLike(N, H, W, fine)
    opt.device = dev
    mm = (MMClassifer if fine else MMClassiferCoarse)(opt)
    mm.detector.load_state_dict(synthetic.synthetic_state_dict(opt))
    return mm


def _gt_labels(dev, batch, H, W):
    from deepi2p_amd import prep
    pc = torch.from_numpy(batch["pc"]).to(dev)
    P_gt = torch.from_numpy(batch["P_gt"][:, :3, :]).float().to(dev)
    K32 = torch.from_numpy(batch["K"]).float().to(dev)
    return prep.project_labels(pc, P_gt, K32, H, W, 32)


@pytest.mark.parametrize("override,h2d_mode,split", [(False, "copy_stream", False), (True, "copy_stream", False), (True, "eager", False),
                                                     (False, "copy_stream", True)])
def test_pnp_graph_replay_equals_eager_and_plain_calls(dev, override, h2d_mode, split):
    from deepi2p_amd.pipeline import RegistrationExecutor
    from deepi2p_amd.registration_pnp import PnPPipeline
    B, N, H, W = 3, 2048, 64, 128
    mm = _mm(dev, N, H, W)
    batches = [synthetic.make_batch(700 + i, B, N=N, H=H, W=W) for i in range(3)]
    host = [{k: torch.from_numpy(b[k]) for k in NAMES} for b in batches]
    K = torch.from_numpy(batches[0]["K"]).to(dev)
    pipe = PnPPipeline(H, W, iterations=64, seed=5)
    samples = pipe.draw(B, dev)
    labels = _gt_labels(dev, batches[0], H, W) if override else None
    outs = {}
    for graph in (True, False):
        ex = RegistrationExecutor(mm, pipe, K, host[0], n_streams=2, use_graph=graph, samples=samples, labels_override=labels,
                                  h2d_mode=h2d_mode, split_solver=split)
        ex.warm_up(with_h2d=True)
        assert ex.use_graph == graph, ex.graph_error
        got = []
        for i in (0, 1, 2):                           # three batches over two slots: slot 0 is reused with new host data
            t = ex.submit(host[i])
            got.append({k: ex.result(t)[k].clone() for k in KEYS})
        outs[graph] = got
    for a, b in zip(outs[True], outs[False]):
        for k in KEYS:
            assert torch.equal(a[k], b[k]), k
    for i, g in enumerate(outs[True]):
        d = {k: host[i][k].to(dev) for k in NAMES}
        coarse, fine = mm.detector.predict_labels(*[d[k] for k in NAMES])
        co, fi = labels if labels is not None else (coarse, fine)
        ref = pipe(d["pc"], co, fi, K.to(torch.float64).contiguous(), samples)
        ref.update(pred=coarse, fine_pred=fine)
        torch.cuda.synchronize()
        for k in KEYS:
            assert torch.equal(g[k], ref[k]), (i, k)
    if override:
        assert int((outs[True][0]["n_corr"] > 0).sum()) == B     # the GT labels reach PnP


def test_pnp_executor_at_config2_with_gt_labels(dev):
    """configs[2]: B = 64, 20480 points, 160 x 512 (L = 80), 500 EPnP RANSAC samples, GT labels through labels_override (random weights
    predict nothing); the reference's cell-corner observations -> the 2 m / 8 deg bound of the config-2 test."""
    from deepi2p_amd.pipeline import RegistrationExecutor
    from deepi2p_amd.registration_pnp import PnPPipeline
    from oracle import frustum_lm as flm
    B, N, H, W = 64, 20480, 160, 512
    mm = _mm(dev, N, H, W)
    b = synthetic.make_batch(301, B, N=N, H=H, W=W)
    host = {k: torch.from_numpy(b[k]) for k in NAMES}
    pipe = PnPPipeline(H, W, iterations=500, seed=0)
    ex = RegistrationExecutor(mm, pipe, torch.from_numpy(b["K"]), host, n_streams=2, labels_override=_gt_labels(dev, b, H, W))
    out = ex.result(ex.submit(host))
    assert ex.use_graph, ex.graph_error
    assert out["pred"].shape == (B, N) and out["fine_pred"].shape == (B, N)
    assert int(out["fine_pred"].min()) >= 0 and int(out["fine_pred"].max()) < 80
    P = out["P"].cpu().numpy()
    ok = sum(1 for i in range(B) if (lambda tr: tr[0] < 2.0 and tr[1] < 8.0)(flm.get_P_diff(P[i], b["P_gt"][i])))
    assert ok >= 0.7 * B, ok


def test_pnp_executor_rejects_a_coarse_only_model_and_mixed_arguments(dev):
    from deepi2p_amd.pipeline import RegistrationExecutor
    from deepi2p_amd.registration import RegistrationPipeline
    from deepi2p_amd.registration_pnp import PnPPipeline
    B, N, H, W = 2, 1024, 64, 128
    b = synthetic.make_batch(9, B, N=N, H=H, W=W)
    host = {k: torch.from_numpy(b[k]) for k in NAMES}
    K = torch.from_numpy(b["K"])
    with pytest.raises(ValueError, match="coarse-only"):
        RegistrationExecutor(_mm(dev, N, H, W, fine=False), PnPPipeline(H, W), K, host, n_streams=1)
    mm = _mm(dev, N, H, W)
    with pytest.raises(ValueError, match="pair"):
        RegistrationExecutor(mm, PnPPipeline(H, W), K, host, n_streams=1, labels_override=torch.zeros(B, N, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError, match="samples"):
        RegistrationExecutor(mm, RegistrationPipeline(H, W), K, host, n_streams=1, samples=torch.zeros(B, 4, 6, dtype=torch.int32, device=dev))


def test_pnp_pipeline_scales_K_like_the_reference(dev):
    from deepi2p_amd.registration_pnp import PnPPipeline, camera_matrix_scaling
    K = np.stack([synthetic.make_K(160, 512), synthetic.make_K(160, 512, 0.6)])
    got = PnPPipeline(160, 512).scale_K(torch.from_numpy(K).to(dev)).cpu().numpy()
    assert np.array_equal(got, np.stack([camera_matrix_scaling(k, 1 / 32) for k in K]))
