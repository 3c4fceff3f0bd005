"""GPU: the result overlays (csrc/vis.hip, deepi2p_amd/visualization.py, visualize= of both executors).

Everything here is bit-equality of u8 canvases.  Against tests/golden/vis_golden.npz (the reference's own loops over a stub cv2) for the
three functions, from both image forms; against tests/vis_oracle.py (which test_vis_host.py ties to the same golden) where the golden has
no case: batches of different frames, N = 1, canvas widths that are no multiple of four, f32 images with halves and values outside
0..255.  The registration inputs drawn here are moved off the ties as the golden's are (vis_oracle.near_tie: 1e-6 px, the one ordering
between the device's fp64 dot products and numpy's that cannot be pinned).  The executors' canvases are compared with the eager functions
applied to the same step's own outputs."""
import numpy as np
import pytest
import torch

from deepi2p_amd import evaluation, prep, synthetic, visualization
from tests import vis_oracle

pytestmark = pytest.mark.gpu
NAMES = ("pc", "intensity", "sn", "node_a", "node_b", "img")
N_CASES = 6
VIS_KEYS = {"vis_registration", "vis_classification"}


@pytest.fixture(scope="module")
def G(golden):
    return golden("vis_golden.npz")


def _case(G, kind, i):
    k = "%s%d_" % (kind, i)
    return {n[len(k):]: G[n] for n in G.files if n.startswith(k)}


def _np(t):
    return t.cpu().numpy()


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _forms(img_hwc):
    """the two image forms of one u8 [B,H,W,3] array: u8 HWC and the network's f32 CHW"""
    return img_hwc, np.ascontiguousarray(img_hwc.transpose(0, 3, 1, 2)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- 1. the golden
def test_classification_equals_the_golden(dev, G):
    for i in range(N_CASES):
        c = _case(G, "cls", i)
        H, W, Hd, Wd, N, s = (int(v) for v in c["dims"])
        pxpy, cp, cg, fp, fg = (_t(c[k][None], dev) for k in ("pxpy", "coarse_pred", "coarse_gt", "fine_pred", "fine_gt"))
        for img in _forms(c["img"][None]):
            fine = visualization.classification_overlay(pxpy, cp, cg, fp, fg, _t(img, dev), fine_scale=s, H_delta=Hd, W_delta=Wd)
            coarse = visualization.classification_overlay_coarse(pxpy, cp, cg, _t(img, dev), H_delta=Hd, W_delta=Wd)
            assert np.array_equal(_np(fine)[0], c["fine"]), (i, img.dtype)
            assert np.array_equal(_np(coarse)[0], c["coarse"]), (i, img.dtype)


def test_registration_equals_the_golden(dev, G):
    for i in range(N_CASES):
        c = _case(G, "reg", i)
        H, W, Hd, Wd, N, exact = (int(v) for v in c["dims"])
        pc, P, K, labels = (_t(c[k][None], dev) for k in ("pc", "P", "K", "labels"))
        for img in _forms(c["img"][None]):
            out = visualization.registration_overlay(pc, P, K, labels, _t(img, dev), H_delta=Hd, W_delta=Wd)
            assert np.array_equal(_np(out)[0], c["canvas"]), (i, img.dtype)


# ---------------------------------------------------------------------------------------------------------------- 2. the oracle
def _frames(seed, B, N, H, W, Hd, Wd):
    """B different frames: classification and registration operands as numpy arrays, the registration points off the ties"""
    rng = np.random.default_rng(seed)
    lo, hi = np.array([-Wd - 3.0, -Hd - 3.0])[None, :, None], np.array([W + Wd + 3.0, H + Hd + 3.0])[None, :, None]
    pxpy = rng.uniform(lo, hi, (B, 2, N))
    half = rng.random((B, 2, N)) < 0.3
    pxpy[half] = np.floor(pxpy[half]) + 0.5
    pxpy = pxpy.astype(np.float32)
    for j, v in enumerate((np.inf, -np.inf, np.nan, 1e30, -1e30)[:max(N - 1, 0)]):
        pxpy[j % B, j % 2, j] = v
    cp, cg = ((rng.random((B, N)) < 0.6).astype(np.int32) for _ in range(2))
    if N == 1:                                          # the one point is drawn, on a tie of each parity
        cp[:], cg[:], pxpy[:, 0, 0], pxpy[:, 1, 0] = 1, 1, W // 2 + 0.5, H // 2 - 0.5
    fp, fg = (rng.integers(0, 3, (B, N)).astype(np.int32) for _ in range(2))
    img = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    f32 = rng.uniform(-40.0, 300.0, (B, 3, H, W)).astype(np.float32)            # below 0, above 255 ...
    tie = rng.random(f32.shape) < 0.3
    f32[tie] = np.floor(f32[tie]) + 0.5                                         # ... and exact halves of both parities
    K = np.tile(np.array([[W * 0.6, 0, W / 2 + 0.3], [0, W * 0.6, H / 2 - 0.2], [0, 0, 1]]), (B, 1, 1))
    P = np.tile(np.identity(4), (B, 1, 1))
    pc = np.zeros((B, 3, N), np.float32)
    for b in range(B):
        a = rng.uniform(-0.4, 0.4)
        P[b, :3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
        P[b, :3, 3] = rng.uniform(-1, 1, 3)
        bad = np.ones(N, bool)
        while bad.any():
            n = int(bad.sum())
            z = rng.uniform(1.0, 12.0, n) * np.where(rng.random(n) < 0.1, -1.0, 1.0)
            cam = np.stack([rng.uniform(-Wd - 3, W + Wd + 3, n), rng.uniform(-Hd - 3, H + Hd + 3, n), np.ones(n)])
            cam = np.linalg.inv(K[b]) @ cam * z
            pc[b][:, bad] = (np.linalg.inv(P[b]) @ np.concatenate([cam, np.ones((1, n))]))[:3].astype(np.float32)
            bad = vis_oracle.near_tie(pc[b], P[b], K[b])
    labels = (rng.random((B, N)) < 0.5).astype(np.int32)
    return dict(pxpy=pxpy, cp=cp, cg=cg, fp=fp, fg=fg, img=img, f32=f32, pc=pc, P=P, K=K, labels=labels)


# canvas width 34: one pixel per thread; 48 with the image at a multiple of four: four pixels per thread, vector image loads; N = 1
@pytest.mark.parametrize("B,N,H,W,Hd,Wd,s", [(3, 200, 18, 30, 5, 2, 8), (3, 700, 16, 32, 4, 8, 8), (2, 1, 16, 32, 4, 8, 16), (1, 1, 9, 7, 0, 0, 4)])
def test_batches_equal_the_oracle(dev, B, N, H, W, Hd, Wd, s):
    f = _frames(11 + N, B, N, H, W, Hd, Wd)
    d = {k: _t(v, dev) for k, v in f.items()}
    for key in ("img", "f32"):
        fine = _np(visualization.classification_overlay(d["pxpy"], d["cp"], d["cg"], d["fp"], d["fg"], d[key], fine_scale=s, H_delta=Hd, W_delta=Wd))
        coarse = _np(visualization.classification_overlay_coarse(d["pxpy"], d["cp"], d["cg"], d[key], H_delta=Hd, W_delta=Wd))
        reg = _np(visualization.registration_overlay(d["pc"], d["P"], d["K"], d["labels"], d[key], H_delta=Hd, W_delta=Wd))
        for b in range(B):                              # every frame against ITS operands: no key leaks from one frame's plane to the next
            img = f[key][b]
            assert np.array_equal(fine[b], vis_oracle.classification(f["pxpy"][b], f["cp"][b], f["cg"][b], f["fp"][b], f["fg"][b], img, s, Hd, Wd))
            assert np.array_equal(coarse[b], vis_oracle.classification(f["pxpy"][b], f["cp"][b], f["cg"][b], None, None, img, 0, Hd, Wd))
            assert np.array_equal(reg[b], vis_oracle.registration(f["pc"][b], f["P"][b], f["K"][b], f["labels"][b], img, Hd, Wd))
            if N == 1:
                assert not np.array_equal(fine[b], vis_oracle.base_canvas(img, Hd, Wd, s))
    if B > 1 and N > 1:
        assert not np.array_equal(reg[0], reg[1]) and not np.array_equal(fine[0], fine[1])


def test_empty_cloud_is_the_base_canvas(dev):
    f = _frames(3, 2, 0, 16, 32, 4, 8)
    out = visualization.registration_overlay(*(_t(f[k], dev) for k in ("pc", "P", "K", "labels", "img")), H_delta=4, W_delta=8)
    for b in range(2):
        assert np.array_equal(_np(out)[b], vis_oracle.base_canvas(f["img"][b], 4, 8))


# ---------------------------------------------------------------------------------------------------------------- 3. graphs
def test_into_forms_replay_in_a_graph(dev):
    """the three *_into calls captured once and replayed twice with other inputs in between: each replay is the eager result for the inputs
    it found, so the key planes are cleared inside the capture"""
    B, N, H, W, Hd, Wd, s = 2, 300, 16, 32, 4, 8, 8
    sets = [_frames(70 + i, B, N, H, W, Hd, Wd) for i in range(3)]
    d = {k: _t(v, dev) for k, v in sets[0].items()}
    bufs = [visualization.buffers(B, H, W, dev, Hd, Wd) for _ in range(3)]

    def launch():
        visualization.classification_overlay_into(d["pxpy"], d["cp"], d["cg"], d["fp"], d["fg"], d["f32"], *bufs[0], fine_scale=s, H_delta=Hd, W_delta=Wd)
        visualization.classification_overlay_coarse_into(d["pxpy"], d["cp"], d["cg"], d["img"], *bufs[1], H_delta=Hd, W_delta=Wd)
        visualization.registration_overlay_into(d["pc"], d["P"], d["K"], d["labels"], d["img"], *bufs[2], H_delta=Hd, W_delta=Wd)

    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        launch()                                        # eager once: the library is loaded before the capture
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        launch()
    for f in sets[1:]:
        for k, v in f.items():
            d[k].copy_(_t(v, dev))
        for canvas, ws in bufs:
            ws.fill_(255)                               # stale keys of the largest index: a replay that did not clear them shows no base
        torch.cuda.synchronize(dev)
        g.replay()
        torch.cuda.synchronize(dev)
        want = (visualization.classification_overlay(d["pxpy"], d["cp"], d["cg"], d["fp"], d["fg"], d["f32"], fine_scale=s, H_delta=Hd, W_delta=Wd),
                visualization.classification_overlay_coarse(d["pxpy"], d["cp"], d["cg"], d["img"], H_delta=Hd, W_delta=Wd),
                visualization.registration_overlay(d["pc"], d["P"], d["K"], d["labels"], d["img"], H_delta=Hd, W_delta=Wd))
        for (canvas, ws), w in zip(bufs, want):
            assert torch.equal(canvas, w)
        assert np.array_equal(_np(bufs[2][0])[1], vis_oracle.registration(f["pc"][1], f["P"][1], f["K"][1], f["labels"][1], f["img"][1], Hd, Wd))


# ---------------------------------------------------------------------------------------------------------------- 4. executors
def _bits(a, b, keys):
    for k in keys:
        assert _np(a[k]).tobytes() == _np(b[k]).tobytes(), k


def test_executor_overlays(dev):
    """B = 2 on two slots, three batches (slot 0 is used twice), evaluate=True, visualize="both": both canvases are the eager functions on
    the step's own outputs; with visualize=None the dict has the keys it had, and every other output of all three executors (built without
    the argument, with None, with "both") is the same bits"""
    from deepi2p_amd.pipeline import K_NAME, RegistrationExecutor
    from tests.test_gpu_evaluation import EVAL_KEYS, PLAIN_KEYS
    from tests.test_gpu_pipeline import _setup
    B, H, W = 2, 64, 128
    mm, pipe, K, restarts, batches, host = _setup(dev, B=B)
    labels = torch.from_numpy(batches[0]["labels"]).to(dev)
    subs = [dict(host[i], P=torch.from_numpy(batches[i]["P_gt"].copy())) for i in range(3)]
    kw = dict(n_streams=2, restarts=restarts, labels_override=labels, evaluate=True)
    ex = RegistrationExecutor(mm, pipe, K, subs[0], visualize="both", **kw)
    plain = RegistrationExecutor(mm, pipe, K, subs[0], **kw)
    none = RegistrationExecutor(mm, pipe, K, subs[0], visualize=None, **kw)
    assert not hasattr(none.slots[0], "vis") and set(ex.slots[0].vis) == {"registration", "classification"}
    K32 = K.float()
    for i, hb in enumerate(subs):
        out = ex.result(ex.submit(hb))
        assert ex.use_graph, ex.graph_error
        assert set(out) == PLAIN_KEYS | EVAL_KEYS | VIS_KEYS
        slot = ex.slots[i % 2]
        pc, img = hb["pc"].to(dev), hb["img"].to(dev)
        assert tuple(out["vis_registration"].shape) == tuple(out["vis_classification"].shape) == (B, H + 200, W + 200, 3)
        want = visualization.registration_overlay(pc, out["P"], slot.dev[K_NAME], out["pred"], img)
        assert torch.equal(out["vis_registration"], want), i
        pxpy = prep.project_labels(pc, hb["P"].float().to(dev), K32, H, W, 32, want_pxpy=True)[2]
        want = visualization.classification_overlay_coarse(pxpy, out["pred"], out["coarse_gt"], img)
        assert torch.equal(out["vis_classification"], want), i
        base = visualization.registration_overlay(pc[:, :, :0].contiguous(), out["P"], slot.dev[K_NAME], out["pred"][:, :0].contiguous(), img)
        assert not torch.equal(out["vis_registration"], base) and not torch.equal(out["vis_classification"], base)      # points were drawn
        keep = {k: out[k].clone() for k in PLAIN_KEYS | EVAL_KEYS}
        for other in (plain, none):
            o = other.result(other.submit(hb))
            assert set(o) == PLAIN_KEYS | EVAL_KEYS
            _bits(o, keep, sorted(PLAIN_KEYS | EVAL_KEYS))
    ex.synchronize(), plain.synchronize()
    for a, b in zip(ex.slots, plain.slots):
        assert _np(a.eval_acc.buf).tobytes() == _np(b.eval_acc.buf).tobytes()      # the statistics too
    reg_only = RegistrationExecutor(mm, pipe, K, host[0], n_streams=1, restarts=restarts, labels_override=labels, visualize="registration")
    out = reg_only.result(reg_only.submit(host[0]))
    assert set(out) == PLAIN_KEYS | {"vis_registration"}
    assert torch.equal(out["vis_registration"], visualization.registration_overlay(host[0]["pc"].to(dev), out["P"], reg_only.slots[0].dev[K_NAME],
                                                                                   out["pred"], host[0]["img"].to(dev)))


def test_executor_overlays_pnp_in_the_enu_frame(dev):
    """PnP mode with the fine head and a frame="enu" pipeline: the classification overlay is the fine variant, and the registration overlay
    is drawn from the CONVERTED points with P_cam, as the reference does it"""
    from deepi2p_amd.pipeline import K_NAME, RegistrationExecutor
    from deepi2p_amd.registration_pnp import PnPPipeline
    from tests.test_gpu_evaluation import _to_enu
    from tests.test_gpu_pnp_executor import _mm
    B, N, H, W = 2, 1024, 64, 128
    mm = _mm(dev, N, H, W)
    b = synthetic.make_batch(9, B, N=N, H=H, W=W)
    hb = {k: torch.from_numpy(b[k]) for k in NAMES}
    hb["pc"] = torch.from_numpy(_to_enu(b["pc"]))
    hb["P"] = torch.from_numpy(b["P_gt"] @ evaluation.P_CONVERT)
    K = torch.from_numpy(b["K"])
    pipe = PnPPipeline(H, W, iterations=64, seed=5, frame="enu")
    gt = prep.project_labels(hb["pc"].to(dev), hb["P"].float().to(dev), K.float().to(dev), H, W, 32, want_pxpy=True)
    ex = RegistrationExecutor(mm, pipe, K, hb, n_streams=1, labels_override=gt[:2], evaluate=True, visualize="both")
    out = ex.result(ex.submit(hb))
    assert ex.use_graph, ex.graph_error
    pc, img, K64 = hb["pc"].to(dev), hb["img"].to(dev), ex.slots[0].dev[K_NAME]
    want = visualization.registration_overlay(evaluation.enu2cam_points(pc), out["P_cam"], K64, out["pred"], img)
    assert torch.equal(out["vis_registration"], want)
    want = visualization.classification_overlay(gt[2], out["pred"], out["coarse_gt"], out["fine_pred"], out["fine_gt"], img, fine_scale=32)
    assert torch.equal(out["vis_classification"], want)
    assert not torch.equal(want, visualization.classification_overlay_coarse(gt[2], out["pred"], out["coarse_gt"], img))      # the grid at least


def test_raw_executor_passes_the_option_through(dev):
    """the smallest configuration of test_gpu_raw_frames.py, one step: the canvases are the eager functions on the prepared frame"""
    from deepi2p_amd.pipeline import K_NAME
    from deepi2p_amd.raw_pipeline import RawFrameExecutor
    from deepi2p_amd.registration import RegistrationPipeline
    from tests.test_gpu_raw_frames import H, W, _KP, _mm, _opt
    B = 2
    scans = [synthetic.make_velodyne_scan(np.random.default_rng(60 + i), azimuths=300) for i in range(2)]
    raw = np.stack([synthetic.make_camera_image(np.random.default_rng(100 + i)) for i in range(2)])
    K, Pc = _KP(B)
    batch = dict(image=torch.from_numpy(raw), K_raw=torch.from_numpy(K), Pc=torch.from_numpy(Pc), seed=31, scans=scans)
    mm = _mm(dev, False)
    pipe = RegistrationPipeline(H, W, R=4, seed=3)
    restarts = pipe.draw(B, dev)
    ex = RawFrameExecutor(mm, pipe, _opt(), batch, sum(len(s) for s in scans), max(len(s) for s in scans), n_streams=1,
                          restarts=restarts, evaluate=True, visualize="both")
    out = ex.result(ex.submit(batch))
    assert ex.use_graph, ex.graph_error
    assert VIS_KEYS <= set(out) and tuple(out["vis_registration"].shape) == (B, H + 200, W + 200, 3)
    slot = ex.slots[0]
    d, prepared = slot.dev, slot.prepared
    assert torch.equal(out["vis_registration"], visualization.registration_overlay(d["pc"], out["P"], d[K_NAME], out["pred"], d["img"]))
    pxpy = prep.project_labels(d["pc"], prepared[5], prepared[7], H, W, 32, want_pxpy=True)[2]
    assert torch.equal(out["vis_classification"], visualization.classification_overlay_coarse(pxpy, out["pred"], out["coarse_gt"], d["img"]))
    plain = RawFrameExecutor(mm, pipe, _opt(), batch, sum(len(s) for s in scans), max(len(s) for s in scans), n_streams=1,
                             restarts=restarts, evaluate=True)
    o = plain.result(plain.submit(batch))
    assert set(o) == set(out) - VIS_KEYS
    _bits(o, out, ["P", "pred", "rte", "rre", "flags", "accuracy", "coarse_gt", "status", "P_scan"])
