"""GPU parity of di2p_point_head_labels_x3 (layers 1-2 of the fine per-point head and both argmaxes as one launch on the bf16 matrix
instructions with exact three-way fp32 splits, head_labels_x3.hip) against a float64 evaluation of the two layers, against the path it
replaces (layer 1 on the bf16x3 pointwise kernel, layer 2 on the fp32 kernel, two argmax_channels launches) and against argmax_channels on
its own scores; then KeypointDetector.predict_labels on the full-size golden frame of the imported reference.
Reference: per_point_pn of models/networks_united.py:57-74 (fine models: 736 -> 256 -> 256 -> 2 + L), argmax of
models/multimodal_classifier.py:100-117."""
import numpy as np
import pytest
import torch

from tests import fullsize_golden as fg

pytestmark = pytest.mark.gpu
REL = 1e-3


def _case(dev, B, N, P, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    d = dict(y0=torch.relu(r(B, 256, N)), W1=r(256, 256) / 16, W2=r(256, P) / 16, sc1=torch.rand(256, generator=g) + 0.5,
             sh1=r(256) * 0.1, sh2=r(P) * 0.1)
    return {k: v.to(dev).contiguous() for k, v in d.items()}


def _packed(d):
    from deepi2p_amd import ops
    return {"W1p": ops.head_labels_pack(d["W1"]), "W2p": ops.head_labels_pack(d["W2"]), "P": d["W2"].shape[1],
            "sc1": d["sc1"], "sh1": d["sh1"], "relu1": True, "sc2": None, "sh2": d["sh2"]}


def _pack_model(Wt, tile_major):
    """NumPy model of the 32-row A-fragment order of both head packers: the bf16x3 split by masking to the upper 16 bits, rows past M zero;
    entry (row tile t, K-step s) = [3 planes][64 lanes][8], lane i + 32 half holds k = 16 s + 8 half + 0..7 of row 32 t + i; entries
    [tile][K-step] (di2p_head_labels_x3_pack) or [K-step][tile] (di2p_head_x3_pack)."""
    K, M = Wt.shape
    T = -(-M // 32)
    W = np.zeros((K, 32 * T), np.float32)
    W[:, :M] = Wt
    p0 = W.view(np.uint32) & 0xFFFF0000
    r = W - p0.view(np.float32)
    p1 = r.view(np.uint32) & 0xFFFF0000
    p2 = (r - p1.view(np.float32)).view(np.uint32)
    planes = (np.stack([p0, p1, p2]) >> 16).astype(np.uint16).reshape(3, K // 16, 2, 8, T, 32)      # [plane][s][half][e][t][i]
    return np.ascontiguousarray(planes.transpose((4, 1, 0, 2, 5, 3) if tile_major else (1, 4, 0, 2, 5, 3))).tobytes()


@pytest.mark.parametrize("which,K,M", [("head_x3", 96, 128), ("head_x3", 128, 128), ("labels", 256, 82), ("labels", 256, 256),
                                       ("labels", 256, 1402)])
def test_head_packers_match_the_documented_layout(dev, which, K, M):
    """di2p_head_x3_pack and di2p_head_labels_x3_pack write the 32-row A-fragment order of the split weights, byte for byte."""
    from deepi2p_amd import ops
    Wt = torch.randn(K, M, generator=torch.Generator().manual_seed(K + M)) * 3
    pack = ops.head_x3_pack if which == "head_x3" else ops.head_labels_pack
    got = pack(Wt.to(dev).contiguous()).cpu().numpy().tobytes()
    assert got == _pack_model(Wt.numpy(), tile_major=which == "labels")


def _run(d, packed, with_scores=True):
    from deepi2p_amd import ops
    B, _, N = d["y0"].shape
    s = torch.full((B, packed["P"], N), float("nan"), device=d["y0"].device) if with_scores else None
    c, f = ops.point_head_labels(d["y0"], packed, N, scores_out=s)
    return c, f, s


def _ref64(d):
    y1 = torch.relu(torch.einsum("km,bkn->bmn", d["W1"].double(), d["y0"].double()) * d["sc1"].double().view(1, -1, 1)
                    + d["sh1"].double().view(1, -1, 1))
    return torch.einsum("kp,bkn->bpn", d["W2"].double(), y1) + d["sh2"].double().view(1, -1, 1)


def _unfused(d):
    """The tail predict_labels replaces: layer 1 on the bf16x3 pointwise kernel, layer 2 on the fp32 kernel, two argmax_channels."""
    from deepi2p_amd import ops
    N = d["y0"].shape[2]
    P = d["W2"].shape[1]
    y1 = ops.pointwise_gemm([ops.Src(d["y0"])], d["W1"], 256, N, scale=d["sc1"], shift=d["sh1"], relu=True, x3=True)
    s = ops.pointwise_gemm([ops.Src(y1)], d["W2"], P, N, shift=d["sh2"], x3=False)
    return s, ops.argmax_channels(s[:, 0:2]), ops.argmax_channels(s[:, 2:])


def _margin(ref):
    if ref.shape[1] == 1:                                  # a single channel: always decided
        return torch.full_like(ref[:, 0], float("inf"))
    top = ref.topk(2, dim=1).values
    return top[:, 0] - top[:, 1]


@pytest.mark.parametrize("N", [4096, 30000])
@pytest.mark.parametrize("P", [3, 52, 82, 242, 1402])
def test_head_labels_x3_scores_and_labels_vs_fp64_and_the_unfused_path(dev, P, N):
    """P = 2 + L for L = 1, 50 (nuScenes 160 x 320), 80 (KITTI 160 x 512), 240 (Oxford 384 x 640), 1400 (configs[3] 896 x 1600);
    N = 30000 leaves a ragged last 64-point tile (30000 % 64 = 48)."""
    from deepi2p_amd import ops
    B = 2
    d = _case(dev, B, N, P, 100 + P)
    packed = _packed(d)
    coarse, fine, s = _run(d, packed)
    ref = _ref64(d)
    s_old, c_old, f_old = _unfused(d)
    e_new = float((s.double() - ref).abs().max())
    e_old = float((s_old.double() - ref).abs().max())
    bound = 1.25 * e_old + 1e-7 * max(1.0, float(ref.abs().max()))
    assert e_new <= bound, (e_new, e_old)
    # the labels are argmax_channels of the kernel's own scores, bit for bit
    assert torch.equal(coarse, ops.argmax_channels(s[:, 0:2])) and torch.equal(fine, ops.argmax_channels(s[:, 2:]))
    # where float64 decides clearly, the fused labels are float64's and the unfused path's
    for lab, old, r in ((coarse, c_old, ref[:, 0:2]), (fine, f_old, ref[:, 2:])):
        clear = _margin(r) > 8 * bound
        assert float(clear.double().mean()) > 0.5           # not a vacuous comparison
        assert torch.equal(lab[clear].long(), r.argmax(1)[clear]) and torch.equal(lab[clear], old[clear])
    # the labels do not depend on whether scores are written
    c2, f2, _ = _run(d, packed, with_scores=False)
    assert torch.equal(c2, coarse) and torch.equal(f2, fine)


def test_head_labels_x3_ties_and_nans_follow_argmax_channels(dev):
    """Exact ties (zero weight columns with equal biases, within a 32-channel tile and across tiles) and NaN channels give argmax_channels'
    answer on the kernel's own scores: the first maximum, the first NaN."""
    from deepi2p_amd import ops
    B, N, P = 2, 3000, 82
    d = _case(dev, B, N, P, 7)
    d["W2"][:, [0, 1]] = 0.0
    d["sh2"][[0, 1]] = 0.25                               # coarse: a tie -> channel 0
    d["W2"][:, [12, 13, 31, 32, 60]] = 0.0
    d["sh2"][[12, 13, 31, 32, 60]] = 50.0                 # fine: five tied maxima across three tiles -> channel 12 (label 10)
    packed = _packed(d)
    coarse, fine, s = _run(d, packed)
    assert torch.equal(coarse, ops.argmax_channels(s[:, 0:2])) and torch.equal(fine, ops.argmax_channels(s[:, 2:]))
    assert bool((coarse == 0).all()) and bool((fine == 10).all())
    # NaN channels (in the second and third row tile) rank above everything: the first one wins; the coarse NaN likewise
    d["sh2"][[70, 45, 1]] = float("nan")
    coarse, fine, s = _run(d, _packed(d))
    assert torch.equal(coarse, ops.argmax_channels(s[:, 0:2])) and torch.equal(fine, ops.argmax_channels(s[:, 2:]))
    assert bool((coarse == 1).all()) and bool((fine == 43).all())
    # NaN inputs at some points: whatever the epilogues make of them, the labels are argmax_channels' on the scores
    d = _case(dev, B, N, P, 8)
    d["y0"][0, 5, 100:140] = float("nan")
    d["y0"][1, :, 2999] = float("nan")
    coarse, fine, s = _run(d, _packed(d))
    assert torch.equal(coarse, ops.argmax_channels(s[:, 0:2])) and torch.equal(fine, ops.argmax_channels(s[:, 2:]))


def test_head_labels_x3_is_deterministic_and_batch_independent(dev):
    B, N, P = 4, 5000, 242
    d = _case(dev, B, N, P, 21)
    packed = _packed(d)
    c, f, s = _run(d, packed)
    c2, f2, s2 = _run(d, packed)
    assert torch.equal(c, c2) and torch.equal(f, f2) and torch.equal(s, s2)
    for i in (0, 3):
        one = dict(d, y0=d["y0"][i:i + 1].contiguous())
        c1, f1, s1 = _run(one, packed)
        assert torch.equal(c1[0], c[i]) and torch.equal(f1[0], f[i]) and torch.equal(s1[0], s[i])


def test_head_labels_x3_rejects_bad_operands(dev):
    from deepi2p_amd import ops
    d = _case(dev, 1, 256, 82, 3)
    packed = _packed(d)
    with pytest.raises(RuntimeError, match="W1p / W2p"):
        ops.point_head_labels(d["y0"], dict(packed, P=100), 256)
    with pytest.raises(RuntimeError, match="y0"):
        ops.point_head_labels(d["y0"][:, :128].contiguous(), packed, 256)
    with pytest.raises(RuntimeError, match="scores_out"):
        ops.point_head_labels(d["y0"], packed, 256, scores_out=torch.empty(1, 80, 256, device=dev))


def _det(dev, N, H, W, fine):
    from deepi2p_amd import synthetic
    from deepi2p_amd.networks import KeypointDetector
    opt = synthetic.OptLike(N, H, W, fine)
    det = KeypointDetector(opt)
    det.load_state_dict(synthetic.synthetic_state_dict(opt))
    return det.to(dev).eval(), opt


def test_predict_labels_on_the_fullsize_reference_golden(dev, golden):
    """The full-size frame of the imported reference (B = 1, N = 20480, 160 x 512, L = 80): predict_labels meets the rule
    test_gpu_fullsize.py applies to forward() -- label flips below 0.1 %, none where the reference's own margin exceeds the tolerance --
    and its scores pass fg.check_logits."""
    from deepi2p_amd import ops
    g = golden("network_fullsize_golden.npz")
    b, N, H, W, stride = fg.inputs(g)
    det, opt = _det(dev, N, H, W, True)
    x = [torch.from_numpy(b[k]).to(dev) for k in fg.NAMES]
    L = det.H_fine_res * det.W_fine_res
    scores = torch.empty((1, 2 + L, N), device=dev)
    coarse, fine = det.predict_labels(*x, scores_out=scores)
    sc = scores.cpu().numpy()
    assert fg.check_logits(g, "fine_model", sc[:, 0:2], sc[:, 2:], REL, 1e-3)
    for head, lab in (("coarse", coarse), ("fine", fine)):
        key = "fine_model_" + head
        tol = REL * float(g[key + "_absmax"]) + 1e-7
        ref = np.unpackbits(g[key + "_labels"], axis=1)[:, :N] if head == "coarse" else g[key + "_labels"]
        diff = lab.cpu().numpy() != ref
        assert not np.any(diff & (g[key + "_margin"] > 2 * tol)), key
        assert diff.mean() < 1e-3, (key, diff.mean())
    assert torch.equal(coarse, ops.argmax_channels(scores[:, 0:2])) and torch.equal(fine, ops.argmax_channels(scores[:, 2:]))
    c2, f2 = det.predict_labels(*x)
    assert torch.equal(c2, coarse) and torch.equal(f2, fine)
    # forward() is untouched by the new method: its labels agree with predict_labels' where the margins are clear
    fc, ff = det(*x)
    assert (ops.argmax_channels(ff) != fine).float().mean() < 1e-3


def test_predict_labels_of_a_coarse_only_model(dev):
    from deepi2p_amd import ops, synthetic
    N, H, W = 2048, 64, 128
    det, opt = _det(dev, N, H, W, False)
    b = synthetic.make_batch(3, 2, N=N, H=H, W=W)
    x = [torch.from_numpy(b[k]).to(dev) for k in fg.NAMES]
    coarse, fine = det.predict_labels(*x)
    assert fine is None and torch.equal(coarse, ops.argmax_channels(det(*x)))
