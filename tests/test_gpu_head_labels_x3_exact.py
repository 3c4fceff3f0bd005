"""GPU: di2p_point_head_labels_x3 with operands for which both layers are exact (tests/head_x3_cases.py): the scores must equal the fp64
evaluation BIT FOR BIT, and the labels a channel-by-channel first-maximum scan of the FP64 REFERENCE -- not of the kernel's own scores.
Integer scores tie constantly (family A draws its output channels from a few identical classes, so every fine maximum is attained in several
row tiles and in both half-wave row groups): the first-maximum rule is exercised across lanes, half-waves, row tiles and the eight waves.
Pinned besides: the split of y0 while it is staged, epilogue 1's re-split and scatter of y1 into fragment order over y0's LDS, both layer-2
schedulings (CT2 = 1 up to P = 128, 2 from 129), the persistent walk over tiles, and a y0 whose row stride is larger than N.  The last one
goes to the C entry directly: ops.point_head_labels passes y0's strides on, but its require_cuda check turns every non-contiguous tensor away
first (asserted below), so the entry's `row_stride >= N` path has no caller in Python yet.
tests/test_x3_fused_cases_host.py asserts the bounds and the ties on the reference alone.  Reference: per_point_pn of
models/networks_united.py:57-74 and the argmaxes of models/multimodal_classifier.py:100-117, in fp64 on the CPU."""
import ctypes

import pytest
import torch

from tests import head_x3_cases as hc
from tests import x3_exact_cases as xc

pytestmark = pytest.mark.gpu


def _cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _describe(idx, N, P):
    b, c, n = idx[0], (idx[1] if len(idx) == 3 else None), idx[-1]
    where = "point %d of 64-point tile %d of its frame (column tile %d; the last tile: %s)" % (n % 64, n // 64, (n % 64) // 32, n // 64 == (N - 1) // 64)
    if c is None:
        return "first differing (b, n) = %s: %s" % (idx, where)
    return "first differing (b, c, n) = %s: %s; channel %d of row tile %d of %d, half-wave row group %d" % (idx, where, c % 32, c // 32, (P + 31) // 32, (c % 8) // 4)


def _same(got, ref, what, N, P):
    got = got.cpu()
    idx = xc.first_mismatch(got, ref)
    assert idx is None, "head_labels_x3 %s: %s (got %r, expected %r; %d of %d differ)" % (
        what, _describe(idx, N, P), got[idx].item(), ref[idx].item(), int((got != ref).sum()), ref.numel())
    assert torch.equal(got, ref)


def _run_all(dev, d, N, P, what):
    from deepi2p_amd import ops
    for name, _, bound in d["stages"]:
        assert float(bound.max()) < hc.LIMIT, (what, name)          # on the reference alone (the host test, for this device's sizes)
    y0 = d["y0"].to(dev)
    B = y0.shape[0]
    W1p = ops.head_labels_pack(d["W1"].to(dev).contiguous())
    dv = lambda t: None if t is None else t.to(dev)
    for i, (W2, scores, coarse, fine) in enumerate(d["tails"]):
        packed = {"W1p": W1p, "W2p": ops.head_labels_pack(W2.to(dev).contiguous()), "P": P, "sc1": dv(d["sc1"]), "sh1": dv(d["sh1"]),
                  "relu1": d["relu1"], "sc2": dv(d["sc2"]), "sh2": dv(d["sh2"])}
        s = torch.full((B, P, N), float("nan"), device=dev)
        c, f = ops.point_head_labels(y0, packed, N, scores_out=s)
        c2, f2 = ops.point_head_labels(y0, packed, N)
        tag = "%s, output layer %d of %d" % (what, i, len(d["tails"]))
        _same(s, scores, tag + ", scores", N, P)
        _same(c, coarse, tag + ", coarse labels", N, P)
        _same(f, fine, tag + ", fine labels", N, P)
        _same(c2, coarse, tag + ", coarse labels without scores", N, P)
        _same(f2, fine, tag + ", fine labels without scores", N, P)


@pytest.mark.parametrize("family", hc.LABEL_FAMILIES)
@pytest.mark.parametrize("config", hc.LABEL_CONFIGS, ids=hc.labels_config_id)
def test_head_labels_x3_scores_and_labels_equal_fp64(dev, config, family):
    B, N, P = config
    if N is None:
        N = hc.labels_big_n(_cus(dev))
        assert B * -(-N // 64) == _cus(dev) + 3          # three workgroups loop twice, the others once
    _run_all(dev, hc.labels_case(family, B, N, P), N, P, (family, hc.labels_config_id(config)))


@pytest.mark.parametrize("family", ["A", "B"])
def test_head_labels_x3_y0_with_a_row_stride_larger_than_n(dev, family):
    """y0 as a column slice of a wider buffer that is NaN behind column N (row stride N + 27, the batch stride with it), handed to
    di2p_point_head_labels_x3 itself: scores and labels equal the reference of the contiguous case bit for bit.  A NaN that the staging read
    would show in the scores and, ranking above every number, in the labels."""
    from deepi2p_amd import _lib, ops
    B, N, P = 3, 65, 129
    d = hc.labels_case(family, B, N, P)
    for name, _, bound in d["stages"]:
        assert float(bound.max()) < hc.LIMIT, (family, name)
    big = torch.full((B, 256, N + 27), float("nan"), device=dev)
    big[:, :, :N] = d["y0"].to(dev)
    y0 = big[:, :, :N]
    assert y0.stride() == (256 * (N + 27), N + 27, 1) and not y0.is_contiguous()
    W2, scores, coarse, fine = d["tails"][0]
    keep = [ops.head_labels_pack(d["W1"].to(dev).contiguous()), ops.head_labels_pack(W2.to(dev).contiguous()), d["sc1"].to(dev), d["sh1"].to(dev),
            None if d["sc2"] is None else d["sc2"].to(dev), None if d["sh2"] is None else d["sh2"].to(dev)]
    with pytest.raises(RuntimeError, match="contiguous"):          # the wrapper does not admit the view
        ops.point_head_labels(y0, {"W1p": keep[0], "W2p": keep[1], "P": P, "sc1": keep[2], "sh1": keep[3], "relu1": d["relu1"], "sc2": keep[4],
                                   "sh2": keep[5]}, N)
    for with_scores in (True, False):
        s = torch.full((B, P, N), float("nan"), device=dev) if with_scores else None
        c = torch.full((B, N), -1, dtype=torch.int32, device=dev)
        f = torch.full((B, N), -1, dtype=torch.int32, device=dev)
        h = _lib.HeadLabelsX3T()
        h.y0, h.batch_stride, h.row_stride, h.K = _lib.ptr(y0), y0.stride(0), y0.stride(1), 256
        h.W1p, h.scale1, h.shift1, h.relu1 = _lib.ptr(keep[0]), _lib.ptr(keep[2]), _lib.ptr(keep[3]), int(bool(d["relu1"]))
        h.W2p, h.scale2, h.shift2, h.P = _lib.ptr(keep[1]), _lib.ptr(keep[4]), _lib.ptr(keep[5]), P
        h.scores, h.coarse, h.fine = _lib.ptr(s), _lib.ptr(c), _lib.ptr(f)
        _lib.call("di2p_point_head_labels_x3", ctypes.byref(h), B, N, _lib.stream())
        tag = "%s, row stride %d, scores %s" % (family, N + 27, with_scores)
        if with_scores:
            _same(s, scores, tag + ", scores", N, P)
        _same(c, coarse, tag + ", coarse labels", N, P)
        _same(f, fine, tag + ", fine labels", N, P)
