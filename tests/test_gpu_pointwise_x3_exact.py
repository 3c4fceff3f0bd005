"""GPU: the bf16x3 pointwise GEMMs (di2p_pointwise_gemm_x3, di2p_pointwise_gemm_x3p) with operands for which the bf16x3 arithmetic is exact
(tests/x3_exact_cases.py; cases and fp64 references: tests/pointwise_x3_cases.py).  Every call is ops.pointwise_gemm(..., x3=True) and must
equal the fp64 einsum of the same operands bit for bit: every source kind, ragged K-steps and N tiles, partial 128-row tiles, every
epilogue, and the split-planes hand-over into both planes kernels."""
import pytest
import torch

from tests import pointwise_x3_cases as pw
from tests import x3_exact_cases as xc

pytestmark = pytest.mark.gpu


def _same(got, ref, what, M):
    got, ref = got.cpu(), ref.float()
    idx = xc.first_mismatch(got, ref)
    assert idx is None, "%s: first differing index %s of %s (got %r, expected %r; %d of %d differ; last 128-row tile starts at row %d)" % (
        what, idx, tuple(ref.shape), float(got[idx]), float(ref[idx]), int((got != ref).sum()), ref.numel(), (M - 1) // 128 * 128)
    assert torch.equal(got, ref)


def _srcs(ops, _lib, dev, parts):
    out = []
    for kind, t, gi in parts:
        if kind == "dense":
            out.append(ops.Src(t.to(dev)))
        elif kind == "gather":
            out.append(ops.Src(t.to(dev), _lib.SRC_GATHER, gidx=gi.to(dev)))
        else:
            out.append(ops.Src(t.to(dev), _lib.SRC_GROUP, group=pw.GROUP))
    return out


@pytest.mark.parametrize("family", xc.FAMILIES)
@pytest.mark.parametrize("case", pw.SOURCE_CASES, ids=pw.source_id)
def test_pointwise_x3_sources_are_exact(dev, case, family):
    from deepi2p_amd import _lib, ops
    (K, M, N), kind = case
    c = pw.source_case(family, K, M, N, kind)
    Wt = c["w"].t().contiguous().to(dev)
    y = ops.pointwise_gemm(_srcs(ops, _lib, dev, c["parts"]), Wt, M, N, x3=True)
    _same(y, c["ref"], "family %s, %s" % (family, pw.source_id(case)), M)


@pytest.mark.parametrize("case", pw.EPILOGUE_CASES, ids=pw.source_id)
def test_pointwise_x3_epilogues_are_exact_on_family_a(dev, case):
    from deepi2p_amd import ops
    (K, M, N), kind = case
    c = pw.epilogue_case(K, M, N, kind)
    kw = dict(c["kw"])
    for name in ("scale", "shift", "batch_bias"):
        if name in kw:
            kw[name] = kw[name].to(dev)
    if "gathered" in kw:
        kw["gathered"] = [tuple(None if t is None else t.to(dev) for t in tab) for tab in kw["gathered"]]
    got = ops.pointwise_gemm([ops.Src(c["x"].to(dev))], c["w"].t().contiguous().to(dev), M, N, x3=True, **kw)
    if isinstance(c["ref"], tuple):
        assert isinstance(got, tuple) and len(got) == 2
        _same(got[0], c["ref"][0], pw.source_id(case) + " (full output)", M)
        _same(got[1], c["ref"][1], pw.source_id(case) + " (group maxima)", M)
    else:
        _same(got, c["ref"], pw.source_id(case), M)


@pytest.mark.parametrize("M2", pw.PLANES["M2"])
@pytest.mark.parametrize("family", pw.PLANES["families"])
def test_pointwise_x3_planes_handover_is_exact(dev, family, M2):
    """a first layer writes its output as split planes; di2p_pointwise_gemm_x3p consumes them on the 128-row kernel (M = 384) and on the
    256-row kernel (M = 256)"""
    from deepi2p_amd import ops
    K, M1, N = pw.PLANES["K"], pw.PLANES["M1"], pw.PLANES["N"]
    c = pw.planes_case(family, M2)
    planes = ops.pointwise_gemm([ops.Src(c["x"].to(dev))], c["w1"].t().contiguous().to(dev), M1, N, x3=True, planes_out=True)
    assert isinstance(planes, ops.X3Planes)
    _same(planes.float(), c["ref1"], "family %s: the planes of the first layer" % family, M1)
    y2 = ops.pointwise_gemm([planes], c["w2"].t().contiguous().to(dev), M2, N)
    _same(y2, c["ref2"], "family %s: the consumer of the planes (M = %d)" % (family, M2), M2)
