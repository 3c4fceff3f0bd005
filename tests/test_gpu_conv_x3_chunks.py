"""GPU: di2p_conv3x3_x3 at the seams of its chunk structure.  The kernel runs the first chunk of input channels apart from the others (its
first product into every accumulator starts from the constant zero), the chunks between in a loop, the last one apart again (it stages no
patch), and the epilogue reads every accumulator once, adding the small products' set in that read.  One, two and three chunks are the three
ways through that code -- first alone, first + last, first + loop + last -- so the cases pin the chunk count, on every tile configuration:

  stride 1   each of the four configurations at the row length of its stage (W = 128, 64, 32, 16: a constant-row-length instance), 1, 2 and
             3 chunks (Cin = 16/32/48 on the 32 x 32 x 16 instruction, 32/64/96 on the 16 x 16 x 32 one), Cout = one Cout tile of the
             configuration; and one layer on its run-time-row-length instance whose last tile is ragged (2 chunks, Cout a tile and a piece);
  stride 2   each of the three constant-row-length instances, 1 and 2 chunks, with the fused 1 x 1 / stride-2 downsample branch.

Operands: small integers (tests/x3_exact_cases.py, family A: |x| <= 8, |w| <= 2; every partial sum is an integer below 2^24, so the bf16x3
arithmetic drops no bit in any order), scale 1, an integer shift, an integer residual.  Each case runs with residual and ReLU on and with
both off, and the output must equal the fp64 convolution (torch.nn.functional.conv2d on the CPU, models/resnet.py:56-72,160-164) BIT FOR BIT.
A case the library does not support FAILS: nothing here skips."""
import functools
from collections import namedtuple

import pytest
import torch

from tests import x3_exact_cases as xc

pytestmark = pytest.mark.gpu

Case = namedtuple("Case", "cfg Cin H W Cout stride chunks pwt ragged")
B = 2
_KS = (16, 16, 32, 32)             # input channels per chunk of configuration 0..3
_MT = (64, 128, 128, 64)           # output channels per workgroup (one Cout tile)
_ROW = (128, 64, 32, 16)           # the row length of the stage each configuration runs at 160 x 512


def _cases():
    out = []
    for cfg in range(4):
        for n in (1, 2, 3):
            out.append(Case(cfg, n * _KS[cfg], 3, _ROW[cfg], _MT[cfg], 1, n, _ROW[cfg] + 2, False))
    # run-time row length (no instance is compiled for W + 2), last tile ragged, a partial second Cout tile
    for cfg, (H, W) in enumerate(((11, 32), (6, 32), (6, 16), (3, 32))):
        out.append(Case(cfg, 2 * _KS[cfg], H, W, _MT[cfg] + 8, 1, 2, 0, True))
    # stride 2: configuration 1 at W = 128, 2 at W = 64, 3 at W = 32
    for cfg, (H, W) in ((1, (6, 128)), (2, (6, 64)), (3, (4, 32))):
        for n in (1, 2):
            out.append(Case(cfg, n * _KS[cfg], H, W, _MT[cfg], 2, n, W + 2, None))
    return out


CASES = _cases()


def _id(c):
    return "cfg%d-s%d-%dch-%dx%dx%d-%d%s" % (c.cfg, c.stride, c.chunks, c.Cin, c.H, c.W, c.Cout, "-runtime-ragged" if c.pwt == 0 else "")


def _tap_major(w):
    return w.permute(2, 3, 1, 0).reshape(-1, w.shape[0]).contiguous()


@functools.lru_cache(maxsize=None)
def _layer(c):
    """operands and fp64 references of a case, made once (callers do not write to them)"""
    L = dict(xc.conv_layer("A", B, c.Cin, c.H, c.W, c.Cout, c.stride))
    g = torch.Generator().manual_seed(xc.seed_of("chunks", tuple(c)))
    L["shift"] = torch.randint(-4, 5, (c.Cout,), generator=g).to(torch.float32)
    L["scale"] = torch.ones(c.Cout)
    assert float(L["absum"].max()) + 4 + 16 < xc.LIMIT and (c.stride == 1 or float(L["absumd"].max()) < xc.LIMIT)
    lin = L["ref"] + L["shift"].double().view(1, -1, 1, 1)
    L["plain"] = lin.float()
    L["full"] = torch.relu(lin + L["residual"].double()).float()
    assert bool((L["full"] != L["plain"]).any())
    return L


def _same(c, got, ref, what):
    got = got.cpu()
    idx = xc.first_mismatch(got, ref)
    assert idx is None, "%s %s: first differing index (b, co, oh, ow) = %s, got %r, expected %r; %d of %d differ" % (
        _id(c), what, idx, float(got[idx]), float(ref[idx]), int((got != ref).sum()), ref.numel())
    assert torch.equal(got, ref)


def test_every_case_is_supported_and_runs_where_it_claims():
    """host code of the built library: a case that is not supported, or that runs on another instance or chunk count than its row says,
    fails here and does not skip"""
    from deepi2p_amd import ops
    assert len({_id(c) for c in CASES}) == len(CASES) == 22
    for c in CASES:
        shape = (B, c.Cin, c.H, c.W)
        assert ops.conv3x3_x3_supported(shape, c.Cout, c.stride, cfg=c.cfg), _id(c)
        p = ops.conv3x3_x3_plan(shape, c.Cout, c.stride, cfg=c.cfg)
        assert p is not None and (p["cfg"], p["chunks"], p["pwt"]) == (c.cfg, c.chunks, c.pwt), (_id(c), p)
        if c.ragged:
            assert p["ragged_segments"] != 0 and p["partial_cout"] != 0, (_id(c), p)
        if c.stride == 2:
            assert p["instance"] in (4, 5, 6), (_id(c), p)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_chunk_seams_are_exact(dev, case):
    from deepi2p_amd import ops
    c = case
    assert ops.conv3x3_x3_supported((B, c.Cin, c.H, c.W), c.Cout, c.stride, cfg=c.cfg), "unsupported: %s" % _id(c)
    L = _layer(c)
    x, scale, shift, res = L["x"].to(dev), L["scale"].to(dev), L["shift"].to(dev), L["residual"].to(dev)
    Wp = ops.bf16x3_pack(_tap_major(L["w"]).to(dev))
    ds = None
    if c.stride == 2:
        ds = (ops.bf16x3_pack(L["wd"].t().contiguous().to(dev)), torch.ones(c.Cout, device=dev), torch.zeros(c.Cout, device=dev))
    for on in (True, False):
        out = ops.conv3x3_x3(x, Wp, c.Cout, scale, shift, c.stride, on, residual=res if on else None, downsample=ds, cfg=c.cfg)
        y, yd = out if c.stride == 2 else (out, None)
        _same(c, y, L["full"] if on else L["plain"], "residual and ReLU %s" % ("on" if on else "off"))
        if yd is not None:
            _same(c, yd, L["refd"].float(), "downsample branch")
