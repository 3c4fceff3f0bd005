"""GPU: di2p_stem_x3 with operands for which the bf16x3 arithmetic, the epilogue, the ReLU and the pool are exact (tests/stem_x3_cases.py): the
pooled output must equal the fp64 evaluation of the same operands BIT FOR BIT.  The kernel max-pools its own convolution, so the pooled
output of random operands shows a convolution pixel only where it wins its window; family D (one tap per output channel, 16 sign phases x 4
orderings of distinct magnitudes) makes every in-image convolution pixel win a window in some frame -- tap offsets, halo zeros, the nine-row
input ring and the padded eighth kx column are pinned at every border pixel.  tests/test_x3_fused_cases_host.py asserts the bounds and that
coverage on the reference alone.  Reference: F.conv2d / F.max_pool2d in fp64 on the CPU, models/resnet.py:137-141,197-201."""
import pytest
import torch

from tests import stem_x3_cases as sc
from tests import x3_exact_cases as xc

pytestmark = pytest.mark.gpu


def _run(dev, L, frames=None):
    from deepi2p_amd import ops
    x = L["x"] if frames is None else L["x"][frames].contiguous()
    return ops.stem_x3(x.to(dev), ops.stem_x3_weights(L["w"].to(dev)), L["scale"].to(dev), L["shift"].to(dev)).cpu()


def _same(H, W, name, got, ref):
    idx = xc.first_mismatch(got, ref)
    assert idx is None, "stem_x3 %dx%d launch %s: %s (got %r, expected %r; %d of %d differ)" % (
        H, W, name, sc.describe(H, W, idx), float(got[idx]), float(ref[idx]), int((got != ref).sum()), ref.numel())
    assert torch.equal(got, ref)


@pytest.mark.parametrize("name", ["A", "B", "C", "D12"])
@pytest.mark.parametrize("shape", sc.SHAPES, ids=sc.shape_id)
def test_dense_families_pooled_equality(dev, shape, name):
    """A: small integers, scale in {0.5, 1, 2}, shifts of both signs; B: wide x (the staging split, products (0,0), (0,1), (0,2)); C: wide w, one
    input channel per frame (the packer, (0,0), (1,0), (2,0)); D12: one tap, two planes on both sides (the (1,1) product)"""
    H, W = shape
    from deepi2p_amd import ops
    assert ops.stem_x3_supported(H, W)
    L = sc.launch(name, H, W)
    _same(H, W, name, _run(dev, L), L["ref"])


@pytest.mark.parametrize("k", sc.D_SETS)
@pytest.mark.parametrize("shape", sc.SHAPES, ids=sc.shape_id)
def test_family_d_every_convolution_pixel_under_the_pool(dev, shape, k):
    """64 frames in which every in-image convolution pixel of weight set k is the positive maximum of some window, and the two all-zero
    cases: all-negative x (frame 64), and all-positive x against the negated weights"""
    H, W = shape
    L = sc.launch("D%d" % k, H, W)
    got = _run(dev, L)
    _same(H, W, "D%d" % k, got, L["ref"])
    assert not bool(got[sc.N_COVER].any())
    Ln = sc.launch("N%d" % k, H, W)
    gotn = _run(dev, Ln)
    _same(H, W, "N%d" % k, gotn, Ln["ref"])
    assert not bool(gotn.any())


def test_a_frame_alone_equals_the_frame_in_its_batch(dev):
    """the cases above are frames of one launch: the kernel is batch independent"""
    H, W = 44, 128
    for name, frames in (("D1", [0, 37, 64]), ("A", [2])):
        L = sc.launch(name, H, W)
        whole = _run(dev, L)
        for f in frames:
            assert torch.equal(_run(dev, L, [f])[0], whole[f]), (name, f)
