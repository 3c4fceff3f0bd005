"""GPU: di2p_conv3x3_x3 on EVERY kernel instance (tests/conv_x3_cases.py) with operands for which the bf16x3 arithmetic is exact
(tests/x3_exact_cases.py): the output must equal the fp64 convolution of the same operands BIT FOR BIT -- which of the six split products is
issued, which plane a fragment holds, halo and zero padding, the stride-2 parity de-interleave, the dump entry of surplus staging items and
the dropped stores past the frame and past Cout are each pinned, on each instance, where a statistical bound would let a lost low-order bit
at one tile edge pass.  Reference: F.conv2d in fp64 on the CPU (exact: everything stays below 2^53), models/resnet.py:56-72,160-164."""
import pytest
import torch
import torch.nn.functional as F

from tests import conv_x3_cases as cx
from tests import x3_exact_cases as xc

pytestmark = pytest.mark.gpu


def _tap_major(w):
    return w.permute(2, 3, 1, 0).reshape(-1, w.shape[0]).contiguous()


def _same(case, got, ref, what):
    """torch.equal, and on a mismatch where the first differing element lies"""
    got = got.cpu()
    ref = ref.float()
    idx = xc.first_mismatch(got, ref)
    assert idx is None, "%s %s: %s (got %r, expected %r; %d of %d differ)" % (
        cx.case_id(case), what, cx.describe(case, idx), float(got[idx]), float(ref[idx]), int((got != ref).sum()), ref.numel())
    assert torch.equal(got, ref)


def _run(ops, dev, case, L, Wp, scale, shift, relu, residual=None, wd=None):
    """one launch in the case's configuration; stride 2 with the fused downsample branch (scale 1, shift 0) -> (y, y_ds | None)"""
    x = L["x"].to(dev)
    if case.stride == 1:
        return ops.conv3x3_x3(x, Wp, case.Cout, scale, shift, 1, relu, residual=residual, cfg=case.cfg), None
    one, zero = torch.ones(case.Cout, device=dev), torch.zeros(case.Cout, device=dev)
    return ops.conv3x3_x3(x, Wp, case.Cout, scale, shift, 2, relu, residual=residual, downsample=(ops.bf16x3_pack(wd.t().contiguous().to(dev)), one, zero),
                          cfg=case.cfg)


@pytest.mark.parametrize("case", cx.CASES, ids=cx.case_id)
def test_plan_names_the_expected_instance_on_this_device(dev, case):
    """the table was made for 256 compute units; the tests below cover the instances only if the device's own plan agrees"""
    from deepi2p_amd import ops
    p = ops.conv3x3_x3_plan((cx.B, case.Cin, case.H, case.W), case.Cout, case.stride, cfg=case.cfg)
    assert p is not None and (p["instance"], p["fallback"], p["cfg"]) == (case.instance, case.fallback, case.cfg), p
    assert cx.plan_flags(p, case) == set(case.flags), p


@pytest.mark.parametrize("case", cx.CASES, ids=cx.case_id)
def test_family_a_small_integers_and_the_whole_epilogue(dev, case):
    from deepi2p_amd import ops
    L = xc.conv_layer("A", cx.B, case.Cin, case.H, case.W, case.Cout, case.stride)
    Wp = ops.bf16x3_pack(_tap_major(L["w"]).to(dev))
    scale, shift, res = L["scale"], L["shift"], L["residual"]
    lin = L["ref"] * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
    for with_res in (False, True):
        for relu in (False, True):
            full = lin + res.double() if with_res else lin
            y, yd = _run(ops, dev, case, L, Wp, scale.to(dev), shift.to(dev), relu, residual=res.to(dev) if with_res else None, wd=L.get("wd"))
            _same(case, y, torch.relu(full) if relu else full, "family A (residual %s, relu %s)" % (with_res, relu))
            if yd is not None:
                _same(case, yd, L["refd"], "family A, downsample branch")


@pytest.mark.parametrize("family", ["B", "C", "D"])
@pytest.mark.parametrize("case", cx.CASES, ids=cx.case_id)
def test_wide_families_pin_the_six_products(dev, case, family):
    """B: products (0,0), (0,1), (0,2) and the staging split; C: (0,0), (1,0), (2,0), the packers and the A-fragment loads; D: (1,1), (0,1),
    (1,0), (0,0) on one term per output -- a scaled copy of one shifted input channel: tap offsets, halo zeros, the parity layout."""
    from deepi2p_amd import ops
    L = xc.conv_layer(family, cx.B, case.Cin, case.H, case.W, case.Cout, case.stride)
    one, zero = torch.ones(case.Cout, device=dev), torch.zeros(case.Cout, device=dev)
    packs = [("bf16x3_pack", ops.bf16x3_pack(_tap_major(L["w"]).to(dev)))]
    if family in "CD":
        # straight from the filter bank: the fast path (Cin % 32 == 0) or the general one, under an exact consumer
        packs.append(("bf16x3_pack_conv3x3", ops.bf16x3_pack_conv3x3(L["w"].to(dev))))
        assert torch.equal(packs[0][1], packs[1][1]), "the two packers disagree"
    for name, Wp in packs:
        y, yd = _run(ops, dev, case, L, Wp, one, zero, False, wd=L.get("wd"))
        _same(case, y, L["ref"], "family %s (%s)" % (family, name))
        if yd is not None:
            _same(case, yd, L["refd"], "family %s, downsample branch" % family)


@pytest.mark.parametrize("case", cx.CASES, ids=cx.case_id)
def test_a_frame_does_not_depend_on_its_batch_or_the_run(dev, case):
    """cx_plan prices every layer for the nominal step whatever B is: a frame computed alone equals the same frame inside B = 3 bit for
    bit, with integer operands (family A) and with random normal ones; two runs of the same call are bit-identical."""
    from deepi2p_amd import ops
    g = torch.Generator().manual_seed(xc.seed_of("batch", tuple(case[:9])))
    xa = xc.activations("A", (3, case.Cin, case.H, case.W), xc.seed_of("xa", tuple(case[:9])))
    wa = xc.weights("A", case.Cout, (case.Cin, 3, 3), xc.seed_of("wa", tuple(case[:9])))
    xn = torch.randn(3, case.Cin, case.H, case.W, generator=g)
    wn = torch.randn(case.Cout, case.Cin, 3, 3, generator=g) / (9 * case.Cin) ** 0.5
    wdn = torch.randn(case.Cout, case.Cin, generator=g) / case.Cin ** 0.5
    scale, shift = (torch.rand(case.Cout, generator=g) + 0.5).to(dev), torch.randn(case.Cout, generator=g).to(dev)
    for x, w in ((xa, wa), (xn, wn)):
        Wp = ops.bf16x3_pack(_tap_major(w).to(dev))
        Wpd = ops.bf16x3_pack(wdn.t().contiguous().to(dev)) if case.stride == 2 else None
        xd = x.to(dev)

        def run(frames):
            if case.stride == 1:
                return (ops.conv3x3_x3(frames, Wp, case.Cout, scale, shift, 1, True, cfg=case.cfg),)
            return ops.conv3x3_x3(frames, Wp, case.Cout, scale, shift, 2, True, downsample=(Wpd, scale, shift), cfg=case.cfg)
        whole, again = run(xd), run(xd)
        for u, v in zip(whole, again):
            assert torch.equal(u, v), "two runs of the same call differ"
        for b in (0, 2):
            for u, v in zip(run(xd[b:b + 1].contiguous()), whole):
                assert torch.equal(u[0], v[b]), "frame %d alone differs from the same frame in a batch of 3" % b


def test_conv3x3_x3_all_four_configurations_agree(dev):
    """The four tile configurations are four blockings of the same sums: each, on a layer of the table that runs on it, inside the bound of
    test_conv3x3_x3_every_configuration_agrees on random normal operands -- and where two configurations can run the same layer, equal
    up to the order of fp32 additions.  All four must run."""
    from deepi2p_amd import ops
    ran = set()
    for cfg in range(4):
        case = next(c for c in cx.CASES if c.cfg == cfg and c.kind == "pipelined" and c.stride == 1)
        g = torch.Generator().manual_seed(3 + cfg)
        x = torch.randn(cx.B, case.Cin, case.H, case.W, generator=g)
        w = torch.randn(case.Cout, case.Cin, 3, 3, generator=g) / (9 * case.Cin) ** 0.5
        ref = F.conv2d(x.double(), w.double(), padding=1)
        tol = 3e-6 * (9 * case.Cin) ** 0.5 * float(ref.abs().max()) + 1e-6
        Wp = ops.bf16x3_pack(_tap_major(w).to(dev))
        one, zero = torch.ones(case.Cout, device=dev), torch.zeros(case.Cout, device=dev)
        for other in range(4):
            if not ops.conv3x3_x3_supported(x.shape, case.Cout, 1, cfg=other):
                continue
            y = ops.conv3x3_x3(x.to(dev), Wp, case.Cout, one, zero, 1, False, cfg=other).cpu()
            assert float((y.double() - ref).abs().max()) <= tol, (cfg, other)
            ran.add(other)
        assert cfg in ran
    assert ran == {0, 1, 2, 3}
