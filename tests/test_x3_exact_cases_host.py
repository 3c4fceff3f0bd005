"""CPU: the operand families of tests/x3_exact_cases.py keep the condition their exactness rests on, for every family and every shape the GPU
tests use: all operands are integers, and the sum of ABSOLUTE products of every output is below 2^24 -- so every partial sum of every
accumulator, in any order and blocking and for any subset of the six split products, is an integer below 2^24 and the bf16 matrix
instructions drop nothing.  Checked on the fp64 reference alone, never on a kernel."""
import pytest
import torch

from tests import conv_x3_cases as cx
from tests import pointwise_x3_cases as pw
from tests import x3_exact_cases as xc


def _integers(*ts):
    return all(bool((t == t.round()).all()) for t in ts)


def _exact(ref, absum):
    """the reference is an integer tensor that fp32 holds exactly, and no partial sum can leave 2^24"""
    return float(absum.max()) < xc.LIMIT and _integers(ref) and torch.equal(ref.float().double(), ref)


def test_the_split_of_an_integer_is_three_integers_of_its_sign():
    v = xc.activations("B", (4, 8, 64), 1)
    p0, p1, p2 = xc.planes(v)
    assert torch.equal((p0 + p1) + p2, v) and _integers(p0, p1, p2)
    for p in (p0, p1, p2):
        assert bool((p * v >= 0).all())                                        # |p0| + |p1| + |p2| == |v|: absolute products bound the split products
        assert torch.equal((p.view(torch.int32) & 0xffff), torch.zeros_like(p, dtype=torch.int32))      # each is a bf16
    assert bool((p2 != 0).float().mean() >= 0.5)
    d0, d1, d2 = xc.planes(xc.activations("D", (2, 8, 32), 2))
    assert bool((d1 != 0).all()) and bool((d2 == 0).all())                     # family D: exactly two planes


@pytest.mark.parametrize("family", xc.FAMILIES)
def test_family_properties(family):
    Cin, Cout = 48, 72
    w = xc.weights(family, Cout, (Cin, 3, 3), 5)
    x = xc.activations(family, (2, Cin, 5, 32), 6)
    assert _integers(w, x) and torch.equal(w, xc.weights(family, Cout, (Cin, 3, 3), 5))          # seeded
    if family == "A":
        assert float(x.abs().max()) <= 8 and float(w.abs().max()) <= 2
        s, h, r = xc.epilogue(Cout, (2, Cout, 5, 32), 7)
        assert set(s.tolist()) <= {0.5, 1.0, 2.0} and float(h.abs().max()) <= 4 and float(r.abs().max()) <= 16 and _integers(h, r)
    if family == "B":
        assert bool((x.abs() % 2 == 1).all()) and float(x.abs().max()) < 2 ** 18
        assert float(w.abs().max()) == 1 and int((w != 0).flatten(1).sum(1).max()) <= 63
    if family == "C":
        assert bool((w.abs() % 2 == 1).all()) and float(w.abs().max()) < 2 ** 18 and float(x.abs().max()) == 1
        used = torch.nonzero(x.abs().sum((0, 2, 3))).flatten().tolist()
        assert len(used) <= 7 and {8, 15, Cin - 1} <= set(used)
        xp = xc.activations("C", (2, 160, 64), 6, max_channels=63)
        used = torch.nonzero(xp.abs().sum((0, 2))).flatten().tolist()
        assert len(used) <= 63 and {8, 15, 159} <= set(used)
    if family == "D":
        nz = torch.nonzero(w.flatten(1))
        assert nz.shape[0] == Cout and float(w.abs().max()) < 2 ** 12 and float(x.abs().max()) < 2 ** 12
        assert bool((x.abs() % 2 == 1).all()) and bool((w.flatten(1).abs().sum(1) % 2 == 1).all())
        taps, chans = (nz[:, 1] % 9).tolist(), (nz[:, 1] // 9).tolist()
        assert taps[:9] == list(range(9)) and chans[:3] == [0, 7, 14] and set(chans) == set(range(Cin))


@pytest.mark.parametrize("case", cx.CASES, ids=cx.case_id)
def test_conv_cases_stay_below_2_to_24(case):
    for family in xc.FAMILIES:
        L = xc.conv_layer(family, cx.B, case.Cin, case.H, case.W, case.Cout, case.stride)
        assert _integers(L["x"], L["w"]) and _exact(L["ref"], L["absum"]), (family, float(L["absum"].max()))
        assert float(L["ref"].abs().max()) > 0
        if case.stride == 2:
            assert _integers(L["wd"]) and _exact(L["refd"], L["absumd"]), family
        if family == "A":
            # the epilogue of an integer accumulator: halves at most, far below 2^24
            full = L["ref"] * L["scale"].double().view(1, -1, 1, 1) + L["shift"].double().view(1, -1, 1, 1) + L["residual"].double()
            assert torch.equal(full.float().double(), full) and float(full.abs().max()) < 2 ** 20
        if family == "D":
            # the output is a scaled copy of one shifted input channel: at most one term per output
            assert float((L["absum"] - L["ref"].abs()).abs().max()) == 0


@pytest.mark.parametrize("case", pw.SOURCE_CASES, ids=pw.source_id)
def test_pointwise_source_cases_stay_below_2_to_24(case):
    (K, M, N), kind = case
    for family in xc.FAMILIES:
        c = pw.source_case(family, K, M, N, kind)
        assert c["full"].shape == (pw.B, K, N) and sum(p[1].shape[1] for p in c["parts"]) == K
        assert _integers(c["w"], c["full"]) and _exact(c["ref"], c["absum"]), (family, float(c["absum"].max()))


def test_pointwise_epilogue_and_planes_cases_are_exact_in_fp32():
    for (K, M, N), kind in pw.EPILOGUE_CASES:
        c = pw.epilogue_case(K, M, N, kind)
        assert float(c["absum"].max()) < xc.LIMIT
        for r in (c["ref"] if isinstance(c["ref"], tuple) else (c["ref"],)):
            assert torch.equal(r.float().double(), r), kind                      # every stage is a multiple of 1/8 far below 2^24
    for family in pw.PLANES["families"]:
        for M2 in pw.PLANES["M2"]:
            c = pw.planes_case(family, M2)
            assert _exact(c["ref1"], c["absum1"]) and _exact(c["ref2"], c["absum2"]), (family, M2)
            if family == "B":
                assert bool((xc.planes(c["ref1"].float())[2] != 0).float().mean() >= 0.5)       # the planes handed over are three deep
