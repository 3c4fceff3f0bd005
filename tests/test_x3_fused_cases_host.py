"""CPU: the cases of tests/stem_x3_cases.py and tests/head_x3_cases.py keep the conditions the exact GPU tests of di2p_stem_x3,
di2p_point_head_x3 and di2p_point_head_labels_x3 rest on -- every operand an integer (a multiple of 1/2 behind a scale of 1/2), |scale| * sum
of absolute products + |shift| below 2^24 at EVERY stage, every stage held exactly by fp32 -- and the coverage each family claims: plane
depths, the pool coverage of the stem's family D, the ties of the labels' family A, the index patterns of the table cases.  All of it on the
fp64 references alone, never on a kernel.  The compute-unit count (the two N that depend on it) is the MI355X's 256 here; the GPU tests
assert the same bounds for the device they run on."""
import pytest
import torch
import torch.nn.functional as F

from tests import head_x3_cases as hc
from tests import stem_x3_cases as sc
from tests import x3_exact_cases as xc

CUS = 256


def _grid(t, step=1.0):
    return bool(((t / step) == (t / step).round()).all())


def _held_by_fp32(t):
    return torch.equal(t.float().double(), t.double())


# ------------------------------------------------------------------------------------------------------------------------------- stem

@pytest.mark.parametrize("shape", sc.SHAPES, ids=sc.shape_id)
def test_stem_launches_stay_below_2_to_24(shape):
    H, W = shape
    for name in sc.LAUNCHES:
        L = sc.launch(name, H, W)
        assert _grid(L["x"]) and _grid(L["w"]) and _grid(L["shift"]) and set(L["scale"].tolist()) <= {0.5, 1.0, 2.0}, name
        assert float(L["absum"].max()) < xc.LIMIT, (name, float(L["absum"].max()))
        assert _grid(L["conv"], 0.5) and _held_by_fp32(L["conv"]) and _held_by_fp32(L["ref"]), name
        assert tuple(L["ref"].shape) == (L["x"].shape[0], 64, H // 4, W // 4)
        if name[0] == "N" or name in ("D0", "D1", "D2"):
            assert not bool(L["ref"][-1].any()) and float(L["conv"][-1].abs().max()) > 0, name          # the all-zero frames are zero by the ReLU alone
        else:
            assert float(L["ref"].max()) > 0
    # the launch rule the shape is in the table for
    assert sc.prw(H) == {4: 1, 12: 1, 8: 1, 36: 2, 44: 2, 96: 3, 160: 5}[H] and ((H // 4) % sc.prw(H) != 0) == (H in (36, 44))


@pytest.mark.parametrize("shape", sc.SHAPES, ids=sc.shape_id)
def test_stem_family_properties(shape):
    H, W = shape
    A, B, C, D12 = (sc.launch(n, H, W) for n in ("A", "B", "C", "D12"))
    assert float(A["x"].abs().max()) <= 8 and float(A["w"].abs().max()) <= 2 and float(A["shift"].min()) < 0 < float(A["shift"].max())
    clipped = float((A["conv"] <= 0).double().mean())
    assert 0.2 < clipped < 0.8                                                                        # the ReLU clips regions, not everything
    assert float(B["x"].abs().min()) >= 2 ** 16 and float(B["x"].abs().max()) < 2 ** 18 and bool((B["x"].abs() % 2 == 1).all())
    assert bool((xc.planes(B["x"])[2] != 0).float().mean() >= 0.5)
    assert float(B["w"].abs().max()) == 1 and int((B["w"] != 0).flatten(1).sum(1).max()) <= 63
    assert float(C["w"].abs().min()) >= 2 ** 16 and float(C["w"].abs().max()) < 2 ** 18 and bool((xc.planes(C["w"])[2] != 0).float().mean() >= 0.5)
    for c in range(3):                                                                                # one case per input channel
        assert torch.nonzero(C["x"][c].abs().sum((1, 2))).flatten().tolist() == [c] and float(C["x"][c].abs().max()) == 1
    for t in (D12["x"], D12["w"][D12["w"] != 0]):
        p = xc.planes(t.contiguous())
        assert bool((p[1] != 0).all()) and bool((p[2] == 0).all()) and float(t.min()) < 0 < float(t.max())
    assert {t for k in sc.D_SETS for t in sc.d_taps(k)} == set(range(147))                            # the three sets use all 147 taps
    for k in sc.D_SETS:
        w = sc.d_weights(k)
        assert bool(((w != 0).flatten(1).sum(1) == 1).all()) and float(w.max()) < 2 ** 8 and float(w.min()) == 0
        assert bool((w.flatten(1).sum(1) % 2 == 1).all())
        assert torch.nonzero(w.flatten(1))[:, 1].tolist() == sc.d_taps(k)


@pytest.mark.parametrize("k", sc.D_SETS)
@pytest.mark.parametrize("shape", sc.SHAPES, ids=sc.shape_id)
def test_stem_family_d_shows_every_in_image_convolution_pixel(shape, k):
    """the set of convolution pixels that are the strictly positive maximum of some pool window in some coverage frame is EXACTLY the set of
    pixels whose tap lies inside the image"""
    H, W = shape
    L = sc.launch("D%d" % k, H, W)
    x = L["x"][:sc.N_COVER]
    assert float(x.abs().max()) < 2 ** 16 and bool((x.abs() % 2 == 1).all())
    for f in (0, sc.N_COVER - 1):                                                                     # distinct magnitudes, monotone in raster order
        d = x[f, 0].abs().flatten().diff()
        assert bool((d > 0).all()) or bool((d < 0).all())
    for f, (pr, pc) in enumerate(sc.PHASES):                                                          # positive exactly on the phase
        pos = x[f, 0] > 0
        assert int(pos.sum()) == (H // 4) * (W // 4) and bool(pos[pr::4, pc::4].all())
    act = torch.relu(L["conv"][:sc.N_COVER])
    seen = sc.coverage(act, L["ref"][:sc.N_COVER])
    inside = sc.in_image(k, H, W)
    assert torch.equal(seen, inside), "%d of %d in-image pixels shown, %d outside" % (int((seen & inside).sum()), int(inside.sum()), int((seen & ~inside).sum()))
    assert not bool(inside.all()) and bool(inside.any())                                              # some taps do reach into the padding
    # the slicing reference is the convolution: against F.conv2d in fp64 (a few frames on the large shapes)
    frames = list(range(L["x"].shape[0])) if H * W <= 44 * 128 else [0, 21, 42, 63, 64]
    conv = F.conv2d(L["x"][frames].double(), L["w"].double(), stride=2, padding=3)
    assert torch.equal(conv, L["conv"][frames].double())
    assert torch.equal(F.max_pool2d(torch.relu(conv), 3, 2, 1).float(), L["ref"][frames])


def test_stem_describe_names_the_places():
    text = sc.describe(44, 128, (1, 5, 10, 0))
    assert "border row / column: True" in text and "True / True" in text and "boundary column: False" in text
    assert "boundary column: True" in sc.describe(36, 384, (0, 0, 3, 32)) and "False / False" in sc.describe(96, 128, (0, 0, 4, 5))


# ------------------------------------------------------------------------------------------------------------------------------- head

def _stages_exact(d, what):
    for name, val, bound in d["stages"]:
        assert float(bound.max()) < hc.LIMIT, (what, name, float(bound.max()))
        assert _grid(val) and _held_by_fp32(val), (what, name)


def _head_n(c):
    return c[1] if c[1] else hc.head_big_n(CUS)


@pytest.mark.parametrize("config", hc.HEAD_CONFIGS, ids=hc.head_config_id)
def test_head_cases_stay_below_2_to_24_at_every_layer(config):
    B, _, P, nodes = config
    N = _head_n(config)
    for family in hc.HEAD_FAMILIES:
        d = hc.head_case(family, B, N, P, nodes)
        what = (family, config)
        _stages_exact(d, what)
        ops = [d[k] for k in ("first", "second", "W0", "W1", "sc0", "sh0", "sc1", "sh1", "Ga", "Gb")] + [w for w, _ in d["tails"]]
        assert all(_grid(t) for t in ops), what
        assert set(d["sc0"].tolist()) | set(d["sc1"].tolist()) <= {1.0, 2.0}
        y0, y1 = d["stages"][0][1], d["stages"][1][1]
        if family[0] == "B":
            # layer 1's operand is three planes deep: at least half its values have a non-zero third plane
            assert bool((xc.planes(y0.float())[2] != 0).float().mean() >= 0.5), what
            assert int((d["W1"] != 0).sum(0).max()) <= 31 and float(d["W1"].abs().max()) == 1
            assert bool(((d["W0"] != 0).sum(0) == 1).all()) and set(torch.nonzero(d["W0"])[:, 0].tolist()) == set(range(96))
            if family == "B" and B * N >= 8:
                assert bool((y0 == 0).any())                                                           # the ReLU clips the negative rows
        if family == "C0":
            x = torch.cat((d["first"], d["second"]), 1)
            used = torch.nonzero(x.abs().sum((0, 2))).flatten().tolist()
            assert len(used) <= 63 and (B * N < 16 or {8, 15, 95} <= set(used)) and float(d["W0"].abs().min()) >= 2 ** 16
        if family == "C1":
            used = torch.nonzero(y0.abs().sum((0, 2))).flatten().tolist()
            assert len(used) <= 63 and (B * N < 16 or {8, 15, 127} <= set(used)) and float(y0.abs().max()) <= 1 and float(d["W1"].abs().min()) >= 2 ** 16
        if family in ("D0", "D1"):
            W, act = (d["W0"], torch.cat((d["first"], d["second"]), 1)) if family == "D0" else (d["W1"], y0.float())
            assert bool(((W != 0).sum(0) == 1).all())
            for t in (W[W != 0], act[act != 0]):
                p = xc.planes(t.contiguous())
                assert bool((p[1] != 0).all()) and bool((p[2] == 0).all())
        if family in ("T", "Tw"):
            assert float(d["Ga"].abs().max()) > 2 ** 17 and float(d["Ga"].abs().max()) <= 2 ** 18
            for idx, n in ((d["ia"], nodes[0]), (d["ib"], nodes[1])):
                flat = idx.reshape(-1, 3)
                assert int(idx.min()) == 0 and int(idx.max()) == n - 1
                assert bool(((flat[:, 0] == flat[:, 1]) & (flat[:, 1] == flat[:, 2])).any())
                if 3 * N >= 2 * n:
                    assert set(idx.flatten().tolist()) == set(range(n)), what                         # every node is used
            if family == "Tw":
                assert set(d["wa"].flatten().tolist()) <= {1.0, 2.0, 4.0} and d["wb"] is not None
            else:
                assert d["wa"] is None and d["wb"] is None
        if len(d["tails"]) > 1:
            # the one-hot output layers of the case show every row of layer 1 (four of them at the big N)
            rows = set(torch.cat([torch.nonzero(w)[:, 0] for w, _ in d["tails"]]).tolist())
            assert rows == set(range(128)) or (N > 4096 and len(rows) == 4 * P)
        assert float(y1.abs().max()) > 0


def test_head_launch_rule_of_the_chosen_sizes():
    """N = 1000 with B = 3: parts = 2, two trips per wave; the big N: waves with unequal trip counts on both paths (head_big_n)"""
    assert hc.head_trips(3, 1000, CUS, 1) == (2, 2) and hc.head_trips(3, 1000, CUS, 2)[1] >= 2
    for cus in (CUS, 304, 64):
        N = hc.head_big_n(cus)
        assert N % 32 != 0
        for tab in (0, 1, 2):
            lo, hi = hc.head_trips(1, N, cus, tab)
            assert hi >= 2 and lo < hi, (cus, tab, lo, hi)
    # 302 nodes fit the 160 KB test of the LDS path, 303 do not (8 * 128 floats + nodes * 132 floats)
    assert (8 * 128 + 302 * 132) * 4 <= 160 * 1024 < (8 * 128 + 303 * 132) * 4


# ----------------------------------------------------------------------------------------------------------------------------- labels

def _labels_n(c):
    return c[1] if c[1] else hc.labels_big_n(CUS)


@pytest.mark.parametrize("config", hc.LABEL_CONFIGS, ids=hc.labels_config_id)
def test_labels_cases_stay_below_2_to_24_and_family_a_ties(config):
    B, _, P = config
    N = _labels_n(config)
    for family in hc.LABEL_FAMILIES:
        d = hc.labels_case(family, B, N, P)
        what = (family, config)
        _stages_exact(d, what)
        assert all(_grid(t) for t in [d["y0"], d["W1"], d["sc1"], d["sh1"]] + [t[0] for t in d["tails"]]), what
        y1 = d["stages"][0][1]
        if family[0] == "A":
            tiles, halves, coarse = hc.tie_span(d["stages"][1][1])
            assert coarse > 0, what
            lab = set(d["tails"][0][2].flatten().tolist())
            # A-: two identical coarse channels, every point a tie; A: ties, and both labels by a strict comparison
            assert lab == {0} if family == "A-" else (B * N < 8 or lab == {0, 1}), what
            if family == "A":
                s = d["stages"][1][1]
                assert B * N < 8 or (bool((s[:, 0] > s[:, 1]).any()) and bool((s[:, 1] > s[:, 0]).any())), what
            if P > 32:
                # ties of the fine maximum that span two row tiles, and the two half-wave row groups
                assert tiles > 0 and halves > 0, what
        if family[0] == "B":
            assert bool((xc.planes(d["y0"])[2] != 0).float().mean() >= 0.5) and int((d["W1"] != 0).sum(0).max()) <= 31
        if family == "C1":
            used = torch.nonzero(d["y0"].abs().sum((0, 2))).flatten().tolist()
            assert len(used) <= 63 and (B * N < 16 or {8, 15, 255} <= set(used)) and float(d["W1"].abs().min()) >= 2 ** 16
        if family == "C2":
            used = torch.nonzero(y1.abs().sum((0, 2))).flatten().tolist()
            assert len(used) <= 63 and float(y1.abs().max()) <= 1 and float(d["tails"][0][0].abs().min()) >= 2 ** 16
        if family == "E":
            assert bool((xc.planes(y1.float())[2] != 0).float().mean() >= 0.5)                        # a wide y1 reaches layer 2
            assert int((d["tails"][0][0] != 0).sum(0).max()) <= 31
        if len(d["tails"]) > 1:
            rows = set(torch.cat([torch.nonzero(t[0])[:, 0] for t in d["tails"]]).tolist())
            assert rows == set(range(256)), what                                                       # the selections show every row of layer 1
        for _, s, coarse_lab, fine_lab in d["tails"][:2]:
            # the first-maximum scan against torch's argmax on the same fp64 values where the maximum is unique
            for lab, part in ((coarse_lab, s[:, 0:2]), (fine_lab, s[:, 2:])):
                top = part.max(1, keepdim=True).values
                unique = (part == top).sum(1) == 1
                assert torch.equal(lab[unique].long(), part.argmax(1)[unique])
                assert bool((torch.gather(part, 1, lab.long().unsqueeze(1)) == top).all())
                first = (part == top).float().argmax(1)                                               # the first channel that attains it
                assert torch.equal(lab.long(), first)


def test_labels_launch_rule_of_the_chosen_sizes():
    N = hc.labels_big_n(CUS)
    tiles = -(-N // 64)
    assert tiles == CUS + 3 and N % 64 != 0                # three workgroups loop twice, the others once
    assert [(P + 31) // 32 for P in (3, 33, 128, 129, 290)] == [1, 2, 4, 5, 10]
