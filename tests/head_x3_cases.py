"""Operands for which di2p_point_head_x3 (three layers in registers) and di2p_point_head_labels_x3 (two layers and both argmaxes) are EXACT: the
premise of tests/x3_exact_cases.py carried through chained layers -- all operands integers, the sum of absolute products of EVERY layer,
times |scale| plus |shift|, below 2^24 -- so the matrix instructions, the fp32 fma chains of the gathered node rows and of head_x3's output
layer, ReLU and max drop nothing in any order, and every stage equals its fp64 evaluation bit for bit.  Generators only: seeded, CPU, no GPU code.

A case is a dict of operands (the keyword names of the tests' _run helpers) and `stages`: [(name, fp64 value, bound)] for every layer, where
bound = |scale| * sum |x||w| + |shift| per output.  Callers must not write to what they get.

Families (head: W0t f32[96,128], W1t f32[128,128], W2t f32[128,P]; labels: W1t f32[256,256], W2t f32[256,P]; "selection" = one +-1 per
output row, cycling over the inputs; "one-hot" = selection without the sign):
  A / A-   small integers everywhere: x in [-8, 8], weights in [-2, 2] (labels: [-3, 3] in one coarse column), hidden scales in {1, 2}, integer
           shifts; ReLU on / off
  B / B-   first layer a selection against wide x (odd, 2^16 <= |x| < 2^18): its output is a copy three planes deep; the next layer in
           {-1, 0, 1} with at most 31 non-zeros per row; head: the last layer one-hot.  B: ReLU on, x positive and one selection row in eight
           negative (so that more than half the copy survives); B-: ReLU off, both signs
  C0/C1 (head), C1/C2 (labels)   that layer wide and dense (odd, 2^16 <= |w| < 2^18) against activations in {-1, 0, 1}, non-zero in at most
           63 channels, among them the first and last of a group of 8 and the last channel; the other layers selections
  D0/D1 (head), D1/D2 (labels)   that layer one term per output with two planes on both sides (odd, 2^8 <= |.| < 2^12); the others selections
  T / Tw   (head) integer node tables up to 2^18, interpolation weights absent / powers of two in {1, 2, 4}; index patterns: node 0, the last
           node, all three neighbours equal, every node used where 3 N >= nodes
  E        (labels) wide y0 through a selection W1: a wide y1 against W2 in {-1, 0, 1} with at most 31 non-zeros per row
"""
import functools

import torch

from tests import x3_exact_cases as xc

LIMIT = xc.LIMIT


def _ints(lo, hi, shape, g):
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).float()


def selection(K, M, g, signed=True, rows=None, negative_every=0, offset=0):
    """Wt f32[K,M]: output row m reads input (m + offset) mod K (rows: only these output rows are non-zero) with a random sign, or a negative
    one in every `negative_every`-th row"""
    w = torch.zeros(K, M)
    sign = torch.randint(0, 2, (M,), generator=g) * 2 - 1 if signed else torch.ones(M)
    if negative_every:
        sign = torch.where(torch.arange(M) % negative_every == negative_every - 1, -1, 1)
    for m in (range(M) if rows is None else rows):
        w[(m + offset) % K, m] = float(sign[m])
    return w


def sparse_pm1(K, M, g, nnz=31):
    return xc.weights("B", M, (K,), int(torch.randint(0, 2 ** 31, (1,), generator=g)), nnz=nnz).t().contiguous()


def wide(K, M, g):
    return xc._odd((K, M), 18, g, low_bits=16)


def one_term(K, M, g):
    """one odd weight with 2^8 <= |w| < 2^12 per output row, walking the inputs with stride 7"""
    w = torch.zeros(K, M)
    w[(7 * torch.arange(M)) % K, torch.arange(M)] = xc._odd((M,), 12, g, low_bits=8)
    return w


def sparse_activations(shape, g, max_channels=63):
    """f32[B,C,N] in {-1, 0, 1}, non-zero in at most max_channels channels (xc.c_channels)"""
    x = torch.zeros(shape)
    ch = xc.c_channels(shape[1], max_channels, int(torch.randint(0, 2 ** 31, (1,), generator=g)))
    x[:, ch] = _ints(-1, 1, (shape[0], len(ch), shape[2]), g)
    return x, ch


def _layer(Wt, x, scale=None, shift=None, relu=False, extra=None, extra_abs=None):
    """(y fp64, bound fp64) of y = relu?(scale * (Wt^T x + extra) + shift), x fp64[B,K,N]"""
    z = torch.einsum("km,bkn->bmn", Wt.double(), x)
    a = torch.einsum("km,bkn->bmn", Wt.double().abs(), x.abs())
    if extra is not None:
        z, a = z + extra, a + extra_abs
    if scale is not None:
        z, a = z * scale.double().view(1, -1, 1), a * scale.double().abs().view(1, -1, 1)
    if shift is not None:
        z, a = z + shift.double().view(1, -1, 1), a + shift.double().abs().view(1, -1, 1)
    return (torch.relu(z) if relu else z), a


# ---------------------------------------------------------------------------------------------------------------- di2p_point_head_x3

HEAD_FAMILIES = ("A", "A-", "B", "B-", "C0", "C1", "D0", "D1", "T", "Tw")
# (B, N, P, nodes): N = 1000 is two trips per wave with parts > 1; 302 nodes are the last pair that fits the 160 KB LDS test, (152, 151) the
# first that takes the memory path by itself; N = None: head_big_n(compute units)
HEAD_CONFIGS = [(1, 1, 1, (1, 1)), (3, 31, 2, (16, 16)), (1, 32, 4, (128, 128)), (3, 33, 1, (151, 151)), (3, 1000, 2, (128, 128)),
                (1, 1000, 4, (152, 151)), (3, 1000, 4, (151, 151)), (1, None, 2, (16, 16))]


def head_big_n(cus):
    """B = 1: 4 cus + 5 blocks of 32 points, the last one ragged.  Memory path (grid = cus workgroups of 4 waves, stride 4 cus): five waves take
    two trips, the others one.  Tables in LDS (parts = cus / 4 at most): every wave takes several trips, of unequal number, and the frame's
    last block is a wave's LAST trip but not its first -- the block the prefetch index min(g + g_stride, g_end - 1) reaches exactly."""
    return 32 * (4 * cus + 5) - 7


def head_trips(B, N, cus, tab):
    """(min, max) trips per wave under the launch rule of di2p_point_head_x3 (tab: the head_x3_tab knob), and whether the tables are in LDS"""
    nblk = -(-N // 32)
    total = B * nblk
    def trips(first, stride, end):
        return len(range(first, end, stride))
    if tab == 0:
        grid = -(-total // 4) if total // 4 < cus else cus
        t = [trips(w, grid * 4, total) for w in range(grid * 4)]
    else:
        parts = -(-cus // B)
        while parts > 1 and nblk < parts * 16:
            parts -= 1
        nw = 4 if tab == 2 else 8
        t = [trips(w, parts * nw, nblk) for w in range(parts * nw)]
    return min(t), max(t)


def head_config_id(c):
    return "B%d-N%s-P%d-%dx%d" % (c[0], c[1] if c[1] else "big", c[2], c[3][0], c[3][1])


def _indices(B, N, nodes):
    """idx i32[B,N,3]: neighbour j of point n is node (3 n + j) mod nodes (every node where 3 N >= nodes); every seventh point has all three
    equal, another seventh (0, last, 0)"""
    n = torch.arange(N).view(1, N, 1)
    idx = (3 * n + torch.arange(3).view(1, 1, 3) + torch.arange(B).view(B, 1, 1)) % nodes
    same = (n % nodes).expand(B, N, 3)
    ends = torch.tensor([0, nodes - 1, 0]).view(1, 1, 3).expand(B, N, 3)
    idx = torch.where(n % 7 == 3, same, idx)
    idx = torch.where(n % 7 == 5, ends, idx)
    return idx.to(torch.int32).contiguous()


@functools.lru_cache(maxsize=8)
def head_case(family, B, N, P, nodes):
    g = xc._gen(xc.seed_of("head", family, B, N, P, nodes))
    one, zero = torch.ones(128), torch.zeros(128)
    d = {"sc0": one, "sh0": zero, "sc1": one, "sh1": zero, "sc2": None, "sh2": None, "relu0": True, "relu1": True, "relu2": False,
         "Ga": torch.zeros(B, nodes[0], 128), "Gb": torch.zeros(B, nodes[1], 128), "ia": _indices(B, N, nodes[0]), "ib": _indices(B, N, nodes[1]),
         "wa": None, "wb": None}
    x = None
    # a one-hot output layer shows P of layer 1's 128 rows: the case carries a list of them that shows every row (four of them at the big N)
    hots = [selection(128, P, g, signed=False, offset=o) for o in range(0, 128, P)][:4 if N > 4096 else None]
    hot = hots[0]
    if family in ("A", "A-"):
        x = _ints(-8, 8, (B, 96, N), g)
        d.update(W0=_ints(-2, 2, (96, 128), g), W1=_ints(-2, 2, (128, 128), g), W2=_ints(-2, 2, (128, P), g),
                 sc0=_ints(1, 2, (128,), g), sh0=_ints(-4, 4, (128,), g), sc1=_ints(1, 2, (128,), g), sh1=_ints(-64, 64, (128,), g),
                 sc2=_ints(1, 2, (P,), g), sh2=_ints(-64, 64, (P,), g), Ga=_ints(-8, 8, (B, nodes[0], 128), g), Gb=_ints(-8, 8, (B, nodes[1], 128), g),
                 wa=_ints(1, 2, (B, N, 3), g), relu0=family == "A", relu1=family == "A", relu2=family == "A")
    elif family in ("B", "B-"):
        x = xc._odd((B, 96, N), 18, g, low_bits=16)
        on = family == "B"
        d.update(W0=selection(96, 128, g, negative_every=8 if on else 0), W1=sparse_pm1(128, 128, g), W2=hot, relu0=on, relu1=on)
        if on:
            x = x.abs()
    elif family == "C0":
        x, _ = sparse_activations((B, 96, N), g)
        d.update(W0=wide(96, 128, g), W1=selection(128, 128, g), W2=hot)
    elif family == "C1":
        rows = xc.c_channels(128, 63, xc.seed_of("rows", B, N))
        x = _ints(-1, 1, (B, 96, N), g)
        d.update(W0=selection(96, 128, g, rows=rows), W1=wide(128, 128, g), W2=hot, relu0=False)
    elif family == "D0":
        x = xc._odd((B, 96, N), 12, g, low_bits=8)
        d.update(W0=one_term(96, 128, g), W1=selection(128, 128, g), W2=hot, relu0=False, relu1=False)
    elif family == "D1":
        x = xc._odd((B, 96, N), 12, g, low_bits=8)
        d.update(W0=selection(96, 128, g), W1=one_term(128, 128, g), W2=hot, relu0=False, relu1=False)
    elif family in ("T", "Tw"):
        x = _ints(-8, 8, (B, 96, N), g)
        d.update(W0=_ints(-2, 2, (96, 128), g), W1=selection(128, 128, g), W2=hot, relu0=False,
                 Ga=_ints(-2 ** 18, 2 ** 18, (B, nodes[0], 128), g), Gb=_ints(-2 ** 18, 2 ** 18, (B, nodes[1], 128), g))
        if family == "Tw":
            d.update(wa=2.0 ** _ints(0, 2, (B, N, 3), g), wb=2.0 ** _ints(0, 2, (B, N, 3), g))
    else:
        raise ValueError(family)
    d["first"], d["second"] = x[:, :32].contiguous(), x[:, 32:].contiguous()
    # ---- fp64 reference of every stage
    t = torch.zeros(B, 128, N, dtype=torch.float64)
    ta = torch.zeros(B, 128, N, dtype=torch.float64)
    for G, idx, w in ((d["Ga"], d["ia"], d["wa"]), (d["Gb"], d["ib"], d["wb"])):
        rows = torch.gather(G.double(), 1, idx.long().reshape(B, N * 3, 1).expand(B, N * 3, 128)).reshape(B, N, 3, 128)
        ww = (w.double() if w is not None else torch.ones(B, N, 3, dtype=torch.float64)).unsqueeze(3)
        t += (rows * ww).sum(2).transpose(1, 2)
        ta += (rows.abs() * ww.abs()).sum(2).transpose(1, 2)
    y0, b0 = _layer(d["W0"], x.double(), d["sc0"], d["sh0"], d["relu0"], extra=t, extra_abs=ta)
    y1, b1 = _layer(d["W1"], y0, d["sc1"], d["sh1"], d["relu1"])
    d["stages"] = [("y0", y0, b0), ("y1", y1, b1)]
    d["tails"] = []                                # [(W2, fp32 reference)]: the output layers this case runs with
    for W2 in (hots if d["W2"] is hot else [d["W2"]]):
        out, b2 = _layer(W2, y1, d["sc2"], d["sh2"], d["relu2"])
        d["stages"].append(("out", out, b2))
        d["tails"].append((W2, out.float()))
    return d


# ------------------------------------------------------------------------------------------------------ di2p_point_head_labels_x3

LABEL_FAMILIES = ("A", "A-", "B", "B-", "C1", "C2", "D1", "D2", "E")
# (B, N, P): P = 33: 2 row tiles (CT2 = 1); 128: 4 row tiles, the last P with CT2 = 1; 129: 5 row tiles (CT2 = 2); 290: 10 row tiles, two units
# for two of the eight waves; N = None: labels_big_n(compute units)
LABEL_CONFIGS = [(1, 1, 3), (3, 63, 33), (1, 64, 128), (3, 65, 129), (1, 200, 290), (3, 200, 33), (3, 1, 129), (1, None, 33)]


def labels_big_n(cus):
    """B = 1: cus + 3 tiles of 64 points, the last one ragged: three workgroups loop twice, the others once"""
    return 64 * (cus + 3) - 5


def labels_config_id(c):
    return "B%d-N%s-P%d" % (c[0], c[1] if c[1] else "big", c[2])


def first_maximum(s):
    """channel-by-channel scan with a strict comparison over dim 1 of s[B,C,N] -> i32[B,N]: the first maximum wins"""
    best, lab = s[:, 0].clone(), torch.zeros(s.shape[0], s.shape[2], dtype=torch.int32)
    for c in range(1, s.shape[1]):
        up = s[:, c] > best
        best = torch.where(up, s[:, c], best)
        lab = torch.where(up, torch.full_like(lab, c), lab)
    return lab


def tie_span(scores):
    """(points whose fine maximum is attained in two row tiles of 32 channels, points whose fine maximum is attained in both half-wave row
    groups (channel mod 8 below / from 4), points with a coarse tie) of scores[B,P,N]"""
    fine = scores[:, 2:]
    at = fine == fine.max(1, keepdim=True).values                        # [B, P - 2, N]
    c = torch.arange(2, scores.shape[1])
    tile, half = c // 32, (c % 8) // 4
    def spans(key):
        lo = torch.where(at, key.view(1, -1, 1), 10 ** 6).min(1).values
        hi = torch.where(at, key.view(1, -1, 1), -1).max(1).values
        return int((hi > lo).sum())
    return spans(tile), spans(half), int((scores[:, 0] == scores[:, 1]).sum())


def _labels_a(B, N, P, relu, g):
    """family A with TIED output channels: the fine channels fall into a few classes of identical (W2 column, scale, shift), assigned at
    random -- every fine maximum is attained by a whole class, the first channel of which must win; the last channel shares its class with
    channel 4 (another row tile for P > 32, the other half-wave row group).  Coarse: without the ReLU (A-) the two channels are identical, every
    point a tie; with it (A) channel 1 is channel 0 plus y1[r1] - y1[r2] for two rows drawn at random -- a tie where the ReLU clips both rows
    (label 0 by the first-maximum rule), label 1 or label 0 by a strict comparison elsewhere"""
    Q = max(1, min(8, (P - 2) // 4))
    cls = torch.randint(0, Q, (P - 2,), generator=g)
    if P > 4:
        cls[P - 3] = cls[2]
    colW, colS, colH = _ints(-2, 2, (256, Q), g), _ints(1, 2, (Q,), g), _ints(-64, 64, (Q,), g)
    W2, sc2, sh2 = torch.empty(256, P), torch.empty(P), torch.empty(P)
    W2[:, 2:], sc2[2:], sh2[2:] = colW[:, cls], colS[cls], colH[cls]
    W2[:, :2], sc2[:2], sh2[:2] = _ints(-2, 2, (256, 1), g), 1.0, float(_ints(-8, 8, (1,), g))
    if relu:
        r1, r2 = torch.randperm(256, generator=g)[:2].tolist()
        W2[r1, 1] += 1.0
        W2[r2, 1] -= 1.0
    return {"y0": _ints(-8, 8, (B, 256, N), g), "W1": _ints(-2, 2, (256, 256), g), "W2": W2, "sc1": _ints(1, 2, (256,), g),
            "sh1": _ints(-64, 64, (256,), g), "relu1": relu, "sc2": sc2, "sh2": sh2}


def _labels_operands(family, B, N, P, g):
    one, zero = torch.ones(256), torch.zeros(256)
    d = {"sc1": one, "sh1": zero, "relu1": True, "sc2": None, "sh2": None}
    # a selection as output layer shows P of layer 1's 256 rows: the case carries a list of them that shows every row
    d["W2s"] = sels = [selection(256, P, g, offset=o) for o in range(0, 256, P)]
    sel2 = sels[0]
    if family in ("A", "A-"):
        return _labels_a(B, N, P, family == "A", g)
    if family in ("B", "B-"):
        y0 = xc._odd((B, 256, N), 18, g, low_bits=16)
        d.update(y0=y0, W1=sparse_pm1(256, 256, g), W2=sel2, relu1=family == "B")
    elif family == "C1":
        d.update(y0=sparse_activations((B, 256, N), g)[0], W1=wide(256, 256, g), W2=sel2)
    elif family == "C2":
        rows = xc.c_channels(256, 63, xc.seed_of("rows", B, N, P))
        d.update(y0=_ints(-1, 1, (B, 256, N), g), W1=selection(256, 256, g, rows=rows), W2=wide(256, P, g), relu1=False)
    elif family == "D1":
        d.update(y0=xc._odd((B, 256, N), 12, g, low_bits=8), W1=one_term(256, 256, g), W2=sel2, relu1=False)
    elif family == "D2":
        d.update(y0=xc._odd((B, 256, N), 12, g, low_bits=8), W1=selection(256, 256, g), W2=one_term(256, P, g), relu1=False)
    elif family == "E":
        d.update(y0=xc._odd((B, 256, N), 18, g, low_bits=16), W1=selection(256, 256, g), W2=sparse_pm1(256, P, g), relu1=False)
    else:
        raise ValueError(family)
    return d


@functools.lru_cache(maxsize=8)
def labels_case(family, B, N, P):
    """family A is drawn again (at most 64 times, seeds in order) until its reference has the ties the host test asserts"""
    for attempt in range(64):
        g = xc._gen(xc.seed_of("labels", family, B, N, P, attempt))
        d = _labels_operands(family, B, N, P, g)
        y1, b1 = _layer(d["W1"], d["y0"].double(), d["sc1"], d["sh1"], d["relu1"])
        s, b2 = _layer(d["W2"], y1, d["sc2"], d["sh2"])
        if family[0] != "A":
            break
        tiles, halves, coarse = tie_span(s)
        both = family == "A-" or B * N < 8 or len(set(first_maximum(s[:, 0:2]).flatten().tolist())) == 2
        if coarse > 0 and both and (P <= 32 or (tiles > 0 and halves > 0)):
            break
    else:
        raise AssertionError("no family-A case with the asserted ties in 64 draws: %r" % ((family, B, N, P),))
    d["stages"] = [("y1", y1, b1)]
    d["tails"] = []                                # [(W2, fp32 scores, coarse, fine)]: the output layers this case runs with
    for W2 in (d["W2s"] if "W2s" in d and d["W2"] is d["W2s"][0] else [d["W2"]]):
        s, b2 = _layer(W2, y1, d["sc2"], d["sh2"])
        d["stages"].append(("scores", s, b2))
        d["tails"].append((W2, s.float(), first_maximum(s[:, 0:2]), first_maximum(s[:, 2:])))
    return d
