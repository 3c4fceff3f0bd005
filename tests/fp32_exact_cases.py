"""Operands for which the fp32-MFMA INFERENCE kernels (csrc/gemm.hip, csrc/conv.hip, csrc/winograd.hip) are EXACT, with their fp64 references
(and of the stem, csrc/stem.hip; generators, case tables and references only: seeded, CPU, no GPU code).

The premise (tools/probe_mfma_rounding.hip, as in tests/train_exact_cases.py): v_mfma_f32_32x32x2_f32 and v_mfma_f32_16x16x4_f32 are exact fma
chains.  If every operand is a multiple of one power of two and the sum of the absolute products of an output -- the whole epilogue counted
in -- stays below 2^24 of that unit, every partial sum in any tiling, K-step order, split-K slice order or prefetch depth is exact and the
kernel must equal the fp64 contraction bit for bit.  tests/test_fp32_exact_cases_host.py proves the bounds and asks the library's routing
queries (ops.pointwise_route, ops.conv2d_route, ops.winograd_route, ops.point_chain_route, ops.point_head_route) which kernel instance every case runs on;
tests/test_gpu_fp32_exact.py runs the kernels.

Operand families (x: the activations, w: the weights):

  S    small dense integers, x in [-8, 8], w in [-4, 4], non-zero in the last row, the last column and at the last reduction index; with an
       epilogue of exact operands: scale in {1/2, 1, 2}, integer shift / residual / batch_bias, gathered tables of integers with weights in
       {1/4, 1/2, 1, 2, 4} or none, ReLU on and off.  Everything is a multiple of 2^-3: the bound is asserted on 8 x the values.
  IDA  identity-coded activations: x holds the id (flat row-major index + 1) of each of its elements, w is one-hot along K with value 1.  The
       output is the id of the element the kernel read: a mismatch decodes to "read (b', k', n') instead of (b, k, n)".
  IDB  identity-coded weights: w holds ids, x is one-hot along K.
       The one-hot positions of both walk the critical set of the route (`critical_k`): 0, K - 1, both sides of every K-step boundary, of
       every source boundary of the virtual concatenation and of every split-K slice boundary, the first row of the last K-step.
  P    signed selection: ONE +-1 weight per output row, x arbitrary normal finite float32 bit patterns (full 24-bit mantissas, every exponent
       but the denormals' and infinity's).  The output is a signed copy of one input row: exact for any float (every other product is +-0).
       Pins that no stager, LDS layout or fragment load truncates or permutes an operand.  For the convolutions: one tap per output channel,
       the output is a shifted copy of one input channel -- every border pixel, the halo zeros, the stride-2 parity, the odd last row.
  Pw   the mirror: full-mantissa weights, activations one-hot along K.

Dense sources also live as strided views inside NaN-filled buffers (train_exact_cases.place): a read outside the operand poisons the output.
"""
import collections
import contextlib
import functools
import math

import torch
import torch.nn.functional as F

from tests.train_exact_cases import LAYOUTS, decode, ids, one_hot, place, small, unplace  # noqa: F401  (re-exported for the tests)
from tests.x3_exact_cases import first_mismatch, seed_of  # noqa: F401

LIMIT = float(1 << 24)
UNIT = 8.0                                   # every value of family S and its epilogue is a multiple of 1 / UNIT
NAN = float("nan")
GUARD = 64                                   # floats of NaN before and after every output
FAMILIES = ("S", "IDA", "IDB", "P", "Pw")
GW = (0.25, 0.5, 1.0, 2.0, 4.0)
NODES, GK = 24, 3


def _gen(*what):
    return torch.Generator().manual_seed(seed_of(*what))


def _edges(t, dims):
    for d in dims:
        s = t.select(d, t.shape[d] - 1)
        s[s == 0] = 1.0
    return t


def any_floats(shape, g):
    """arbitrary normal finite float32 values: random sign, exponent field in [1, 254], random 23-bit fraction"""
    shape = tuple(int(s) for s in shape)
    sign = torch.randint(0, 2, shape, generator=g, dtype=torch.int64) << 31
    expo = torch.randint(1, 255, shape, generator=g, dtype=torch.int64) << 23
    frac = torch.randint(0, 1 << 23, shape, generator=g, dtype=torch.int64)
    bits = sign | expo | frac
    bits = torch.where(bits >= 1 << 31, bits - (1 << 32), bits).to(torch.int32)
    v = bits.view(torch.float32)
    assert bool(torch.isfinite(v).all()) and float(v.abs().min()) >= 2.0 ** -126
    return v


def walk(n, crit, K, g, rot=0):
    """n reduction indices: the critical set first (rotated by rot), then a stride-7 walk through all of K"""
    crit = sorted(set(crit))
    out = [crit[(i + rot) % len(crit)] for i in range(min(n, len(crit)))]
    out += [(7 * i + rot) % K for i in range(n - len(out))]
    return torch.tensor(out, dtype=torch.int64)


def critical_k(K, bk, bounds=()):
    """reduction indices at which a K-stepped contraction can go wrong: 0, K-1, both sides of every K-step boundary and of every extra
    boundary (source boundaries, split-K slice boundaries), the first row of the last K-step"""
    crit = {0, K - 1, (K - 1) // bk * bk}
    for b in list(range(bk, K, bk)) + [b for b in bounds if 0 < b < K]:
        crit.update((b - 1, b))
    return sorted(k for k in crit if 0 <= k < K)


def guarded(shape):
    """(flat NaN buffer, view of `shape` at GUARD floats) -- what a kernel writes into; the bands before and after must stay NaN"""
    n = math.prod(shape)
    buf = torch.full((n + 2 * GUARD,), NAN)
    return buf, buf[GUARD:GUARD + n].view(*shape)


# ===================================================================================================== di2p_pointwise_gemm
# src: dense | concat (5 + 64 + rest) | gather | group8 | group16;  layout (dense only): a key of LAYOUTS, applied to x as [B][K][N];
# epi: none | affine | relu | bias | g1 | g2 | transpose | gmax8 | gmax16_full;  knob: "" | pw_novec | conv_depth1
PwCase = collections.namedtuple("PwCase", "family B M K N src layout epi knob")
PW_INSTANCES = [(0, 32, 128, 0, 1), (0, 64, 128, 0, 1), (0, 128, 128, 0, 1)] + [(1, 64, bn, d, p) for bn in (64, 128) for d in (0, 1) for p in (1, 2)]


def pw_instance(rt):
    return (rt["vec"], rt["bm"], rt["bn"], rt["dense"], rt["depth"])


def _pw_table():
    out = []

    def add(family, M, K, N, src="dense", layout="c", epi="none", knob="", B=3):
        c = PwCase(family, B, M, K, N, src, layout, epi, knob)
        if c not in out:
            out.append(c)

    fams = ("S", "IDA", "IDB", "P", "Pw")
    # ---- scalar stager, K-step 16: K around the steps (1, 15, 16, 17, 33), ragged M and N tiles
    for i, (M, K, N) in enumerate(((1, 1, 1), (2, 15, 129), (32, 16, 60), (32, 33, 132), (30, 17, 4),                    # 32 x 128
                                   (33, 1, 1), (64, 15, 129), (33, 16, 64), (64, 33, 132), (65, 17, 130), (65, 33, 129),   # 64 x 128 (M = 65: N % 4 != 0)
                                   (130, 33, 60))):                                                                      # 64 x 128 off the 16-byte stager by the knob pw_novec
        for f in fams:
            add(f, M, K, N, knob="pw_novec" if M == 130 else "")
    # the 128 x 128 scalar tile: B * ceil(N / 128) * ceil(M / 128) >= 256 off the 16-byte stager (N odd); K tiny
    for f, K in (("S", 1), ("IDA", 33), ("IDB", 17), ("P", 33), ("Pw", 16)):
        add(f, 130, K, 8193, B=2)
    # ---- 16-byte stager, K-step 32: K in 1, 31, 32, 33, 64, 65, 97 (depth 2 from K = 65 on); N % 64 == 0 -> 64 x 64 tiles, else 64 x 128
    for i, K in enumerate((1, 31, 32, 33, 64, 65, 97)):
        for f in fams:
            add(f, (68, 132)[i % 2], K, (64, 192)[i % 2])
            add(f, (132, 68)[i % 2], K, (132, 60, 4)[i % 3])
    for f in fams:
        for K in (33, 97):
            add(f, 132, K, 64, knob="conv_depth1")
            add(f, 68, K, 132, knob="conv_depth1")
    # ---- the DENSE = false loader: a base offset of one float, a row stride / batch stride that is no multiple of 4, gather and group sources
    for f in ("S", "IDA", "P"):
        for K in (33, 97):
            add(f, 68, K, 64, layout="off1")
            add(f, 132, K, 132, layout="ld1")
            add(f, 68, K, 192, layout="bs1")
            add(f, 132, K, 60, src="gather")
            add(f, 68, K, 64, src="group16")
            add(f, 68, K, 136, src="group8")
        add(f, 68, 1, 64, layout="off1")                                   # one K-step, ragged M tile
        add(f, 132, 31, 132, layout="ld1")
        add(f, 68, 97, 64, layout="off1", knob="conv_depth1")             # depth 1 through four K-steps
        add(f, 132, 97, 132, layout="ld1", knob="conv_depth1")
    # ---- layouts that keep the dense loader: row stride N + 4, batch-stride gap of 4
    for f in ("S", "IDA", "P"):
        for lay in ("ld4", "bs4", "ld4bs4"):
            add(f, 68, 97, 64, layout=lay)
            add(f, 132, 33, 132, layout=lay)
            add(f, 33, 33, 129, layout=lay)
    for lay in ("ld1", "off1", "bs1"):
        add("S", 64, 33, 129, layout=lay)
        add("IDA", 30, 17, 60, layout=lay)
    # ---- the virtual concatenation 5 + 64 + rest on both stagers, gather / group on the scalar stager
    for f in ("S", "IDA", "IDB", "P"):
        add(f, 132, 97, 132, src="concat")
        add(f, 68, 70, 64, src="concat")
        add(f, 64, 81, 129, src="concat")
        add(f, 32, 70, 60, src="concat")
    for f in ("S", "IDA"):
        add(f, 33, 33, 129, src="gather")
        add(f, 32, 17, 64, src="group16")
        add(f, 64, 33, 136, src="group8")
    # ---- epilogues (family S; gathered / transposed outputs need M % 4 == 0)
    for epi in ("affine", "relu", "bias", "g1", "g2", "transpose", "gmax8", "gmax16_full"):
        add("S", 132, 97, 192, epi=epi)
        add("S", 68, 33, 144 if epi.startswith("gmax") else 132, epi=epi)
        add("S", 64, 33, 144 if epi.startswith("gmax") else 129 if epi in ("affine", "relu", "bias") else 132, epi=epi)
        add("S", 32, 17, 48, epi=epi)
    add("S", 130, 1, 8193, epi="affine", B=2)
    add("S", 130, 17, 8193, epi="bias", B=2)
    return out


PW_CASES = _pw_table()


def pw_id(c):
    return "%s-b%d-%dx%dx%d-%s-%s-%s%s" % (c.family, c.B, c.M, c.K, c.N, c.src, c.layout, c.epi, "-" + c.knob if c.knob else "")


def pw_dense(c):
    """does the case's source set qualify for the dense 16-byte loader (the `dense` argument of the route)?  Buffers are 16-byte aligned."""
    if c.src not in ("dense", "concat"):
        return False
    dld, off, bpad = LAYOUTS[c.layout]
    return (c.N + dld) % 4 == 0 and off % 4 == 0 and (c.K * (c.N + dld) + bpad) % 4 == 0


def pw_route(c):
    from deepi2p_amd import _lib, ops
    if c.knob:
        with _lib.option(c.knob, 1):
            return ops.pointwise_route(c.M, c.K, c.N, c.B, pw_dense(c), True)
    return ops.pointwise_route(c.M, c.K, c.N, c.B, pw_dense(c), True)


def pw_splits(c):
    return (5, 64, c.K - 69) if c.src == "concat" else (c.K,)


@functools.lru_cache(maxsize=64)
def pw_case(c):
    """dict: w f32[M,K]; parts = [(kind, tensor, gidx | None, group)] (tensor [B,C,n]); full f32[B,K,N] the virtual concatenation; acc / absum the
    fp64 contraction and the sum of absolute products; kw: epilogue operands (CPU); ref: fp64 of what the call writes (tuple for also_full);
    bound: the largest sum of absolute values through the whole epilogue, in units of 1 / UNIT; pos: the one-hot positions (ID, P families)"""
    B, M, K, N = c.B, c.M, c.K, c.N
    g = _gen("pw", c)
    rt = pw_route(c)
    sp = pw_splits(c)
    crit = critical_k(K, rt["bk"], bounds=[sum(sp[:i]) for i in range(1, len(sp))])
    n_in = {"gather": NODES, "group8": N // 8, "group16": N // 16}.get(c.src, N)          # columns of the stored source
    d = dict(route=rt, crit=crit)
    # ---- the stored source [B, K, n_in] and the weights [M, K]
    if c.family == "S":
        src = _edges(small((B, K, n_in), 8, g), (1, 2))
        w = _edges(small((M, K), 4, g), (0, 1))
    elif c.family in ("IDA", "P"):
        src = ids((B, K, n_in)) if c.family == "IDA" else any_floats((B, K, n_in), g)
        d["pos"] = pos = walk(M, crit, K, g)
        w = one_hot(pos, K)
        if c.family == "P":
            w = w * (torch.randint(0, 2, (M, 1), generator=g) * 2 - 1)
    else:
        w = ids((M, K)) if c.family == "IDB" else any_floats((M, K), g)
        d["pos"] = pos = torch.stack([walk(n_in, crit, K, g, rot=b) for b in range(B)])      # [B, n_in]
        src = one_hot(pos, K).transpose(1, 2).contiguous()                                     # [B, K, n_in]
    # ---- sources
    if c.src == "gather":
        gi = torch.randint(0, NODES, (B, N), generator=g, dtype=torch.int32)
        gi[:, 0], gi[:, -1] = NODES - 1, 0
        gi[:, 1:1 + min(N - 2, NODES)] = torch.arange(min(N - 2, NODES), dtype=torch.int32)        # every node is read
        full = torch.gather(src, 2, gi.long().unsqueeze(1).expand(B, K, N))
        parts = [("gather", src, gi, 1)]
    elif c.src.startswith("group"):
        grp = int(c.src[5:])
        full = src.repeat_interleave(grp, dim=2)
        parts = [("group", src, None, grp)]
    else:
        full = src
        parts = [("dense", t.contiguous(), None, 1) for t in torch.split(src, sp, dim=1)]
    acc = torch.einsum("mk,bkn->bmn", w.double(), full.double())
    absum = torch.einsum("mk,bkn->bmn", w.double().abs(), full.double().abs())
    # ---- epilogue (family S only)
    kw, v, bound = {}, acc, absum
    if c.epi != "none":
        assert c.family == "S"
        kw["relu"] = c.epi in ("relu", "g1", "gmax8")
        if c.epi == "bias":
            kw["batch_bias"] = small((B, M), 64, g)
            v, bound = v + kw["batch_bias"].double().unsqueeze(2), bound + kw["batch_bias"].double().abs().unsqueeze(2)
        if c.epi in ("g1", "g2"):
            kw["gathered"] = []
            for t in range(1 if c.epi == "g1" else 2):
                tab = small((B, NODES, M), 32, g)
                gi = torch.randint(0, NODES, (B, N, GK), generator=g, dtype=torch.int32)
                gw = None if t == 1 else torch.tensor(GW)[torch.randint(0, len(GW), (B, N, GK), generator=g)]
                kw["gathered"].append((tab, gi, gw))
                rows = torch.gather(tab.double().unsqueeze(1).expand(B, N, NODES, M), 2, gi.long().unsqueeze(3).expand(B, N, GK, M))   # [B,N,GK,M]
                if gw is not None:
                    rows = rows * gw.double().unsqueeze(3)
                v, bound = v + rows.sum(2).transpose(1, 2), bound + rows.abs().sum(2).transpose(1, 2)
        kw["scale"] = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (M,), generator=g)]
        kw["shift"] = small((M,), 4, g)
        v = v * kw["scale"].double().view(1, M, 1) + kw["shift"].double().view(1, M, 1)
        bound = bound * kw["scale"].double().view(1, M, 1) + kw["shift"].double().abs().view(1, M, 1)
        if kw["relu"]:
            v = torch.relu(v)
    ref = v
    if c.epi == "transpose":
        kw["transpose_out"] = True
        ref = v.transpose(1, 2).contiguous()
    if c.epi == "gmax8":
        kw["group_max"] = 8
        ref = v.view(B, M, N // 8, 8).max(dim=3)[0]
    if c.epi == "gmax16_full":
        kw.update(group_max=16, also_full=True)
        ref = (v, v.view(B, M, N // 16, 16).max(dim=3)[0])
    d.update(w=w, parts=parts, full=full, acc=acc, absum=absum, kw=kw, ref=ref, bound=bound * UNIT)
    return d


# ===================================================================================================== di2p_conv2d / di2p_conv2d_ws
# family: S (with epi: none | affine | res_relu) | T (one tap per output channel, x any floats) | TID (one tap, x ids);
# ws: "full" (the workspace di2p_conv2d_workspace_bytes asks for) | "none" (di2p_conv2d) | "small" (4 bytes short);  xoff: x starts xoff floats
# into its (16-byte aligned) buffer;  knob: "" | conv_depth1 | conv_s2scalar | conv_nosplit
ConvCase = collections.namedtuple("ConvCase", "family B Cin H W Cout KH KW stride pad tap_major epi ws xoff knob")
# (kernel, bm, bn, bk, variant, depth, splits > 1 ? splits : 1) the route can return
CONV_SCALAR = [(0, bm, bn, bk) for bm in (64, 128) for bn in (64, 128) for bk in (16, 32)]
CONV_VEC = [(1, 64, bn, v, dp) for bn in (64, 128) for v in (1, 2, 22) for dp in (1, 2)]
CONV_SPLITS = (2, 3)


def conv_out(n, k, stride, pad):
    return (n + 2 * pad - k) // stride + 1


def _conv_table():
    out = []

    def add(family, B, Cin, H, W, Cout, k, stride, pad, tap=False, epi="none", ws="full", xoff=0, knob=""):
        KH, KW = k if isinstance(k, tuple) else (k, k)
        c = ConvCase(family, B, Cin, H, W, Cout, KH, KW, stride, pad, tap, epi, ws, xoff, knob)
        if c not in out:
            out.append(c)

    # ---- scalar stager, 64 x 64 tiles: K-step 16 on the weight's own order (any Cin) and tap-major (Cin 16, 48), K-step 32 tap-major off the
    #      16-byte stager (OW % 4 != 0, Cout % 4 != 0, stride 3, a 3x3 without its padding).  1x1 / pad 0, 3x3, an even filter, 7x7 / 2.
    for f in ("S", "T", "TID"):
        add(f, 3, 1, 1, 1, 1, 1, 1, 0)                                   # one K row, one pixel
        add(f, 3, 3, 5, 7, 5, 3, 1, 1)                                   # K = 27: two K-steps, ragged
        add(f, 3, 5, 6, 9, 66, 3, 2, 1)                                  # K = 45: three K-steps, the last ragged; two M tiles
        add(f, 3, 3, 9, 14, 8, 7, 2, 3)                                  # 7x7 / 2 with OW = 7: the generic kernel
        add(f, 3, 2, 6, 8, 6, 2, 2, 0)                                   # an even filter
        add(f, 3, 16, 5, 7, 5, 3, 1, 1, tap=True)                        # tap-major, K-step 16: nine K-steps
        add(f, 3, 48, 4, 6, 66, 1, 1, 0, tap=True)                       # tap-major, K-step 16: three K-steps
        add(f, 3, 32, 5, 7, 6, 3, 1, 1, tap=True)                        # tap-major, K-step 32, OW % 4 != 0
        add(f, 3, 32, 5, 8, 6, 1, 1, 0, tap=True)                        # ... Cout % 4 != 0, one K-step
        add(f, 3, 32, 7, 10, 8, 3, 3, 1, tap=True)                       # ... stride 3
    # ---- the larger scalar tiles need >= 512 workgroups: 64 x 128 (Cout 65: ceil(Ntot / 128) >= 256), 128 x 128 (Cout 129: the same),
    #      128 x 64 (Cout 129..192 with Ntot in 16321..21760).  K tiny: 1x1 filters.
    for f in ("S", "TID"):
        for Cin, tap, W in ((2, False, 10881), (16, True, 10881), (32, True, 10881), (33, False, 10881)):
            if f == "TID" and Cin == 33:
                continue
            add(f, 3, Cin, 1, W, 65, 1, 1, 0, tap=tap)                    # Ntot = 32643 -> 64 x 128
            add(f, 3, Cin, 1, W, 129, 1, 1, 0, tap=tap)                   # -> 128 x 128
            add(f, 3, Cin, 1, 5443, 129, 1, 1, 0, tap=tap)                # Ntot = 16329 -> 128 x 64
    for Cout, W in ((65, 10881), (129, 10881), (129, 5443)):              # ... and three K-steps of 32 on each of them
        add("S", 3, 96, 1, W, Cout, 1, 1, 0, tap=True)
    # ---- 16-byte stager (tap-major, Cin % 32 == 0, OW % 4 == 0, Cout % 4 == 0): 64 x 128 for Cout <= 64, else 64 x 64; stride variants
    for f in ("S", "T", "TID"):
        for Cout in (8, 68):
            for knob in ("", "conv_depth1"):
                add(f, 3, 32, 5, 8, Cout, 1, 1, 0, tap=True, knob=knob)          # variant 1, one K-step
                add(f, 3, 32, 5, 8, Cout, 3, 1, 1, tap=True, knob=knob)          # variant 1, nine K-steps
                add(f, 3, 64, 2, 4, Cout, (1, 3), 1, 1, tap=True, knob=knob)     # variant 1, a 1 x 3 filter, W = 4
                add(f, 3, 32, 5, 16, Cout, 3, 2, 1, tap=True, knob=knob)         # variant 22: aligned windows, odd last row
                add(f, 3, 32, 5, 16, Cout, 1, 2, 0, tap=True, knob=knob)         # variant 22, 1x1
                add(f, 3, 32, 5, 7, Cout, 3, 2, 1, tap=True, knob=knob)          # variant 2: W != 2 OW
                add(f, 3, 32, 6, 8, Cout, 2, 2, 0, tap=True, knob=knob)          # variant 2: an even filter
                add(f, 3, 32, 5, 7, Cout, 1, 2, 0, tap=True, knob=knob)          # variant 2, 1x1: one K-step
            add(f, 3, 32, 5, 16, Cout, 3, 2, 1, tap=True, xoff=1)                # variant 2: misaligned x
            add(f, 3, 32, 5, 16, Cout, 3, 2, 1, tap=True, knob="conv_s2scalar")  # variant 2: by knob
    # ---- split-K: Cin % 32 == 0, Cin KH KW / 32 >= 24, Cout >= 128, fewer than 32 per-frame workgroups: 3 slices, 2 from 24 workgroups on
    for f in ("S", "TID"):
        for ws in ("full", "none", "small"):
            add(f, 3, 96, 5, 8, 128, 3, 1, 1, tap=True, ws=ws)                   # 27 K-steps in 3 slices
            add(f, 3, 96, 5, 16, 132, 3, 2, 1, tap=True, ws=ws)                  # ... on the window loader, ragged M tile
        add(f, 3, 96, 23, 32, 128, 3, 1, 1, tap=True)                            # 24 per-frame workgroups: 2 slices (13 + 14 K-steps)
        add(f, 3, 96, 5, 8, 128, 3, 1, 1, tap=True, knob="conv_nosplit")
        add(f, 3, 96, 5, 8, 128, 3, 1, 1, tap=True, knob="conv_depth1")
    # ---- the 7x7 / 2 row-decoding stager (weights in their own order, OW % 4 == 0, Cout % 4 == 0)
    for f in ("S", "T", "TID"):
        add(f, 3, 3, 9, 16, 8, 7, 2, 3)                                  # K = 147: five K-steps, the last ragged
        add(f, 3, 1, 5, 8, 68, 7, 2, 3)                                  # K = 49; two M tiles
    # ---- epilogues
    for epi in ("affine", "res_relu"):
        add("S", 3, 5, 6, 9, 66, 3, 2, 1, epi=epi)
        add("S", 3, 32, 5, 16, 68, 3, 2, 1, tap=True, epi=epi)
        add("S", 3, 32, 5, 8, 8, 3, 1, 1, tap=True, epi=epi)
        add("S", 3, 96, 5, 8, 128, 3, 1, 1, tap=True, epi=epi)
        add("S", 3, 3, 9, 16, 8, 7, 2, 3, epi=epi)
        add("S", 3, 2, 1, 10881, 129, 1, 1, 0, epi=epi)
    return out


CONV_CASES = _conv_table()


def conv_id(c):
    return "%s-b%d-c%d-%dx%d-o%d-k%dx%ds%dp%d-%s-%s-ws%s%s%s" % (c.family, c.B, c.Cin, c.H, c.W, c.Cout, c.KH, c.KW, c.stride, c.pad,
                                                              "tap" if c.tap_major else "own", c.epi, c.ws, "-xoff%d" % c.xoff if c.xoff else "",
                                                              "-" + c.knob if c.knob else "")


def conv_ws_bytes(c, B=None):
    """the workspace the case passes: (bytes the library asks for, bytes given)"""
    from deepi2p_amd import ops
    need = ops.conv2d_workspace_bytes((c.B if B is None else B, c.Cin, c.H, c.W), c.Cout, c.KH, c.KW, c.stride, c.pad, c.tap_major)
    return need, {"full": need, "none": 0, "small": max(need - 4, 0)}[c.ws]


def conv_route(c, B=None):
    from deepi2p_amd import _lib, ops

    def ask():
        return ops.conv2d_route((c.B if B is None else B, c.Cin, c.H, c.W), c.Cout, c.KH, c.KW, c.stride, c.pad, c.tap_major,
                                x_aligned=c.xoff % 4 == 0, wt_aligned=True, workspace_bytes=conv_ws_bytes(c, B)[1])
    if c.knob:
        with _lib.option(c.knob, 1):
            return ask()
    return ask()


def conv_instance(rt):
    if rt["kernel"] == 0:
        return (0, rt["bm"], rt["bn"], rt["bk"])
    if rt["kernel"] == 2:
        return (2,)
    return (1, rt["bm"], rt["bn"], rt["variant"], rt["depth"])


def conv_k_order(c):
    """k -> (ci, kh, kw) of the rows of Wt, as a permutation: Wt = w.permute(...).reshape(K, Cout)"""
    return (2, 3, 1, 0) if c.tap_major else (1, 2, 3, 0)


def conv_wt(c, w):
    return w.permute(*conv_k_order(c)).reshape(-1, c.Cout).contiguous()


@functools.lru_cache(maxsize=16)
def conv_case(c):
    """dict: x f32[B,Cin,H,W], w f32[Cout,Cin,KH,KW], Wt f32[K,Cout] in the case's row order, scale / shift f32[Cout], residual | None, relu,
    acc / absum (fp64 convolution and the sum of absolute products), ref (fp64, through the epilogue), bound (in units of 1 / UNIT),
    pos i64[Cout] (T / TID: the row of Wt that holds the channel's one weight), route, crit"""
    g = _gen("conv", c)
    B, Cin, H, W, Cout, KH, KW = c.B, c.Cin, c.H, c.W, c.Cout, c.KH, c.KW
    K = Cin * KH * KW
    rt = conv_route(c)
    d = dict(route=rt)
    bounds = []
    if rt["splits"] > 1:                                                  # slice z runs the K-steps [T z / splits, T (z + 1) / splits)
        T = K // rt["bk"]
        bounds = [T * z // rt["splits"] * rt["bk"] for z in range(1, rt["splits"])]
    d["crit"] = crit = critical_k(K, rt["bk"], bounds)
    if c.family == "S":
        x = _edges(small((B, Cin, H, W), 8, g), (1, 2, 3))
        w = _edges(small((Cout, Cin, KH, KW), 4, g), (0, 1, 2, 3))
    else:
        x = ids((B, Cin, H, W)) if c.family == "TID" else any_floats((B, Cin, H, W), g)
        d["pos"] = pos = walk(Cout, crit, K, g)
        sign = torch.ones(Cout, 1) if c.family == "TID" else (torch.randint(0, 2, (Cout, 1), generator=g) * 2 - 1).float()
        wt = (one_hot(pos, K) * sign).t().contiguous()                                          # [K, Cout] in the case's row order
        shape = (KH, KW, Cin, Cout) if c.tap_major else (Cin, KH, KW, Cout)
        inv = (3, 2, 0, 1) if c.tap_major else (3, 0, 1, 2)
        w = wt.view(*shape).permute(*inv).contiguous()
    Wt = conv_wt(c, w)
    acc = F.conv2d(x.double(), w.double(), stride=c.stride, padding=c.pad)
    absum = F.conv2d(x.double().abs(), w.double().abs(), stride=c.stride, padding=c.pad)
    scale, shift, residual, relu = torch.ones(Cout), torch.zeros(Cout), None, False
    v, bound = acc, absum
    if c.epi != "none":
        scale = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (Cout,), generator=g)]
        shift = small((Cout,), 4, g)
        v = v * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
        bound = bound * scale.double().view(1, -1, 1, 1) + shift.double().abs().view(1, -1, 1, 1)
        if c.epi == "res_relu":
            residual, relu = small(tuple(acc.shape), 16, g), True
            v, bound = torch.relu(v + residual.double()), bound + residual.double().abs()
    d.update(x=x, w=w, Wt=Wt, scale=scale, shift=shift, residual=residual, relu=relu, acc=acc, absum=absum, ref=v, bound=bound * UNIT)
    return d


# ===================================================================================================== di2p_conv3x3_winograd
# Weights are multiples of 4, so U = G g G^T (G has halves: a product of two is a quarter) is an integer; V = B^T d B is a signed sum of four
# pixels; the bound is asserted on the transform pipeline itself (`wino_pipeline`), the expected output is the plain fp64 convolution.
# family S: x in [-8, 8], w in 4 * [-2, 2];  T: one tap of value +-4 per output channel, x integers in [-2^12, 2^12] (a shifted copy is NOT
# exact for arbitrary floats in the transform domain: V adds and subtracts neighbouring pixels).
WinoCase = collections.namedtuple("WinoCase", "family B Cin H W Cout epi knobs dgrad")
WINO_KNOBS = ((), (("wino_cob", 32),), (("wino_cob", 64),), (("wino_cob", 32), ("wino_kc", 8)), (("wino_cob", 64), ("wino_kc", 8)),
              (("wino_cob", 32), ("wino_kc", 4)), (("wino_cob", 64), ("wino_kc", 4)), (("wino_reg", 1),), (("wino_reg", 2),), (("wino_reg", 3),))
WINO_INSTANCES = [(0, cob, kc) for cob in (32, 64) for kc in (4, 8)] + [(1, 4), (1, 2)]
WINO_G = torch.tensor([[1.0, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1.0]], dtype=torch.float64)
WINO_BT = torch.tensor([[1.0, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=torch.float64)
WINO_AT = torch.tensor([[1.0, 1, 1, 0], [0, 1, -1, -1]], dtype=torch.float64)


def _wino_table():
    out = []

    def add(family, B, Cin, H, W, Cout, epi="none", knobs=(), dgrad=False):
        c = WinoCase(family, B, Cin, H, W, Cout, epi, knobs, dgrad)
        if c not in out:
            out.append(c)

    shapes = [(8, 1, 4, 32), (16, 2, 6, 64), (24, 5, 66, 96), (8, 5, 6, 64), (24, 2, 4, 64), (16, 5, 66, 64)]
    for i, (Cin, H, W, Cout) in enumerate(shapes):
        for knobs in WINO_KNOBS:
            if dict(knobs).get("wino_cob") == 64 and Cout % 64:
                continue
            for f in ("S", "T"):
                add(f, 3, Cin, H, W, Cout, knobs=knobs)
    for knobs in ((), (("wino_reg", 1),), (("wino_reg", 2),), (("wino_reg", 3),), (("wino_cob", 64), ("wino_kc", 8), ("wino_reg", 1))):
        for epi in ("affine", "relu", "res", "res_relu"):
            add("S", 3, 16, 5, 6, 64, epi=epi, knobs=knobs)
        for f in ("S", "T"):
            add(f, 3, 16, 5, 6, 64, knobs=knobs, dgrad=True)
            add(f, 3, 24, 2, 66, 32, knobs=knobs, dgrad=True)
    # the automatic choice of the register-resident kernel: ceil(tiles / 64) * (Cout / 32) >= 256 (co-block 64 by itself needs 768 x 32 tiles: its instance is the forced one's, the threshold is asserted on the query)
    add("S", 3, 8, 64, 170, 64)          # 8160 tiles
    add("T", 3, 8, 64, 170, 64)
    return out


WINO_CASES = _wino_table()


def wino_id(c):
    return "%s-b%d-c%d-%dx%d-o%d-%s%s%s" % (c.family, c.B, c.Cin, c.H, c.W, c.Cout, c.epi, "".join("-%s%d" % (k[5:], v) for k, v in c.knobs),
                                          "-dgrad" if c.dgrad else "")


@contextlib.contextmanager
def knobs(pairs):
    """with knobs((("wino_cob", 32), ...)): every knob set for the block (nested _lib.option)"""
    from deepi2p_amd import _lib
    with contextlib.ExitStack() as stack:
        for k, v in pairs:
            stack.enter_context(_lib.option(k, v))
        yield


def wino_route(c, B=None):
    from deepi2p_amd import ops
    with knobs(c.knobs):
        return ops.winograd_route((c.B if B is None else B, c.Cin, c.H, c.W), c.Cout)


def wino_instance(rt):
    return (1, rt["waves"]) if rt["reg"] else (0, rt["cob"], rt["kc"])


def wino_pipeline(x, w):
    """The F(2x2, 3x3) pipeline in fp64 on x[B,Cin,H,W], w[Cout,Cin,3,3]: (U [16,Cin,Cout], V [16,B,Cin,TH,TW], the largest sum over ci of
    |U||V| of any transform position and tile, the largest A^T |M| A, y [B,Cout,2 TH,2 TW] of the pipeline)"""
    B, Cin, H, W = x.shape
    TH, TW = (H + 1) // 2, (W + 1) // 2
    U = torch.einsum("ix,ocxy,jy->ijco", WINO_G, w.double(), WINO_G)                            # [4,4,Cin,Cout]
    xp = F.pad(x.double(), (1, 2 * TW - W + 1, 1, 2 * TH - H + 1))
    d = xp.unfold(2, 4, 2).unfold(3, 4, 2)                                                      # [B,Cin,TH,TW,4,4]
    V = torch.einsum("ix,bcthxy,jy->ijbcth", WINO_BT, d, WINO_BT)                               # [4,4,B,Cin,TH,TW]
    Mm = torch.einsum("ijco,ijbcth->ijboth", U, V)
    Mabs = torch.einsum("ijco,ijbcth->ijboth", U.abs(), V.abs())
    y = torch.einsum("pi,ijboth,qj->botphq", WINO_AT, Mm, WINO_AT).reshape(B, -1, 2 * TH, 2 * TW)
    yabs = torch.einsum("pi,ijboth,qj->botphq", WINO_AT.abs(), Mabs, WINO_AT.abs())
    return U.reshape(16, Cin, -1), V.reshape(16, B, Cin, TH, TW), float(Mabs.max()), float(yabs.max()), y[:, :, :H, :W]


@functools.lru_cache(maxsize=16)
def wino_case(c):
    """dict: x f32[B,Cin,H,W]; weight f32 -- the layer's forward filter [Cout,Cin,3,3], or with dgrad the FORWARD filter [Cin,Cout,3,3] of the layer
    whose input gradient this is; w the filter the convolution applies; scale, shift, residual, relu; acc, ref (fp64), bound"""
    g = _gen("wino", c._replace(knobs=()))
    B, Cin, H, W, Cout = c.B, c.Cin, c.H, c.W, c.Cout
    if c.family == "S":
        x = _edges(small((B, Cin, H, W), 8, g), (1, 2, 3))
        w = 4.0 * _edges(small((Cout, Cin, 3, 3), 2, g), (0, 1, 2, 3))
    else:
        x = small((B, Cin, H, W), 1 << 12, g)
        pos = walk(Cout, critical_k(Cin * 9, 72), Cin * 9, g)
        w = (one_hot(pos, Cin * 9) * 4.0 * (torch.randint(0, 2, (Cout, 1), generator=g) * 2 - 1)).view(Cout, Cin, 3, 3)
    d = dict(x=x, w=w)
    # dgrad: the kernel convolves x (= dY) with w; the caller hands the forward filter wf[Cin_g = Cout_f, ...]: w[o, c] = flip(wf[c, o])
    d["weight"] = w.flip(2, 3).transpose(0, 1).contiguous() if c.dgrad else w
    acc = F.conv2d(x.double(), w.double(), padding=1)
    if c.dgrad:
        d["grad_ref"] = torch.nn.grad.conv2d_input((B, Cout, H, W), d["weight"].double(), x.double(), padding=1)
    scale, shift, residual, relu = torch.ones(Cout), torch.zeros(Cout), None, c.epi in ("relu", "res_relu")
    v = acc
    eb = 0.0
    if c.epi != "none":
        scale = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (Cout,), generator=g)]
        shift = small((Cout,), 4, g)
        v = v * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
        eb = 4.0
        if c.epi.startswith("res"):
            residual = small(tuple(acc.shape), 16, g)
            v = v + residual.double()
            eb += 16.0
        if relu:
            v = torch.relu(v)
    d.update(scale=scale, shift=shift, residual=residual, relu=relu, acc=acc, ref=v, epi_bound=eb)
    return d


# ===================================================================================================== di2p_attention_pool
# out[b,c,m] = (sum_hw feat[b,c,hw] score[b,hw,m]) / HW: the kernel divides the exact integer sum by (float)HW with one IEEE division; the
# reference is the fp64 quotient rounded once to fp32 (two integers below 2^24: fp64 carries 53 >= 2 * 24 + 2 bits, so the double rounding is
# innocuous).  HW a power of two and odd.
AttnCase = collections.namedtuple("AttnCase", "family B C HW Mn")
ATTN_SHAPES = ((1, 1, 1), (65, 33, 65), (70, 2, 130), (64, 64, 64))
ATTN_CASES = [AttnCase(f, 3, C, HW, Mn) for (C, HW, Mn) in ATTN_SHAPES for f in ("S", "IDA", "IDB")]


def attn_id(c):
    return "%s-b%d-c%d-hw%d-m%d" % (c.family, c.B, c.C, c.HW, c.Mn)


@functools.lru_cache(maxsize=None)
def attn_case(c):
    g = _gen("attn", c)
    B, C, HW, Mn = c.B, c.C, c.HW, c.Mn
    crit = critical_k(HW, 16)
    d = {}
    if c.family == "S":
        feat, score = _edges(small((B, C, HW), 8, g), (1, 2)), _edges(small((B, HW, Mn), 4, g), (1, 2))
    elif c.family == "IDA":
        feat = ids((B, C, HW))
        d["pos"] = pos = torch.stack([walk(Mn, crit, HW, g, rot=b) for b in range(B)])           # [B, Mn]
        score = one_hot(pos, HW).transpose(1, 2).contiguous()
    else:
        score = ids((B, HW, Mn))
        d["pos"] = pos = torch.stack([walk(C, crit, HW, g, rot=b) for b in range(B)])            # [B, C]
        feat = one_hot(pos, HW)
    acc = torch.bmm(feat.double(), score.double())
    absum = torch.bmm(feat.double().abs(), score.double().abs())
    d.update(feat=feat, score=score, acc=acc, absum=absum, ref=(acc / float(HW)).float())
    return d


# ===================================================================================================== di2p_batch_gemv / di2p_batch_gemv2
# out[b,m] = sum_k Wt[k0 + k, m] v[b,k]: four slices of per = ceil(Kv / 4) indices, added as (s0 + s1) + (s2 + s3); gemv2 adds a second pair.
GemvCase = collections.namedtuple("GemvCase", "family B M Kv k0 Kv1 k1")
GEMV_GRID = [(M, Kv, k0) for M in (1, 63, 64, 65, 130) for Kv, k0 in ((1, 0), (3, 2), (4, 0), (5, 7), (64, 1), (131, 3))]
GEMV_CASES = ([GemvCase(f, 3, M, Kv, k0, 0, 0) for (M, Kv, k0) in GEMV_GRID for f in ("S", "IDB")]
              + [GemvCase(f, 3, M, Kv, k0, Kv1, k0 + Kv + 2) for (M, Kv, k0) in GEMV_GRID[::2] for Kv1 in (1, 6, 33) for f in ("S", "IDB")][::3])


def gemv_id(c):
    return "%s-b%d-m%d-kv%d-k%d%s" % (c.family, c.B, c.M, c.Kv, c.k0, "-kv%d-k%d" % (c.Kv1, c.k1) if c.Kv1 else "")


def gemv_critical(Kv):
    per = (Kv + 3) // 4
    return critical_k(Kv, per)


@functools.lru_cache(maxsize=None)
def gemv_case(c):
    """dict: Wt f32[rows, M] (rows beyond the ranges read are NaN), v / v1 f32[B,Kv], ref fp64 [B,M], absum"""
    g = _gen("gemv", c)
    rows = max(c.k0 + c.Kv, c.k1 + c.Kv1) + 3
    Wt = torch.full((rows, c.M), NAN)
    ref, absum, d = torch.zeros(c.B, c.M, dtype=torch.float64), torch.zeros(c.B, c.M, dtype=torch.float64), {}
    for name, k0, Kv in (("v", c.k0, c.Kv), ("v1", c.k1, c.Kv1)):
        if not Kv:
            continue
        if c.family == "S":
            blk, v = _edges(small((Kv, c.M), 4, g), (0, 1)), _edges(small((c.B, Kv), 8, g), (1,))
        else:
            blk = ids((rows, c.M))[k0:k0 + Kv]
            pos = torch.tensor([gemv_critical(Kv)[(b + len(d)) % len(gemv_critical(Kv))] for b in range(c.B)])
            d["pos_" + name] = pos
            v = one_hot(pos, Kv)
        Wt[k0:k0 + Kv] = blk
        d[name] = v
        ref += v.double() @ blk.double()
        absum += v.double().abs() @ blk.double().abs()
    d.update(Wt=Wt, ref=ref, absum=absum)
    return d


# ===================================================================================================== di2p_point_chain
# Two or three layers of width M in {32, 64}: layer 0 reads ONE dense source of K0 <= M channels with the pointwise epilogue (batch_bias, gathered
# tables), layers 1 and 2 are M x M.  Families per chain (the bound holds per layer, as in tests/head_x3_cases.py):
#   S    small integers all the way: x in [-4, 4], every w in [-1, 1] with at most 8 non-zeros per row, integer shifts, ReLU on layers 0 and 1
#   ID   x ids, layer 0 one-hot over the critical set of its K-step, the later layers one-hot ROTATIONS (row m reads hidden row (m + rot) mod M),
#        so that every hidden row is observed at the output
ChainCase = collections.namedtuple("ChainCase", "family B M K0 layers N epi")
CHAIN_INSTANCES = [(M, ks0, nl) for M, kss in ((32, (4, 16)), (64, (16, 32))) for ks0 in kss for nl in (2, 3)]
CHAIN_N = (1, 4, 63, 64, 65)


def chain_uneven_n(M, K0, layers, B, cus):
    """the smallest N > 65 whose trips do not divide evenly among the waves in flight on `cus` compute units"""
    from deepi2p_amd import ops
    for N in range(66, 1 << 20, 31):
        rt = ops.point_chain_route(M, K0, layers, B, N, cus)
        if rt["total"] > 4 * rt["wgs"] and rt["total"] % (4 * rt["wgs"]):
            return N
    raise AssertionError("no uneven N")


def _chain_table():
    out = []
    for M in (32, 64):
        for i, K0 in enumerate((1, 8, 9, 32, 33, M)):
            if K0 > M:
                continue
            for layers in (2, 3):
                for j, N in enumerate(CHAIN_N):
                    fam = ("S", "ID")[(i + j + layers) % 2]
                    epi = ("none", "bias", "g1", "relu0")[(i + j) % 4] if fam == "S" else "none"
                    c = ChainCase(fam, 3, M, K0, layers, N, epi)
                    if c not in out:
                        out.append(c)
                for fam in ("S", "ID"):
                    c = ChainCase(fam, 3, M, K0, layers, 0, "none")                        # N = 0: the uneven N of the device, from the route query
                    if c not in out:
                        out.append(c)
    return out


CHAIN_CASES = _chain_table()


def chain_id(c):
    return "%s-b%d-m%d-k%d-l%d-n%s-%s" % (c.family, c.B, c.M, c.K0, c.layers, c.N or "uneven", c.epi)


def chain_route(c, cus, N=None):
    from deepi2p_amd import ops
    return ops.point_chain_route(c.M, c.K0, c.layers, c.B, N or c.N, cus)


@functools.lru_cache(maxsize=32)
def chain_case(c, N=None):
    """dict: x f32[B,K0,N]; layers = [(w f32[M,K], scale | None, shift | None, relu)]; kw (layer 0: batch_bias / gathered); outs = the fp64 output of
    every layer; bounds = the largest sum of absolute values of every layer, in units of 1 / UNIT^2 (scale 1/2 times a
    gathered weight 1/2: multiples of 1/4, carried through the integer layers behind; 1/64 is the safe side)"""
    N = N or c.N
    g = _gen("chain", c, N)
    B, M, K0 = c.B, c.M, c.K0
    ks0 = (4 if K0 <= 8 else 16) if M == 32 else (16 if K0 <= 32 else 32)
    layers, kw = [], {}
    if c.family == "S":
        x = _edges(small((B, K0, N), 4, g), (1, 2))
        for l in range(c.layers):
            K = K0 if l == 0 else M
            w = torch.zeros(M, K)
            for m in range(M):
                p = torch.randperm(K, generator=g)[:8]
                w[m, p] = (torch.randint(0, 2, (len(p),), generator=g) * 2 - 1).float()
            w[:, K - 1] = 1.0
            scale = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (M,), generator=g)] if l == 0 else None
            layers.append((w, scale, small((M,), 4, g), l < c.layers - 1 or c.epi == "relu0"))
        if c.epi == "bias":
            kw["batch_bias"] = small((B, M), 16, g)
        if c.epi == "g1":
            tab = small((B, NODES, M), 8, g)
            gi = torch.randint(0, NODES, (B, N, GK), generator=g, dtype=torch.int32)
            kw["gathered"] = [(tab, gi, torch.tensor(GW[1:4])[torch.randint(0, 3, (B, N, GK), generator=g)])]
    else:
        x = ids((B, K0, N))
        pos = walk(M, critical_k(K0, ks0), K0, g)
        layers.append((one_hot(pos, K0), None, None, False))
        for l in range(1, c.layers):
            rot = (torch.arange(M) + 5 * l + 1) % M
            layers.append((one_hot(rot, M), None, None, False))
        kw["pos"] = pos
    outs, bounds, v = [], [], x.double()
    for l, (w, scale, shift, relu) in enumerate(layers):
        a = torch.einsum("mk,bkn->bmn", w.double(), v)
        bd = torch.einsum("mk,bkn->bmn", w.double().abs(), v.abs())
        if l == 0 and "batch_bias" in kw:
            a, bd = a + kw["batch_bias"].double().unsqueeze(2), bd + kw["batch_bias"].double().abs().unsqueeze(2)
        if l == 0 and "gathered" in kw:
            tab, gi, gw = kw["gathered"][0]
            rows = torch.gather(tab.double().unsqueeze(1).expand(B, N, NODES, M), 2, gi.long().unsqueeze(3).expand(B, N, GK, M)) * gw.double().unsqueeze(3)
            a, bd = a + rows.sum(2).transpose(1, 2), bd + rows.abs().sum(2).transpose(1, 2)
        if scale is not None:
            a, bd = a * scale.double().view(1, M, 1), bd * scale.double().view(1, M, 1)
        if shift is not None:
            a, bd = a + shift.double().view(1, M, 1), bd + shift.double().abs().view(1, M, 1)
        if relu:
            a = torch.relu(a)
        outs.append(a)
        bounds.append(float(bd.max()) * (UNIT * UNIT if c.family == "S" else 1.0))          # ID: integers throughout
        v = a
    return dict(x=x, layers=layers, kw={k: v for k, v in kw.items() if k != "pos"}, pos=kw.get("pos"), outs=outs, bounds=bounds, N=N)


# ===================================================================================================== di2p_point_head
# Three layers K0 -> 128 -> 128 -> P <= 4 in one launch, on the LDS-tile kernel or (knob head_reg, K0 <= 96, at most two sources, an even
# first source of two) the wave-autonomous kernel; both gathered tables with k = 3 take the G33 epilogue of either.  The bound holds per layer.
#   family "x3:<F>": the operands of tests/head_x3_cases.head_case family F (K0 = 96 as 32 + 64 channels, both tables: G33) -- integers whose
#                    per-layer bounds that module's host test proves; every one-hot output layer of the case is run, so every hidden row is seen
#   family A / A-:   small integers of our own for the other shapes: K0 in {4, 96, 100}, one or two sources, an odd first source, two, one or
#                    no gathered table (one or none: the branch without G33); ReLU on / off
# split: channels of each source; tables: gathered tables given (A / A-: 0, 1 or 2 of HEAD_NODES nodes; the x3 families always give both, and
# the field holds their node count); reg: the knob head_reg
HeadCase = collections.namedtuple("HeadCase", "family B N P K0 split tables reg")
HEAD_INSTANCES = [(reg, g33) for reg in (0, 1) for g33 in (0, 1)]
HEAD_NODES = 16


def head_uneven_n(B, cus):
    """the smallest N % 4 == 0 at which the wave-autonomous kernel's waves take unequal numbers of trips on `cus` compute units"""
    from deepi2p_amd import _lib, ops
    with _lib.option("head_reg", 1):
        for N in range(36, 1 << 22, 36):
            rt = ops.point_head_route(96, 2, 32, B, N, cus)
            if rt["total"] > 8 * rt["wgs"] and rt["total"] % (8 * rt["wgs"]):
                return N
    raise AssertionError("no uneven N")


def _head_table():
    from tests import head_x3_cases as hx
    out = []
    for reg in (0, 1):
        for i, fam in enumerate(hx.HEAD_FAMILIES):
            for B, N, P, nodes in ((3, 68, 2, 16), (1, 4, 4, 1), (3, 1000, 4, 128))[i % 2::2] + ((3, 32, 1, 128),)[:i % 3 == 0]:
                out.append(HeadCase("x3:" + fam, B, N, P, 96, (32, 64), nodes, reg))
        for fam in ("A", "A-"):
            for K0, split in ((4, (4,)), (96, (96,)), (96, (32, 64)), (96, (33, 63)), (100, (100,)), (100, (36, 64)), (48, (2, 46))):
                for tables in (2, 1, 0):
                    out.append(HeadCase(fam, 3, (68, 132, 4)[tables], 1 + (K0 + tables) % 4, K0, split, tables, reg))
            out.append(HeadCase(fam, 3, 0, 2, 96, (32, 64), 2, reg))                 # N = 0: the uneven N of the device, from the route query
            out.append(HeadCase(fam, 3, 0, 3, 96, (96,), 1, reg))
    return out


HEAD_CASES = _head_table()


def head_id(c):
    return "%s-b%d-n%s-p%d-k%d-%s-t%s-reg%d" % (c.family, c.B, c.N or "uneven", c.P, c.K0, "+".join(str(v) for v in c.split), c.tables, c.reg)


def head_g33(c):
    return c.family.startswith("x3:") or c.tables == 2


def head_route(c, cus, N=None):
    from deepi2p_amd import _lib, ops
    with _lib.option("head_reg", c.reg):
        return ops.point_head_route(c.K0, len(c.split), c.split[0], c.B, N or c.N, cus, g33=head_g33(c))


@functools.lru_cache(maxsize=8)
def head_case(c, N=None):
    """dict: srcs = [f32[B,Ci,N]]; W0 f32[K0,128], W1 f32[128,128]; sc0 sh0 sc1 sh1 sc2 sh2 relu0 relu1 relu2; gathered = [(table, idx, w | None)];
    tails = [(W2 f32[128,P], fp64 output)]; stages = [(name, fp64 value, bound)] of every layer; y0, y1 fp64"""
    from tests import head_x3_cases as hx
    N = N or c.N
    B, P, K0 = c.B, c.P, c.K0
    if c.family.startswith("x3:"):
        h = hx.head_case(c.family[3:], B, N, P, (c.tables, c.tables))
        d = {k: h[k] for k in ("W0", "W1", "sc0", "sh0", "sc1", "sh1", "sc2", "sh2", "relu0", "relu1", "relu2", "stages")}
        d["srcs"] = [h["first"], h["second"]]
        d["gathered"] = [(h["Ga"], h["ia"], h["wa"]), (h["Gb"], h["ib"], h["wb"])]
        d["tails"] = [(W2, st[1]) for (W2, _), st in zip(h["tails"], h["stages"][2:])]
        return d
    g = _gen("head", c, N)
    on = c.family == "A"
    x = _edges(small((B, K0, N), 8, g), (1, 2))
    d = dict(W0=_edges(small((K0, 128), 2, g), (0, 1)), W1=small((128, 128), 1, g), sc0=hx._ints(1, 2, (128,), g), sh0=small((128,), 4, g),
             sc1=hx._ints(1, 2, (128,), g), sh1=small((128,), 64, g), sc2=hx._ints(1, 2, (P,), g), sh2=small((P,), 64, g), relu0=on, relu1=on, relu2=on)
    d["srcs"] = [t.contiguous() for t in torch.split(x, c.split, dim=1)]
    d["gathered"] = []
    t = torch.zeros(B, 128, N, dtype=torch.float64)
    ta = torch.zeros(B, 128, N, dtype=torch.float64)
    for i in range(c.tables):
        G, idx = small((B, HEAD_NODES, 128), 8, g), hx._indices(B, N, HEAD_NODES)
        w = hx._ints(1, 2, (B, N, 3), g) if i == 0 else None
        d["gathered"].append((G, idx, w))
        rows = torch.gather(G.double(), 1, idx.long().reshape(B, N * 3, 1).expand(B, N * 3, 128)).reshape(B, N, 3, 128)
        ww = (w.double() if w is not None else torch.ones(B, N, 3, dtype=torch.float64)).unsqueeze(3)
        t += (rows * ww).sum(2).transpose(1, 2)
        ta += (rows.abs() * ww).sum(2).transpose(1, 2)
    y0, b0 = hx._layer(d["W0"], x.double(), d["sc0"], d["sh0"], on, extra=t, extra_abs=ta)
    y1, b1 = hx._layer(d["W1"], y0, d["sc1"], d["sh1"], on)
    W2 = _edges(small((128, P), 1, g), (0, 1))
    out, b2 = hx._layer(W2, y1, d["sc2"], d["sh2"], on)
    d["stages"] = [("y0", y0, b0), ("y1", y1, b1), ("out", out, b2)]
    d["tails"] = [(W2, out)]
    return d


# ===================================================================================================== di2p_conv7x7s2_stem and its packer
# conv 7x7 / 2 / pad 3, 3 -> 64, scale / shift, optional ReLU, compared BEFORE any pooling, on integer pixels 0..255.  A workgroup owns two output
# rows x 128 pixels; at most 512 persistent workgroups walk the (frame, row pair, column tile) items.  Shapes: those of tests/stem_x3_cases.py,
# the smallest and an odd one, and one with more items (516) than workgroups and a one-pixel last column tile.
#   S          w in [-2, 2], scale in {1/2, 1, 2}, integer shift in [-64, 64], ReLU on
#   D0 D1 D2   the tap sets of stem_x3_cases.d_taps: ONE weight per output channel (odd, below 2^8, the sign alternating with the channel),
#              all 147 taps between them; the output is a scaled copy of one shifted input channel: borders, halo zeros, stride-2 parity
StemCase = collections.namedtuple("StemCase", "family B H W")
STEM_SHAPES = [(1, 1), (5, 7)] + [(4, 128), (12, 128), (8, 256), (36, 384), (44, 128), (96, 128), (160, 128)] + [(344, 258)]
STEM_CASES = [StemCase(f, 3, H, W) for (H, W) in STEM_SHAPES for f in ("S", "D0", "D1", "D2") if (H, W) != (344, 258) or f in ("S", "D1")]


def stem_id(c):
    return "%s-b%d-%dx%d" % (c.family, c.B, c.H, c.W)


def stem_items(c):
    """(work items, persistent workgroups) of the launch"""
    OH, OW = (c.H - 1) // 2 + 1, (c.W - 1) // 2 + 1
    total = c.B * -(-OH // 2) * -(-OW // 128)
    return total, min(total, 512)


def stem_packed(w):
    """the packer's layout: Wp[(ci * 7 + ky) * 8 + kx][co] = w[co][ci][ky][kx], kx = 7: zero"""
    return F.pad(w, (0, 1)).permute(1, 2, 3, 0).reshape(168, 64).contiguous()


@functools.lru_cache(maxsize=4)
def stem_case(c):
    from tests import stem_x3_cases as sx
    g = _gen("stem", c)
    x = torch.randint(0, 256, (c.B, 3, c.H, c.W), generator=g).float()
    x[:, :, -1, :][x[:, :, -1, :] == 0] = 1.0
    x[:, :, :, -1][x[:, :, :, -1] == 0] = 1.0
    if c.family == "S":
        w = _edges(small((64, 3, 7, 7), 2, g), (0, 1, 2, 3))
        scale = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (64,), generator=g)]
        shift, relu = small((64,), 64, g), True
    else:
        w = sx.d_weights(int(c.family[1])) * torch.where(torch.arange(64) % 2 == 1, -1.0, 1.0).view(64, 1, 1, 1)
        scale, shift, relu = torch.ones(64), torch.zeros(64), False
    acc = F.conv2d(x.double(), w.double(), stride=2, padding=3)
    absum = F.conv2d(x.double().abs(), w.double().abs(), stride=2, padding=3)
    v = acc * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
    bound = (absum * scale.double().view(1, -1, 1, 1) + shift.double().abs().view(1, -1, 1, 1)) * 2.0          # halves: units of 1/2
    return dict(x=x, w=w, scale=scale, shift=shift, relu=relu, acc=acc, ref=torch.relu(v) if relu else v, bound=bound)
