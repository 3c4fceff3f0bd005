"""Operands for which the fp32 matrix kernels of the training step (csrc/train.hip) are EXACT, with their fp64 references (generators and
references only: seeded, CPU, no GPU code).

The premise (tools/probe_mfma_rounding.hip): v_mfma_f32_32x32x2_f32 is an exact fma chain.  With integer operands and the sum of the absolute
products of every output at most 2^24, every partial sum of every accumulator -- in any chunking, tile or order, the fp32 sum over the chunks'
partial tiles included -- is an integer below 2^24 and therefore exact: the kernel must equal the fp64 contraction bit for bit.
tests/test_train_exact_cases_host.py proves the bound for every case below; tests/test_gpu_train_exact.py runs the kernels.

Two operand families:

  S    small dense integers: the first operand (A, dy) in [-8, 8], the second (B, x, W, weights) in [-4, 4]; non-zero in the last row, the last
       column and at the last reduction index, so that losing any of them changes the expected output.  Every term is counted once.
  ID   identity-coded: one operand holds the distinct integer id (flat row-major index + 1) of each of its elements, the other is one-hot along
       the reduction index with value 1.  The output is then the id of the element the kernel read: a mismatch decodes (`decode`) to "read
       (z', i', r') instead of (z, i, r)".  Both ways round ("IDA": the first operand coded, "IDB": the second).  The one-hot positions cover
       the critical set of the chunk plan (`critical_set`: 0, R-1, both sides of every chunk boundary, the first and last valid index of the
       last K-step), which is asked from the library's own routing function (ops.rc_route), not restated.

Strided operands (`place`) live inside larger NaN-filled buffers: the ld - R gap of every row, guard rows before and after and the batch-stride
gap are NaN, so a read outside the operand poisons the output.
"""
import collections
import functools
import itertools

import torch

from tests.x3_exact_cases import first_mismatch, seed_of  # noqa: F401  (re-exported for the tests)

LIMIT = float(1 << 24)
RC_BK = 32                                   # reduction indices per K-step of the rc-GEMM kernels
NAN = float("nan")
ALPHAS = (1.0, 0.25, -3.0)


def _gen(*what):
    return torch.Generator().manual_seed(seed_of(*what))


def small(shape, lim, g):
    """integers in [-lim, lim] as f32"""
    return torch.randint(-lim, lim + 1, tuple(shape), generator=g).to(torch.float32)


def _nonzero_edges(t, dims):
    """replace the zeros of the last slice of t along each of `dims` by 1 (family S: losing an edge must change the result)"""
    for d in dims:
        s = t.select(d, t.shape[d] - 1)
        s[s == 0] = 1.0
    return t


def ids(shape):
    """the id of every element: flat row-major index + 1, as f32 (exact: the host test bounds them by 2^24)"""
    n = 1
    for s in shape:
        n *= int(s)
    return torch.arange(1, n + 1, dtype=torch.float64).view(*shape).to(torch.float32)


def decode(value, shape):
    """the index tuple of the element whose id is `value`, or None if it is no id of an operand of this shape"""
    v = float(value)
    n = 1
    for s in shape:
        n *= int(s)
    if v != v or v != int(v) or not 1 <= int(v) <= n:
        return None
    flat, idx = int(v) - 1, []
    for s in reversed(shape):
        idx.append(flat % s)
        flat //= s
    return tuple(reversed(idx))


def critical_set(R, rch, chunks):
    """the reduction indices at which a chunked, K-stepped reduction can go wrong"""
    last_begin = (chunks - 1) * rch
    steps = (R - last_begin + RC_BK - 1) // RC_BK
    crit = {0, R - 1, last_begin + (steps - 1) * RC_BK}
    for c in range(1, chunks):
        crit.update((c * rch - 1, c * rch))
    assert all(0 <= r < R for r in crit)
    return sorted(crit)


def one_hot_positions(Z, n, crit, R, g):
    """pos i64[Z, n]: the first len(crit) rows of every batch walk the critical set (rotated by the batch), the rest are random"""
    pos = torch.randint(0, R, (Z, n), generator=g)
    for z in range(Z):
        for i in range(min(n, len(crit))):
            pos[z, i] = crit[(i + z) % len(crit)]
    return pos


def one_hot(pos, R):
    out = torch.zeros(tuple(pos.shape) + (R,))
    out.scatter_(-1, pos.unsqueeze(-1), 1.0)
    return out


# ------------------------------------------------------------------------------------------------ strided operands in NaN-filled buffers
# name -> (ld - R, base offset in floats, batch-stride padding in floats)
LAYOUTS = {"c": (0, 0, 0), "ld4": (4, 0, 0), "ld1": (1, 0, 0), "off1": (0, 1, 0), "bs4": (0, 0, 4), "bs1": (0, 0, 1), "ld4bs4": (4, 0, 4)}
Placed = collections.namedtuple("Placed", "buf offset ld batch_stride")


def place(t, layout):
    """t f32[Z, n, R] laid out as `layout` inside a NaN-filled flat buffer: Placed(buf, offset of element (0,0,0) in floats, ld, batch stride).
    The guards (a multiple of 64 floats: the alignment of the operand is that of the buffer plus the layout's offset) cover more than the 32
    floats a 16-byte stager could stray."""
    dld, off, bpad = LAYOUTS[layout] if isinstance(layout, str) else layout
    Z, n, R = t.shape
    ld = R + dld
    bs = n * ld + bpad
    guard = (2 * ld + 63) // 64 * 64
    buf = torch.full((guard + off + Z * bs + guard,), NAN)
    buf.as_strided((Z, n, R), (bs, ld, 1), guard + off).copy_(t)
    return Placed(buf, guard + off, ld, bs)


def unplace(p, Z, n, R):
    return p.buf.as_strided((Z, n, R), (p.batch_stride, p.ld, 1), p.offset)


# ------------------------------------------------------------------------------------------------ di2p_bmm_rc
RcCase = collections.namedtuple("RcCase", "family Z rows cols R reduce_z alpha layA layB tile64")
RC_DIMS = (1, 5, 63, 64, 65, 129, 130, 255)
RC_R = (1, 31, 32, 33, 36, 515, 516, 772, 2050, 2305, 2308, 2592)
RC_R_EXTRA = (1800, 4352)                    # seven and seventeen chunks (rc_reduce_kernel: per_group 7 and 17)


def _rc_table():
    out = []

    def add(family, Z, rows, cols, R, reduce_z, alpha=1.0, layA="c", layB="c", tile64=0):
        c = RcCase(family, Z, rows, cols, R, reduce_z, alpha, layA, layB, tile64)
        if c not in out:
            out.append(c)

    # every R against a walk through the row / column sizes, both Z, both reduce_z, every alpha
    for i, R in enumerate(RC_R):
        for v in range(2):
            rows, cols = RC_DIMS[(i + 5 * v) % 8], RC_DIMS[(3 * i + 2 + 3 * v) % 8]
            add("S", (1, 3)[(i + v) % 2], rows, cols, R, (i // 2 + v) % 2, ALPHAS[(i + v) % 3])
    # the reduction kernel: per_group 1, 7, 8, 9, 17 without reduce_z (Z = 1 and 3) and 9 = 3 x 3, 24 = 3 x 8, 27 = 3 x 9 with it
    for R, Z, reduce_z, alpha in ((36, 1, 1, -3.0), (1800, 1, 0, 0.25), (1800, 3, 0, 1.0), (2050, 1, 1, -3.0), (2305, 3, 0, 0.25), (4352, 1, 0, -3.0),
                                  (4352, 1, 1, 1.0), (772, 3, 1, 0.25), (2050, 3, 1, 1.0), (2308, 3, 1, -3.0), (1800, 1, 1, 1.0)):
        add("S", Z, 5, 65, R, reduce_z, alpha)
    # layouts, on each operand alone and on both: at a 64-tile shape and at a 128-tile shape (where a layout that keeps 16-byte rows stays on
    # rc_gemm_kernel<128,true,true> and any other falls to the scalar stagers)
    for lay in ("ld4", "ld1", "off1", "bs4", "bs1", "ld4bs4"):
        for la, lb in ((lay, "c"), ("c", lay), (lay, lay)):
            add("S", 3, 65, 63, 516, 0, 1.0, la, lb)
            add("S", 3, 129, 130, 36, 1, 0.25, la, lb)
    add("S", 3, 5, 64, 2308, 0, 1.0, "ld4", "bs4")
    add("S", 3, 64, 5, 2305, 1, 1.0, "ld1", "off1")
    add("S", 3, 63, 1, 31, 0, -3.0, "bs1", "ld4")
    # big cases: 128 x 128 tiles, and the same operands on 64 x 64 tiles
    for Z, rows, cols, R, reduce_z, alpha, la, lb in ((1, 129, 130, 32, 0, 1.0, "c", "c"), (3, 255, 255, 2592, 1, 1.0, "c", "c"),
                                                      (1, 130, 129, 2308, 0, -3.0, "c", "c"), (3, 255, 130, 516, 0, 0.25, "c", "c"),
                                                      (3, 129, 255, 772, 1, 1.0, "ld4", "bs4"), (1, 255, 129, 36, 1, 1.0, "ld4bs4", "ld4")):
        for tile64 in (0, 1):
            add("S", Z, rows, cols, R, reduce_z, alpha, la, lb, tile64)
    # identity-coded, both ways round: scalar stagers (R % 4 != 0, or a layout without 16-byte rows), 16-byte stagers on 64 x 64 tiles, and
    # 128 x 128 tiles with their 64-tile rerun; the one-hot side has at least 40 rows
    for fam, (rows, cols) in (("IDA", (5, 65)), ("IDB", (63, 5)), ("IDA", (65, 64)), ("IDB", (64, 65))):
        for R in (33, 36, 516, 772, 2050, 2305, 2308, 2592):
            add(fam, 1 if R in (33, 2050) else 3, rows, cols, R, 1 if R in (36, 2305) else 0)
    for fam in ("IDA", "IDB"):
        for R, Z, reduce_z, la, lb in ((2308, 1, 0, "c", "c"), (2592, 3, 1, "ld4", "ld4bs4"), (36, 3, 0, "c", "c"), (2305, 1, 0, "c", "c")):
            for tile64 in ((0, 1) if R % 4 == 0 else (0,)):
                add(fam, Z, 129, 130, R, reduce_z, 1.0, la, lb, tile64)
        add(fam, 3, 65, 64, 2308, 0, 1.0, "ld1", "c")
        add(fam, 3, 65, 64, 516, 1, 1.0, "c", "off1")
        add(fam, 3, 65, 64, 2308, 0, 1.0, "bs1", "bs1")
    # whatever else above may take 128 x 128 tiles gets its 64-tile twin too (the host test asks the routing query which ones do)
    for c in list(out):
        if min(c.rows, c.cols) >= 128 and c.R % 4 == 0 and c.R >= 32 and {c.layA, c.layB} <= {"c", "ld4", "bs4", "ld4bs4"}:
            add(*c._replace(tile64=1))
    return out


RC_CASES = _rc_table()


def rc_id(c):
    return "%s-z%d-%dx%dx%d-%s%s-%s-%s%s" % (c.family, c.Z, c.rows, c.cols, c.R, "rz" if c.reduce_z else "b", "" if c.alpha == 1.0 else "-a%g" % c.alpha,
                                            c.layA, c.layB, "-t64" if c.tile64 else "")


def rc_operands(family, Z, rows, cols, R):
    """(A f32[Z,rows,R], B f32[Z,cols,R]) of the family; ID asks the library's routing function for the chunk plan (any stager pair: the plan
    depends on the tile only through the number of tiles, and both tiles are checked by the host test)"""
    what = (family, Z, rows, cols, R)
    g = _gen("rc", what)
    if family == "S":
        return _nonzero_edges(small((Z, rows, R), 8, g), (1, 2)), _nonzero_edges(small((Z, cols, R), 4, g), (1, 2))
    from deepi2p_amd import ops
    rt = ops.rc_route("strided", Z, rows, cols, R, False, False)
    crit = critical_set(R, rt["rch"], rt["chunks"])
    if family == "IDA":
        return ids((Z, rows, R)), one_hot(one_hot_positions(Z, cols, crit, R, g), R)
    if family == "IDB":
        return one_hot(one_hot_positions(Z, rows, crit, R, g), R), ids((Z, cols, R))
    raise ValueError(family)


def contract(A, B, reduce_z, alpha=1.0):
    """(fp64 reference of alpha * sum_r A[z,i,r] B[z,j,r] (summed over z with reduce_z), the sum of absolute products per output)"""
    ref = torch.einsum("zir,zjr->zij", A.double(), B.double())
    absum = torch.einsum("zir,zjr->zij", A.double().abs(), B.double().abs())
    if reduce_z:
        ref, absum = ref.sum(0), absum.sum(0)
    return ref * alpha, absum


@functools.lru_cache(maxsize=None)
def _rc_dense(family, Z, rows, cols, R, reduce_z):
    A, B = rc_operands(family, Z, rows, cols, R)
    ref, absum = contract(A, B, reduce_z)
    return A, B, ref, absum


def rc_case(c):
    """dict: A, B (dense f32), pa, pb (Placed), ref (fp64, alpha applied), absum; callers must not write to the tensors (shared)"""
    A, B, ref, absum = _rc_dense(c.family, c.Z, c.rows, c.cols, c.R, c.reduce_z)
    return dict(A=A, B=B, pa=place(A, c.layA), pb=place(B, c.layB), ref=ref * c.alpha, absum=absum)


def rc_explain(c, idx, got):
    """family ID: which element the kernel read instead (idx: index into the output, got: the value there)"""
    if c.family == "S" or c.alpha != 1.0:
        return ""
    coded_shape = (c.Z, c.rows, c.R) if c.family == "IDA" else (c.Z, c.cols, c.R)
    if c.reduce_z:
        return " (the sum over z of the ids; got decodes only without reduce_z)"
    return " (read element %s of the coded operand %s)" % (decode(got, coded_shape), coded_shape)


# ------------------------------------------------------------------------------------------------ di2p_bmm_km
KmCase = collections.namedtuple("KmCase", "family Z rows cols K alpha dlda dldb bpad")
KM_DIMS = (1, 63, 64, 65, 130)
KM_K = (1, 15, 16, 17, 40)


def _km_table():
    out = []
    for i, K in enumerate(KM_K):
        for v in range(3):
            rows, cols = KM_DIMS[(i + 2 * v) % 5], KM_DIMS[(2 * i + v + 1) % 5]
            out.append(KmCase("S", (1, 3)[(i + v) % 2], rows, cols, K, ALPHAS[(i + v) % 3], (0, 3, 1)[v], (0, 1, 4)[(i + v) % 3], (0, 5)[v % 2]))
    for K in KM_K:
        out.append(KmCase("IDA", 3, 65, 130, K, 1.0, 2, 0, 3))
        out.append(KmCase("IDB", 3, 130, 63, K, 1.0, 0, 1, 1))
    out.append(KmCase("S", 3, 130, 130, 40, -3.0, 1, 1, 1))
    out.append(KmCase("S", 1, 1, 1, 1, 0.25, 0, 0, 0))
    return out


KM_CASES = _km_table()


def km_id(c):
    return "%s-z%d-%dx%dx%d-a%g-ld+%d+%d-bs+%d" % (c.family, c.Z, c.rows, c.cols, c.K, c.alpha, c.dlda, c.dldb, c.bpad)


@functools.lru_cache(maxsize=None)
def km_case(c):
    """dict: A f32[Z,K,rows], B f32[Z,K,cols] (k-major), pa, pb (Placed: ld = rows + dlda / cols + dldb), ref (fp64), absum.  The one-hot side
    of family ID is one-hot along k; its positions walk 0, K-1 and both sides of the 16-wide K-step, then every k."""
    g = _gen("km", c)
    Z, rows, cols, K = c.Z, c.rows, c.cols, c.K
    crit = sorted({0, K - 1, min(15, K - 1), min(16, K - 1)}) + list(range(K))
    if c.family == "S":
        A, B = _nonzero_edges(small((Z, K, rows), 8, g), (1, 2)), _nonzero_edges(small((Z, K, cols), 4, g), (1, 2))
    elif c.family == "IDA":
        A, B = ids((Z, K, rows)), one_hot(one_hot_positions(Z, cols, crit, K, g), K).transpose(1, 2).contiguous()
    else:
        A, B = one_hot(one_hot_positions(Z, rows, crit, K, g), K).transpose(1, 2).contiguous(), ids((Z, K, cols))
    ref = torch.einsum("zki,zkj->zij", A.double(), B.double()) * c.alpha
    absum = torch.einsum("zki,zkj->zij", A.double().abs(), B.double().abs())
    return dict(A=A, B=B, pa=place(A, (c.dlda, 0, c.bpad)), pb=place(B, (c.dldb, 0, c.bpad)), ref=ref, absum=absum)


def km_explain(c, got):
    if c.family == "S":
        return ""
    shape = (c.Z, c.K, c.rows) if c.family == "IDA" else (c.Z, c.K, c.cols)
    return " (read element %s of the coded operand %s)" % (decode(got, shape), shape)


# ------------------------------------------------------------------------------------------------ convolutions: d weight and d input
FILTERS = ((1, 1), (2, 2), (3, 3), (7, 7), (1, 3), (3, 2))
STRIDES = (1, 2, 3)
PADS = (0, 1, 3)
ConvCase = collections.namedtuple("ConvCase", "family B Cin H W Cout KH KW stride pad")


def conv_out(c):
    return (c.H + 2 * c.pad - c.KH) // c.stride + 1, (c.W + 2 * c.pad - c.KW) // c.stride + 1


def conv_id(c):
    return "%s-b%d-%dx%dx%d-co%d-k%dx%d-s%d-p%d" % (c.family, c.B, c.Cin, c.H, c.W, c.Cout, c.KH, c.KW, c.stride, c.pad)


def uncovered(c):
    """the input has trailing rows or columns that no window covers"""
    return (c.H + 2 * c.pad - c.KH) % c.stride != 0 or (c.W + 2 * c.pad - c.KW) % c.stride != 0


def _grid(sizes, cins, couts, families):
    """every filter x stride x pad, walking the plane sizes (the next one the filter fits), channel counts, batch sizes and families"""
    out, n = [], 0
    for (KH, KW), stride, pad in itertools.product(FILTERS, STRIDES, PADS):
        hs = [s for s in sizes if s + 2 * pad >= KH]
        ws = [s for s in sizes if s + 2 * pad >= KW]
        H, W = hs[n % len(hs)], ws[(n // 2 + 1) % len(ws)]
        out.append(ConvCase(families[n % len(families)], (1, 3)[n % 2], cins[n % len(cins)], H, W, couts[(n // 3) % len(couts)], KH, KW, stride, pad))
        n += 1
    return out


DGRAD_SIZES = (1, 2, 5, 9, 11, 13)


def _dgrad_table():
    out = _grid(DGRAD_SIZES, (1, 5, 65), (1, 3, 17), ("S", "S", "IDY", "S", "IDW"))
    out += [ConvCase("S", 3, 65, 13, 11, 17, 3, 3, 2, 1), ConvCase("IDY", 1, 65, 9, 13, 17, 3, 3, 2, 1), ConvCase("IDW", 3, 5, 11, 13, 3, 7, 7, 2, 3),
            ConvCase("S", 1, 1, 1, 1, 1, 1, 1, 1, 0), ConvCase("S", 3, 65, 1, 1, 17, 3, 3, 1, 1), ConvCase("IDY", 3, 65, 1, 1, 17, 7, 7, 2, 3),
            # K = Cout KH KW on both sides of the 16-wide K-step: 15, 16, 17 (Cout 5 and 4 are additions to the listed channel counts)
            ConvCase("S", 1, 5, 9, 5, 5, 1, 3, 1, 1), ConvCase("S", 3, 5, 5, 9, 4, 2, 2, 2, 0), ConvCase("S", 1, 65, 13, 5, 17, 1, 1, 2, 0),
            ConvCase("IDY", 1, 5, 11, 9, 5, 1, 3, 3, 1), ConvCase("IDW", 3, 1, 9, 11, 4, 2, 2, 1, 1)]
    return out


DGRAD_CASES = _dgrad_table()
WGRAD_SIZES = (2, 5, 9, 11, 13)


def _wgrad_table():
    out = _grid(WGRAD_SIZES, (1, 5, 65), (3, 65, 64, 63), ("S", "S", "IDX", "S", "IDY"))
    for fam in ("S", "IDX", "IDY"):
        out += [
            ConvCase(fam, 3, 5, 4, 4, 65, 3, 3, 3, 0),          # OH*OW = 1, a trailing row and column no window covers
            ConvCase(fam, 1, 65, 1, 33, 63, 1, 3, 1, 0),        # 31 = 1 x 31: one-row planes
            ConvCase(fam, 3, 8, 4, 8, 64, 3, 3, 1, 1),          # 32 = 4 x 8: one K-step on the 16-byte stager; Cin*9 = 72
            ConvCase(fam, 1, 5, 6, 8, 3, 2, 2, 1, 0),           # 35 = 5 x 7
            ConvCase(fam, 3, 2, 12, 12, 65, 7, 7, 2, 3),        # 36 = 6 x 6, two K-steps, the second with four indices; Cin*49 = 98
            ConvCase(fam, 1, 65, 10, 10, 5, 1, 1, 3, 3),        # 36 with pad > K/2: whole rows of the output read padding only
            ConvCase(fam, 3, 7, 24, 24, 65, 3, 3, 1, 1),        # 576 = 24 x 24: two chunks; Cin*9 = 63
            ConvCase(fam, 1, 11, 48, 47, 63, 3, 2, 2, 1),       # 576 from a rectangular filter at stride 2, uncovered trailing row; Cin*6 = 66
        ]
    out.append(ConvCase("S", 1, 1, 1, 1, 1, 1, 1, 1, 0))        # planes of one pixel
    return out


WGRAD_CASES = _wgrad_table()


def conv_references(x, w_shape, dy, w, stride, pad, x_shape):
    """fp64 (d weight from (x, dy), d input from (dy, w)) by torch.nn.grad; either may be None"""
    from torch.nn import grad as G
    dw = None if x is None else G.conv2d_weight(x.double(), tuple(w_shape), dy.double(), stride=stride, padding=pad)
    dx = None if w is None else G.conv2d_input(tuple(x_shape), w.double(), dy.double(), stride=stride, padding=pad)
    return dw, dx


@functools.lru_cache(maxsize=None)
def wgrad_case(c):
    """dict x f32[B,Cin,H,W], dy f32[B,Cout,OH,OW], ref f64[Cout,Cin,KH,KW], absum.  IDX: x coded, dy one-hot along the output pixels (one
    pixel per (b, co), walking the critical set of the plan); IDY: dy coded, x one-hot (one pixel per (b, ci))."""
    g = _gen("wgrad", c)
    OH, OW = conv_out(c)
    R = OH * OW
    xs, ys = (c.B, c.Cin, c.H, c.W), (c.B, c.Cout, OH, OW)
    if c.family == "S":
        dy, x = _nonzero_edges(small(ys, 8, g), (1, 2, 3)), _nonzero_edges(small(xs, 4, g), (1, 2, 3))
    elif c.family == "IDX":
        from deepi2p_amd import ops
        rt = ops.rc_route("wgrad", c.B, c.Cout, c.Cin * c.KH * c.KW, R, False, False)
        x = ids(xs)
        dy = one_hot(one_hot_positions(c.B, c.Cout, critical_set(R, rt["rch"], rt["chunks"]), R, g), R).view(ys)
    elif c.family == "IDY":
        dy = ids(ys)
        corners = [0, c.H * c.W - 1, c.W - 1, (c.H - 1) * c.W]
        x = one_hot(one_hot_positions(c.B, c.Cin, corners, c.H * c.W, g), c.H * c.W).view(xs)
    else:
        raise ValueError(c.family)
    ws = (c.Cout, c.Cin, c.KH, c.KW)
    ref, _ = conv_references(x, ws, dy, None, c.stride, c.pad, xs)
    absum, _ = conv_references(x.abs(), ws, dy.abs(), None, c.stride, c.pad, xs)
    return dict(x=x, dy=dy, ref=ref, absum=absum)


@functools.lru_cache(maxsize=None)
def dgrad_case(c):
    """dict dy f32[B,Cout,OH,OW], w f32[Cout,Cin,KH,KW], ref f64[B,Cin,H,W], absum.  IDY: dy coded, w one-hot (one tap of one output channel
    per input channel, walking all of them); IDW: w coded, dy one-hot (one output pixel of one channel per frame)."""
    g = _gen("dgrad", c)
    OH, OW = conv_out(c)
    xs, ys, ws = (c.B, c.Cin, c.H, c.W), (c.B, c.Cout, OH, OW), (c.Cout, c.Cin, c.KH, c.KW)
    K = c.Cout * c.KH * c.KW
    if c.family == "S":
        dy, w = _nonzero_edges(small(ys, 8, g), (1, 2, 3)), _nonzero_edges(small(ws, 4, g), (0, 1, 2, 3))
    elif c.family == "IDY":
        dy = ids(ys)
        pos = torch.tensor([[0, K - 1, min(15, K - 1), min(16, K - 1)][ci] if ci < 4 else (5 * ci + 1) % K for ci in range(c.Cin)])
        w = one_hot(pos, K).view(c.Cin, c.Cout, c.KH, c.KW).transpose(0, 1).contiguous()
    elif c.family == "IDW":
        w = ids(ws)
        n = c.Cout * OH * OW
        dy = one_hot(one_hot_positions(1, c.B, [n - 1, 0, n // 2], n, g)[0], n).view(ys)
    else:
        raise ValueError(c.family)
    _, ref = conv_references(None, ws, dy, w, c.stride, c.pad, xs)
    _, absum = conv_references(None, ws, dy.abs(), w.abs(), c.stride, c.pad, xs)
    return dict(dy=dy, w=w, ref=ref, absum=absum)


def conv_explain(c, got, coded_shape):
    if c.family == "S":
        return ""
    return " (as an id of the coded operand %s: element %s; with B > 1 the weight gradient sums one id per frame)" % (coded_shape, decode(got, coded_shape))


# ------------------------------------------------------------------------------------------------ di2p_gather_backward
GatherCase = collections.namedtuple("GatherCase", "family mode B C J M pattern")       # mode: "k1", "k1w", "k3w"
GATHER_M = (1, 63, 64, 65, 130)
GATHER_C = (1, 65)
GATHER_J = (1, 31, 33, 515, 2305)
GATHER_PATTERNS = ("random", "one", "perm", "dup2", "dup3")


def _gather_table():
    out, n = [], 0
    for mode in ("k1", "k1w", "k3w"):
        patterns = GATHER_PATTERNS if mode == "k3w" else GATHER_PATTERNS[:3]
        for i, J in enumerate(GATHER_J):
            for v, pattern in enumerate(patterns):
                out.append(GatherCase("S", mode, (1, 3)[n % 2], GATHER_C[(n // 2) % 2], J, GATHER_M[(i + v + n // 7) % 5], pattern))
                n += 1
    # identity-coded dy through the plain gather: every critical j goes to a node of its own, every other j to the last node (C = 3 is an
    # addition: the last node's sum of ids stays below 2^24)
    for J in (33, 515, 2305):
        for C, M in ((1, 130), (3, 65)):
            out.append(GatherCase("ID", "k1", 1, C, J, M, "critical"))
    return out


GATHER_CASES = _gather_table()


def gather_id(c):
    return "%s-%s-b%d-c%d-j%d-m%d-%s" % (c.family, c.mode, c.B, c.C, c.J, c.M, c.pattern)


def gather_reference(dy, idx, w, M):
    """fp64 index_add: out[b,c,m] = sum_j dy[b,c,j] sum_k w[b,j,k] [idx[b,j,k] == m]; and the sum of absolute products"""
    B, C, J = dy.shape
    ref, absum = torch.zeros(B, C, M, dtype=torch.float64), torch.zeros(B, C, M, dtype=torch.float64)
    for b in range(B):
        for k in range(idx.shape[2]):
            wk = torch.ones(J, dtype=torch.float64) if w is None else w[b, :, k].double()
            ref[b].index_add_(1, idx[b, :, k].long(), dy[b].double() * wk)
            absum[b].index_add_(1, idx[b, :, k].long(), dy[b].double().abs() * wk.abs())
    return ref, absum


@functools.lru_cache(maxsize=None)
def gather_case(c):
    """dict dy f32[B,C,J], idx i32[B,J,k], w f32[B,J,k] | None, k, ref f64[B,C,M], absum, unreferenced bool[B,M]"""
    g = _gen("gather", c)
    B, C, J, M = c.B, c.C, c.J, c.M
    k = 3 if c.mode == "k3w" else 1
    # nodes nobody references: the first and the middle one, where there are at least three
    allowed = torch.tensor([m for m in range(M) if M < 3 or m not in (0, M // 2)])
    if c.pattern == "critical":
        from deepi2p_amd import ops
        rt = ops.rc_route("gather", B, C, M, J, False, False)
        crit = critical_set(J, rt["rch"], rt["chunks"])
        assert len(crit) < M - 1
        idx = torch.full((B, J, 1), M - 1, dtype=torch.int64)
        for n, j in enumerate(crit):
            idx[:, j, 0] = 1 + n                       # node 0 stays unreferenced
    elif c.pattern == "one":
        idx = torch.full((B, J, k), M - 1, dtype=torch.int64)
    elif c.pattern == "perm":
        perm = torch.stack([allowed[torch.randperm(len(allowed), generator=g)] for _ in range(B)])          # [B, len(allowed)]
        idx = torch.stack([perm[:, (torch.arange(J) + kk) % perm.shape[1]] for kk in range(k)], dim=2)
    else:
        idx = allowed[torch.randint(0, len(allowed), (B, J, k), generator=g)]
        if c.pattern == "dup2":
            idx[:, :, 2] = idx[:, :, 0]
        elif c.pattern == "dup3":
            idx[:, :, 1] = idx[:, :, 0]
            idx[:, :, 2] = idx[:, :, 0]
    w = None
    if c.mode != "k1":
        w = small((B, J, k), 3, g)                     # zero and negative weights included
        w[:, J - 1, :] = torch.tensor([2.0, -1.0, 3.0][:k])
    dy = ids((B, C, J)) if c.family == "ID" else _nonzero_edges(small((B, C, J), 8, g), (1, 2))
    ref, absum = gather_reference(dy, idx, w, M)
    unref = torch.ones(B, M, dtype=torch.bool)
    for b in range(B):
        unref[b, idx[b].reshape(-1)] = False
    return dict(dy=dy, idx=idx.to(torch.int32), w=w, k=k, ref=ref, absum=absum, unreferenced=unref)


# ------------------------------------------------------------------------------------------------ di2p_channel_sum
SumCase = collections.namedtuple("SumCase", "family B C N")          # family "S", "dyadic" or "wide"
SUM_N = (1, 255, 256, 257, 4095, 8192, 8193, 70001)
SUM_BITS = {"dyadic": 16, "wide": 24}
SUM_CASES = [SumCase(f, B, C, N) for f in ("S", "dyadic", "wide") for N in SUM_N for B in (1, 3) for C in (1, 64, 65)]


def sum_id(c):
    return "%s-b%d-c%d-n%d" % c


def sum_case(c):
    """(x f32[B,C,N], ref f32[C] = the fp64 sum rounded once).  dyadic: x = k / 256 with |k| < 2^16 -- every fp64 partial sum is an exact
    multiple of 2^-8 below 2^27, so the fp64 sum is exact in any order, while an fp32 sum over the channel would round.  wide: |k| < 2^24, the
    whole fp32 significand -- still exact in fp64 (below 2^34), but already the sum of two values needs 25 bits: a single fp32 addition
    anywhere, even in a per-thread chain of a few elements (which the 17 bits of `dyadic` survive), rounds."""
    g = _gen("sum", c)
    if c.family == "S":
        x = _nonzero_edges(small((c.B, c.C, c.N), 8, g), (0, 2))
    else:
        lim = 1 << SUM_BITS[c.family]
        x = torch.randint(-lim + 1, lim, (c.B, c.C, c.N), generator=g).to(torch.float32) / 256.0
    return x, x.double().sum((0, 2)).float()
