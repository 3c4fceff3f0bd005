"""Operands and fp64 references for the kernels of the training step that are NOT matrix products: train-mode BatchNorm (forward and backward),
the 3x3/2 max-pool and its backward, the arg-max routers, the dropout mask application, the classifier loss, Adam, and two neighbours
(index_max on its split path with a ragged N, the global average pool).  Generators and references only: seeded, CPU, no GPU code.
tests/test_train_pointwise_cases_host.py proves the premises stated here; tests/test_gpu_train_pointwise_exact.py runs the kernels.

BatchNorm.  x = k / 256 with |k| < 2^12.  Then sum x is a multiple of 2^-8 below 2^(12 + 18 - 8) and sum x^2 a multiple of 2^-16 below
2^(24 + 18 - 16) for up to 2^18 values per channel: every fp64 partial sum, in any order and any chunking, is exact, and so is the batch mean's
numerator.  The backward entry point takes save_mean and save_invstd as operands: mean = j / 256 and invstd a power of two make
xhat = (x - mean) * invstd exact in fp32 (a multiple of 2^-10 below 2^6), g * xhat exact in fp64 and every partial sum of it exact.
Every (b, c) row carries sentinels of magnitude >= 8 at the positions where a chunked, 256-strided reduction can lose or double an element
(`critical_positions`): 0, N - 1, both sides of every chunk boundary of the plan (`red_plan`, restated from csrc/train.hip and checked against
di2p_channel_reduce_workspace_bytes by the host test), and 255 / 256.
"""
import collections

import numpy as np
import torch

from tests.x3_exact_cases import first_mismatch, seed_of  # noqa: F401  (re-exported for the tests)

NAN = float("nan")
U32 = 2.0 ** -24                       # unit roundoff of fp32
NAN_PAYLOAD_BITS = 0x7FC01234          # the NaN that operands carry: not the NaN the output buffers are filled with


def _gen(*what):
    return torch.Generator().manual_seed(seed_of(*what))


def payload_nan():
    return torch.tensor([NAN_PAYLOAD_BITS], dtype=torch.int32).view(torch.float32)[0]


def ints(shape, lim, g):
    """integers in [-lim, lim] as f32"""
    return torch.randint(-lim, lim + 1, tuple(shape), generator=g).to(torch.float32)


def dyadic(shape, g, bits=12):
    """k / 256 with |k| < 2^bits"""
    lim = 1 << bits
    return torch.randint(-lim + 1, lim, tuple(shape), generator=g).to(torch.float32) / 256.0


def sentinels(shape, g):
    """+-(2048 + r) / 256 with 0 <= r < 2048: magnitude in [8, 16), still k / 256 with |k| < 2^12"""
    mag = (2048 + torch.randint(0, 2048, tuple(shape), generator=g)).to(torch.float32) / 256.0
    return mag * (torch.randint(0, 2, tuple(shape), generator=g).to(torch.float32) * 2 - 1)


def within_one_ulp(got, ref64):
    """got f32 equals the fp64 reference rounded to fp32, or the float next to it"""
    r = ref64.to(torch.float32)
    inf = torch.full_like(r, float("inf"))
    return (got == r) | (got == torch.nextafter(r, inf)) | (got == torch.nextafter(r, -inf))


# ------------------------------------------------------------------------------------------------ the chunk plan of the channel reductions
def red_plan(B, C, N):
    """(SN chunks per row, elements per chunk, S = B * SN partial pairs per channel, workspace bytes): csrc/train.hip red_plan"""
    SN = min(max(N // 4096, 1), 16)
    per = -(-N // SN)
    SN = -(-N // per)
    S = B * SN
    return SN, per, S, C * S * 16 + C * 8


def critical_positions(N):
    SN, per, _, _ = red_plan(1, 1, N)
    crit = {0, N - 1, 255, 256}
    for c in range(1, SN):
        crit.update((c * per - 1, c * per))
    return sorted(p for p in crit if 0 <= p < N)


# ------------------------------------------------------------------------------------------------ BatchNorm
BnCase = collections.namedtuple("BnCase", "B C N flags")          # flags: three bits, read by bn_forward_flags / bn_backward_flags
BN_N = (1, 2, 255, 256, 257, 4095, 4096, 8191, 8193, 12289, 65537, 70001)
_BN_BC = ((1, 1), (3, 64), (1, 65), (3, 1), (1, 64), (3, 65))
BN_MOMENTUM, BN_EPS = 0.1, 1e-5


def _bn_table():
    """every N with one B = 1 and one B = 3 shape, the channel counts rotating (the full product of the issue's sets, thinned: every (B, C) pair
    meets a single-chunk, a two-chunk and a many-chunk N); N = 1 needs two values per channel, so B = 2; the two largest N keep B * C small"""
    out = []
    for i, N in enumerate(BN_N):
        pairs = (_BN_BC[(2 * i) % 6], _BN_BC[(2 * i + 1) % 6])
        if N == 1:
            pairs = ((2, 1), (2, 65))
        elif N == 65537:
            pairs = ((1, 65), (3, 1))
        elif N == 70001:
            pairs = ((1, 64), (3, 1))
        for t, (B, C) in enumerate(pairs):
            out.append(BnCase(B, C, N, (3 * i + 5 * t) % 8))
    return out


BN_CASES = _bn_table()


def bn_id(c):
    return "b%d-c%d-n%d-f%d" % c


def bn_forward_flags(c):
    return dict(residual=bool(c.flags & 1), relu=bool(c.flags & 2), running=bool(c.flags & 4))


def bn_backward_flags(c):
    """relu: g = dy * [y > 0]; dres: the residual gradient is asked for; y_null: with relu off, y is NULL (otherwise a NaN-filled buffer)"""
    return dict(relu=bool(c.flags & 1), dres=bool(c.flags & 2), y_null=bool(c.flags & 4) and not c.flags & 1)


def _plant(t, g):
    """sentinels at the critical positions of every row of t f32[B, C, N]"""
    crit = critical_positions(t.shape[2])
    t[:, :, crit] = sentinels((t.shape[0], t.shape[1], len(crit)), g)
    return crit


def bn_forward_case(c):
    """operands and the fp64 statistics.  sum0 / sum1 (f64[C]) are the exact sums of x and x^2."""
    f = bn_forward_flags(c)
    g = _gen("bn_fwd", c)
    x = dyadic((c.B, c.C, c.N), g)
    crit = _plant(x, g)
    gamma, beta = torch.randn(c.C, generator=g), torch.randn(c.C, generator=g)
    res = torch.randn(c.B, c.C, c.N, generator=g) if f["residual"] else None
    rm0 = dyadic((c.C,), g) if f["running"] else None
    rv0 = dyadic((c.C,), g).abs() + 0.5 if f["running"] else None
    count = float(c.B * c.N)
    xd = x.double()
    s0, s1 = xd.sum((0, 2)), (xd * xd).sum((0, 2))
    mu = s0 / count
    var = (s1 / count - mu * mu).clamp_min(0.0)
    eps, mom = float(np.float32(BN_EPS)), float(np.float32(BN_MOMENTUM))
    invstd = 1.0 / torch.sqrt(var + eps)
    out = dict(x=x, gamma=gamma, beta=beta, res=res, rm0=rm0, rv0=rv0, crit=crit, count=count, sum0=s0, sum1=s1, mean=mu, invstd=invstd)
    if f["running"]:
        unb = var * count / (count - 1.0) if count > 1.0 else var
        out["rm"] = (1.0 - mom) * rm0.double() + mom * mu
        out["rv"] = (1.0 - mom) * rv0.double() + mom * unb
    return out


def bn_forward_y(case, relu, mean32, invstd32):
    """(y in fp64 from the statistics the device saved, the bound on |y - that|): 4 * 2^-24 * (|x - mean| invstd |gamma| + |beta| + |res|).
    The kernel rounds the difference, the two products and the sum with beta (or, contracted, the difference, one product and the fused
    multiply-add) and the sum with the residual: each rounding errs by at most 2^-24 of its own result.  ReLU is 1-Lipschitz."""
    xd = case["x"].double()
    d = xd - mean32.double()[None, :, None]
    prod = d * invstd32.double()[None, :, None] * case["gamma"].double()[None, :, None]
    y = prod + case["beta"].double()[None, :, None]
    mag = prod.abs() + case["beta"].double().abs()[None, :, None]
    if case["res"] is not None:
        y = y + case["res"].double()
        mag = mag + case["res"].double().abs()
    if relu:
        y = y.clamp_min(0.0)
    return y, 4.0 * U32 * mag


# y of the backward call: the forward output, of which only the sign matters (g = dy where y > 0).  20 equally likely values:
# positives (one tiny, one subnormal), both zeros, negatives, NaN
_Y_TABLE = [1.0, 2.5, 1.0, 0.125, 3.0, 1.0, 7.0, 1e-30, 1e-45, 0.0, 0.0, 0.0, -0.0, -0.0, -1.0, -2.5, -1e-30, -1e-45, NAN, NAN]


def bn_backward_case(c):
    f = bn_backward_flags(c)
    g = _gen("bn_bwd", c)
    x, dy = dyadic((c.B, c.C, c.N), g), dyadic((c.B, c.C, c.N), g)
    mean = torch.randint(-256, 257, (c.C,), generator=g).to(torch.float32) / 256.0
    invstd = torch.tensor([0.25, 0.5, 1.0, 2.0])[torch.randint(0, 4, (c.C,), generator=g)]
    gamma = torch.randn(c.C, generator=g)
    y = torch.tensor(_Y_TABLE)[torch.randint(0, len(_Y_TABLE), (c.B, c.C, c.N), generator=g)]
    crit = _plant(x, g)                  # |x - mean| >= 7 there, so |xhat| >= 1.75
    _plant(dy, g)
    y[:, :, crit] = 1.0                  # and the sentinel counts whatever relu says
    keep = (y > 0) if f["relu"] else torch.ones_like(y, dtype=torch.bool)
    gg = torch.where(keep, dy, torch.zeros(()))
    xhat = (x - mean[None, :, None]) * invstd[None, :, None]            # fp32, exact (host test)
    count = float(c.B * c.N)
    t0, t1 = gg.double(), gg.double() * xhat.double()
    a0, a1 = t0.sum((0, 2)), t1.sum((0, 2))
    m0, m1 = (a0 / count).float(), (a1 / count).float()
    gi = (gamma * invstd).double()[None, :, None]
    dx = gi * (gg.double() - m0.double()[None, :, None] - xhat.double() * m1.double()[None, :, None])
    bound = 5.0 * U32 * gi.abs() * (gg.double().abs() + m0.double().abs()[None, :, None] + (xhat.double() * m1.double()[None, :, None]).abs())
    return dict(x=x, dy=dy, y=y, gamma=gamma, mean=mean, invstd=invstd, crit=crit, count=count, g=gg, xhat=xhat, a0=a0, a1=a1, term0=t0, term1=t1,
                dbeta=a0.float(), dgamma=a1.float(), dx=dx, bound=bound, keep=keep)


# ------------------------------------------------------------------------------------------------ max-pool 3x3 / stride 2 / pad 1
PoolCase = collections.namedtuple("PoolCase", "B C H W xoff yoff")          # offsets of the x and y pointers in floats
POOL_FWD_CASES = ([PoolCase(2, 3, H, W, 0, 0) for H, W in ((1, 8), (5, 8), (7, 16), (33, 64))]                  # the four-outputs-per-lane kernel
                  + [PoolCase(2, 3, 5, 8, 1, 0), PoolCase(2, 3, 7, 16, 0, 1), PoolCase(2, 3, 33, 64, 1, 1)]       # W % 8 == 0 but misaligned: scalar
                  + [PoolCase(2, 3, H, W, 0, 0) for H, W in ((1, 1), (2, 2), (6, 2), (9, 7), (33, 65))])


def pool_id(c):
    return "b%d-c%d-%dx%d-x%d-y%d" % c


def pool_out(H, W):
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


def pool_forward_uses_vec4(c):
    """di2p_maxpool3x3s2's choice: four outputs per lane when W % 8 == 0 and both pointers are 16-byte aligned"""
    return c.W % 8 == 0 and c.xoff % 4 == 0 and c.yoff % 4 == 0


def pool_forward_case(c):
    """plane 0 random, 1 all negative, 2 all -inf, 3 all equal, the rest random; the reference is torch's own max_pool2d on the CPU"""
    g = _gen("pool_fwd", c)
    x = torch.randn(c.B * c.C, c.H, c.W, generator=g)
    x[1] = -x[1].abs() - 0.5
    x[2] = float("-inf")
    x[3] = 1.25
    x = x.view(c.B, c.C, c.H, c.W)
    return x, torch.nn.functional.max_pool2d(x, 3, 2, 1)


POOL_LDS_MAX_W = 1213          # the widest plane whose 11 input rows and 5 window rows fit 64 KiB of LDS
POOL_BWD_CASES = ([PoolCase(2, 3, H, W, 0, 0) for H, W in ((1, 1), (2, 2), (7, 9), (8, 33), (9, 7), (33, 64), (8, 600))]
                  + [PoolCase(1, 2, 9, POOL_LDS_MAX_W, 0, 0), PoolCase(1, 2, 9, POOL_LDS_MAX_W + 1, 0, 0)]
                  + [PoolCase(1, 65535, 2, 2, 0, 0), PoolCase(1, 65536, 2, 2, 0, 0)])


def maxpool_uses_lds(shape):
    """di2p_maxpool3x3s2_backward's choice, as tests/test_gpu_training_shapes.py::_maxpool_uses_lds states it"""
    B, C, H, W = shape
    OW = (W - 1) // 2 + 1
    return (11 * W + 5 * OW) * 4 <= 64 * 1024 and B * C <= 65535


def pool_backward_case(c):
    """x in {0, 1, 2} (most windows hold their maximum several times: the FIRST one in scan order takes the gradient), dy integers in [-8, 8]
    without zeros (an input pixel is the arg-max of at most four windows: the sums are exact); the reference is torch's fp64 autograd"""
    g = _gen("pool_bwd", c)
    x = torch.randint(0, 3, (c.B, c.C, c.H, c.W), generator=g).to(torch.float32)
    OH, OW = pool_out(c.H, c.W)
    dy = ints((c.B, c.C, OH, OW), 8, g)
    dy[dy == 0] = 3.0
    xd = x.double().requires_grad_(True)
    torch.nn.functional.max_pool2d(xd, 3, 2, 1).backward(dy.double())
    return x, dy, xd.grad.float()


# ------------------------------------------------------------------------------------------------ arg-max routers
GroupCase = collections.namedtuple("GroupCase", "rows K")
GROUP_CASES = [GroupCase(r, K) for r in (1, 255, 256, 257) for K in (1, 2, 16, 17)]


def group_id(c):
    return "r%d-k%d" % c


def group_case(c):
    """x: integers in [-2, 2] (ties), a tenth -inf, a twentieth NaN; row 1 all -inf, row 2 all NaN, row 3 all equal.  arg: np.argmax -- the
    first maximum, and the first NaN if there is one.  y = x[arg] bit for bit; the backward puts dy (non-zero integers) at arg, +0 elsewhere."""
    g = _gen("group", c)
    x = ints((c.rows, c.K), 2, g)
    r = torch.rand(c.rows, c.K, generator=g)
    x[r < 0.10] = float("-inf")
    x[r > 0.95] = payload_nan()
    if c.rows > 3:
        x[1] = float("-inf")
        x[2] = payload_nan()
        x[3] = -1.0
    arg = torch.from_numpy(np.argmax(x.numpy(), axis=1).astype(np.int32))
    y = x.gather(1, arg.long()[:, None])[:, 0]
    dy = ints((c.rows,), 8, g)
    dy[dy == 0] = 5.0
    dx = torch.zeros(c.rows, c.K)
    dx.scatter_(1, arg.long()[:, None], dy[:, None])
    return dict(x=x, arg=arg, y=y, dy=dy, dx=dx)


SegCase = collections.namedtuple("SegCase", "M C mask pattern")          # mask "binary" | "half" | "none"; pattern "distinct" | "dup"
SEG_B = 2
SEG_CASES = [SegCase(M, C, m, p) for M in (1, 127, 128, 129) for C in (1, 65) for m in ("binary", "half", "none") for p in ("distinct", "dup")]


def seg_id(c):
    return "m%d-c%d-%s-%s" % c


def seg_case(c):
    """dx[b, c, max_idx[b, c, m]] += dv[b, c, m] * mask[b, m] over N = 2 M + 1 points.  dv: non-zero integers in [-8, 8]; indices distinct per
    (b, c) row, or drawn from a few values so that several m add into one element (integer or half-integer sums below 2^24: exact in any order);
    positions 0 and M - 1 and a tenth of the rest alternate between -1 and N, which the kernel must ignore."""
    g = _gen("seg", c)
    B, N = SEG_B, 2 * c.M + 1
    dv = ints((B, c.C, c.M), 8, g)
    dv[dv == 0] = 2.0
    if c.pattern == "distinct":
        idx = torch.stack([torch.randperm(N, generator=g)[:c.M] for _ in range(B * c.C)]).view(B, c.C, c.M)
    else:
        idx = torch.randint(0, max(1, c.M // 4), (B, c.C, c.M), generator=g)
    oob = torch.rand(B, c.C, c.M, generator=g) < 0.1
    oob[:, :, 0] = True
    oob[:, :, c.M - 1] = True
    if c.M == 1:
        oob[0] = False                                   # with one node per row, frame 0 keeps its index and frame 1 loses it
    which = torch.where((torch.arange(c.M)[None, None, :] + torch.arange(c.C)[None, :, None]) % 2 == 0, -1, N)
    idx = torch.where(oob, which.expand(B, c.C, c.M), idx).to(torch.int32)
    mask = None
    if c.mask != "none":
        mask = (torch.rand(B, c.M, generator=g) < 0.7).to(torch.float32) * (1.0 if c.mask == "binary" else 0.5)
        if c.mask == "half" and c.M > 1:
            mask[:, 1] = 1.0
    w = torch.ones(B, 1, c.M) if mask is None else mask[:, None, :]
    ref = np.zeros((B, c.C, N))
    contrib = (dv.double() * w.double()).numpy()
    ok = ((idx >= 0) & (idx < N)).numpy()
    bi, ci, mi = np.nonzero(ok)
    np.add.at(ref, (bi, ci, idx.numpy()[bi, ci, mi]), contrib[bi, ci, mi])
    absum = np.zeros((B, c.C, N))
    np.add.at(absum, (bi, ci, idx.numpy()[bi, ci, mi]), np.abs(contrib[bi, ci, mi]))
    referenced = np.zeros((B, c.C, N), dtype=bool)
    live = ok & (w.expand(B, c.C, c.M).numpy() != 0)
    bi, ci, mi = np.nonzero(live)
    referenced[bi, ci, idx.numpy()[bi, ci, mi]] = True
    return dict(dv=dv, idx=idx, mask=mask, N=N, ref=torch.from_numpy(ref).float(), absum=float(absum.max()), unreferenced=torch.from_numpy(~referenced))


# ------------------------------------------------------------------------------------------------ di2p_apply_mask
MaskCase = collections.namedtuple("MaskCase", "n align")
MASK_ALIGN = {"aligned": (0, 0, 0), "x4": (4, 0, 0), "y4": (0, 4, 0), "m1": (0, 0, 1), "m4": (0, 0, 4)}          # byte offsets of x, y, mask
MASK_CASES = [MaskCase(n, a) for n in (1, 7, 8, 9, 2048, 2055, 2056) for a in MASK_ALIGN]
MASK_SCALE = float(np.float32(1.0) / np.float32(0.7))


def mask_id(c):
    return "n%d-%s" % c


def apply_mask_uses_vec8(c):
    """di2p_apply_mask's choice: eight per thread when n % 8 == 0, x and y are 16-byte and the mask 8-byte aligned"""
    xo, yo, mo = MASK_ALIGN[c.align]
    return c.n % 8 == 0 and xo % 16 == 0 and yo % 16 == 0 and mo % 8 == 0


def apply_mask_case(c):
    """mask bytes from {0, 1, 2, 255} (the first eight fixed: every byte lane of the 8-byte mask word differs from its neighbour); x random
    with inf under any byte and NaN under zero bytes only; y = x * scale as numpy's fp32 multiply gives it, exactly 0 where the byte is 0"""
    g = _gen("mask", c)
    mask = torch.tensor([0, 1, 2, 255], dtype=torch.uint8)[torch.randint(0, 4, (c.n,), generator=g)]
    mask[:8] = torch.tensor([1, 0, 2, 0, 255, 0, 0, 1], dtype=torch.uint8)[:c.n]
    x = torch.randn(c.n, generator=g)
    r = torch.rand(c.n, generator=g)
    x[r < 0.1] = float("inf")
    x[(r > 0.8) & (mask == 0)] = NAN
    if c.n > 1:
        x[1] = NAN
    with np.errstate(invalid="ignore"):
        ref = np.where(mask.numpy() != 0, x.numpy() * np.float32(MASK_SCALE), np.float32(0.0)).astype(np.float32)
    return x, mask, torch.from_numpy(ref)


# ------------------------------------------------------------------------------------------------ di2p_classifier_loss
LossCase = collections.namedtuple("LossCase", "B N L scenario variant")
LOSS_SCENARIOS = ("mixed", "none_inside", "all_inside", "ties", "gaps", "big_fine")
LOSS_VARIANTS = ("full", "no_fine", "no_dfine", "no_dcoarse")
LOSS_ALPHA, LOSS_GAMMA, LOSS_COARSE_ALPHA = 0.5, 2.0, 50.0
LOSS_TOL = 1e-5


def _loss_table():
    out, j = [], 0
    for N in (1, 255, 256, 257, 700):
        for B in (1, 3):
            for L in (1, 2, 80):
                out.append(LossCase(B, N, L, LOSS_SCENARIOS[j % 6], LOSS_VARIANTS[(j // 2) % 4]))
                j += 1
    for s in LOSS_SCENARIOS:                      # every scenario with every output asked for, on a ragged last block and on a third block
        out.append(LossCase(3, 257, 80, s, "full"))
        out.append(LossCase(1, 700, 2, s, "full"))
    return list(dict.fromkeys(out))


LOSS_CASES = _loss_table()


def loss_id(c):
    return "b%d-n%d-l%d-%s-%s" % c


def loss_critical(N):
    return sorted({p for p in (0, 255, 256, N - 1) if 0 <= p < N})


def loss_case(c):
    """scores and labels.  Points 0, 255, 256 and N - 1 of every frame are confidently wrong in both heads (coarse gap 20 against the label,
    fine gap 20 for another class), so each of them carries a large share of the loss (`loss_without_point`)."""
    g = _gen("loss", c)
    B, N, L = c.B, c.N, c.L
    coarse = torch.randn(B, 2, N, generator=g) * 2.0
    fine = torch.randn(B, L, N, generator=g) * 2.0
    clab = torch.randint(0, 2, (B, N), generator=g)
    flab = torch.randint(0, L, (B, N), generator=g)
    if c.scenario == "none_inside":
        clab[:] = 0
    elif c.scenario == "all_inside":
        clab[:] = 1
    elif c.scenario == "ties":
        t = torch.rand(B, N, generator=g) < 0.25
        coarse[:, 1][t] = coarse[:, 0][t]                                   # x0 == x1: class 0 is predicted
        if L > 1:                                                           # two classes share the maximum: the first is predicted
            top = fine.max(1).values
            a, b = torch.randint(0, L, (B, N), generator=g), torch.randint(0, L, (B, N), generator=g)
            fine.scatter_(1, a[:, None], top[:, None])
            fine.scatter_(1, b[:, None], top[:, None])
    elif c.scenario == "gaps":
        t = torch.rand(B, N, generator=g)
        coarse[:, 0][t < 0.1] += 100.0
        coarse[:, 1][t > 0.9] += 100.0
    elif c.scenario == "big_fine":
        fine += 1e4
    crit = loss_critical(N)
    for p in crit:
        wrong = 1 - clab[:, p]
        coarse[:, :, p] = 0.0
        coarse[torch.arange(B), wrong, p] = 20.0
        if L > 1:
            other = (flab[:, p] + 1) % L
            base = 1e4 if c.scenario == "big_fine" else 0.0
            fine[:, :, p] = base
            fine[torch.arange(B), other, p] = base + 20.0
    return dict(coarse=coarse, fine=fine, clab=clab.to(torch.int32), flab=flab.to(torch.int32), crit=crit)


def loss_reference(case, with_fine=True, keep=None):
    """oracle/losses_torch in fp64 with autograd.  keep (bool [B, N], optional): the points whose terms reach the sums -- a point that is not
    kept is lost the way a kernel loses it: its focal term is missing from the sum over B * N, its fine term and its count from the fine mean.
    -> dict(out = the six numbers, d_coarse, d_fine)"""
    from oracle import losses_torch as lt
    coarse = case["coarse"].double().requires_grad_(True)
    fine = case["fine"].double().requires_grad_(True)
    clab, flab = case["clab"].long(), case["flab"].long()
    B, _, N = coarse.shape
    L = fine.shape[1]
    if keep is None:
        cl = lt.focal_loss(coarse, clab, LOSS_ALPHA, LOSS_GAMMA) * LOSS_COARSE_ALPHA
        keep = torch.ones(B, N, dtype=torch.bool)
    else:
        p = torch.softmax(coarse, 1) + 1e-6
        h = torch.zeros_like(coarse).scatter_(1, clab.unsqueeze(1), 1.0) + 1e-6
        per_point = (h * (-LOSS_ALPHA * torch.pow(-p + 1.0, LOSS_GAMMA) * torch.log(p))).sum(1)
        cl = (per_point * keep).sum() / (B * N) * LOSS_COARSE_ALPHA
    correct = float((((coarse[:, 1] > coarse[:, 0]).long() == clab) & keep).sum())
    inside = ((clab == 1) & keep).reshape(B * N)
    cnt = float(inside.sum())
    out = [None, float(cl.detach()), 0.0, np.float64(correct) / np.float64(B * N), 0.0, cnt if with_fine else 0.0]      # no fine head: nothing is counted
    d_coarse, = torch.autograd.grad(cl, coarse)
    d_fine = torch.zeros_like(fine)
    if with_fine:
        fs = fine.permute(0, 2, 1).reshape(B * N, L)[inside]
        fl_lab = flab.reshape(B * N)[inside]
        with np.errstate(invalid="ignore", divide="ignore"):
            out[4] = np.float64(float((fs.argmax(1) == fl_lab).sum())) / np.float64(cnt)
        if cnt > 0:
            fl = torch.nn.functional.cross_entropy(fs, fl_lab)
            d_fine, = torch.autograd.grad(fl, fine)
            out[2] = float(fl.detach())
        else:
            out[2] = NAN
    out[0] = out[1] + out[2]
    return dict(out=np.array(out, dtype=np.float64), d_coarse=d_coarse.detach(), d_fine=d_fine.detach())


# ------------------------------------------------------------------------------------------------ di2p_adam_step
AdamCase = collections.namedtuple("AdamCase", "n step")
ADAM_CASES = [AdamCase(n, s) for n in (1, 255, 256, 257) for s in (1, 10000)]
ADAM_LR, ADAM_B1, ADAM_B2, ADAM_EPS = 1e-3, 0.9, 0.999, 1e-8
ADAM_TOL = 2e-6                   # of the abs-max: tests/test_training.py::test_hip_adam_matches_torch


def adam_id(c):
    return "n%d-step%d" % c


def adam_case(c):
    """one torch.optim.Adam step (weight_decay 0, amsgrad off) in fp64 on the fp32 hyper-parameters the kernel receives"""
    g = _gen("adam", c)
    p, gr, m = torch.randn(c.n, generator=g), torch.randn(c.n, generator=g), torch.randn(c.n, generator=g) * 0.1
    v = torch.rand(c.n, generator=g) * 0.01
    lr, b1, b2, eps = (float(np.float32(h)) for h in (ADAM_LR, ADAM_B1, ADAM_B2, ADAM_EPS))
    m1 = b1 * m.double() + (1.0 - b1) * gr.double()
    v1 = b2 * v.double() + (1.0 - b2) * gr.double() ** 2
    bc1, bc2 = 1.0 - b1 ** c.step, 1.0 - b2 ** c.step
    p1 = p.double() - (lr / bc1) * (m1 / (v1.sqrt() / bc2 ** 0.5 + eps))
    return dict(p=p, g=gr, m=m, v=v, p1=p1, m1=m1, v1=v1)


# ------------------------------------------------------------------------------------------------ index_max, split path, ragged N
ImaxCase = collections.namedtuple("ImaxCase", "B C N K")
IMAX_CASES = [ImaxCase(1, 3, 4099, 5), ImaxCase(1, 1, 8191, 9), ImaxCase(2, 2, 4098, 130)]


def imax_id(c):
    return "b%d-c%d-n%d-k%d" % c


def imax_slices(c):
    """(S, slice): how di2p_index_max_* splits N when it is given a workspace (csrc/index_max.hip launch)"""
    S = 1
    while c.B * c.C * S < 1024 and c.N // (S * 2) >= 2048:
        S *= 2
    return S, ((c.N + S - 1) // S + 3) & ~3


def imax_case(c):
    """data: integers in [-3, 3] (ties: the first n wins), some at or under the floor of -1000, some NaN; clusters K - 1 (and K - 2 when
    K > 2) are empty, cluster 0 holds only values under the floor.  The maxima of the whole row sit on both sides of every slice boundary and at
    N - 1.  -> data, index, mask, max_idx (oracle/ops_np.index_max_forward), the values with and without the mask"""
    from oracle import ops_np
    g = _gen("imax", c)
    used = max(1, c.K - 2) if c.K > 2 else max(1, c.K - 1)
    data = ints((c.B, c.C, c.N), 3, g)
    r = torch.rand(c.B, c.C, c.N, generator=g)
    data[r < 0.05] = -1000.0
    data[(r >= 0.05) & (r < 0.08)] = -2000.0
    data[r > 0.97] = NAN
    index = torch.randint(1 if used > 1 else 0, used, (c.B, c.N), generator=g)
    S, sl = imax_slices(c)
    edges = sorted({c.N - 1} | {p for s in range(1, S) for p in (s * sl - 1, s * sl) if p < c.N})
    for i, p in enumerate(edges):
        data[:, :, p] = 4.0 + (i % 2)
    if used > 1:                                   # cluster 0: a few points, all under the floor
        under = torch.arange(7, c.N, 501)
        index[:, under] = 0
        data[:, :, under] = -1000.0
    data[:, :, 0] = 1.0
    index = index.to(torch.int32)
    mask = (torch.rand(c.B, c.K, generator=g) < 0.8).to(torch.float32)
    d, ix = data.numpy(), index.numpy()
    idx = ops_np.index_max_forward(d, ix, c.K)
    none = np.ones((c.B, c.C, c.K), dtype=bool)
    for b in range(c.B):
        for k in range(c.K):
            members = d[b][:, ix[b] == k]
            none[b, :, k] = ~(members > np.float32(-1000.0)).any(axis=1) if members.shape[1] else True
    picked = np.take_along_axis(d, idx.astype(np.int64), axis=2)
    val_mask = picked * mask.numpy()[:, None, :]
    val_nomask = picked * np.where(none, np.float32(0.0), np.float32(1.0))
    return dict(data=data, index=index, mask=mask, idx=torch.from_numpy(idx), val_mask=torch.from_numpy(val_mask.astype(np.float32)),
                val_nomask=torch.from_numpy(val_nomask.astype(np.float32)), none=none, edges=edges)


# ------------------------------------------------------------------------------------------------ di2p_global_avgpool
AVG_HW = (1, 63, 64, 65, 80, 2560)
AVG_ROWS = ((1, 5), (2, 4))          # (B, C): five rows leave the last workgroup of four ragged


def avgpool_case(B, C, HW):
    """integers in [-8, 8]: every fp32 partial sum is an integer below 2^24, so the sum is exact in any order and the mean is one division"""
    x = ints((B, C, HW), 8, _gen("avg", B, C, HW))
    x[:, :, HW - 1] = 7.0
    ref = (x.double().sum(2).float().numpy() / np.float32(HW)).astype(np.float32)
    return x, torch.from_numpy(ref)
