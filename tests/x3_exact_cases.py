"""Operands for which the bf16x3 arithmetic is EXACT (generators only: seeded, CPU, no GPU code).

The premise (csrc/bf16x3.h, tools/probe_mfma_rounding.hip): the bf16 matrix instructions align every product to the largest addend and truncate
below ITS last bit.  If every operand is an integer and every partial sum of every accumulator is an integer below 2^24, no bit is ever below
the last bit of an fp32 addend: nothing is dropped, in any summation order or blocking, and the kernel's output equals an fp64 contraction of
the same operands bit for bit.  The split of an integer yields integer planes of its own sign (each plane is a truncation toward zero), so the
same holds for every one of the six split products and for accumulators that collect only some of them; the sum of the absolute split
products of an output is sum |x| |w|, which conv_reference / gemm_reference compute and the host test bounds by 2^24.

A contraction is described by its weights W f32[M, *kshape] (kshape = (Cin, 3, 3) for the 3x3 convolution, (Cin,) for a 1x1 / pointwise
layer) and its activations x f32[B, C, *spatial].  Four families:

  A  small dense integers: x in [-8, 8], w in [-2, 2]; with `epilogue`: scale in {0.5, 1, 2}, integer shift in [-4, 4], integer residual in
     [-16, 16].  Pins indexing and the whole epilogue.
  B  wide activations: x odd with 2^16 <= |x| < 2^18 (all three planes non-zero for at least half the values), w in {-1, 0, 1} with at most 63
     non-zeros per output channel: |sum| < 63 * 2^18 < 2^24.  Pins the staging split and the products (0,0), (0,1), (0,2).
  C  wide weights: w odd with 2^16 <= |w| < 2^18, dense; x in {-1, 0, 1}, non-zero in at most `max_channels` input channels (7 for the 3x3
     convolution: 63 terms per receptive field; 63 for a pointwise layer), among them the first and the last of a channel group of 8 and the
     last channel of the layer.  Pins the weight packers, the A-fragment loads and the products (0,0), (1,0), (2,0).
  D  one term, two planes on both sides: every output channel has exactly ONE non-zero weight, odd with 2^8 <= |w| < 2^12, whose position cycles
     through all taps and channels as the output channel runs; x dense odd with 2^8 <= |x| < 2^12.  Every product is below 2^24: pins (1,1), (0,1),
     (1,0), (0,0) exactly, and the output is a scaled copy of one shifted input channel -- tap offsets, halo zeros, parity layouts.
"""
import functools
import math
import zlib

import torch

FAMILIES = ("A", "B", "C", "D")
LIMIT = float(1 << 24)
D_STEP = 7           # family D's one weight of output channel co: tap co mod 9 of input channel (7 co) mod Cin


def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def _odd(shape, bits, g, low_bits=0):
    """odd integers with 2^low_bits <= |v| < 2^bits, both signs.  (An odd 18-bit value has a non-zero third plane unless the two bits behind
    its leading eight are both zero: drawn from [2^16, 2^18), two thirds of the values are three planes deep.)"""
    mag = torch.randint((1 << low_bits) >> 1, 1 << (bits - 1), shape, generator=g) * 2 + 1
    sign = torch.randint(0, 2, shape, generator=g) * 2 - 1
    return (mag * sign).to(torch.float32)


def planes(v):
    """the three bf16 terms of the split (bf16x3.h: truncate to the upper 16 bits, of the value, of the remainder, the rest) as fp32 tensors"""
    def hi16(t):
        return (t.contiguous().view(torch.int32) & -65536).view(torch.float32)
    p0 = hi16(v)
    r = v - p0
    p1 = hi16(r)
    return p0, p1, r - p1


def seed_of(*what):
    """a stable seed from a description of the case (the same operands in the host test, the GPU test and every run)"""
    return zlib.crc32(repr(what).encode())


def weights(family, M, kshape, seed, nnz=63):
    """W f32[M, *kshape] of `family`; nnz: family B's non-zeros per output channel (at most 63)"""
    g = _gen(seed)
    kshape = tuple(int(k) for k in kshape)
    K = math.prod(kshape)
    if family == "A":
        return torch.randint(-2, 3, (M,) + kshape, generator=g).to(torch.float32)
    if family == "B":
        w = torch.zeros(M, K)
        nnz = min(nnz, 63, K)
        for m in range(M):
            pos = torch.randperm(K, generator=g)[:nnz]
            w[m, pos] = (torch.randint(0, 2, (nnz,), generator=g) * 2 - 1).to(torch.float32)
        assert int((w != 0).sum(1).max()) <= 63
        return w.view((M,) + kshape)
    if family == "C":
        w = _odd((M,) + kshape, 18, g, low_bits=16)
        assert float(w.abs().max()) < 2 ** 18 and bool((planes(w)[2] != 0).float().mean() >= 0.5)
        return w
    if family == "D":
        C, inner = kshape[0], K // kshape[0]          # channels; taps per channel
        assert math.gcd(D_STEP, C) == 1, "family D walks the channels with a stride coprime to their number"
        w = torch.zeros(M, K)
        val = _odd((M,), 12, g, low_bits=8)           # 2^8 <= |w|: two planes
        for m in range(M):
            w[m, ((D_STEP * m) % C) * inner + m % inner] = val[m]
        assert bool(((w != 0).sum(1) == 1).all())
        return w.view((M,) + kshape)
    raise ValueError(family)


def c_channels(C, max_channels, seed):
    """the input channels family C's activations live in: first and last of a channel group of 8, the layer's last channel, then random ones"""
    g = _gen(seed)
    first = 8 if C > 16 else 0
    must = [first, first + 7, C - 1]
    rest = [c for c in torch.randperm(C, generator=g).tolist() if c not in must]
    return sorted(set(must + rest[:max(0, min(max_channels, C) - len(set(must)))]))


def activations(family, shape, seed, max_channels=7):
    """x f32[B, C, *spatial] of `family`; max_channels: family C only"""
    g = _gen(seed)
    shape = tuple(int(s) for s in shape)
    if family == "A":
        return torch.randint(-8, 9, shape, generator=g).to(torch.float32)
    if family == "B":
        x = _odd(shape, 18, g, low_bits=16)
        assert float(x.abs().max()) < 2 ** 18
        assert bool((planes(x)[2] != 0).float().mean() >= 0.5), "family B: at least half the values have a non-zero third plane"
        return x
    if family == "C":
        x = torch.zeros(shape)
        ch = c_channels(shape[1], max_channels, seed)
        assert len(ch) <= max_channels
        x[:, ch] = torch.randint(-1, 2, (shape[0], len(ch)) + shape[2:], generator=g).to(torch.float32)
        return x
    if family == "D":
        x = _odd(shape, 12, g, low_bits=8)
        assert bool((planes(x)[1] != 0).all()) and bool((planes(x)[2] == 0).all())
        return x
    raise ValueError(family)


def epilogue(M, out_shape, seed):
    """family A's epilogue operands: scale f32[M] in {0.5, 1, 2}, integer shift f32[M] in [-4, 4], integer residual f32[out_shape] in [-16, 16]"""
    g = _gen(seed)
    scale = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (M,), generator=g)]
    shift = torch.randint(-4, 5, (M,), generator=g).to(torch.float32)
    residual = torch.randint(-16, 17, tuple(out_shape), generator=g).to(torch.float32)
    return scale, shift, residual


def conv_reference(x, w, stride):
    """(fp64 convolution, sum of absolute products per output) of a 3x3 / pad 1 (w[M,C,3,3]) or 1x1 / pad 0 (w[M,C] or [M,C,1,1]) layer"""
    import torch.nn.functional as F
    if w.dim() == 2:
        w = w.view(w.shape[0], w.shape[1], 1, 1)
    pad = w.shape[-1] // 2
    return (F.conv2d(x.double(), w.double(), stride=stride, padding=pad),
            F.conv2d(x.double().abs(), w.double().abs(), stride=stride, padding=pad))


@functools.lru_cache(maxsize=None)
def conv_layer(family, B, Cin, H, W, Cout, stride):
    """The operands of one exact 3x3 layer, computed once and shared (callers must not write to them): dict with x f32[B,Cin,H,W],
    w f32[Cout,Cin,3,3], ref / absum (fp64 convolution and the sum of absolute products per output); stride 2 also the 1x1 / stride-2
    downsample branch of the same family: wd f32[Cout,Cin], refd, absumd; family A also scale, shift, residual."""
    what = (family, B, Cin, H, W, Cout, stride)
    L = {"x": activations(family, (B, Cin, H, W), seed_of("x", what), max_channels=7),
         "w": weights(family, Cout, (Cin, 3, 3), seed_of("w", what))}
    L["ref"], L["absum"] = conv_reference(L["x"], L["w"], stride)
    if stride == 2:
        L["wd"] = weights(family, Cout, (Cin,), seed_of("wd", what))
        L["refd"], L["absumd"] = conv_reference(L["x"], L["wd"], 2)
    if family == "A":
        L["scale"], L["shift"], L["residual"] = epilogue(Cout, L["ref"].shape, seed_of("e", what))
    return L


def gemm_reference(x, w):
    """(fp64 W @ x, sum of absolute products per output) for x[B,K,N], w[M,K]"""
    return torch.einsum("mk,bkn->bmn", w.double(), x.double()), torch.einsum("mk,bkn->bmn", w.double().abs(), x.double().abs())


def first_mismatch(got, ref):
    """index tuple of the first differing element (row-major), or None; NaNs differ from everything"""
    bad = ~(got == ref)
    if not bool(bad.any()):
        return None
    flat = int(torch.nonzero(bad.reshape(-1))[0])
    idx = []
    for s in reversed(got.shape):
        idx.append(flat % s)
        flat //= s
    return tuple(reversed(idx))
