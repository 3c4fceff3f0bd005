"""Operands for which di2p_stem_x3 (conv 7x7 / 2 / pad 3, 3 -> 64, scale / shift, ReLU, max-pool 3x3 / 2 / pad 1 in one launch) is EXACT
(the premise of tests/x3_exact_cases.py: operands on one binary grid, every sum of absolute products below 2^24 grid units).  Generators only:
seeded, CPU, no GPU code.  ReLU and the pool's maxima are exact, so the pooled output must equal the fp64 evaluation bit for bit.

The kernel pools its own convolution: a pooled output shows a convolution pixel only where that pixel wins its window.  Families A, B, C
compare pooled outputs of dense operands; family D is built so that EVERY convolution pixel is seen in some frame (coverage(), asserted by
tests/test_x3_fused_cases_host.py on the reference alone).

A launch has one weight set; the many cases of a shape are frames of its batch.  LAUNCHES names them; launch(name, H, W) returns
dict(x f32[F,3,H,W], w f32[64,3,7,7], scale, shift f32[64], conv (scale * convolution + shift before the ReLU), absum (scale * sum of absolute
products + |shift|), ref f32[F,64,H/4,W/4]).  Callers must not write to what they get.

  A   x in [-8, 8], w in [-2, 2], scale in {0.5, 1, 2}, integer shift in [-64, 64] (both signs: the ReLU clips about half of every frame)
  B   x odd, 2^16 <= |x| < 2^18; w in {-1, 0, 1}, at most 63 non-zeros per output channel
  C   w odd, 2^16 <= |w| < 2^18, dense; frame c has x in {-1, 0, 1} in input channel c only (49 terms per window)
  D0, D1, D2   output channel co has ONE non-zero weight, at flat tap (11 (co + 64 k)) mod 147 of (ci, ky, kx): the three sets use all 147 taps.
      The weight is odd and positive, below 2^8.  The convolution is a scaled copy of one shifted input pixel.  Frames: 16 phases x 4 orderings
      -- x is positive where (row mod 4, column mod 4) equals the phase and negative elsewhere, |x| = 2 rank + 1 < 2^16 with the rank running
      in raster order, rows and columns each ascending or descending -- so that a frame's positive convolution pixels sit two apart in both
      directions (or there are none, for a phase whose parity the tap never samples) and every in-image convolution pixel is the strictly
      positive maximum of a window in some frame.  The weights are positive for that reason: with a negative weight three of four parity
      classes are positive and a window's centre never wins.  Then one frame of all-negative x, whose exact output is zero everywhere (a
      padding read that is not zero shows up here or in N0..N2)
  N0, N1, N2   the weights of D0..D2 negated against one frame of all-positive x: zero everywhere, too
  D12 the taps of D0 with odd weights 2^8 <= |w| < 2^12 of both signs against dense odd x of the same range: two planes on both sides,
      the (1,1) product
"""
import functools

import torch
import torch.nn.functional as F

from tests import x3_exact_cases as xc

# (H, W): see SHAPE_NOTES
SHAPES = [(4, 128), (12, 128), (8, 256), (36, 384), (44, 128), (96, 128), (160, 128)]
SHAPE_NOTES = {(4, 128): "one pooled row; three of four waves have no columns", (36, 384): "prw = 2, short last workgroup",
               (44, 128): "prw = 2, short last workgroup", (96, 128): "prw = 3: the ring wraps more than once",
               (160, 128): "prw = 5: the benchmark's row count"}
D_SETS = (0, 1, 2)
D_TAP_STEP = 11
PHASES = [(r, c) for r in range(4) for c in range(4)]
ORDERINGS = [(False, False), (False, True), (True, False), (True, True)]          # (rows descending, columns descending)
N_COVER = len(PHASES) * len(ORDERINGS)


def shape_id(s):
    return "%dx%d" % s


def prw(H):
    """pooled rows per workgroup (the launch rule of di2p_stem_x3)"""
    PH = H // 4
    return -(-PH // 8) if PH >= 8 else 1


def d_taps(k):
    """flat tap (ci * 49 + ky * 7 + kx) of each output channel in weight set k"""
    return [(D_TAP_STEP * (co + 64 * k)) % 147 for co in range(64)]


def d_weights(k, wide=False):
    g = xc._gen(xc.seed_of("stem D w", k, wide))
    val = xc._odd((64,), 12, g, low_bits=8) if wide else xc._odd((64,), 8, g).abs()
    w = torch.zeros(64, 147)
    w[torch.arange(64), torch.tensor(d_taps(k))] = val
    return w.view(64, 3, 7, 7)


def d_frames(H, W):
    """the 64 coverage frames and one all-negative frame, f32[65,3,H,W]"""
    assert 2 * H * W + 1 < 2 ** 16
    rows, cols = torch.arange(H).view(H, 1), torch.arange(W).view(1, W)
    frames = []
    for rdesc, cdesc in ORDERINGS:
        rank = (H - 1 - rows if rdesc else rows) * W + (W - 1 - cols if cdesc else cols)
        mag = (2 * rank + 1).float()
        for pr, pc in PHASES:
            frames.append(torch.where((rows % 4 == pr) & (cols % 4 == pc), mag, -mag))
    frames.append(-frames[0].abs())
    return torch.stack(frames).unsqueeze(1).expand(-1, 3, -1, -1).contiguous()


def one_tap_conv(x, w):
    """the convolution of a filter bank with one non-zero weight per output channel, as slices of the padded input (exact in fp32: one product
    below 2^24 per output) -> f32[F,64,H/2,W/2]; equals F.conv2d in fp64 (asserted by the host test)"""
    Fr, _, H, W = x.shape
    xp = F.pad(x, (3, 3, 3, 3))
    out = torch.empty(Fr, 64, H // 2, W // 2)
    flat = w.view(64, 147)
    for co in range(64):
        t = int(torch.nonzero(flat[co])[0])
        ci, ky, kx = t // 49, (t % 49) // 7, t % 7
        out[:, co] = xp[:, ci, ky:ky + H:2, kx:kx + W:2] * flat[co, t]
    return out


def in_image(k, H, W):
    """bool[64,H/2,W/2]: the convolution pixels of weight set k whose single tap reads inside the image"""
    oy, ox = torch.arange(H // 2).view(-1, 1), torch.arange(W // 2).view(1, -1)
    m = torch.empty(64, H // 2, W // 2, dtype=torch.bool)
    for co, t in enumerate(d_taps(k)):
        ky, kx = (t % 49) // 7, t % 7
        ry, rx = 2 * oy + ky - 3, 2 * ox + kx - 3
        m[co] = (ry >= 0) & (ry < H) & (rx >= 0) & (rx < W)
    return m


def coverage(act, pooled):
    """bool[64,OH,OW]: the pixels of act f32[F,64,OH,OW] (after the ReLU) that are the strictly positive maximum of a pool window (pooled =
    max_pool2d(act, 3, 2, 1)) in some frame"""
    Fr, C, OH, OW = act.shape
    PH, PW = pooled.shape[2:]
    ap = F.pad(act, (1, 1, 1, 1), value=-1.0)
    seen = torch.zeros(C, OH + 2, OW + 2, dtype=torch.bool)
    for dy in (0, 1, 2):                    # padded row 2 ph + dy = convolution row 2 ph + dy - 1
        for dx in (0, 1, 2):
            sl = ap[:, :, dy:dy + 2 * PH:2, dx:dx + 2 * PW:2]
            seen[:, dy:dy + 2 * PH:2, dx:dx + 2 * PW:2] |= ((sl == pooled) & (sl > 0)).any(0)
    return seen[:, 1:-1, 1:-1]


def _finish(x, w, scale, shift, conv=None, absum=None):
    if conv is None:
        conv = F.conv2d(x.double(), w.double(), stride=2, padding=3)
        absum = F.conv2d(x.double().abs(), w.double().abs(), stride=2, padding=3)
    s, h = scale.to(conv.dtype).view(1, -1, 1, 1), shift.to(conv.dtype).view(1, -1, 1, 1)
    lin = conv * s + h
    return {"x": x, "w": w, "scale": scale, "shift": shift, "conv": lin, "absum": absum * s.abs() + h.abs(),
            "ref": F.max_pool2d(torch.relu(lin), 3, 2, 1).float()}


def _unit():
    return torch.ones(64), torch.zeros(64)


def _build(name, H, W):
    what = ("stem", name, H, W)
    g = xc._gen(xc.seed_of("e", what))
    if name == "A":
        scale = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (64,), generator=g)]
        shift = torch.randint(-64, 65, (64,), generator=g).float()
        return _finish(xc.activations("A", (3, 3, H, W), xc.seed_of("x", what)), xc.weights("A", 64, (3, 7, 7), xc.seed_of("w", what)), scale, shift)
    if name == "B":
        return _finish(xc.activations("B", (2, 3, H, W), xc.seed_of("x", what)), xc.weights("B", 64, (3, 7, 7), xc.seed_of("w", what)), *_unit())
    if name == "C":
        x = torch.zeros(3, 3, H, W)
        for c in range(3):
            x[c, c] = torch.randint(-1, 2, (H, W), generator=g).float()
        return _finish(x, xc.weights("C", 64, (3, 7, 7), xc.seed_of("w", what)), *_unit())
    k = int(name[1]) if name != "D12" else 0
    if name == "D12":
        return _finish(xc.activations("D", (2, 3, H, W), xc.seed_of("x", what)), d_weights(0, wide=True), *_unit())
    w = d_weights(k)
    if name[0] == "N":
        w, x = -w, d_frames(H, W)[-1:].abs()
    else:
        x = d_frames(H, W)
    conv = one_tap_conv(x, w)                 # fp32, exact: one product per output
    return _finish(x, w, *_unit(), conv=conv, absum=conv.abs())


LAUNCHES = ["A", "B", "C", "D0", "D1", "D2", "N0", "N1", "N2", "D12"]


@functools.lru_cache(maxsize=2)          # (a D launch of the largest shape holds 200 MB; building one takes 0.2 s)
def launch(name, H, W):
    return _build(name, H, W)


def describe(H, W, idx):
    """where a pooled output index (b, co, ph, pw) lies: the facts the exact tests report with a mismatch"""
    b, co, ph, pw = idx
    PH, PW, p = H // 4, W // 4, prw(H)
    return ("first differing index (b, co, ph, pw) = %s; border row / column: %s; first / last pooled row of its workgroup (prw = %d): %s / %s; "
            "in a 64-column wave boundary column: %s"
            % (idx, ph in (0, PH - 1) or pw in (0, PW - 1), p, ph % p == 0, ph % p == p - 1 or ph == PH - 1, pw % 32 in (0, 31) and 0 < pw < PW - 1))
