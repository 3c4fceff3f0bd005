"""Numpy fp64 restatement of csrc/world.hip (deepi2p_amd/world.py's docstring fixes the formulas): the same operations in the same order,
one rounding each, so the device results are compared bit for bit.  The ray tests ARE synthetic._ray_box / _ray_pole; the draws are
oracle/rng_np.py's Philox.  Test code: nothing here is used by the package."""
import warnings

import numpy as np

from deepi2p_amd import synthetic, world
from oracle import rng_np

TAG_WORLD = 7
MASK = np.uint64(0xFFFFFFFF)


def trace(table, count, o, d):
    """one frame: table f64[32,16], count, o f64[3], d f64[n,3] -> (t f64[n] (inf on a miss), prim i32[n] (-1 on a miss))"""
    o, d = np.asarray(o, dtype=np.float64), np.asarray(d, dtype=np.float64)
    n = d.shape[0]
    if count == 0 or n == 0:
        return np.full(n, np.inf), np.full(n, -1, np.int32)
    hits = []
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        for g in table[:count]:
            if g[0] == world.BOX:
                hits.append(synthetic._ray_box(o, d, g[1:4], g[4:7]))
            elif g[0] == world.CYLINDER:
                hits.append(synthetic._ray_pole(o, d, g[1], g[2], g[3], g[4], g[5]))
            else:
                t = (g[1] - o[2]) / np.minimum(d[:, 2], -1e-12)
                hits.append(np.where((d[:, 2] < 0) & (t > 0), t, np.inf))
    T = np.stack(hits, axis=1)
    which = np.argmin(T, axis=1)          # the first of equal minima
    t = T[np.arange(n), which]
    return t, np.where(t < np.inf, which, -1).astype(np.int32)


def _cell(h, cell):
    q = np.clip(np.floor(h / cell), -4503599627370496.0, 4503599627370496.0)
    return q.astype(np.int64).astype(np.uint64) & MASK


def _byte(c):
    return np.floor(np.clip(c, 0.0, 255.0) + 0.5).astype(np.uint8)


def shade(table, o, d, t, prim, max_range):
    """colours u8[n,3] of the hits (rows with prim < 0 are left 0)"""
    n = d.shape[0]
    out = np.zeros((n, 3), np.uint8)
    hit = prim >= 0
    if not hit.any():
        return out
    d, t, prim = d[hit], t[hit], prim[hit]
    g = table[prim]
    kind = g[:, 0]
    h = o[None] + t[:, None] * d
    q = np.stack([_cell(h[:, k], g[:, 11]) for k in range(3)], 1)
    with np.errstate(all="ignore"):
        inv = 1.0 / d
        mn = np.minimum((g[:, 1:4] - o[None]) * inv, (g[:, 4:7] - o[None]) * inv)          # box rows only
    face = np.where(mn[:, 0] == t, 0, np.where(mn[:, 1] == t, 1, 2))
    with np.errstate(all="ignore"):
        nl = ((h[:, 0] - g[:, 1]) / g[:, 3]) * world.LIGHT[0] + ((h[:, 1] - g[:, 2]) / g[:, 3]) * world.LIGHT[1]          # cylinder rows only
        s_cyl = 0.6 + 0.4 * np.where(nl > 0.0, nl, 0.0)
    is_box, is_cyl = kind == world.BOX, kind == world.CYLINDER
    s = np.where(is_box, world.SHADE[face], np.where(is_cyl, s_cyl, 1.0))
    drop = np.zeros((len(t), 3), bool)          # the axes left out of the cell
    drop[is_box, face[is_box]] = True
    drop[is_cyl, 0] = drop[is_cyl, 1] = True
    drop[~is_box & ~is_cyl, 2] = True
    q = np.where(drop, np.uint64(0), q)
    k = ((q[:, 0] * np.uint64(73856093)) & MASK) ^ ((q[:, 1] * np.uint64(19349663)) & MASK) ^ ((q[:, 2] * np.uint64(83492791)) & MASK) \
        ^ ((prim.astype(np.uint64) * np.uint64(2654435761)) & MASK)
    k ^= k >> np.uint64(13)
    k = (k * np.uint64(0x5bd1e995)) & MASK
    k ^= k >> np.uint64(15)
    tex = world.TEX[(k & np.uint64(7)).astype(np.int64)]
    far = t / max_range
    fade = 1.0 - 0.5 * np.where(far > 1.0, 1.0, far)
    out[hit] = np.stack([_byte((((g[:, 7 + c] * s) * tex) * fade) * 255.0) for c in range(3)], 1)
    return out


def render_camera(table, count, K, M, H0, W0, max_range=world.MAX_RANGE):
    """one frame -> dict(image u8[H0,W0,3], depth f32[H0,W0], prim i32[H0,W0], t f64[H0,W0])"""
    v, u = (a.reshape(-1).astype(np.float64) for a in np.mgrid[0:H0, 0:W0])
    xc, yc = (u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1]
    d = np.stack([(M[i, 0] * xc + M[i, 1] * yc) + M[i, 2] for i in range(3)], 1)
    o = np.array(M[:3, 3], dtype=np.float64)
    t, prim = trace(table, count, o, d)
    img = shade(table, o, d, t, prim, max_range)
    gy = (v + 0.5) / float(H0)
    sky = np.stack([_byte(world.SKY_TOP[c] + world.SKY_SPAN[c] * gy) for c in range(3)], 1)
    img = np.where((prim >= 0)[:, None], img, sky)
    depth = np.where(prim >= 0, t, 0.0).astype(np.float32)
    return dict(image=img.reshape(H0, W0, 3), depth=depth.reshape(H0, W0), prim=prim.reshape(H0, W0), t=t.reshape(H0, W0))


def _philox(r, frame, block, seed):
    f = np.full_like(r, frame)
    return rng_np.philox4x32_10(r, f, np.full_like(r, block), np.full_like(r, TAG_WORLD), seed & rng_np.MASK, (seed >> 32) & rng_np.MASK)


def _gauss(p):
    return np.sqrt(-2.0 * np.log(rng_np.u53(p[0], p[1]))) * np.cos(6.283185307179586476925 * rng_np.u53(p[2], p[3]))


def scan_dirs(elev, azim):
    """sensor-frame directions f64[beams * azimuths, 3], beam-major"""
    cE, sE, cA, sA = elev[:, 0], elev[:, 1], azim[:, 0], azim[:, 1]
    return np.stack([(cE[:, None] * cA[None]).reshape(-1), (cE[:, None] * sA[None]).reshape(-1), np.repeat(sE, len(cA))], 1)


def render_scan(table, count, elev, azim, seed, frame, pose=None, max_range=world.MAX_RANGE, dropout=world.DROPOUT, range_sigma=world.RANGE_SIGMA,
                intensity_sigma=world.INTENSITY_SIGMA):
    """one frame (azim f64[azimuths,2], frame = frame0 + b) -> dict(rows f32[n,4] the kept rows, keep bool[R], t f64[R] and prim i32[R] before
    the noise, points64 f64[n,3] the kept returns before the float32 rounding, dirs f64[R,3])"""
    M = np.eye(4) if pose is None else np.asarray(pose, dtype=np.float64)
    s = scan_dirs(elev, azim)
    d = np.stack([(M[i, 0] * s[:, 0] + M[i, 1] * s[:, 1]) + M[i, 2] * s[:, 2] for i in range(3)], 1)
    t, prim = trace(table, count, np.array(M[:3, 3]), d)
    r = np.arange(len(s), dtype=np.uint64)
    p0 = _philox(r, frame, 0, seed)
    keep = (t < max_range) & (rng_np.u53(p0[0], p0[1]) >= dropout)
    tn = t.copy()
    inten = np.where(prim >= 0, table[np.maximum(prim, 0), 10], 0.0)
    if range_sigma > 0.0:
        tn = tn + range_sigma * _gauss(_philox(r, frame, 1, seed))
    if intensity_sigma > 0.0:
        inten = inten + intensity_sigma * _gauss(_philox(r, frame, 2, seed))
    inten = np.clip(inten, 0.0, 1.0)
    with np.errstate(all="ignore"):
        p64 = s * tn[:, None]
    rows = np.concatenate([p64, inten[:, None]], 1)[keep].astype(np.float32)
    return dict(rows=rows, keep=keep, t=t, prim=prim, points64=p64[keep], dirs=s)
