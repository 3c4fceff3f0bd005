"""Numpy fp64 restatement of the push-broom profile render of csrc/world.hip (di2p_world_render_profiles; deepi2p_amd/world.py fixes the
formulas), one sub-map at a time: the same operations in the same order, one rounding each, so the noise-free device rows are compared
bit for bit.  The ray tests and the Box-Muller are tests/world_oracle.py's (trace, _gauss), imported; the draws are its _philox with the
stream tag of the profiles, 8, in place of the scan's 7 -- _philox reads the tag from its module, so it is called through _philox8, which
sets it for the call.  Test code: nothing here is used by the package."""
import numpy as np

from deepi2p_amd import world
from oracle import rng_np
from tests import world_oracle as wo

TAG_PROFILES = 8


def _philox8(r, frame, block, seed):
    """world_oracle._philox with the fourth counter word 8"""
    saved, wo.TAG_WORLD = wo.TAG_WORLD, TAG_PROFILES
    try:
        return wo._philox(r, frame, block, seed)
    finally:
        wo.TAG_WORLD = saved


def beam_dirs(M, beam):
    """R . (c, s, 0) per beam, every entry (R_i0 c + R_i1 s) + R_i2 0 -> f64[beams,3]"""
    c, s = beam[:, 0], beam[:, 1]
    with np.errstate(all="ignore"):
        return np.stack([(M[i, 0] * c + M[i, 1] * s) + M[i, 2] * 0.0 for i in range(3)], 1)


def render_profiles(table, count, laser_to_world, beam, seed, frame, max_range=world.LMS_MAX_RANGE, dropout=world.LMS_DROPOUT,
                    range_sigma=world.LMS_RANGE_SIGMA, reflectance_sigma=world.REFLECTANCE_SIGMA):
    """one sub-map: table f64[32,16], count, laser_to_world f64[S,4,4], beam f64[beams,2]; frame = frame0 + the index in the batch of the
    sub-map's first profile -> dict(rows f64[n,3] the kept rows, counts i64[S], keep bool[S,beams], t f64[S,beams] and prim i32[S,beams]
    before the noise, origins f64[S,3], dirs f64[S,beams,3], world64 f64[n,3] the kept returns o + t d before the noise, in world
    coordinates)"""
    L = np.asarray(laser_to_world, dtype=np.float64).reshape(-1, 4, 4)
    beam = np.asarray(beam, dtype=np.float64)
    S, beams = L.shape[0], beam.shape[0]
    k = np.arange(beams, dtype=np.uint64)
    c, sn = beam[:, 0], beam[:, 1]
    rows, keeps, ts, prims, dirs, returns = [], [], [], [], [], []
    for s in range(S):
        M = L[s]
        o = np.array(M[:3, 3])
        d = beam_dirs(M, beam)
        t, prim = wo.trace(table, count, o, d)
        p0 = _philox8(k, frame + s, 0, seed)
        keep = (t < max_range) & (rng_np.u53(p0[0], p0[1]) >= dropout)
        tn = t.copy()
        refl = np.where(prim >= 0, table[np.maximum(prim, 0), 10], 0.0)
        if range_sigma > 0.0:
            tn = tn + range_sigma * wo._gauss(_philox8(k, frame + s, 1, seed))
        if reflectance_sigma > 0.0:
            refl = refl + reflectance_sigma * wo._gauss(_philox8(k, frame + s, 2, seed))
        with np.errstate(all="ignore"):
            row = np.stack([tn * c, tn * sn, np.clip(255.0 * refl, 0.0, 255.0)], 1)
            ret = o[None] + t[:, None] * d
        rows.append(row[keep])
        returns.append(ret[keep])
        keeps.append(keep)
        ts.append(t)
        prims.append(prim)
        dirs.append(d)
    cat = lambda parts, width: np.concatenate(parts) if parts else np.zeros((0, width))
    return dict(rows=cat(rows, 3), counts=np.array([int(kp.sum()) for kp in keeps], dtype=np.int64), keep=np.array(keeps).reshape(S, beams),
                t=np.array(ts).reshape(S, beams), prim=np.array(prims, dtype=np.int32).reshape(S, beams), origins=L[:, :3, 3].copy(),
                dirs=np.array(dirs).reshape(S, beams, 3), world64=cat(returns, 3))


def render_batch(world_pair, submap_offsets, laser_to_world, beam, seed, frame0=0, **kw):
    """the batch, sub-map after sub-map (offsets accepted as they are: non-decreasing from 0) -> (rows f64[n,3], scan_offsets i64[S+1], the
    per-sub-map dicts)"""
    table, count = world_pair
    off = [int(v) for v in submap_offsets]
    L = np.asarray(laser_to_world, dtype=np.float64).reshape(-1, 4, 4)
    subs = [render_profiles(table[b], int(count[b]), L[off[b]:off[b + 1]], beam, seed, frame0 + off[b], **kw) for b in range(len(off) - 1)]
    counts = np.zeros(L.shape[0], np.int64)
    for b, sub in enumerate(subs):
        counts[off[b]:off[b + 1]] = sub["counts"]
    rows = np.concatenate([sub["rows"] for sub in subs]) if subs else np.zeros((0, 3))
    return rows, np.concatenate([[0], np.cumsum(counts)]), subs
