"""numpy restatement of the map normals (csrc/map_normals.hip) and of di2p_map_crop_normals (csrc/map_index.hip).

The neighbours are scan_prep_oracle.neighbors_brute on (double) of the float32 rows: the at most max_nn rows with d2 < r^2 in ascending
(d2, row), exact fp64.  The normals are scan_prep_oracle.normals behind the axis permutation that brings up_axis to z, with the orient sign:
that oracle orients to +z and falls back to (0, 0, 1), so orient times its result is oriented to orient . e_up and falls back to it.
crop_normals is the kernel's formula operation for operation (numpy never fuses a multiply with an add)."""
import numpy as np

from tests import scan_prep_oracle as spo


def positions(points):
    """f32[M,4] rows -> f64[M,3]"""
    return np.asarray(points, dtype=np.float32)[:, :3].astype(np.float64)


def neighbors(points, radius=0.6, max_nn=30):
    """-> (count i32[M], idx i32[M,max_nn], -1 padded)"""
    return spo.neighbors_brute(positions(points), radius, max_nn)


def _perm(up_axis):
    return [k for k in range(3) if k != up_axis] + [up_axis]


def normals(points, cnt, idx, up_axis=2, orient=1):
    """-> (normals f64[M,3] with orient * n[up_axis] >= 0 and orient * e_up below 3 neighbours, eigenvalues f64[M,3] ascending)"""
    perm = _perm(up_axis)
    n, lam = spo.normals(positions(points)[:, perm], cnt, idx)
    out = np.empty_like(n)
    out[:, perm] = float(orient) * n
    return out, lam


def well_conditioned(cnt, lam):
    """the rows test_normals_against_oracle (tests/test_gpu_scan_prep.py) compares directions on"""
    gap = (lam[:, 1] - lam[:, 0]) / np.maximum(lam[:, 2], 1e-300)
    return (cnt >= 3) & (gap > 1e-3)


def ties_at_the_cut(points, radius=0.6, max_nn=30):
    """bool[M]: the max_nn-th and the (max_nn + 1)-th distance are exactly equal, so the (d2, row) rule decides who is in"""
    pos = positions(points)
    c2, n2 = spo.neighbors_brute(pos, radius, max_nn + 1)
    full = c2 == max_nn + 1
    d = spo.d2(pos[np.where(n2 >= 0, n2, 0)], pos[:, None, :])
    return full & (d[:, max_nn - 1] == d[:, max_nn])


def cell_candidates(points, radius=0.6):
    """i64[M]: the rows in the 27 cells around every row's cell, on the kernel's grid (edge radius (1 + 2^-20) over the map's own bounds)"""
    pos = positions(points)
    cell = radius * (1.0 + 2.0 ** -20)
    c = np.floor((pos - pos.min(0)) / cell).astype(np.int64)
    occ = {}
    for k in map(tuple, c):
        occ[k] = occ.get(k, 0) + 1
    out = np.zeros(len(pos), np.int64)
    for i, (x, y, z) in enumerate(map(tuple, c)):
        out[i] = sum(occ.get((x + dx, y + dy, z + dz), 0) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1))
    return out


def crop_normals(normals_map, index, offsets, T_map_prior):
    """-> f32[offsets[B],3]: out[k][i] = (float)((T[0][i] n0 + T[1][i] n1) + T[2][i] n2), n = (double)normals_map[index[k]], T of k's frame"""
    nm = np.asarray(normals_map, dtype=np.float32)
    T_map_prior = np.asarray(T_map_prior, dtype=np.float64)
    total = int(offsets[-1])
    out = np.zeros((total, 3), np.float32)
    for b in range(len(T_map_prior)):
        s, e = int(offsets[b]), int(offsets[b + 1])
        if e <= s:
            continue
        T = T_map_prior[b]
        n = nm[np.asarray(index[s:e], dtype=np.int64)].astype(np.float64)
        with np.errstate(invalid="ignore"):
            for i in range(3):
                out[s:e, i] = ((T[0, i] * n[:, 0] + T[1, i] * n[:, 1]) + T[2, i] * n[:, 2]).astype(np.float32)
    return out
