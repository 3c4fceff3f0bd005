"""numpy restatement of csrc/map_index.hip, operation for operation: every value that decides a bit is float64, every operation rounded once
(numpy never fuses a multiply with an add), the sums in the order the header states.  build() is di2p_map_index_build, crop() di2p_map_crop
with its statuses, pose() di2p_map_pose; brute_force() is the keep rule applied to the unsorted map, the reference the oracle itself is
checked against (tests/test_map_index_host.py)."""
import numpy as np

ST_OK, ST_TOO_MANY, ST_EMPTY, ST_PRIOR = 0, 1, 4, 5


def ground_axes(up_axis):
    """the ground axes (a, b): the two that are not up_axis, ascending"""
    return [k for k in range(3) if k != up_axis]


def default_grid(points, cell, up_axis):
    """MapIndex.build's origin=None: origin = floor(min / cell) cell, nx and ny from the map's own extent"""
    a, b = ground_axes(up_axis)
    p = np.asarray(points, dtype=np.float64)
    cell = np.float64(cell)
    origin = np.floor(np.array([p[:, a].min(), p[:, b].min()]) / cell) * cell
    n = np.floor((np.array([p[:, a].max(), p[:, b].max()]) - origin) / cell).astype(np.int64) + 1
    return origin, int(n[0]), int(n[1])


def cell_ids(points, cell, up_axis, origin, nx, ny):
    """-> (id i64[M] with nx ny for a row that is not finite or outside the grid, ok bool[M])"""
    a, b = ground_axes(up_axis)
    p = np.asarray(points, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        fx = np.floor((p[:, a].astype(np.float64) - np.float64(origin[0])) / np.float64(cell))
        fy = np.floor((p[:, b].astype(np.float64) - np.float64(origin[1])) / np.float64(cell))
        ok = np.isfinite(p[:, :3]).all(axis=1) & (fx >= 0) & (fx <= nx - 1) & (fy >= 0) & (fy <= ny - 1)
    ids = np.full(len(p), nx * ny, np.int64)
    ids[ok] = fy[ok].astype(np.int64) * nx + fx[ok].astype(np.int64)
    return ids, ok


def build(points, cell, up_axis, origin, nx, ny):
    """-> dict(cell_start i32[nx ny + 1], order i32[M], sorted f32[M,4], status int) and the grid; status 1: the arrays are unspecified"""
    p = np.ascontiguousarray(points, dtype=np.float32)
    ids, ok = cell_ids(p, cell, up_axis, origin, nx, ny)
    order = np.argsort(ids, kind="stable").astype(np.int32)
    cell_start = np.searchsorted(ids[order], np.arange(nx * ny + 1), side="left").astype(np.int32)
    return dict(cell_start=cell_start, order=order, sorted=p[order], status=0 if ok.all() else 1, M=len(p), cell=float(cell), up_axis=int(up_axis),
                origin=(float(origin[0]), float(origin[1])), nx=int(nx), ny=int(ny))


def _axis_window(c, r, origin, cell, n):
    with np.errstate(over="ignore"):
        f0 = np.floor(((np.float64(c) - np.float64(r)) - np.float64(origin)) / np.float64(cell))
        f1 = np.floor(((np.float64(c) + np.float64(r)) - np.float64(origin)) / np.float64(cell))
    if not f0 <= n - 1 or not f1 >= 0:
        return 1, 0
    return (0 if f0 < 0 else int(f0)), (n - 1 if f1 > n - 1 else int(f1))


def window(ix, T, r):
    """the clamped window (ix0, ix1, iy0, iy1) of a finite prior and a positive radius, or None when the disc misses the grid"""
    a, b = ground_axes(ix["up_axis"])
    ix0, ix1 = _axis_window(T[a, 3], r, ix["origin"][0], ix["cell"], ix["nx"])
    iy0, iy1 = _axis_window(T[b, 3], r, ix["origin"][1], ix["cell"], ix["ny"])
    return None if ix0 > ix1 or iy0 > iy1 else (ix0, ix1, iy0, iy1)


def keep(p, T, r, up_axis):
    """the strict keep rule on float32 rows p[n,4] -> bool[n]"""
    a, b = ground_axes(up_axis)
    dx = p[:, a].astype(np.float64) - np.float64(T[a, 3])
    dy = p[:, b].astype(np.float64) - np.float64(T[b, 3])
    return dx * dx + dy * dy < np.float64(r) * np.float64(r)


def to_prior(p, T):
    """kept float32 rows in the prior frame: q_i = (float)((T[0][i] d0 + T[1][i] d1) + T[2][i] d2), d_k = (double)p[k] - T[k][3]"""
    T = np.asarray(T, dtype=np.float64)
    d = [p[:, k].astype(np.float64) - T[k, 3] for k in range(3)]
    out = np.empty((len(p), 4), np.float32)
    for i in range(3):
        out[:, i] = ((T[0, i] * d[0] + T[1, i] * d[1]) + T[2, i] * d[2]).astype(np.float32)
    out[:, 3] = p[:, 3]
    return out


def frame_rows(ix, T, r):
    """the stored rows (positions in `sorted`) frame (T, r) keeps, in visiting order: window cells iy-major, a cell's rows in stored order
    -> (positions i64[n], window cells)"""
    w = window(ix, T, r)
    if w is None:
        return np.zeros(0, np.int64), 0
    ix0, ix1, iy0, iy1 = w
    pos = []
    for iy in range(iy0, iy1 + 1):
        for jx in range(ix0, ix1 + 1):
            c = iy * ix["nx"] + jx
            s = np.arange(ix["cell_start"][c], ix["cell_start"][c + 1], dtype=np.int64)
            pos.append(s[keep(ix["sorted"][s], T, r, ix["up_axis"])])
    return np.concatenate(pos), (ix1 - ix0 + 1) * (iy1 - iy0 + 1)


def crop(ix, T_map_prior, radius, cap, max_frame_points, max_cells):
    """-> (rows f32[offsets[B],4], offsets i32[B+1], index i32[offsets[B]], status i32[B]): di2p_map_crop's outputs up to its last row"""
    T_map_prior = np.asarray(T_map_prior, dtype=np.float64)
    radius = np.asarray(radius, dtype=np.float64)
    B = len(T_map_prior)
    rows, index, offsets, status = [], [], [0], []
    for b in range(B):
        T, r = T_map_prior[b], radius[b]
        st, pos = ST_OK, np.zeros(0, np.int64)
        if not np.isfinite(T).all() or not np.isfinite(r) or not r > 0:
            st = ST_PRIOR
        else:
            pos, cells = frame_rows(ix, T, r)
            if cells > max_cells:
                st = ST_TOO_MANY
            elif len(pos) > max_frame_points or offsets[-1] + len(pos) > cap:
                st = ST_TOO_MANY
            elif len(pos) == 0:
                st = ST_EMPTY
        if st == ST_OK:
            rows.append(to_prior(ix["sorted"][pos], T))
            index.append(ix["order"][pos])
        offsets.append(offsets[-1] + (len(pos) if st == ST_OK else 0))
        status.append(st)
    rows = np.concatenate(rows) if rows else np.zeros((0, 4), np.float32)
    index = np.concatenate(index).astype(np.int32) if index else np.zeros(0, np.int32)
    return rows, np.asarray(offsets, np.int32), index, np.asarray(status, np.int32)


def brute_force(points, T, r, up_axis):
    """the map rows frame (T, r) keeps, by the keep rule over the unsorted map: ascending map row"""
    return np.nonzero(keep(np.asarray(points, dtype=np.float32), np.asarray(T, dtype=np.float64), r, up_axis))[0]


def pose(T_map_prior, P_scan):
    """di2p_map_pose: A . [R^T | -R^T t], every entry a dot product in ascending k, products and sums rounded separately"""
    A, P = np.asarray(T_map_prior, dtype=np.float64), np.asarray(P_scan, dtype=np.float64)
    out = np.empty_like(A)
    for n in range(len(A)):
        a, p = A[n], P[n]
        m = np.zeros((4, 4))
        for i in range(3):
            for j in range(3):
                m[i, j] = p[j, i]
            m[i, 3] = -((p[0, i] * p[0, 3] + p[1, i] * p[1, 3]) + p[2, i] * p[2, 3])
        m[3, 3] = 1.0
        for i in range(4):
            for j in range(4):
                acc = a[i, 0] * m[0, j]
                for k in range(1, 4):
                    acc = acc + a[i, k] * m[k, j]
                out[n, i, j] = acc
    return out
