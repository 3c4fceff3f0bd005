"""numpy / scipy restatement of the raw-scan preparation (deepi2p_amd/scan_prep.py, csrc/scan_prep.hip): Open3D is not available, so
Open3D's VoxelDownSample / EstimateNormals / OrientNormalsToAlignWithDirection and the loader's fake-colour intensity average are pinned
by restatement only.  Arithmetic follows the kernels' fp64 formulas exactly where the tests compare bits."""
import numpy as np
from scipy.spatial import cKDTree

AXIS_BITS = 21


def compose(ix, iy, iz):
    return (ix.astype(np.int64) << (2 * AXIS_BITS)) | (iy.astype(np.int64) << AXIS_BITS) | iz.astype(np.int64)


def voxel_down_sample(pts4, voxel, normals=None, min_points=0):
    """pts4 f32[n,4] -> dict(keys i64[m], points f32[m,3], cen f64[m,3], intensity f32[m], normals f32[m,3] | None, inv i64[n]).
    Output in ascending key; every sum in ascending input index (np.bincount)."""
    pts4 = np.asarray(pts4, dtype=np.float32)
    n = pts4.shape[0]
    if n == 0:
        return dict(keys=np.zeros(0, np.int64), points=np.zeros((0, 3), np.float32), cen=np.zeros((0, 3)), intensity=np.zeros(0, np.float32),
                    normals=None if normals is None else np.zeros((0, 3), np.float32), inv=np.zeros(0, np.int64))
    p = pts4[:, :3].astype(np.float64)
    minb = pts4[:, :3].min(0).astype(np.float64) - voxel * 0.5
    idx = np.floor((p - minb) / voxel).astype(np.int64)
    key = compose(idx[:, 0], idx[:, 1], idx[:, 2])
    if n <= min_points:
        return dict(keys=key, points=pts4[:, :3].copy(), cen=p, intensity=pts4[:, 3].copy(),
                    normals=None if normals is None else np.asarray(normals, np.float32).copy(), inv=np.arange(n))
    uk, inv = np.unique(key, return_inverse=True)
    inv = inv.reshape(-1)
    cnt = np.bincount(inv).astype(np.float64)
    cen = np.stack([np.bincount(inv, weights=p[:, c]) / cnt for c in range(3)], 1)
    imax = np.float64(pts4[:, 3].max())
    c = pts4[:, 3].astype(np.float64) / imax
    inten = ((np.bincount(inv, weights=c) / cnt) * imax).astype(np.float32)
    nrm = None
    if normals is not None:
        nn = np.asarray(normals, np.float32).astype(np.float64)
        nrm = np.stack([np.bincount(inv, weights=nn[:, k]) / cnt for k in range(3)], 1).astype(np.float32)
    return dict(keys=uk, points=cen.astype(np.float32), cen=cen, intensity=inten, normals=nrm, inv=inv)


def voxel_brute(pts4, voxel):
    """the same by an explicit per-voxel loop (checks the oracle itself)"""
    p = np.asarray(pts4, np.float32)[:, :3].astype(np.float64)
    minb = np.asarray(pts4, np.float32)[:, :3].min(0).astype(np.float64) - voxel * 0.5
    groups = {}
    for i in range(p.shape[0]):
        k = tuple(int(np.floor((p[i, c] - minb[c]) / voxel)) for c in range(3))
        groups.setdefault(k, []).append(i)
    keys, cen = [], []
    for k in sorted(groups):
        s = np.zeros(3)
        for i in groups[k]:
            s = s + p[i]
        keys.append((k[0] << 42) | (k[1] << 21) | k[2])
        cen.append(s / float(len(groups[k])))
    return np.array(keys, np.int64), np.array(cen)


def d2(a, b):
    d = a - b
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def neighbors(cen, radius, max_nn):
    """-> (count i32[m], idx i32[m,max_nn] by ascending (d2, index), -1 padded): the <= max_nn nearest with d2 < r^2 (exact fp64)."""
    m = cen.shape[0]
    cnt = np.zeros(m, np.int32)
    out = np.full((m, max_nn), -1, np.int32)
    if m == 0:
        return cnt, out
    K = min(m, max_nn + 34)
    _, cand = cKDTree(cen).query(cen, k=K, distance_upper_bound=radius * (1 + 1e-6))
    cand = np.asarray(cand).reshape(m, K)
    valid = cand < m
    cc = np.where(valid, cand, 0)
    dd = d2(cen[cc], cen[:, None, :])
    dd = np.where(valid & (dd < radius * radius), dd, np.inf)
    order = np.lexsort((cc, dd), axis=-1)[:, :max_nn]
    ds = np.take_along_axis(dd, order, 1)
    ids = np.take_along_axis(cc, order, 1)
    ok = np.isfinite(ds)
    cnt = ok.sum(1).astype(np.int32)
    out = np.where(ok, ids, -1).astype(np.int32)
    return cnt, out


def neighbors_brute(cen, radius, max_nn):
    m = cen.shape[0]
    cnt = np.zeros(m, np.int32)
    out = np.full((m, max_nn), -1, np.int32)
    for q in range(m):
        dd = d2(cen, cen[q])
        ids = np.nonzero(dd < radius * radius)[0]
        ids = ids[np.lexsort((ids, dd[ids]))][:max_nn]
        cnt[q] = len(ids)
        out[q, :len(ids)] = ids
    return cnt, out


def normals(cen, cnt, idx):
    """-> (normals f64[m,3] oriented to +z, eigenvalues f64[m,3] ascending): PCA of each neighbour set, (0,0,1) below 3 neighbours."""
    m = cen.shape[0]
    nrm = np.zeros((m, 3))
    nrm[:, 2] = 1.0
    lam = np.zeros((m, 3))
    if m == 0:
        return nrm, lam
    ii = np.where(idx >= 0, idx, 0)
    w = (idx >= 0).astype(np.float64)
    P = cen[ii]
    k = np.maximum(cnt, 1).astype(np.float64)
    mean = (P * w[..., None]).sum(1) / k[:, None]
    E = (P - mean[:, None, :]) * w[..., None]
    C = np.einsum("mki,mkj->mij", E, E)
    ev, V = np.linalg.eigh(C)
    n = V[:, :, 0]
    use = (cnt >= 3) & (np.abs(C).reshape(m, -1).max(1) > 0)
    nrm[use] = n[use]
    nrm[nrm[:, 2] < 0] *= -1.0
    lam[:] = ev
    return nrm, lam


def nearest_raw(raw4, cen):
    """-> (index i64[m], d2 f64[m]): the nearest raw point (exact fp64 d2, ties -> lower index)."""
    raw = np.asarray(raw4, np.float32)[:, :3].astype(np.float64)
    if cen.shape[0] == 0:
        return np.zeros(0, np.int64), np.zeros(0)
    K = min(8, raw.shape[0])
    _, cand = cKDTree(raw).query(cen, k=K)
    cand = np.asarray(cand).reshape(cen.shape[0], K)
    dd = d2(raw[cand], cen[:, None, :])
    o = np.lexsort((cand, dd), axis=-1)[:, 0]
    return np.take_along_axis(cand, o[:, None], 1)[:, 0], np.take_along_axis(dd, o[:, None], 1)[:, 0]


def preprocess_velodyne(scan, voxel=0.1, sn_radius=0.6, sn_max_nn=30):
    """the offline script's 7 x m float32 record (rows in ascending voxel key)"""
    v = voxel_down_sample(scan, voxel)
    cnt, idx = neighbors(v["cen"], sn_radius, sn_max_nn)
    nrm, _ = normals(v["cen"], cnt, idx)
    nn, _ = nearest_raw(scan, v["cen"])
    inten = np.asarray(scan, np.float32)[nn, 3] if len(nn) else np.zeros(0, np.float32)
    return np.concatenate((v["cen"].T, inten[None].astype(np.float64), nrm.T), 0).astype(np.float32)
