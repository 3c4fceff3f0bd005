"""numpy restatement of csrc/point_ops.hip, value for value.  The kernels round every operation on its own (subtraction, product, sum,
quotient and root each correctly rounded, never a fused multiply-add: the file is built with -ffp-contract=off and takes its root with sqrtf)
and numpy's elementwise float32 arithmetic does the same, so every function here gives the bits the device gives; no tolerance belongs to any
of them.  No torch, no GPU.

kNN rule (the only one): the k winners are the first k in (d^2, node id) order, d^2 compared as its bit pattern; they come out in
(d, node id) order, d = sqrt(d^2) rounded to float32.  A node whose d^2 is NaN is never a winner; d^2 = +inf is the last finite-ranked value."""
import numpy as np

F32 = np.float32
FIX = 16777216.0            # 2^24: cluster sums are kept in 2^-24 fixed point


def knn(query, nodes, k):
    """query f32[B,3,Nq], nodes f32[B,3,M] -> idx i32[B,Nq,k], weights f32[B,Nq,k] = 1 - d / sum(d) (sum left to right).
    k must not exceed the number of nodes with a non-NaN distance."""
    query, nodes = np.asarray(query, F32), np.asarray(nodes, F32)
    B, _, Nq = query.shape
    with np.errstate(all="ignore"):
        dx = query[:, 0, :, None] - nodes[:, 0, None, :]
        dy = query[:, 1, :, None] - nodes[:, 1, None, :]
        dz = query[:, 2, :, None] - nodes[:, 2, None, :]
        d2 = (dx * dx + dy * dy) + dz * dz                                  # B x Nq x M, float32 throughout
        assert d2.dtype == F32
        bits = d2.view(np.uint32).astype(np.int64)                          # d^2 >= +0: unsigned bit order = float order, +inf above all
        bits[np.isnan(d2)] = np.int64(1) << 40                              # a NaN distance ranks behind everything
        win = np.argsort(bits, axis=2, kind="stable")[:, :, :k]             # (d^2, id)
        assert not np.isnan(np.take_along_axis(d2, win, 2)).any(), "k exceeds the number of nodes with a distance"
        win = np.sort(win, axis=2)                                          # by id, so that the stable sort on d below is (d, id)
        d = np.sqrt(np.take_along_axis(d2, win, 2))
        order = np.argsort(d, axis=2, kind="stable")
        idx = np.take_along_axis(win, order, 2).astype(np.int32)
        d = np.take_along_axis(d, order, 2)
        s = d[:, :, 0].copy()
        for j in range(1, k):
            s = s + d[:, :, j]
        w = F32(1.0) - d / s[:, :, None]
    assert d.dtype == F32 and w.dtype == F32
    return idx, w


def cluster_stats(pc, nearest, M):
    """pc f32[B,3,N], nearest i[B,N] -> mean f32[B,3,M], mask f32[B,M]: integer sums of round(pc * 2^24), mean = f32(sum / 2^24) / (f32(count) + 1e-5f)"""
    pc = np.asarray(pc, F32)
    B, _, N = pc.shape
    q = np.rint(pc.astype(np.float64) * FIX).astype(np.int64)
    mean, mask = np.zeros((B, 3, M), F32), np.zeros((B, M), F32)
    for b in range(B):
        cnt = np.bincount(nearest[b], minlength=M).astype(np.int64)
        den = cnt.astype(F32) + F32(1e-5)
        for c in range(3):
            s = np.zeros(M, np.int64)
            np.add.at(s, nearest[b], q[b, c])
            mean[b, c] = (s.astype(np.float64) / FIX).astype(F32) / den
        mask[b] = (cnt > 0).astype(F32)
    return mean, mask


def build_point_input(pc, intensity, sn, cluster_mean, min_idx):
    """-> centers f32[B,3,N] = cluster_mean[:, :, min_idx], aug f32[B,7,N] = cat(pc - centers, intensity, sn)"""
    pc = np.asarray(pc, F32)
    centers = np.take_along_axis(np.asarray(cluster_mean, F32), np.asarray(min_idx)[:, None, :].astype(np.int64).repeat(3, 1), 2)
    aug = np.concatenate((pc - centers, np.asarray(intensity, F32), np.asarray(sn, F32)), axis=1)
    assert aug.dtype == F32
    return centers, aug


def gather_neighbors(database, query, idx):
    """database f32[B,3,Md], query f32[B,3,Mq], idx i[B,Mq,K] -> f32[B,3,Mq*K] = database[:, :, idx] - query"""
    database, query = np.asarray(database, F32), np.asarray(query, F32)
    B, Mq, K = idx.shape
    g = np.take_along_axis(database, np.asarray(idx).reshape(B, 1, Mq * K).astype(np.int64).repeat(3, 1), 2).reshape(B, 3, Mq, K)
    out = (g - query[:, :, :, None]).reshape(B, 3, Mq * K)
    assert out.dtype == F32
    return out


def interpolate(feats, idx, weights):
    """feats f32[B,C,M], idx i[B,Nq,k], weights f32[B,Nq,k] -> f32[B,C,Nq]: acc = 0, then acc = acc + w[j] * f[idx[j]] for j ascending"""
    feats, weights = np.asarray(feats, F32), np.asarray(weights, F32)
    B, C, _ = feats.shape
    _, Nq, k = idx.shape
    acc = np.zeros((B, C, Nq), F32)
    with np.errstate(all="ignore"):
        for j in range(k):
            f = np.take_along_axis(feats, np.asarray(idx)[:, None, :, j].astype(np.int64).repeat(C, 1), 2)
            acc = acc + weights[:, None, :, j] * f
    assert acc.dtype == F32
    return acc


def argmax_channels(scores):
    """scores f32[B,C,N] -> i32[B,N]: the first NaN if there is one, otherwise the first maximum"""
    scores = np.asarray(scores, F32)
    B, C, N = scores.shape
    best, bi = scores[:, 0, :].copy(), np.zeros((B, N), np.int32)
    for c in range(1, C):
        v = scores[:, c, :]
        with np.errstate(invalid="ignore"):
            take = ~np.isnan(best) & (np.isnan(v) | (v > best))
        best = np.where(take, v, best)
        bi = np.where(take, np.int32(c), bi)
    return bi


def channel_max(x):
    """x f32[B,C,N] -> f32[B,C]: the maximum over N, NaN if any element is NaN"""
    return np.max(np.asarray(x, F32), axis=2)            # np.max propagates NaN


def bits(a):
    """float32 array -> its bit patterns with every NaN mapped to one pattern: NaN equals NaN whatever sign or payload the divider produced"""
    a = np.ascontiguousarray(a, F32)
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))
