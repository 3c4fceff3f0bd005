"""CPU: tests/point_ops_oracle.py (the float32 restatement that tests/test_gpu_point_ops.py holds the kernels to, bit for bit) against fp64
brute force, so that the GPU tests do not rest on an unchecked reference.  Bounds are derived from the number of fp32 roundings, not measured."""
import numpy as np
import pytest
import torch

from tests import point_ops_cases as cases
from tests import point_ops_oracle as po

# A term of d^2 = (dx*dx + dy*dy) + dz*dz passes at most five roundings (its difference, which counts twice in the square, its product, two
# sums): d^2 is within 5 * 2^-24 relative, its root within 2.5 * 2^-24, the rounding of the root adds one: 3.5 * 2^-24 < 2^-22 for the
# computed distance, and each side of a comparison may be off by that: 2^-21.
SLACK = 2.0 ** -21


def _dist64(q, n):
    with np.errstate(all="ignore"):
        d = np.sqrt(((q.astype(np.float64)[:, :, :, None] - n.astype(np.float64)[:, :, None, :]) ** 2).sum(1))     # B x Nq x M
    return np.where(np.isnan(d), np.inf, d)                                                                         # a NaN node is never a neighbour


@pytest.mark.parametrize("shape", cases.KNN_LANE + cases.KNN_WAVE)
@pytest.mark.parametrize("scene", ["plain", "edge"])
def test_knn_oracle_vs_fp64_distances(shape, scene):
    B, Nq, M, k = shape
    q, n = cases.plain_scene(B, Nq, M, cases.KNN_SEEDS[shape]) if scene == "plain" else cases.edge_scene(B, Nq, M, k, cases.KNN_SEEDS[shape])
    idx, w = po.knn(q, n, k)
    assert idx.shape == w.shape == (B, Nq, k) and idx.dtype == np.int32 and w.dtype == np.float32
    assert idx.min() >= 0 and idx.max() < M
    assert all(len(set(row)) == k for row in idx.reshape(-1, k)), "a node was returned twice"
    d64 = _dist64(q, n)
    assert np.isfinite(d64).sum(2).min() >= k
    mine = np.take_along_axis(d64, idx.astype(np.int64), 2)
    assert np.isfinite(mine).all(), "a node with a NaN coordinate was selected"
    assert np.all(mine[:, :, 1:] >= mine[:, :, :-1] * (1 - SLACK)), "winners not in ascending fp64 distance"
    kth = np.sort(d64, axis=2)[:, :, k - 1]
    assert np.all(mine.max(2) <= kth * (1 + SLACK)), "the k-th winner is farther than the fp64 k-th smallest distance"


def test_knn_oracle_rows_equal_fp64_topk():
    """On scenes without engineered ties (exact fp64 ties leave torch.topk's order open) the oracle's index rows are torch.topk's on fp64
    distances, up to a share of 1e-3 of the queries."""
    differ = total = 0
    for shape in cases.KNN_LANE + cases.KNN_WAVE:
        B, Nq, M, k = shape
        q, n = cases.plain_scene(B, Nq, M, cases.KNN_SEEDS[shape])
        idx, _ = po.knn(q, n, k)
        ik = torch.topk(torch.from_numpy(_dist64(q, n)), k=k, dim=2, largest=False, sorted=True)[1].numpy()
        differ += int((idx != ik).any(2).sum())
        total += B * Nq
    print("knn oracle vs fp64 topk: %d of %d query rows differ" % (differ, total))
    assert differ <= 1e-3 * total


def test_knn_oracle_engineered_tie():
    """d^2 an ulp apart, equal rounded roots: selection is by d^2 (k = 1 -> node 1), order by (d, id) (k = 2 -> [0, 1])"""
    q = np.zeros((1, 3, 1), np.float32)
    n = np.array([cases.TIE_NODE0, cases.TIE_NODE1], np.float32).T[None].copy()
    d2 = ((q[0, :, 0, None] - n[0]) ** 2).astype(np.float32)
    d2 = (d2[0] + d2[1]) + d2[2]
    assert d2.view(np.uint32).tolist() == [0x3F800001, 0x3F800000] and np.sqrt(d2).tolist() == [1.0, 1.0]
    assert po.knn(q, n, 1)[0].tolist() == [[[1]]]
    i2, w2 = po.knn(q, n, 2)
    assert i2.tolist() == [[[0, 1]]] and w2.tolist() == [[[0.5, 0.5]]]
    qt, nt = cases.tie_scene()
    assert np.array_equal(qt[0, :, [0, 511, 1023]], np.zeros((3, 3), np.float32))
    assert po.knn(qt, nt, 1)[0][0, [0, 511, 1023], 0].tolist() == [1, 1, 1]
    assert po.knn(qt, nt, 2)[0][0, [0, 511, 1023]].tolist() == [[0, 1]] * 3
    # the scene is worth running: a good share of its rows see the pair at equal rounded distances but different squared ones
    dx, dy, dz = (qt[0, c, :, None] - nt[0, c, None, :2] for c in range(3))
    d2 = (dx * dx + dy * dy) + dz * dz
    straddle = (d2[:, 0] != d2[:, 1]) & (np.sqrt(d2[:, 0]) == np.sqrt(d2[:, 1]))
    assert straddle[:1024].sum() >= 50


@pytest.mark.parametrize("B,N,M,stride", cases.CLUSTER)
def test_cluster_oracle_vs_fp64_mean(B, N, M, stride):
    pc, idx = cases.cluster_scene(B, N, M, stride)
    nearest = idx[:, :, 0]
    mean, mask = po.cluster_stats(pc, nearest, M)
    s64, cnt, mean64 = cases.cluster_mean64(pc, nearest, M)
    assert mean.dtype == np.float32 and np.array_equal(mask, (cnt > 0).astype(np.float32))
    assert np.all(np.abs(mean.astype(np.float64) - mean64) <= cases.cluster_bound(s64, cnt))
    assert np.all(mean[:, :, 3::5] == 0) and np.all(mask[:, 3::5] == 0)                    # the empty clusters
    if M > 1 and N > 1:
        assert np.all(cnt[:, M - 1] == 1)                                                   # the one-point cluster
    if N > 2:                                                                               # 1e-9 quantises to 0, 1e4 is kept
        assert np.all(np.rint(pc[:, 1:, 2].astype(np.float64) * po.FIX) == 0) and np.all(pc[:, 0, 1] == np.float32(1e4))


@pytest.mark.parametrize("B,C,M,Nq,k", cases.INTERP)
def test_interpolate_oracle_vs_fp64(B, C, M, Nq, k):
    feats, idx, w = cases.interp_scene(B, C, M, Nq, k)
    out = po.interpolate(feats, idx, w)
    g = np.take_along_axis(feats.astype(np.float64)[:, :, :, None].repeat(k, 3), idx.astype(np.int64)[:, None].repeat(C, 1), 2)    # B x C x Nq x k
    terms = w.astype(np.float64)[:, None] * g
    assert out.dtype == np.float32
    assert np.all(np.abs(out.astype(np.float64) - terms.sum(3)) <= (k + 1) * 2.0 ** -24 * np.abs(terms).sum(3))
    hit = (idx == 0).all(2)                                                                 # only the -0.0 column, weight 0: +0 comes out
    assert not np.signbit(out[np.broadcast_to(hit[:, None, :], out.shape)]).any()


def test_small_oracles():
    g = np.random.default_rng(5)
    pc, inten, sn = (g.standard_normal(s).astype(np.float32) for s in ((2, 3, 9), (2, 1, 9), (2, 3, 9)))
    mean = g.standard_normal((2, 3, 4)).astype(np.float32)
    mi = g.integers(0, 4, (2, 9)).astype(np.int32)
    centers, aug = po.build_point_input(pc, inten, sn, mean, mi)
    for b in range(2):
        for i in range(9):
            assert np.array_equal(centers[b, :, i], mean[b, :, mi[b, i]]) and np.array_equal(aug[b, :3, i], pc[b, :, i] - mean[b, :, mi[b, i]])
    assert np.array_equal(aug[:, 3:4], inten) and np.array_equal(aug[:, 4:], sn)
    idx = g.integers(0, 4, (2, 5, 3)).astype(np.int32)
    qn = g.standard_normal((2, 3, 5)).astype(np.float32)
    gn = po.gather_neighbors(mean, qn, idx).reshape(2, 3, 5, 3)
    for b in range(2):
        for m in range(5):
            for j in range(3):
                assert np.array_equal(gn[b, :, m, j], mean[b, :, idx[b, m, j]] - qn[b, :, m])
    s = np.array([[[1, 5, np.nan, 2], [3, 5, 0, np.nan], [np.nan, 7, np.nan, 2]]], np.float32).transpose(0, 2, 1).copy()    # [1, C=4, N=3]
    assert po.argmax_channels(s).tolist() == [[2, 3, 0]]
    assert po.argmax_channels(np.array([[[1], [9], [9], [3]]], np.float32)).tolist() == [[1]]
    cm = po.channel_max(np.array([[[1, np.nan, 3], [-np.inf, -np.inf, -np.inf], [2, 7, 7]]], np.float32))
    assert np.isnan(cm[0, 0]) and cm[0, 1] == -np.inf and cm[0, 2] == 7
    assert po.bits(np.array([np.nan, -np.nan, 0.0, -0.0], np.float32)).tolist() == [0x7FC00000, 0x7FC00000, 0, 0x80000000]
