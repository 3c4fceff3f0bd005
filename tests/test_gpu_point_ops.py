"""GPU parity of the point<->node kernels: vs plain torch restatements of the reference idioms (the first five tests, with tolerances), and
bit for bit vs tests/point_ops_oracle.py, the numpy float32 restatement of the kernels' own arithmetic (tests/test_point_ops_host.py checks
that one against fp64), on both sides of every dispatch edge."""
import numpy as np
import pytest
import torch

from tests import point_ops_cases as cases
from tests import point_ops_oracle as po

pytestmark = pytest.mark.gpu


def _scene(B, N, M, seed):
    g = torch.Generator().manual_seed(seed)
    pc = torch.randn(B, 3, N, generator=g) * 20
    sel = torch.stack([torch.randperm(N, generator=g)[:M] for _ in range(B)])
    nodes = torch.gather(pc, 2, sel.unsqueeze(1).expand(B, 3, M)).contiguous()
    return pc, nodes


def _check_knn(idx, pc, nodes, k):
    """idx must equal torch.topk up to permutations among (near-)exact distance ties."""
    d = torch.norm(pc.unsqueeze(3) - nodes.unsqueeze(2), dim=1)          # B x N x M
    dk, ik = torch.topk(d, k=k, dim=2, largest=False, sorted=True)
    mine = torch.gather(d, 2, idx.long())
    assert torch.allclose(mine, dk, rtol=1e-6, atol=1e-6)                  # same distances in the same order
    mism = (idx.long() != ik)
    if mism.any():                                                          # only allowed at ties
        assert torch.all((mine - dk).abs()[mism] <= 1e-6 * dk[mism].abs() + 1e-7)
    return float(mism.float().mean())


@pytest.mark.parametrize("B,N,M,k", [(2, 1024, 128, 3), (1, 20480, 128, 3), (2, 128, 128, 16), (3, 77, 5, 1), (2, 500, 64, 4)])
def test_knn_nodes(dev, B, N, M, k):
    from deepi2p_amd import ops
    pc, nodes = _scene(B, N, M, 10 + k)
    idx, w = ops.knn_nodes(pc.to(dev), nodes.to(dev), k, want_weights=True)
    frac = _check_knn(idx.cpu(), pc, nodes, k)
    assert frac < 1e-3
    d = torch.norm(pc.unsqueeze(3) - torch.gather(nodes.unsqueeze(2).expand(B, 3, N, M), 3,
                                                   idx.cpu().long().unsqueeze(1).expand(B, 3, N, k)), dim=1)
    w_ref = 1 - d / d.sum(dim=2, keepdim=True)
    if k > 1:
        torch.testing.assert_close(w.cpu(), w_ref, rtol=1e-5, atol=1e-6)


def test_knn_duplicate_nodes_tie_rule(dev):
    """Duplicated nodes (padding by repetition, data/kitti_pc_img_pose_loader.py:158-171) give exact ties:
    the lower node id must come first."""
    from deepi2p_amd import ops
    pc, nodes = _scene(1, 256, 16, 3)
    nodes = torch.cat((nodes, nodes), dim=2).contiguous()                  # node j == node j+16
    idx = ops.knn_nodes(pc.to(dev), nodes.to(dev), 4).cpu()
    assert torch.all(idx[:, :, 1] == idx[:, :, 0] + 16)
    assert torch.all(idx[:, :, 3] == idx[:, :, 2] + 16)


def test_cluster_stats_and_point_input(dev):
    from deepi2p_amd import ops
    B, N, M = 2, 4096, 128
    pc, nodes = _scene(B, N, M, 4)
    nodes[:, :, -3:] = 1e4                                                  # three nodes nobody is assigned to
    inten, sn = torch.rand(B, 1, N), torch.randn(B, 3, N)
    idx = ops.knn_nodes(pc.to(dev), nodes.to(dev), 3)
    mean, mask, min_idx = ops.cluster_stats(pc.to(dev), idx, M)
    mi = idx[:, :, 0].long().cpu()
    assert torch.equal(min_idx.cpu().long(), mi)
    onehot = torch.nn.functional.one_hot(mi, M).float()                     # B x N x M
    cnt = onehot.sum(1)
    ref_mean = torch.einsum("bcn,bnm->bcm", pc.double(), onehot.double()).float() / (cnt.unsqueeze(1) + 1e-5)
    torch.testing.assert_close(mean.cpu(), ref_mean, rtol=2e-6, atol=2e-5)
    assert torch.equal(mask.cpu(), (cnt > 0).float())
    assert float(mask[:, -3:].sum()) == 0 and torch.all(mean[:, :, -3:] == 0)
    centers, aug = ops.build_point_input(pc.to(dev), inten.to(dev), sn.to(dev), mean, min_idx)
    ref_c = torch.gather(mean.cpu(), 2, mi.unsqueeze(1).expand(B, 3, N))
    assert torch.equal(centers.cpu(), ref_c)
    assert torch.equal(aug.cpu(), torch.cat((pc - ref_c, inten, sn), dim=1))
    # determinism: fixed-point accumulation -> bit-identical across runs
    mean2, _, _ = ops.cluster_stats(pc.to(dev), idx, M)
    assert torch.equal(mean, mean2)


def test_interpolate_gather_argmax_channelmax(dev):
    from deepi2p_amd import ops
    g = torch.Generator().manual_seed(0)
    B, C, M, Nq, k = 2, 70, 128, 1000, 3
    feats = torch.randn(B, C, M, generator=g)
    idx = torch.randint(0, M, (B, Nq, k), generator=g, dtype=torch.int32)
    w = torch.rand(B, Nq, k, generator=g)
    out = ops.interpolate(feats.to(dev), idx.to(dev), w.to(dev)).cpu()
    gath = torch.gather(feats.unsqueeze(3).expand(B, C, M, k), 2, idx.long().unsqueeze(1).expand(B, C, Nq, k))
    torch.testing.assert_close(out, (w.unsqueeze(1) * gath).sum(3), rtol=1e-5, atol=1e-6)
    # many columns (training: 20480 points) run the kernel that keeps the 32-channel table slice in LDS: the same sums in the same order, i.e.
    # the same bits as the gather-from-memory kernel on the same columns (which the first 1000 columns alone still select)
    for kk, Nl in ((3, 2500), (1, 1024), (4, 1500)):
        idx_l = torch.randint(0, M, (B, Nl, kk), generator=g, dtype=torch.int32)
        w_l = torch.rand(B, Nl, kk, generator=g)
        big = ops.interpolate(feats.to(dev), idx_l.to(dev), w_l.to(dev)).cpu()
        small = ops.interpolate(feats.to(dev), idx_l[:, :1000].contiguous().to(dev), w_l[:, :1000].contiguous().to(dev)).cpu()
        assert torch.equal(big[:, :, :1000], small)
        g_l = torch.gather(feats.unsqueeze(3).expand(B, C, M, kk), 2, idx_l.long().unsqueeze(1).expand(B, C, Nl, kk))
        torch.testing.assert_close(big, (w_l.unsqueeze(1) * g_l).sum(3), rtol=1e-5, atol=1e-6)
    db, q = torch.randn(B, 3, M, generator=g), torch.randn(B, 3, 50, generator=g)
    kn = torch.randint(0, M, (B, 50, 16), generator=g, dtype=torch.int32)
    gn = ops.gather_neighbors(db.to(dev), q.to(dev), kn.to(dev)).cpu().view(B, 3, 50, 16)
    ref = torch.gather(db, 2, kn.long().view(B, 1, 800).expand(B, 3, 800)).view(B, 3, 50, 16) - q.unsqueeze(3)
    assert torch.equal(gn, ref)
    s = torch.randn(B, 82, 777, generator=g)
    s[0, 5, 10] = s[0, 3, 10] = 99.0                                         # tie -> first (lowest channel) wins
    am = ops.argmax_channels(s.to(dev)).cpu()
    assert torch.equal(am.long(), torch.max(s, dim=1)[1]) and am[0, 10] == 3
    sl = s.to(dev)[:, 2:, :]                                                 # channel slice with foreign batch stride
    assert torch.equal(ops.argmax_channels(sl).cpu().long(), torch.max(s[:, 2:, :], dim=1)[1])
    assert torch.equal(ops.channel_max(s.to(dev)).cpu(), s.max(dim=2)[0])
    for n in (1, 3, 16, 33, 64, 65):                                         # short rows share a wavefront
        t = torch.randn(3, 37, n, generator=g)
        assert torch.equal(ops.channel_max(t.to(dev)).cpu(), t.max(dim=2)[0])


# ------------------------------------------------------------------------------------------------ exact, against tests/point_ops_oracle.py
def _t(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)                                # a copy: the shared scenes are read-only


def _knn_equals_oracle(dev, q, n, k):
    from deepi2p_amd import ops
    idx, w = ops.knn_nodes(_t(q, dev), _t(n, dev), k, want_weights=True)
    idx2 = ops.knn_nodes(_t(q, dev), _t(n, dev), k)                        # the launch without weights selects the same neighbours
    ref_i, ref_w = po.knn(q, n, k)
    idx, w = idx.cpu().numpy(), w.cpu().numpy()
    np.testing.assert_array_equal(idx, ref_i)
    np.testing.assert_array_equal(idx2.cpu().numpy(), ref_i)
    np.testing.assert_array_equal(po.bits(w), po.bits(ref_w))              # as bit patterns: NaN (d = 0 with k = 1, inf / inf) equals NaN
    return idx, w


def _knn_scene_properties(q, n, k, idx, w):
    """what the scene is there for, stated on the device's result (which already equals the oracle's)"""
    B, _, M = n.shape
    if M - 1 >= k:
        assert np.isnan(n[0, 1, M // 3]) and not (idx[0] == M // 3).any()   # the node with the NaN coordinate is never selected
    if k == M and M >= 2:
        assert (idx[B - 1, :, k - 1] == M - 1).all() and np.isnan(w[B - 1, :, k - 1]).all()      # the node at 3e19: last, still selected
    on_node = (q[:, :, :, None] == n[:, :, None, :]).all(1).any(2)          # B x Nq: the query coincides with a node
    assert on_node.mean() > 0.3
    if k == 1:
        assert np.isnan(w[on_node]).all()                                   # d = 0: 1 - 0 / 0


@pytest.mark.parametrize("B,Nq,M,k", cases.KNN_LANE)
def test_knn_lane_kernel_equals_oracle(dev, B, Nq, M, k):
    assert not cases.is_wave(Nq, M)
    q, n = cases.edge_scene(B, Nq, M, k, cases.KNN_SEEDS[(B, Nq, M, k)])
    idx, w = _knn_equals_oracle(dev, q, n, k)
    _knn_scene_properties(q, n, k, idx, w)


@pytest.mark.parametrize("B,Nq,M,k", cases.KNN_WAVE)
def test_knn_wave_kernel_equals_oracle(dev, B, Nq, M, k):
    assert cases.is_wave(Nq, M)
    q, n = cases.edge_scene(B, Nq, M, k, cases.KNN_SEEDS[(B, Nq, M, k)])
    idx, w = _knn_equals_oracle(dev, q, n, k)
    _knn_scene_properties(q, n, k, idx, w)


@pytest.mark.parametrize("k", [1, 2])
def test_knn_one_tie_rule_on_both_kernels(dev, k):
    """Nodes whose squared distances differ by an ulp while their roots round to the same float: the first 1024 queries run on the wave kernel,
    the same queries plus one more on the lane kernel.  Both select by (d^2, id) and order by (d, id): equal to the oracle, hence to each other.
    (A wave kernel that selects by the rounded root returns node 0 where the rule says node 1 at k = 1.)"""
    q, n = cases.tie_scene()
    qw = np.ascontiguousarray(q[:, :, :1024])
    assert cases.is_wave(1024, 8) and not cases.is_wave(1025, 8)
    iw, ww = _knn_equals_oracle(dev, qw, n, k)
    il, wl = _knn_equals_oracle(dev, q, n, k)
    np.testing.assert_array_equal(iw, il[:, :1024])
    np.testing.assert_array_equal(ww.view(np.uint32), wl[:, :1024].view(np.uint32))          # both from the device: bit-identical, NaN included
    assert iw[0, [0, 511, 1023]].tolist() == ([[1]] * 3 if k == 1 else [[0, 1]] * 3)


@pytest.mark.parametrize("B,N,M,stride", cases.CLUSTER)
def test_cluster_stats_equals_oracle(dev, B, N, M, stride):
    from deepi2p_amd import ops
    pc, idx = cases.cluster_scene(B, N, M, stride)
    mean, mask, min_idx = ops.cluster_stats(_t(pc, dev), _t(idx, dev), M)
    mean2, mask2, min_idx2 = ops.cluster_stats(_t(pc, dev), _t(idx, dev), M)
    assert torch.equal(mean, mean2) and torch.equal(mask, mask2) and torch.equal(min_idx, min_idx2)     # integer sums: run-to-run identical
    ref_mean, ref_mask = po.cluster_stats(pc, idx[:, :, 0], M)
    np.testing.assert_array_equal(min_idx.cpu().numpy(), idx[:, :, 0])
    np.testing.assert_array_equal(mean.cpu().numpy().view(np.uint32), ref_mean.view(np.uint32))
    np.testing.assert_array_equal(mask.cpu().numpy(), ref_mask)
    s64, cnt, mean64 = cases.cluster_mean64(pc, idx[:, :, 0], M)
    assert np.all(np.abs(mean.cpu().numpy().astype(np.float64) - mean64) <= cases.cluster_bound(s64, cnt))


@pytest.mark.parametrize("N", [1, 255, 257])
def test_build_point_input_equals_oracle(dev, N):
    from deepi2p_amd import ops
    g = np.random.default_rng(N)
    B, M = 2, 37
    pc, inten, sn = (g.standard_normal(s).astype(np.float32) * 20 for s in ((B, 3, N), (B, 1, N), (B, 3, N)))
    mean = g.standard_normal((B, 3, M)).astype(np.float32) * 20
    mi = g.integers(0, M, (B, N)).astype(np.int32)
    centers, aug = ops.build_point_input(_t(pc, dev), _t(inten, dev), _t(sn, dev), _t(mean, dev), _t(mi, dev))
    ref_c, ref_a = po.build_point_input(pc, inten, sn, mean, mi)
    np.testing.assert_array_equal(centers.cpu().numpy().view(np.uint32), ref_c.view(np.uint32))
    np.testing.assert_array_equal(aug.cpu().numpy().view(np.uint32), ref_a.view(np.uint32))


@pytest.mark.parametrize("Mq,K", [(1, 1), (255, 1), (300, 1), (17, 15), (25, 12)])
def test_gather_neighbors_equals_oracle(dev, Mq, K):
    from deepi2p_amd import ops
    g = np.random.default_rng(Mq * K + K)
    B, Md = 2, 37                                                               # Md != Mq
    db, q = g.standard_normal((B, 3, Md)).astype(np.float32) * 20, g.standard_normal((B, 3, Mq)).astype(np.float32) * 20
    idx = g.integers(0, Md, (B, Mq, K)).astype(np.int32)
    out = ops.gather_neighbors(_t(db, dev), _t(q, dev), _t(idx, dev))
    assert tuple(out.shape) == (B, 3, Mq * K)
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), po.gather_neighbors(db, q, idx).view(np.uint32))


@pytest.mark.parametrize("B,C,M,Nq,k", cases.INTERP)
def test_interpolate_equals_oracle(dev, B, C, M, Nq, k):
    """both sides of k <= 4, M <= 512, Nq >= 1024 (the kernel with the table slice in LDS): each equals the oracle, so they equal each other"""
    from deepi2p_amd import ops
    feats, idx, w = cases.interp_scene(B, C, M, Nq, k)
    out = ops.interpolate(_t(feats, dev), _t(idx, dev), _t(w, dev)).cpu().numpy()
    np.testing.assert_array_equal(out.view(np.uint32), po.interpolate(feats, idx, w).view(np.uint32))


@pytest.mark.parametrize("C,N", [(1, 257), (82, 257), (5, 1)])
def test_argmax_channels_nan_equals_oracle(dev, C, N):
    from deepi2p_amd import ops
    g = np.random.default_rng(C + N)
    s = g.standard_normal((3, C, N)).astype(np.float32)
    s[0, 0, 0] = np.nan                                                          # a NaN in channel 0
    if C > 4:
        s[1, C // 2, N // 2] = np.nan                                            # in a middle channel
        s[2, 2, N - 1] = s[2, C - 1, N - 1] = np.nan                             # in two channels: the first wins
        s[2, 1, 0] = s[2, 3, 0] = 50.0                                           # two maxima: the first wins (N = 1: behind the NaN)
    am = ops.argmax_channels(_t(s, dev)).cpu().numpy()
    np.testing.assert_array_equal(am, po.argmax_channels(s))
    assert am[0, 0] == 0
    if C > 4:
        assert am[1, N // 2] == C // 2 and am[2, N - 1] == 2 and am[2, 0] == (1 if N > 1 else 2)


@pytest.mark.parametrize("C,N", [(1, 257), (37, 1), (37, 16), (37, 33), (37, 64), (37, 65), (5, 1000)])
def test_channel_max_nan_equals_oracle(dev, C, N):
    from deepi2p_amd import ops
    g = np.random.default_rng(C * 1000 + N)
    x = g.standard_normal((3, C, N)).astype(np.float32)
    x[0, 0, N - 1] = np.nan
    x[1, C // 2, N // 2] = np.nan
    x[1, C // 2, 0] = np.inf                                                     # NaN beats +inf
    x[2, C - 1, :] = -np.inf                                                     # a row of -inf gives -inf
    got = ops.channel_max(_t(x, dev)).cpu().numpy()
    np.testing.assert_array_equal(po.bits(got), po.bits(po.channel_max(x)))
    np.testing.assert_array_equal(np.isnan(got), np.isnan(x).any(2))             # NaN if and only if the row has one
    assert got[2, C - 1] == -np.inf


def test_point_ops_argument_checks(dev):
    """dtype / shape disagreements are refused on the host, before any pointer reaches the library; the size limits by the library, before
    any launch.  No operand here is ever read by a kernel."""
    from deepi2p_amd import _lib, ops
    f = lambda *s: torch.zeros(*s, device=dev)
    i = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dev)
    bad = [
        lambda: ops.knn_nodes(f(2, 3, 8).double(), f(2, 3, 4), 2),
        lambda: ops.knn_nodes(f(2, 3, 8), f(2, 3, 4).double(), 2),
        lambda: ops.knn_nodes(f(2, 3, 8), f(1, 3, 4), 2),                        # B
        lambda: ops.knn_nodes(f(2, 8, 3), f(2, 3, 4), 2),
        lambda: ops.knn_nodes(f(1, 3, 8), f(1, 3, 4097), 2),                     # M
        lambda: ops.cluster_stats(f(2, 3, 8).double(), i(2, 8, 3), 4),
        lambda: ops.cluster_stats(f(2, 3, 8), i(2, 8, 3).long(), 4),
        lambda: ops.cluster_stats(f(2, 3, 8), i(2, 9, 3), 4),                    # N
        lambda: ops.cluster_stats(f(2, 3, 8), i(1, 8, 3), 4),                    # B
        lambda: ops.build_point_input(f(2, 3, 8), f(2, 1, 8), f(2, 3, 8), f(2, 3, 4), i(2, 8).long()),
        lambda: ops.build_point_input(f(2, 3, 8).double(), f(2, 1, 8), f(2, 3, 8), f(2, 3, 4), i(2, 8)),
        lambda: ops.build_point_input(f(2, 3, 8), f(2, 1, 9), f(2, 3, 8), f(2, 3, 4), i(2, 8)),
        lambda: ops.build_point_input(f(2, 3, 8), f(2, 1, 8), f(2, 3, 8), f(1, 3, 4), i(2, 8)),
        lambda: ops.build_point_input(f(2, 3, 8), f(2, 1, 8), f(2, 3, 8), f(2, 3, 4), i(2, 7)),
        lambda: ops.interpolate(f(2, 5, 4), i(2, 8, 3).long(), f(2, 8, 3)),
        lambda: ops.interpolate(f(2, 5, 4).double(), i(2, 8, 3), f(2, 8, 3)),
        lambda: ops.interpolate(f(2, 5, 4), i(2, 8, 3), f(2, 8, 2)),             # k
        lambda: ops.interpolate(f(2, 5, 4), i(2, 8, 3), f(2, 9, 3)),             # Nq
        lambda: ops.interpolate(f(2, 5, 4), i(1, 8, 3), f(1, 8, 3)),             # B
        lambda: ops.gather_neighbors(f(2, 3, 4), f(2, 3, 6), i(2, 6, 3).long()),
        lambda: ops.gather_neighbors(f(2, 3, 4).double(), f(2, 3, 6), i(2, 6, 3)),
        lambda: ops.gather_neighbors(f(2, 3, 4), f(2, 3, 6), i(2, 5, 3)),        # a [B, N, k] index against a [B, 3, N'] cloud
        lambda: ops.gather_neighbors(f(2, 3, 4), f(1, 3, 6), i(2, 6, 3)),
        lambda: ops.channel_max(f(2, 3, 8).double()),
        lambda: ops.channel_max(f(2, 3)),
    ]
    for n, fn in enumerate(bad):
        with pytest.raises(RuntimeError) as e:
            fn()
        assert n == 4 or not isinstance(e.value, _lib.DeepI2PHipError), "case %d reached the library" % n
    with pytest.raises(_lib.DeepI2PHipError, match="4096"):
        ops.knn_nodes(f(1, 3, 8), f(1, 3, 4097), 2)
    with pytest.raises(_lib.DeepI2PHipError, match="M too large"):
        ops.cluster_stats(f(1, 3, 8), i(1, 8, 1), 2049)
