"""Shapes and scenes shared by tests/test_point_ops_host.py (the oracle against fp64) and tests/test_gpu_point_ops.py (the kernels against the
oracle).  Everything is generated on the CPU from a seeded torch generator and handed out as numpy arrays."""
import functools

import numpy as np
import torch

# (B, Nq, M, k).  di2p_knn_nodes runs one wavefront per query when M <= 256 and Nq <= 1024, one lane per query otherwise.
KNN_LANE = [(2, 1025, 5, 1),          # Nq one past the limit
            (1, 1300, 131, 3),        # M % 4 == 3: the unrolled scan's tail
            (2, 7, 257, 4),           # lane path through M > 256, one partial workgroup
            (1, 40, 300, 16),
            (1, 64, 4096, 2)]         # the largest M
KNN_WAVE = [(2, 1024, 256, 16),       # both limits
            (3, 5, 65, 3),            # last workgroup has one live wave, lane 0 holds a second key
            (1, 1, 16, 16),           # k == M
            (2, 9, 1, 1),
            (2, 500, 64, 4)]
KNN_SEEDS = {s: 1 + i for i, s in enumerate(KNN_LANE + KNN_WAVE)}


def is_wave(Nq, M):
    return M <= 256 and Nq <= 1024


def _plain(B, Nq, M, seed):
    """the generator of test_gpu_point_ops._scene (nodes drawn from the cloud) where the cloud has enough points, independent nodes otherwise"""
    g = torch.Generator().manual_seed(seed)
    pc = torch.randn(B, 3, Nq, generator=g) * 20
    if Nq >= M:
        sel = torch.stack([torch.randperm(Nq, generator=g)[:M] for _ in range(B)])
        nodes = torch.gather(pc, 2, sel.unsqueeze(1).expand(B, 3, M)).contiguous()
    else:
        nodes = torch.randn(B, 3, M, generator=g) * 20
    return pc.numpy(), nodes.numpy()


@functools.lru_cache(maxsize=None)
def plain_scene(B, Nq, M, seed):
    q, n = _plain(B, Nq, M, seed)
    q.setflags(write=False)
    n.setflags(write=False)
    return q, n


@functools.lru_cache(maxsize=None)
def edge_scene(B, Nq, M, k, seed):
    """plain scene plus: every second query coincides with a node (d = 0); frame 0 repeats a quarter of its nodes; the last frame has four nodes at
    exactly (0,0,0) (what cluster_mean holds for empty clusters); one node of frame 0 has a NaN coordinate where k still fits into the finite
    ones; one node of the last frame sits at 3e19, so its d^2 overflows to +inf."""
    q, n = _plain(B, Nq, M, seed)
    if M >= 8:
        n[0, :, M // 2:M // 2 + M // 4] = n[0, :, :M // 4]                 # duplicated nodes
        n[B - 1, :, M - 7:M - 3] = 0.0                                     # four nodes at the origin
    for b in range(B):
        rows = np.arange(0, Nq, 2)
        q[b][:, rows] = n[b][:, (rows * 7 + b) % M]                         # d = 0 to that node (and to its duplicate)
    if M - 1 >= k:
        n[0, 1, M // 3] = np.nan                                            # never selected
    if M >= 2:
        n[B - 1, 0, M - 1] = 3e19                                           # ranks last among the nodes with a distance, still selectable
    q.setflags(write=False)
    n.setflags(write=False)
    return q, n


TIE_NODE0, TIE_NODE1 = (1.0, 3.4e-4, 0.0), (1.0, 0.0, 0.0)    # from the origin: d^2 bits 0x3F800001 and 0x3F800000, both roots round to 1.0f


@functools.lru_cache(maxsize=None)
def tie_scene():
    """query f32[1,3,1025], nodes f32[1,3,8].  Nodes 0 and 1 are the engineered pair, nodes 2..7 are far away.  Rows 0, 511 and 1023 are the
    origin; the other rows lie near the plane y = 1.7e-4 that is equidistant from the pair, so that their two squared distances are equal or
    an ulp or two apart.  The first 1024 rows alone run on the wave kernel, all 1025 on the lane kernel."""
    g = torch.Generator().manual_seed(77)
    q = torch.randn(1, 3, 1025, generator=g) * 0.5
    q[0, 1] = 1.7e-4 + torch.randn(1025, generator=g) * 2e-4
    q[0, :, [0, 511, 1023]] = 0.0
    n = torch.zeros(1, 3, 8)
    n[0, :, 0] = torch.tensor(TIE_NODE0)
    n[0, :, 1] = torch.tensor(TIE_NODE1)
    n[0, :, 2:] = 100.0 + 10.0 * torch.arange(6).float().view(1, 6) + torch.randn(3, 6, generator=g)
    q, n = q.numpy(), n.numpy()
    q.setflags(write=False)
    n.setflags(write=False)
    return q, n


# (B, N, M, idx_stride)
CLUSTER = [(2, 1, 1, 1), (3, 1023, 7, 3), (2, 1025, 128, 3), (1, 4096, 2048, 1)]


@functools.lru_cache(maxsize=None)
def cluster_scene(B, N, M, stride):
    """pc f32[B,3,N] with negative coordinates, one of 1e4 and one of 1e-9 (quantises to 0); idx i32[B,N,stride] whose column 0 leaves
    every cluster with id % 5 == 3 empty and gives cluster M-1 exactly one point."""
    g = torch.Generator().manual_seed(100 + N)
    pc = (torch.randn(B, 3, N, generator=g) * 20).numpy()
    if N > 2:
        pc[:, 0, 1] = 1e4
        pc[:, 1, 2] = 1e-9
        pc[:, 2, 2] = -1e-9
    allowed = np.array([i for i in range(M) if i % 5 != 3 and i != M - 1] or [0])
    idx = torch.randint(0, M, (B, N, stride), generator=g, dtype=torch.int32).numpy()
    idx[:, :, 0] = allowed[torch.randint(0, len(allowed), (B, N), generator=g).numpy()]
    if M > 1 and N > 1:
        idx[:, 0, 0] = M - 1
    pc.setflags(write=False)
    idx.setflags(write=False)
    return pc, idx


def cluster_mean64(pc, nearest, M):
    """fp64 sums, counts and means sum / (count + 1e-5) of the unquantised coordinates"""
    B = pc.shape[0]
    s, cnt = np.zeros((B, 3, M)), np.zeros((B, M))
    for b in range(B):
        cnt[b] = np.bincount(nearest[b], minlength=M)
        for c in range(3):
            np.add.at(s[b, c], nearest[b], pc[b, c].astype(np.float64))
    return s, cnt, s / (cnt[:, None, :] + 1e-5)


def cluster_bound(s64, cnt):
    """count * 2^-25 (half a quantisation step per point) + three fp32 roundings of the sum, over the denominator"""
    return (cnt[:, None, :] * 2.0 ** -25 + 3 * 2.0 ** -24 * np.abs(s64)) / (cnt[:, None, :] + 1e-5)


# (B, C, M, Nq, k).  di2p_interpolate keeps the table slice in LDS when k <= 4, M <= 512 and Nq >= 1024.
INTERP = [(2, 70, 128, 1023, 3), (2, 70, 128, 1024, 3), (2, 70, 128, 1025, 3),
          (1, 33, 512, 1024, 3), (1, 33, 513, 1024, 3),
          (2, 1, 128, 1024, 4), (2, 1, 128, 1024, 5),
          (1, 33, 64, 1300, 1), (1, 33, 64, 1300, 2), (1, 70, 7, 1, 4)]


@functools.lru_cache(maxsize=None)
def interp_scene(B, C, M, Nq, k):
    """feats f32[B,C,M], idx i32[B,Nq,k], weights f32[B,Nq,k]; table column 0 is -0.0 and every entry that points at it has weight 0"""
    g = torch.Generator().manual_seed(1000 * k + M + Nq)
    feats = torch.randn(B, C, M, generator=g).numpy()
    idx = torch.randint(0, M, (B, Nq, k), generator=g, dtype=torch.int32).numpy()
    w = torch.rand(B, Nq, k, generator=g).numpy()
    feats[:, :, 0] = -0.0
    w[idx == 0] = 0.0
    for a in (feats, idx, w):
        a.setflags(write=False)
    return feats, idx, w
