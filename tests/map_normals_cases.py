"""The map the map-normals tests share (tests/test_map_normals_host.py, tests/test_gpu_map_normals.py); host only.

normals_map: about 4.5 k float32 rows whose coordinates are multiples of 2^-6, so every d2 is exact in fp64 and the neighbour rule gives the
same answer in any operation order.  It holds
  - 2500 rows on the tilted plane h = x / 4 - y / 8 (+ 0 or +-2^-6) over 6 m x 6 m, on a lattice: many equal distances, ties at the cut;
  - a 600-row wall at x = 5 (+ 0 or +-2^-6) that stands on the plane;
  - a clump of 1200 rows in a 0.5 m cube at negative coordinates: every query near it has more candidates in its 27 cells than the cells
    kernel of scan_prep.hip stages (960), and far more inside the ball than max_nn;
  - two isolated rows (count 1) and a pair 0.25 m apart (count 2): the fallback normal;
  - a 9 x 9 x 3 lattice of step 0.125;
  - exact duplicates of plane and clump rows (distinct neighbours at distance 0);
the rows shuffled, so that a row's number says nothing about its cell.  reference() computes the brute-force oracle once."""
import functools

import numpy as np

from tests import map_normals_oracle as oracle

Q = 2.0 ** -6
RADIUS, MAX_NN = 0.6, 30
SHIFT = np.array([19.0, 7.0, 33.0]) * Q          # exact in float32 and no multiple of the cell edge: the grid lands elsewhere


@functools.lru_cache(maxsize=None)
def _map(seed):
    rng = np.random.default_rng(seed)
    # plane: x on multiples of 2^-4, y on multiples of 2^-3, so that x / 4 - y / 8 is a multiple of 2^-6
    site = rng.choice(96 * 48, 2500, replace=False)
    x, y = (site // 48) / 16.0, (site % 48) / 8.0
    plane = np.stack([x, y, x / 4.0 - y / 8.0 + rng.integers(-1, 2, len(x)) * Q], 1)
    site = rng.choice(96 * 48, 600, replace=False)
    wall = np.stack([5.0 + rng.integers(-1, 2, 600) * Q, (site // 48) / 16.0, 0.625 + (site % 48) / 16.0], 1)
    site = rng.choice(32 ** 3, 1200, replace=False)
    clump = np.array([-3.0, -3.5, -1.0]) + np.stack([site // 1024, (site // 32) % 32, site % 32], 1) * Q
    lone = np.array([[20.0, 20.0, 5.0], [-20.0, 9.0, 1.0], [12.0, -7.0, 0.0], [12.25, -7.0, 0.0]])
    g = np.arange(9) * 0.125
    lattice = np.array([-6.0, 3.0, 0.5]) + np.stack(np.meshgrid(g, g, g[:3], indexing="ij"), -1).reshape(-1, 3)
    dup = np.concatenate([plane[rng.choice(len(plane), 20, replace=False)], clump[rng.choice(len(clump), 5, replace=False)]])
    xyz = np.concatenate([plane, wall, clump, lone, lattice, dup])
    assert np.array_equal(xyz, np.round(xyz / Q) * Q)
    p = np.concatenate([xyz, rng.random((len(xyz), 1))], 1).astype(np.float32)
    return p[rng.permutation(len(p))]


def normals_map(seed=11):
    """f32[M,4] (a copy)"""
    return _map(seed).copy()


@functools.lru_cache(maxsize=None)
def reference(seed=11):
    """dict(points, cnt i32[M], idx i32[M,MAX_NN], tie bool[M]): the brute-force neighbours of normals_map at (RADIUS, MAX_NN), computed once;
    tie: the MAX_NN-th and (MAX_NN + 1)-th distances are exactly equal"""
    p = normals_map(seed)
    pos = oracle.positions(p)
    c2, n2 = oracle.neighbors(p, RADIUS, MAX_NN + 1)
    d = oracle.spo.d2(pos[np.where(n2 >= 0, n2, 0)], pos[:, None, :])
    tie = (c2 == MAX_NN + 1) & (d[:, MAX_NN - 1] == d[:, MAX_NN])
    cnt, idx = np.minimum(c2, MAX_NN).astype(np.int32), n2[:, :MAX_NN].copy()
    for a in (cnt, idx, tie):
        a.setflags(write=False)
    return dict(points=p, cnt=cnt, idx=idx, tie=tie)


def lattice_scan(seed=3, n=3000):
    """f32[n',4]: a scan on the 2^-6 lattice without duplicates, 8 m x 8 m of gently rolling ground with a box on it: as a single frame for
    scan_prep.voxel_down_sample with a voxel below 2^-6, every point is a voxel of its own and its centroid is the point"""
    rng = np.random.default_rng(seed)
    xy = rng.integers(-256, 256, (n, 2)) * Q
    h = np.round((0.2 * np.sin(xy[:, 0]) + 0.1 * xy[:, 1]) / Q) * Q
    box = np.stack([rng.integers(0, 64, 600) * Q, rng.integers(0, 64, 600) * Q, rng.integers(0, 96, 600) * Q], 1)
    xyz = np.unique(np.concatenate([np.concatenate([xy, h[:, None]], 1), box]), axis=0)
    xyz = xyz[rng.permutation(len(xyz))]
    return np.concatenate([xyz, rng.random((len(xyz), 1))], 1).astype(np.float32)
