"""GPU: the cell-cooperative normals kernel (scan_prep.estimate_normals(method="cells"), di2p_estimate_normals_cells) against the
per-query kernel (method="query") on the same VoxelState: normals, neighbour counts and neighbour lists must be equal bit for bit."""
import numpy as np
import pytest
import torch

from deepi2p_amd import scan_prep, synthetic
from tests import scan_prep_oracle as spo

pytestmark = pytest.mark.gpu


def _np(t):
    return t.cpu().numpy()


def _with_intensity(xyz, value=0.5):
    return np.concatenate([xyz, np.full((len(xyz), 1), value)], 1).astype(np.float32)


def _both(frames, voxel, dev, radius=0.6, max_nn=30):
    """-> (voxel offsets, {method: (normals, count, idx)}) for one VoxelState"""
    points, offsets, _ = scan_prep.pack(frames, dev)
    st = scan_prep.voxel_down_sample(points, offsets, voxel)
    out = {}
    for method in ("query", "cells"):
        out[method] = tuple(_np(t) for t in scan_prep.estimate_normals(st, radius, max_nn, want_neighbors=True, method=method))
    assert np.all(_np(st.status) == 0)
    return _np(st.offsets), out


def _assert_same(vo, out):
    n = vo[-1]
    for a, b, name in zip(out["query"], out["cells"], ("normals", "nn_count", "nn_idx")):
        assert np.array_equal(a[:n], b[:n]), name


def _assert_oracle(frame, voxel, normals, cnt, nbr):
    """the assertions of test_gpu_scan_prep.test_normals_against_oracle for one frame"""
    cen = spo.voxel_down_sample(frame, voxel)["cen"]
    c, i = spo.neighbors(cen, 0.6, 30)
    assert np.array_equal(cnt, c)
    same = np.all(np.sort(nbr, 1) == np.sort(i, 1), axis=1)
    if not np.all(same):
        c2, n2 = spo.neighbors(cen, 0.6, 31)
        for q in np.nonzero(~same)[0]:
            d = spo.d2(cen[n2[q]], cen[q])
            assert c2[q] == 31 and d[29] == d[30], q
    nref, lam = spo.normals(cen, c, i)
    n = normals.astype(np.float64)
    gap = (lam[:, 1] - lam[:, 0]) / np.maximum(lam[:, 2], 1e-300)
    well = (c >= 3) & (gap > 1e-3)
    dots = np.abs(np.sum(n * nref, 1))
    assert np.all(dots[well] >= 1 - 1e-7), dots[well].min()
    sure = np.abs(nref[:, 2]) > 1e-6
    assert np.all(n[sure, 2] >= 0)
    assert np.all(n[c < 3] == np.array([0, 0, 1]))


def _patch():
    rng = np.random.default_rng(5)
    xy = np.stack(np.meshgrid(np.arange(20) * 0.05, np.arange(20) * 0.05, indexing="ij"), -1).reshape(-1, 2)
    return np.concatenate([xy, 0.3 * xy[:, :1] + 0.01 * rng.standard_normal((len(xy), 1))], 1)   # 400 points in a 1 m tilted patch


def test_ragged_batch_with_degenerate_frames(dev):
    s0 = synthetic.make_velodyne_scan(np.random.default_rng(10), azimuths=900)
    s1 = synthetic.make_velodyne_scan(np.random.default_rng(11))[:40_000]
    lone = np.array([[0, 0, 0], [10, 0, 0], [20, 0, 0], [40, 0, 0], [40.3, 0, 0], [60, 0, 0], [60, 0.3, 0]], np.float64)
    frames = [s0, s1, np.zeros((0, 4), np.float32), s0[7:8], _with_intensity(lone)]
    vo, out = _both(frames, 0.1, dev)
    _assert_same(vo, out)
    normals, cnt, nbr = out["cells"]
    assert vo[3] == vo[2] and vo[4] - vo[3] == 1
    assert cnt[vo[3]] == 1 and np.array_equal(normals[vo[3]], [0, 0, 1])
    assert np.array_equal(cnt[vo[4]:vo[5]], [1, 1, 1, 2, 2, 2, 2])
    assert np.all(normals[vo[4]:vo[5]] == np.array([0, 0, 1], np.float32))
    for b in (0, 1):
        sl = slice(vo[b], vo[b + 1])
        _assert_oracle(frames[b], 0.1, normals[sl], cnt[sl], nbr[sl])


def test_many_queries_per_cell_dense_patch(dev):
    """400 points in less than four cells: more than 64 queries per cell, more than max_nn neighbours everywhere"""
    frame = _with_intensity(_patch())
    vo, out = _both([frame], 0.01, dev)
    _assert_same(vo, out)
    normals, cnt, nbr = out["cells"]
    assert vo[1] == 400 and np.all(cnt[:400] == 30)
    c, i = spo.neighbors(spo.voxel_down_sample(frame, 0.01)["cen"], 0.6, 30)
    assert np.array_equal(cnt[:400], c) and np.array_equal(nbr[:400], i)
    _assert_oracle(frame, 0.01, normals[:400], cnt[:400], nbr[:400])


def test_exact_ties_on_a_lattice(dev):
    g = np.arange(12) * 0.05
    lat = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    frame = _with_intensity(lat)
    vo, out = _both([frame], 0.01, dev)
    assert vo[1] == 12 ** 3
    _assert_same(vo, out)
    cen = spo.voxel_down_sample(frame, 0.01)["cen"]
    c31, n31 = spo.neighbors(cen, 0.6, 31)
    d = spo.d2(cen[n31], cen[:, None, :])
    assert np.any((c31 == 31) & (d[:, 29] == d[:, 30]))          # the case is what it says: ties at the cut
    c, i = spo.neighbors(cen, 0.6, 30)
    assert np.array_equal(out["cells"][1][:vo[1]], c) and np.array_equal(out["cells"][2][:vo[1]], i)      # ties -> the lower index


def test_candidate_set_above_the_lds_capacity(dev):
    C = scan_prep.NORMALS_CELL_CANDIDATES
    from deepi2p_amd import _lib
    assert _lib.load().di2p_normals_cells_candidates() == C
    rng = np.random.default_rng(8)
    g = np.arange(16) * 0.04
    blk = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) + rng.uniform(-0.003, 0.003, (16 ** 3, 3))
    assert len(blk) >= 2 * C
    frame = _with_intensity(blk)
    cen = spo.voxel_down_sample(frame, 0.01)["cen"]
    assert len(cen) == len(blk)
    c, _ = spo.neighbors(cen, 0.6, 2 * C)
    assert c.max() == 2 * C                                       # at least 2 C points inside one ball: that cell cannot be staged
    vo, out = _both([frame, _with_intensity(_patch())], 0.01, dev)          # a cell that streams next to cells that are staged
    _assert_same(vo, out)
    c30, i30 = spo.neighbors(cen, 0.6, 30)
    assert np.array_equal(out["cells"][1][:vo[1]], c30) and np.array_equal(out["cells"][2][:vo[1]], i30)


def test_frame_isolation(dev):
    s = synthetic.make_velodyne_scan(np.random.default_rng(12), azimuths=450)
    vo1, one = _both([s], 0.1, dev)
    vo2, two = _both([s, s], 0.1, dev)
    _assert_same(vo2, two)
    n = vo1[1]
    assert vo2[1] == n and vo2[2] == 2 * n
    for a, b in zip(one["cells"], two["cells"]):
        assert np.array_equal(a[:n], b[:n]) and np.array_equal(a[:n], b[n:2 * n])


def test_negative_coordinates(dev):
    s = synthetic.make_velodyne_scan(np.random.default_rng(13), azimuths=450)
    s[:, :3] -= 1000.0
    vo, out = _both([s, _with_intensity(_patch() - 1000.0)], 0.1, dev)
    _assert_same(vo, out)
    assert out["cells"][1][:vo[2]].max() == 30


def test_run_twice(dev):
    s = synthetic.make_velodyne_scan(np.random.default_rng(14), azimuths=450)
    points, offsets, _ = scan_prep.pack([s, s[:5000]], dev)
    st = scan_prep.voxel_down_sample(points, offsets, 0.1)
    a = [t.clone() for t in scan_prep.estimate_normals(st, 0.6, 30, want_neighbors=True, method="cells")]
    b = scan_prep.estimate_normals(st, 0.6, 30, want_neighbors=True, method="cells")
    n = int(st.offsets[-1])
    for x, y in zip(a, b):
        assert torch.equal(x[:n], y[:n])
