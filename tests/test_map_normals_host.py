"""Host: the properties of tests/map_normals_cases.normals_map that the GPU tests rely on, asserted as conditions (no GPU test can pass by
skipping); the brute-force neighbour oracle against scan_prep_oracle.neighbors, the cKDTree form; the crop-normals restatement against R^T n;
and every new ValueError path of map_index, reached without a device."""
import numpy as np
import pytest
import torch

from deepi2p_amd import map_index, scan_prep, synthetic
from tests import map_cases as mc
from tests import map_normals_cases as cases
from tests import map_normals_oracle as oracle
from tests import scan_prep_oracle as spo


def _opt():
    return synthetic.OptLike(2048, 64, 128, False)


def _fake_index(normals=None):
    """a MapIndex whose tensors are never read: the argument checks come first"""
    z = torch.zeros((1,), dtype=torch.int32)
    return map_index.MapIndex(torch.zeros((1, 4)), z, z, mc.ORIGIN, mc.CELL, mc.NX, mc.NY, 1, normals)


def test_the_case_has_what_the_gpu_tests_need():
    ref = cases.reference()
    p, cnt, idx = ref["points"], ref["cnt"], ref["idx"]
    assert 4000 < len(p) < 5000 and p.dtype == np.float32 and (p[:, :3] < 0).any()
    pos = oracle.positions(p)
    assert np.array_equal(pos / cases.Q, np.round(pos / cases.Q))                        # every d2 is exact in fp64
    assert ref["tie"].sum() >= 500                                                       # the (d2, row) rule decides these rows' lists
    assert (cnt == 1).any() and (cnt == 2).any() and (cnt == cases.MAX_NN).sum() > 4000
    assert oracle.cell_candidates(p, cases.RADIUS).max() > scan_prep.NORMALS_CELL_CANDIDATES
    assert len(np.unique(pos, axis=0)) <= len(pos) - 25                                  # exact duplicates
    for up_axis in (0, 1, 2):
        n, lam = oracle.normals(p, cnt, idx, up_axis, 1)
        well = oracle.well_conditioned(cnt, lam)
        assert well.sum() >= 0.99 * (cnt >= 3).sum()
        assert np.mean(np.abs(n[:, up_axis]) > 1e-6) > 0.9
    # the shift of the grid-placement test is exact in float32 and moves the rows to other cells
    moved = p[:, :3] + cases.SHIFT.astype(np.float32)
    assert np.array_equal(moved.astype(np.float64), pos + cases.SHIFT)
    cell = cases.RADIUS * (1 + 2.0 ** -20)
    c0, c1 = np.floor((pos - pos.min(0)) / cell), np.floor((pos + cases.SHIFT - (pos + cases.SHIFT).min(0)) / cell)
    assert np.array_equal(c0, c1)          # the bounds move with the map ...
    assert np.any(np.floor(pos / cell) != np.floor((pos + cases.SHIFT) / cell))          # ... the absolute cells do not


def test_brute_force_oracle_equals_the_kdtree_form_and_the_orientation_rule():
    ref = cases.reference()
    p, cnt, idx = ref["points"], ref["cnt"], ref["idx"]
    kc, ki = spo.neighbors(oracle.positions(p), cases.RADIUS, cases.MAX_NN)
    # the cKDTree form asks for max_nn + 34 candidates: exact wherever the ball holds no more than that
    c64, _ = oracle.neighbors(p, cases.RADIUS, 64)
    few = c64 < 64
    assert few.sum() > 500 and np.array_equal(kc[few], cnt[few]) and np.array_equal(ki[few], idx[few])
    assert np.all(idx[:, 0] <= np.arange(len(p)))          # d2 = 0 first: the row itself, or a duplicate with a lower row number
    for up_axis in (0, 1, 2):
        for orient in (1, -1):
            n, _ = oracle.normals(p, cnt, idx, up_axis, orient)
            e = np.zeros(3)
            e[up_axis] = orient
            assert np.all(orient * n[:, up_axis] >= 0) and np.all(n[cnt < 3] == e)
            assert np.abs(np.linalg.norm(n, axis=1) - 1).max() < 1e-12


def test_crop_normals_oracle_is_the_rotation_into_the_prior_frame():
    rng = np.random.default_rng(2)
    nm = rng.standard_normal((50, 3)).astype(np.float32)
    index = rng.integers(0, 50, 30).astype(np.int32)
    offsets = np.array([0, 12, 12, 30], np.int32)
    T = np.stack([mc.prior((1.0, 2.0), 1, mc.rotation(k, 1)) for k in ("generic", "identity", "quarter")])
    out = oracle.crop_normals(nm, index, offsets, T)
    assert out.shape == (30, 3) and out.dtype == np.float32
    for b in range(3):
        s, e = offsets[b], offsets[b + 1]
        if e == s:
            continue
        exact = nm[index[s:e]].astype(np.float64) @ T[b, :3, :3]
        assert np.abs(out[s:e] - exact).max() <= 2.0 ** -22
        if b == 2:
            assert np.array_equal(out[s:e], exact.astype(np.float32))          # a quarter turn is exact


def test_argument_errors_need_no_device():
    p = cases.normals_map()
    for kw, match in ((dict(radius=0.0), "radius"), (dict(radius=float("inf")), "radius"), (dict(radius=float("nan")), "radius"),
                      (dict(max_nn=0), "max_nn"), (dict(max_nn=65), "max_nn"), (dict(orient=0), "orient"), (dict(up_axis=3), "up_axis")):
        with pytest.raises(ValueError, match=match):
            map_index.estimate_normals(p, **kw)
    with pytest.raises(ValueError, match="float32"):
        map_index.estimate_normals(p.astype(np.float64))
    with pytest.raises(ValueError, match="points"):
        map_index.estimate_normals(p[:, :3])
    # MapIndex.build: the user's own normals of a wrong dtype or shape, a bad estimate request
    for normals, match in ((np.zeros((len(p), 3)), "normals"), (np.zeros((len(p) - 1, 3), np.float32), "normals"),
                           (torch.zeros((len(p), 4)), "normals"), (dict(radius=-1.0), "radius"), (dict(max_nn=65), "max_nn"),
                           (dict(orient=2), "orient"), (dict(voxel=0.1), "voxel")):
        with pytest.raises(ValueError, match=match):
            map_index.MapIndex.build(p, 8.0, 2, normals=normals)
    assert _fake_index().normals is None
    with pytest.raises(ValueError, match="want_normals"):
        map_index.CropPlan(_fake_index(), 2, 100, 50, 5.0, want_normals=True)
    with pytest.raises(ValueError, match="want_normals"):
        _fake_index().crop(np.tile(np.eye(4), (2, 1, 1)), 5.0, 50, want_normals=True)
    with pytest.raises(ValueError, match="kitti.*normals="):
        map_index.MapRawPlan(_fake_index(), _opt(), 2, 100, 50, 5.0, (128, 256), dataset="kitti")
    with pytest.raises(ValueError, match="dataset"):
        map_index.MapRawPlan(_fake_index(torch.zeros((1, 3))), _opt(), 2, 100, 50, 5.0, (128, 256), dataset="velodyne")
    # with normals on the index the KITTI plan passes the data-set check: the next argument error is max_frame_points'
    with pytest.raises(ValueError, match="max_frame_points"):
        map_index.MapRawPlan(_fake_index(torch.zeros((1, 3))), _opt(), 2, 100, 1 << 21, 5.0, (128, 256), dataset="kitti")
