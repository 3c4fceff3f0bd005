"""CPU: the raw-scan preparation's numpy oracle against brute force, the synthetic scan generator, the new symbols and the argument
errors of the new entry points (reported through di2p_last_error, before anything touches a device)."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import scan_prep_oracle as spo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["di2p_scan_prep_workspace_bytes", "di2p_voxel_down_sample", "di2p_estimate_normals", "di2p_nearest_raw", "di2p_gather_ragged",
       "di2p_random_choice_ragged", "di2p_random_choice_ragged_workspace_bytes"]


def _small_cloud(rng, n=600):
    p = rng.uniform(-1.5, 1.5, (n, 3))
    p[: n // 3, 2] = 0.05 * rng.standard_normal(n // 3)           # a noisy plane
    p = np.concatenate([p, p[:20]], 0)                               # duplicates
    return np.concatenate([p, rng.random((p.shape[0], 1))], 1).astype(np.float32)


def test_voxel_oracle_matches_brute_force():
    rng = np.random.default_rng(0)
    for voxel in (0.1, 0.25, 0.3):
        pts = _small_cloud(rng)
        v = spo.voxel_down_sample(pts, voxel)
        keys, cen = spo.voxel_brute(pts, voxel)
        assert np.array_equal(v["keys"], keys)
        assert np.array_equal(v["cen"], cen)           # same summation order -> same bits
        assert len(keys) < pts.shape[0]


def test_neighbor_oracle_matches_all_pairs():
    rng = np.random.default_rng(1)
    cen = spo.voxel_down_sample(_small_cloud(rng, 1500), 0.1)["cen"]
    for r, k in ((0.3, 30), (0.6, 30), (0.2, 5)):
        c0, i0 = spo.neighbors(cen, r, k)
        c1, i1 = spo.neighbors_brute(cen, r, k)
        assert np.array_equal(c0, c1) and np.array_equal(i0, i1)
    n, lam = spo.normals(cen, *spo.neighbors(cen, 0.6, 30))
    assert np.allclose(np.linalg.norm(n, axis=1), 1.0) and np.all(n[:, 2] >= 0)


def test_nearest_oracle_matches_brute_force():
    rng = np.random.default_rng(2)
    pts = _small_cloud(rng, 800)
    cen = spo.voxel_down_sample(pts, 0.1)["cen"]
    idx, d2 = spo.nearest_raw(pts, cen)
    raw = pts[:, :3].astype(np.float64)
    for q in range(cen.shape[0]):
        dd = spo.d2(raw, cen[q])
        j = np.lexsort((np.arange(len(dd)), dd))[0]
        assert idx[q] == j and d2[q] == dd[j]


def test_synthetic_velodyne_scan():
    from deepi2p_amd import synthetic
    s = synthetic.make_velodyne_scan(np.random.default_rng(0))
    assert s.dtype == np.float32 and s.shape[1] == 4 and 100_000 <= s.shape[0] <= 130_000
    assert np.all(np.isfinite(s)) and s[:, 3].min() >= 0 and s[:, 3].max() <= 1
    assert abs(np.percentile(s[:, 2], 5) + 1.73) < 0.1          # the ground, 1.73 m below the sensor
    t = synthetic.make_velodyne_scan(np.random.default_rng(0))
    assert np.array_equal(s, t)


def test_new_symbols_declared_exported_and_bound():
    from deepi2p_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "deepi2p_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, src), n
        assert hasattr(lib, n), n
        assert n in _lib.EXPORTS, n
    assert _lib.load().di2p_version() >= 7          # additive entry points: the version number is unchanged


def test_workspace_queries():
    from deepi2p_amd import _lib
    l = _lib.load()
    a, b = l.di2p_scan_prep_workspace_bytes(4, 100_000), l.di2p_scan_prep_workspace_bytes(4, 200_000)
    assert a >= 100_000 * 100 and b > a
    assert l.di2p_scan_prep_workspace_bytes(-1, 10) == 0
    assert l.di2p_random_choice_ragged_workspace_bytes(4, 1000) == l.di2p_random_choice_workspace_bytes(4, 1000)


def test_argument_errors():
    # in a thread of its own: di2p_last_error is per thread, and test_capi_and_host expects "ok" on the main thread
    import concurrent.futures
    with concurrent.futures.ThreadPoolExecutor(1) as ex:
        ex.submit(_argument_errors).result()


def _argument_errors():
    from deepi2p_amd import _lib
    E = _lib.DeepI2PHipError
    fake = 256          # never dereferenced: every call below fails its host-side checks first

    def vox(voxel=0.1, max_extent=200.0, mfp=1 << 20, B=1, p=fake):
        _lib.call("di2p_voxel_down_sample", p, p, B, 10, mfp, voxel, max_extent, 0, None, p, p, None, None, None, None, p, None)
    for bad in (0.0, -0.1, float("inf")):
        with pytest.raises(E, match="voxel size"):
            vox(voxel=bad)
    with pytest.raises(E, match="span above 2\\^21"):
        vox(voxel=1e-5)
    with pytest.raises(E, match="2\\^20"):
        vox(mfp=(1 << 20) + 1)
    with pytest.raises(E, match="null"):
        vox(p=None)
    vox(B=0, p=None)                      # an empty batch is a valid no-op
    with pytest.raises(E, match="max_nn"):
        _lib.call("di2p_estimate_normals", fake, 1, 10, 0.6, 65, 200.0, fake, None, None, fake, None)
    with pytest.raises(E, match="radius"):
        _lib.call("di2p_estimate_normals", fake, 1, 10, 0.0, 30, 200.0, fake, None, None, fake, None)
    with pytest.raises(E, match="span above 2\\^21"):
        _lib.call("di2p_estimate_normals", fake, 1, 10, 1e-5, 30, 200.0, fake, None, None, fake, None)
    with pytest.raises(E, match="null"):
        _lib.call("di2p_estimate_normals", None, 1, 10, 0.6, 30, 200.0, None, None, None, None, None)
    with pytest.raises(E, match="null"):
        _lib.call("di2p_nearest_raw", None, None, None, 2, 10, 0.1, None, None, None, None, None)
    with pytest.raises(E, match="null"):
        _lib.call("di2p_gather_ragged", None, None, None, None, None, None, 2, 8, None, None, None, None)
    with pytest.raises(E, match="null"):
        _lib.call("di2p_random_choice_ragged", 0, 0, 2, None, 100, 8, None, None, None)
    with pytest.raises(E, match="max_src"):
        _lib.call("di2p_random_choice_ragged", 0, 0, 2, fake, (1 << 20) + 1, 8, fake, fake, None)
