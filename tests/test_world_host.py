"""CPU: synthetic worlds (deepi2p_amd.world, csrc/world.hip) without a device -- tests/world_oracle.py against synthetic.make_velodyne_scan
(the scene rule and the ray tests are the same), the camera / LiDAR consistency property on the oracle, the exports and the argument
errors (all raised before anything touches a device)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from deepi2p_amd import _lib, synthetic, world
from tests import world_oracle as wo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["di2p_world_workspace_bytes", "di2p_world_trace", "di2p_world_render_camera", "di2p_world_render_scan"]
CAM_OFFSET = np.array([0.27, 0.06, -0.08])          # camera origin off the sensor (m)
SEEDS = range(6)


@pytest.fixture(scope="module")
def scenes():
    """per seed: the pattern and the world drawn from one generator (make_velodyne_scan's order), and the oracle's noise-free scan"""
    out = []
    for seed in SEEDS:
        rng = np.random.default_rng(seed)
        pattern = world.hdl64_pattern(rng, 1, 64, 900)
        table, count = world.make_world(rng, 1)
        scan = wo.render_scan(table[0], int(count[0]), pattern[0], pattern[1][0], 0, 0, dropout=0.0, range_sigma=0.0, intensity_sigma=0.0)
        out.append((table[0], int(count[0]), scan))
    return out


def test_the_oracle_scan_is_make_velodyne_scans_geometry(scenes):
    for seed, (table, count, scan) in zip(SEEDS, scenes):
        ref = synthetic.make_velodyne_scan(np.random.default_rng(seed), azimuths=900, dropout=0.0, range_sigma=0.0)
        assert scan["rows"].shape == ref.shape and len(ref) > 40000, seed
        assert scan["rows"][:, :3].tobytes() == ref[:, :3].tobytes(), seed          # same scene, same rays, same arithmetic
        assert 1 + 6 + 4 + 3 <= count <= 1 + 9 + 8 + 3 <= world.MAX_PRIMS
        kinds = table[:count, 0]
        assert kinds[0] == world.GROUND and np.all(kinds[-3:] == world.BOX) and 4 <= np.sum(kinds == world.CYLINDER) <= 8
        # the reflectance is the luminance of the albedo, and the intensity column is the reflectance of the primitive hit
        assert np.allclose(table[:count, 7:10] @ world.LUMA, table[:count, 10], rtol=0, atol=1e-15)
        assert np.array_equal(scan["rows"][:, 3], table[scan["prim"][scan["keep"]], 10].astype(np.float32))


def test_every_return_is_seen_or_occluded_from_the_camera(scenes):
    """the ray from the camera origin through a return p hits something at t <= |p - o| (1 + 1e-9): the return's own surface or an occluder"""
    worst, total, same = 0.0, 0, 0
    for table, count, scan in scenes:
        p = scan["points64"]
        v = p - CAM_OFFSET[None]
        dist = np.sqrt((v * v).sum(1))
        t, prim = wo.trace(table, count, CAM_OFFSET, v / dist[:, None])
        assert np.all(t <= dist * (1 + 1e-9)), float((t / dist).max())
        worst, total, same = max(worst, float((t / dist).max() - 1.0)), total + len(p), same + int(np.sum(prim == scan["prim"][scan["keep"]]))
    print("returns %d, worst relative excess %.2e, same primitive %.2f %%" % (total, worst, 100.0 * same / total))
    assert total > 300000 and same > 0.99 * total


def test_an_empty_world_is_sky_and_no_return():
    table, count = np.zeros((1, world.MAX_PRIMS, world.SLOTS)), np.zeros((1,), np.int32)
    pattern = world.hdl64_pattern(np.random.default_rng(0), 1, 4, 9)
    scan = wo.render_scan(table[0], 0, pattern[0], pattern[1][0], 3, 0)
    assert scan["rows"].shape == (0, 4) and not scan["keep"].any()
    cam = wo.render_camera(table[0], 0, np.array([[50.0, 0, 4], [0, 50.0, 3], [0, 0, 1]]), np.eye(4), 7, 9)
    assert np.all(cam["prim"] == -1) and np.all(cam["depth"] == 0) and cam["image"][0, 0, 2] > cam["image"][0, 0, 0]
    assert np.all(np.diff(cam["image"][:, 0].astype(int), axis=0) >= 0)          # the gradient in v


def test_exports():
    from deepi2p_amd import build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "deepi2p_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, src), n
        assert hasattr(lib, n), n
        assert n in _lib.EXPORTS, n
    assert "world.hip" in build.SOURCES and build.PER_FILE_FLAGS["world.hip"] == ["-ffp-contract=off"]
    l = _lib.load()
    assert l.di2p_version() == 9                      # purely additive
    assert l.di2p_world_workspace_bytes(32, 64 * 1800) >= 16 * 32 * 64 * 1800
    assert l.di2p_world_workspace_bytes(-1, 10) == 0 and l.di2p_world_workspace_bytes(1 << 16, 1 << 15) == 0
    assert "7 synthetic-world scan" in open(os.path.join(ROOT, "deepi2p_amd", "csrc", "philox.h")).read()


C_CHECKS = r"""
import ctypes, sys
lib = ctypes.CDLL(sys.argv[1])
lib.di2p_last_error.restype = ctypes.c_char_p
v, i, d, u = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_ulonglong
lib.di2p_world_trace.argtypes = [v, v, i, i, v, v, i, v, v, v]
lib.di2p_world_render_camera.argtypes = [v, v, i, i, v, v, i, i, d, v, v, v, v]
lib.di2p_world_render_scan.argtypes = [v, v, i, i, v, v, v, i, i, d, d, d, d, u, v, i, v, v, v, v, v]
N = None
calls = [("32 primitives", lib.di2p_world_trace, (N, N, 1, 33, N, N, 4, N, N, N)),
         ("bad sizes", lib.di2p_world_trace, (N, N, 1, 32, N, N, -1, N, N, N)),
         ("32 primitives", lib.di2p_world_render_camera, (N, N, 1, 33, N, N, 4, 4, 120.0, N, N, N, N)),
         ("bad sizes", lib.di2p_world_render_camera, (N, N, 1, 32, N, N, -1, 4, 120.0, N, N, N, N)),
         ("2^31", lib.di2p_world_render_scan, (N, N, 40000, 32, N, N, N, 64, 1800, 120.0, 0.0, 0.0, 0.0, 0, N, 0, N, N, N, N, N)),
         ("32 primitives", lib.di2p_world_render_scan, (N, N, 1, 33, N, N, N, 64, 1800, 120.0, 0.0, 0.0, 0.0, 0, N, 0, N, N, N, N, N)),
         ("dropout", lib.di2p_world_render_scan, (N, N, 1, 32, N, N, N, 64, 1800, 120.0, 2.0, 0.0, 0.0, 0, N, 0, N, N, N, N, N))]
for want, fn, args in calls:
    assert fn(*args) == -1 and want in lib.di2p_last_error().decode(), (want, lib.di2p_last_error())
print("checked", len(calls))
"""


def test_the_entry_points_check_their_bounds_before_any_launch():
    """count <= 32, sizes >= 0, capacity < 2^31: -1 and a message in di2p_last_error, every pointer NULL, no device.  In a child process: the
    message is sticky, and other tests read it."""
    import subprocess
    import sys
    from deepi2p_amd import build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    out = subprocess.run([sys.executable, "-c", C_CHECKS, _lib.LIB_PATH], capture_output=True, text=True)
    assert out.returncode == 0 and "checked 7" in out.stdout, out.stderr


def test_argument_errors_are_raised_on_the_host():
    """every array below lives on the host: an error that needed the device would surface as another exception"""
    rng = np.random.default_rng(0)
    w = world.make_world(rng, 2)
    pattern = world.hdl64_pattern(rng, 2, 4, 8)
    K, Pc = np.tile(np.array([[50.0, 0, 4], [0, 50.0, 3], [0, 0, 1]]), (2, 1, 1)), np.tile(np.eye(4), (2, 1, 1))
    with pytest.raises(ValueError, match="pair"):
        world.check_world(w[0])
    with pytest.raises(ValueError, match="table must be float64"):
        world.trace((w[0].astype(np.float32), w[1]), np.zeros((2, 3)), np.zeros((2, 5, 3)))
    with pytest.raises(ValueError, match="table must be float64"):
        world.trace((w[0][:, :31], w[1]), np.zeros((2, 3)), np.zeros((2, 5, 3)))
    with pytest.raises(ValueError, match="count must be int32"):
        world.trace((w[0], w[1].astype(np.int64)), np.zeros((2, 3)), np.zeros((2, 5, 3)))
    with pytest.raises(ValueError, match=r"count must be in \[0, 32\]"):
        world.trace((w[0], np.array([33, 1], np.int32)), np.zeros((2, 3)), np.zeros((2, 5, 3)))
    with pytest.raises(ValueError, match="same number of frames"):
        world.trace((w[0], w[1][:1]), np.zeros((2, 3)), np.zeros((2, 5, 3)))
    bad = w[0].copy()
    bad[1, 2, 11] = 0.0
    with pytest.raises(ValueError, match="frame 1"):
        world.trace((bad, w[1]), np.zeros((2, 3)), np.zeros((2, 5, 3)))
    with pytest.raises(ValueError, match="origin must be"):
        world.trace(w, np.zeros((2, 4)), np.zeros((2, 5, 3)))
    with pytest.raises(ValueError, match="origin must be"):
        world.trace(w, torch.zeros((2, 3)), torch.zeros((2, 5, 3)))          # float32 tensors are not cast silently
    with pytest.raises(ValueError, match="H0, W0"):
        world.render_camera(w, K, Pc, -1, 8)
    with pytest.raises(ValueError, match="K_raw must be"):
        world.render_camera(w, K[:1], Pc, 6, 8)
    with pytest.raises(ValueError, match="focal"):
        world.render_camera(w, K * 0, Pc, 6, 8)
    with pytest.raises(ValueError, match="Pc must be"):
        world.render_camera(w, K, Pc[:, :3], 6, 8)
    with pytest.raises(ValueError, match="invertible"):
        world.render_camera(w, K, Pc * 0, 6, 8)
    with pytest.raises(ValueError, match="T must be"):
        world.render_camera(w, K, Pc, 6, 8, T=np.eye(4))
    with pytest.raises(ValueError, match="pattern"):
        world.render_scan(w, pattern[0], 0)
    with pytest.raises(ValueError, match="pattern"):
        world.render_scan(w, (pattern[0], pattern[1][:1]), 0)
    with pytest.raises(ValueError, match="dropout"):
        world.render_scan(w, pattern, 0, dropout=1.5)
    with pytest.raises(ValueError, match="sigma"):
        world.render_scan(w, pattern, 0, range_sigma=-1.0)
    with pytest.raises(ValueError, match="frame0"):
        world.render_scan(w, pattern, 0, frame0=-1)
    with pytest.raises(ValueError, match="capacity"):
        world.WorldPlan(40000, 4, 4, 64, 1800, device="cpu")
    with pytest.raises(ValueError, match="B must be"):
        world.WorldPlan(-1, 4, 4, 4, 8, device="cpu")
    with pytest.raises(ValueError, match="seed_slot"):
        world.WorldPlan(2, 4, 4, 4, 8, device="cpu", seed_slot=torch.zeros((1,), dtype=torch.int32))
    assert world.camera_pose(Pc).shape == (2, 4, 4)
    e, a = world.hdl64_pattern(np.random.default_rng(1), 3)
    assert e.shape == (64, 2) and a.shape == (3, 1800, 2) and np.allclose((a ** 2).sum(-1), 1) and np.allclose((e ** 2).sum(-1), 1)
