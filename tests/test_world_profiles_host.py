"""CPU: push-broom worlds (deepi2p_amd.world's street, trajectory and traversal inputs; tests/world_profiles_oracle.py) without a device --
the promises of make_street and make_trajectory for six seeds, traversal_inputs against direct fp64 matrix algebra, the camera / laser
consistency property on the oracle over EVERY return, the exports and the argument errors raised before anything touches a device."""
import ctypes
import os
import re

import numpy as np
import pytest

from deepi2p_amd import _lib, synthetic, world
from tests import world_oracle as wo
from tests import world_profiles_oracle as wpo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["di2p_world_profiles_workspace_bytes", "di2p_world_render_profiles"]
SEEDS = range(6)
B, S, LENGTH, CLEARANCE, SKIP = 2, 150, 60.0, 4.0, 0.1 / 16.0
CAL = synthetic.make_lms_traversal(np.random.default_rng(0), 1, 1, 1)          # the mounting of the laser and of the camera
G_LASER, G_CAM = CAL["G_posesource_laser"], CAL["G_cam"]
U = 2.0 ** -53


def _gamma(k):
    return k * U / (1 - k * U)


def _distance_to_centre_line(row, half):
    """x-y distance of a box or a cylinder from the segment y = 0, |x| <= half"""
    if row[0] == world.BOX:
        dx = max(0.0, row[1] - half, -half - row[4])
        dy = max(0.0, row[2], -row[5])
        return float(np.hypot(dx, dy))
    dx = max(0.0, abs(row[1]) - half)
    return float(np.hypot(dx, row[2])) - row[3]


@pytest.fixture(scope="module")
def drives():
    out = []
    for seed in SEEDS:
        rng = np.random.default_rng(seed)
        street = world.make_street(rng, B, LENGTH, CLEARANCE)
        T = world.make_trajectory(rng, B, S, clearance=CLEARANCE, skip_threshold=SKIP)
        out.append((street, T))
    return out


def test_street_and_trajectory_keep_their_promises(drives):
    for seed, ((table, count), T) in zip(SEEDS, drives):
        assert table.shape == (B, world.MAX_PRIMS, world.SLOTS) and count.dtype == np.int32 and T.shape == (B, S, 4, 4)
        assert world.check_world((table, count)) == B
        for b in range(B):
            n = int(count[b])
            rows = table[b, :n]
            assert 8 <= n <= world.MAX_PRIMS and rows[0, 0] == world.GROUND and rows[0, 1] == 0.0, (seed, b)
            kinds = rows[:, 0]
            assert np.sum(kinds == world.GROUND) == 1 and 4 <= np.sum(kinds == world.CYLINDER) <= 6 and np.all(kinds[-2:] == world.BOX)
            boxes = rows[kinds == world.BOX]
            assert np.any(boxes[:-2, 5] < 0) and np.any(boxes[:-2, 2] > 0)                    # buildings on both sides
            assert boxes[-2, 1] >= LENGTH / 2 and boxes[-1, 4] <= -LENGTH / 2                  # the two end walls
            near = min(_distance_to_centre_line(r, LENGTH / 2) for r in rows[1:])
            assert near >= CLEARANCE, (seed, b, near)
            # the laser's origins: inside the corridor, within clearance / 2 of the centre line, outside every box
            o = np.matmul(T[b], G_LASER)[:, :3, 3]
            assert np.all(np.abs(o[:, 1]) <= CLEARANCE / 2) and np.all(np.abs(o[:, 0]) <= LENGTH / 2) and np.all(o[:, 2] > 0), (seed, b)
            inside = (o[:, None, :] >= boxes[None, :, 1:4]) & (o[:, None, :] <= boxes[None, :, 4:7])
            assert not inside.all(2).any(), (seed, b)
            # rigid poses: x forward, y right, z down in a z-up world
            R = T[b, :, :3, :3]
            assert np.allclose(np.matmul(R, R.transpose(0, 2, 1)), np.eye(3), atol=1e-14) and np.allclose(np.linalg.det(R), 1.0)
            assert np.all(R[:, 2, 2] == -1.0) and np.all(R[:, 0, 0] > 0.9)
            step = np.linalg.norm(np.diff(T[b, :, :3, 3], axis=0), axis=1)
            assert step.min() < SKIP < step.max(), (seed, b)                                    # creeping stretches, and driving
    steady = world.make_trajectory(np.random.default_rng(0), 1, S, creep=False)
    assert np.linalg.norm(np.diff(steady[0, :, :3, 3], axis=0), axis=1).min() > 0.19


def test_traversal_inputs_against_direct_matrix_algebra(drives):
    """Every output against the same product formed matrix by matrix; then P_cam_pc . G_cam . inv(T_wv[origin]) = G_cam . inv(T_wv[cam]).
    The bound is the one of tests/test_gpu_raw_frames.py::_p_scan_bound carried over to a chain: each side is the result of k operations
    on 4 x 4 matrices (products of four-term sums; an LU inversion of a 4 x 4 matrix is counted like one, its residual |X A - I| being of
    the order gamma_4 |X| |A| as well), so each differs from the exact entry by at most gamma_4k times the product of the absolute
    matrices of the chain, and the two sides by at most twice that.  Left side: 5 products and 3 inversions (k = 8)."""
    origin, cam = S // 2, np.array([S // 3, S - 1])
    worst = 0.0
    for (street, T) in drives:
        L, poses, c2w, P = world.traversal_inputs(T, origin, cam, G_LASER, G_CAM)
        inv = np.linalg.inv
        for b in range(B):
            To, Tc = T[b, origin], T[b, cam[b]]
            for s in range(0, S, 7):
                assert np.array_equal(L[b, s], T[b, s] @ G_LASER) and np.array_equal(poses[b, s], inv(To) @ T[b, s])
            assert np.array_equal(c2w[b], Tc @ inv(G_CAM)) and np.array_equal(P[b], G_CAM @ inv(Tc) @ To @ inv(G_CAM))
            assert np.array_equal(poses[b, origin], inv(To) @ To) and np.allclose(poses[b, origin], np.eye(4), atol=1e-13)
            left, right = P[b] @ G_CAM @ inv(To), G_CAM @ inv(Tc)
            a = np.abs
            bound = 2.0 * _gamma(4 * 8) * (a(G_CAM) @ a(inv(Tc)) @ a(To) @ a(inv(G_CAM)) @ a(G_CAM) @ a(inv(To)))
            diff = a(left - right)
            assert np.all(diff <= bound), float(diff.max())
            worst = max(worst, float((diff[bound > 0] / bound[bound > 0]).max()))
    print("traversal_inputs: largest |P_cam_pc G_cam inv(T_o) - G_cam inv(T_c)| = %.3f of the bound" % worst)
    with pytest.raises(ValueError, match="origin"):
        world.traversal_inputs(drives[0][1], S, 0, G_LASER, G_CAM)
    with pytest.raises(ValueError, match="G_cam"):
        world.traversal_inputs(drives[0][1], 0, 0, G_LASER, np.eye(3))


def test_every_return_is_seen_or_occluded_from_the_camera(drives):
    """the ray from the camera origin through a noise-free return p (world coordinates) hits something at t <= |p - o| (1 + 1e-9): the
    return's own surface or an occluder.  Every return of every profile is covered -- the property is an inequality, none needs excluding."""
    beam = world.lms_pattern(181)
    worst, total, rays = 0.0, 0, 0
    for (table, count), T in drives:
        L, _, c2w, _ = world.traversal_inputs(T, S // 2, S // 2, G_LASER, G_CAM)
        for b in range(B):
            sub = wpo.render_profiles(table[b], int(count[b]), L[b, ::5], beam, 0, 0, dropout=0.0, range_sigma=0.0, reflectance_sigma=0.0)
            p = sub["world64"]
            assert len(p) == int(sub["keep"].sum()) == int(sub["counts"].sum())
            o = c2w[b, :3, 3]
            v = p - o[None]
            dist = np.sqrt((v * v).sum(1))
            t, _ = wo.trace(table[b], int(count[b]), o, v / dist[:, None])
            assert np.all(t <= dist * (1 + 1e-9)), float((t / dist).max())
            worst, total, rays = max(worst, float((t / dist).max() - 1.0)), total + len(p), rays + sub["keep"].size
    print("camera / laser consistency: %d returns of %d rays, all covered; worst relative excess %.2e" % (total, rays, worst))
    assert total > 50000 and total < rays                  # beams above the horizon at open sky return nothing


def test_the_oracle_row_format():
    """x = t cos, y = t sin in the laser frame (x to the ground): straight down from 1.4 m the row is (1.4, 0, 255 reflectance)"""
    table, count = np.zeros((world.MAX_PRIMS, world.SLOTS)), 1
    table[0] = world._row(world.GROUND, [0.0], np.full(3, 0.25), 0.7)
    M = np.array([[0.0, 0, 1, 2.0], [0, 1, 0, 3.0], [-1.0, 0, 0, 1.4], [0, 0, 0, 1]])          # laser x = world -z
    beam = world.lms_pattern(5, 180.0)
    assert np.array_equal(beam[2], [1.0, 0.0]) and np.allclose(beam[0], [0.0, -1.0], atol=1e-16)
    sub = wpo.render_profiles(table, count, M[None], beam, 3, 0, dropout=0.0, range_sigma=0.0, reflectance_sigma=0.0)
    assert list(sub["keep"][0]) == [False, True, True, True, False] and sub["counts"][0] == 3
    assert np.array_equal(sub["rows"][1], [1.4, 0.0, 255.0 * table[0, 10]]) and np.allclose(sub["world64"][:, 2], 0.0, atol=1e-15)
    noisy = wpo.render_profiles(table, count, M[None], beam, 3, 0, dropout=0.0)
    assert np.array_equal(noisy["keep"], sub["keep"]) and not np.array_equal(noisy["rows"], sub["rows"])
    assert np.all(np.abs(noisy["rows"][:, :2] - sub["rows"][:, :2]) < 0.1) and not np.array_equal(noisy["rows"][:, 2], np.rint(noisy["rows"][:, 2]))


def test_exports():
    from deepi2p_amd import build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "deepi2p_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, src), n
        assert hasattr(lib, n), n
        assert n in _lib.EXPORTS, n
    assert "di2p_world_render_profiles" in doc
    l = _lib.load()
    assert l.di2p_version() == 9                      # purely additive
    assert l.di2p_world_profiles_workspace_bytes(32 * 500, 541) >= 24 * 32 * 500 * 541
    assert l.di2p_world_profiles_workspace_bytes(-1, 10) == 0 and l.di2p_world_profiles_workspace_bytes(1 << 16, 1 << 15) == 0
    assert "8 synthetic-world push-broom" in open(os.path.join(ROOT, "deepi2p_amd", "csrc", "philox.h")).read()


C_CHECKS = r"""
import ctypes, sys
lib = ctypes.CDLL(sys.argv[1])
lib.di2p_last_error.restype = ctypes.c_char_p
v, i, d, u = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_ulonglong
lib.di2p_world_render_profiles.argtypes = [v, v, i, i, v, v, v, i, i, d, d, d, d, u, v, i, v, v, v, v, v, v]
N = None
calls = [("2^31", (N, N, 1, 32, N, N, N, 1 << 16, 1 << 15, 50.0, 0.0, 0.0, 0.0, 0, N, 0, N, N, N, N, N, N)),
         ("32 primitives", (N, N, 1, 33, N, N, N, 4, 4, 50.0, 0.0, 0.0, 0.0, 0, N, 0, N, N, N, N, N, N)),
         ("bad sizes", (N, N, 1, 32, N, N, N, -1, 4, 50.0, 0.0, 0.0, 0.0, 0, N, 0, N, N, N, N, N, N)),
         ("dropout", (N, N, 1, 32, N, N, N, 4, 4, 50.0, 2.0, 0.0, 0.0, 0, N, 0, N, N, N, N, N, N)),
         ("frame0", (N, N, 1, 32, N, N, N, 4, 4, 50.0, 0.0, 0.0, 0.0, 0, N, -1, N, N, N, N, N, N)),
         ("null pointer", (N, N, 1, 32, N, N, N, 4, 4, 50.0, 0.0, 0.0, 0.0, 0, N, 0, N, N, N, N, N, N))]
for want, args in calls:
    assert lib.di2p_world_render_profiles(*args) == -1 and want in lib.di2p_last_error().decode(), (want, lib.di2p_last_error())
print("checked", len(calls))
"""


def test_the_entry_point_checks_its_bounds_before_any_launch():
    """sizes >= 0, count <= 32, capacity < 2^31, the options, null pointers: -1 and a message in di2p_last_error, every pointer NULL, no
    device.  In a child process: the message is sticky, and other tests read it."""
    import subprocess
    import sys
    from deepi2p_amd import build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    out = subprocess.run([sys.executable, "-c", C_CHECKS, _lib.LIB_PATH], capture_output=True, text=True)
    assert out.returncode == 0 and "checked 6" in out.stdout, out.stderr + out.stdout


def test_argument_errors_are_raised_on_the_host():
    rng = np.random.default_rng(0)
    street = world.make_street(rng, 2, 40.0)
    L = np.tile(np.eye(4), (6, 1, 1))
    with pytest.raises(ValueError, match="submap_offsets"):
        world.render_profiles(street, [0, 6], L, world.lms_pattern(5), 0, device="cpu")
    with pytest.raises(ValueError, match="laser_to_world"):
        world.render_profiles(street, [0, 3, 6], L[:, :3], world.lms_pattern(5), 0, device="cpu")
    with pytest.raises(ValueError, match="beam"):
        world.render_profiles(street, [0, 3, 6], L, np.zeros((5, 3)), 0, device="cpu")
    with pytest.raises(ValueError, match="dropout"):
        world.render_profiles(street, [0, 3, 6], L, world.lms_pattern(5), 0, dropout=1.5, device="cpu")
    with pytest.raises(ValueError, match="clearance"):
        world.make_street(rng, 1, 40.0, clearance=0.0)
    with pytest.raises(ValueError, match="fov_deg"):
        world.lms_pattern(5, 400.0)
    with pytest.raises(ValueError, match="2\\^31"):
        world.TraversalPlan(64, 1 << 15, 1 << 10, 4, 4, device="cpu")
