"""Host: the numpy oracle of the map index (tests/map_index_oracle.py) against a brute-force filter and the stated visiting order; every
ValueError path of map_index and map_pipeline.host_map_frames, reached without a device; synthetic.make_map and the frames the GPU tests cut
out of it."""
import numpy as np
import pytest
import torch

from deepi2p_amd import map_index, synthetic
from deepi2p_amd.map_pipeline import host_map_frames
from tests import map_cases as mc
from tests import map_index_oracle as oracle


def _opt():
    return synthetic.OptLike(2048, 64, 128, False)


def _fake_index(nx=mc.NX, ny=mc.NY, cell=mc.CELL):
    """a MapIndex whose tensors are never read: the argument checks come first"""
    z = torch.zeros((1,), dtype=torch.int32)
    return map_index.MapIndex(torch.zeros((1, 4)), z, z, mc.ORIGIN, cell, nx, ny, 1)


# ---------------------------------------------------------------------------------------------------------------- the oracle
@pytest.mark.parametrize("up_axis", [0, 1, 2])
def test_oracle_build_is_the_stable_cell_order(up_axis):
    p = mc.grid_map(up_axis)
    ix = oracle.build(p, mc.CELL, up_axis, mc.ORIGIN, mc.NX, mc.NY)
    assert ix["status"] == 0 and 5500 < ix["M"] < 6500
    ids, _ = oracle.cell_ids(p, mc.CELL, up_axis, mc.ORIGIN, mc.NX, mc.NY)
    want = sorted(range(len(p)), key=lambda i: (ids[i], i))                 # ascending cell, then ascending map row
    assert list(ix["order"]) == want and np.array_equal(ix["sorted"], p[want])
    counts = np.diff(ix["cell_start"])
    assert np.array_equal(counts, np.bincount(ids, minlength=mc.NX * mc.NY)) and ix["cell_start"][-1] == len(p)
    assert counts[mc.EMPTY[1] * mc.NX + mc.EMPTY[0]] == 0 and 690 < counts[mc.DENSE[1] * mc.NX + mc.DENSE[0]] < 720
    assert oracle.default_grid(p, mc.CELL, up_axis)[1:] == (mc.NX, mc.NY)
    assert tuple(oracle.default_grid(p, mc.CELL, up_axis)[0]) == mc.ORIGIN
    assert np.all(np.asarray(p[:, :3], np.float64) / mc.Q == np.round(np.asarray(p[:, :3], np.float64) / mc.Q))


@pytest.mark.parametrize("up_axis,kind", [(0, "identity"), (1, "quarter"), (1, "generic"), (2, "generic")])
def test_oracle_crop_is_the_brute_force_filter_and_the_stated_order(up_axis, kind):
    p = mc.grid_map(up_axis)
    ix = oracle.build(p, mc.CELL, up_axis, mc.ORIGIN, mc.NX, mc.NY)
    T, r = mc.grid_frames(up_axis, kind)
    rows, off, index, status = oracle.crop(ix, T, r, cap=2 * len(p), max_frame_points=len(p), max_cells=mc.NX * mc.NY)
    assert list(status) == [0, 0, oracle.ST_EMPTY, oracle.ST_PRIOR] and list(np.diff(off)[2:]) == [0, 0]
    ids, _ = oracle.cell_ids(p, mc.CELL, up_axis, mc.ORIGIN, mc.NX, mc.NY)
    a, b = oracle.ground_axes(up_axis)
    for f in (0, 1):
        got = index[off[f]:off[f + 1]]
        brute = oracle.brute_force(p, T[f], r[f], up_axis)
        assert len(got) > 100 and sorted(got) == list(brute)                 # as a set: no row twice, none missing
        # as a sequence: iy-major over the cells (= ascending cell id inside a clamped window), ascending map row inside a cell
        assert list(got) == sorted(brute, key=lambda i: (ids[i], i))
        exact = (p[got, :3].astype(np.float64) - T[f, :3, 3]) @ T[f, :3, :3]  # R^T (p - t)
        assert np.abs(rows[off[f]:off[f + 1], :3] - exact).max() <= 2.0 ** -23 * 64 and np.array_equal(rows[off[f]:off[f + 1], 3], p[got, 3])
        if kind != "generic":
            assert np.array_equal(rows[off[f]:off[f + 1], :3], exact.astype(np.float32))
    assert off[2] - off[1] == len(p)                                         # the covering disc keeps the whole map
    dense = ids[index[off[0]:off[1]]]
    assert np.all(dense == mc.DENSE[1] * mc.NX + mc.DENSE[0])


def test_oracle_keep_rule_is_strict():
    p = mc.grid_map(1)
    ix = mc.grid_index(1)
    T = mc.prior((0.0, 0.0), 1)[None]
    _, off, index, status = oracle.crop(ix, T, [5.0], len(p), len(p), 20)
    kept = p[index][:, [0, 2]]
    on = np.all(kept == np.float32(mc.ON_CIRCLE), axis=1)
    inside = np.all(kept == np.float32(mc.INSIDE_CIRCLE), axis=1)
    assert status[0] == 0 and not on.any() and inside.sum() == 1
    assert np.any(np.all(p[:, [0, 2]] == np.float32(mc.ON_CIRCLE), axis=1))


def test_oracle_statuses_and_windows():
    p = mc.grid_map(1)
    ix = mc.grid_index(1)
    T, r = mc.grid_frames(1)
    assert oracle.window(ix, T[0], r[0]) == (2, 2, 2, 2) and oracle.window(ix, T[1], r[1]) == (0, mc.NX - 1, 0, mc.NY - 1)
    assert oracle.window(ix, T[2], r[2]) is None
    full = oracle.crop(ix, T, r, 2 * len(p), len(p), 20)
    n0 = int(full[1][1])
    # frame 1 over max_frame_points: rejected, frame 0 as it was
    small = oracle.crop(ix, T, r, 2 * len(p), len(p) - 1, 20)
    assert list(small[3]) == [0, 1, 4, 5] and list(small[1]) == [0, n0, n0, n0, n0] and np.array_equal(small[0], full[0][:n0])
    # too small a cap rejects the frame that would pass it; too small a max_cells the frame with the wide window
    assert list(oracle.crop(ix, T, r, n0 + 10, len(p), 20)[3]) == [0, 1, 4, 5]
    assert list(oracle.crop(ix, T, r, 2 * len(p), len(p), 19)[3]) == [0, 1, 4, 5]
    assert list(oracle.crop(ix, T[:1], [-1.0], 10, 10, 20)[3]) == [5] and list(oracle.crop(ix, T[:1], [np.inf], 10, 10, 20)[3]) == [5]


def test_oracle_pose_is_the_rigid_inverse_product():
    rng = np.random.default_rng(2)
    A = np.stack([mc.prior(rng.uniform(-50, 50, 2), 1, mc.rotation("generic", 1, s), 1.0) for s in range(4)])
    P = np.stack([mc.prior(rng.uniform(-5, 5, 2), 1, mc.rotation("generic", 1, 10 + s), -0.5) for s in range(4)])
    assert np.abs(oracle.pose(A, P) - A @ np.linalg.inv(P)).max() < 1e-12


# ---------------------------------------------------------------------------------------------------------------- argument errors
def test_build_argument_errors_need_no_device():
    p = mc.grid_map(1)
    for bad, match in ((dict(points=p.astype(np.float64)), "float32"), (dict(points=p[:, :3]), "float32"), (dict(up_axis=3), "up_axis"),
                       (dict(cell=0.0), "cell"), (dict(cell=-1.0), "cell"), (dict(cell=float("nan")), "cell"),
                       (dict(origin=(0.0, np.inf)), "origin"), (dict(origin=(0.0,)), "origin"), (dict(shape=(5, 4)), "origin"),
                       (dict(origin=mc.ORIGIN, shape=(4096, 4097)), "2\\^24"), (dict(cell=1e-4), "2\\^24"), (dict(points=p[:0]), "rows")):
        kw = dict(points=p, cell=mc.CELL, up_axis=1)
        kw.update(bad)
        with pytest.raises(ValueError, match=match):
            map_index.MapIndex.build(kw.pop("points"), **kw)


def test_crop_and_plan_argument_errors_need_no_device():
    ix = _fake_index()
    T, r = mc.grid_frames(1)
    skew = T.copy()
    skew[0, 0, 0] += 1e-5
    last = T.copy()
    last[0, 3, 0] = 0.5
    for args, match in (((T[:, :3], r, 100), "T_map_prior"), ((T.astype(np.int64), r, 100), "T_map_prior"), ((skew, r, 100), "rigid"),
                        ((last, r, 100), "rigid"), ((T, r[:3], 100), "radius"), ((T, "x", 100), "radius"), ((T, r, (1 << 20) + 1), "max_frame_points"),
                        ((T, r, -1), "max_frame_points")):
        with pytest.raises(ValueError, match=match):
            ix.crop(*args)
    with pytest.raises(ValueError, match="cap"):
        ix.crop(T, r, 100, cap=-1)
    with pytest.raises(ValueError, match="max_cells"):
        ix.crop(T, r, 100, max_cells=0)
    for args, match in (((None, 4, 10, 10, 5.0), "MapIndex"), ((ix, -1, 10, 10, 5.0), "B and cap"), ((ix, 4, -1, 10, 5.0), "B and cap"),
                        ((ix, 4, 10, 1 << 21, 5.0), "max_frame_points"), ((ix, 4, 10, 10, 0.0), "max_radius"), ((ix, 4, 10, 10, np.inf), "max_radius")):
        with pytest.raises(ValueError, match=match):
            map_index.CropPlan(*args)
    with pytest.raises(ValueError, match="2\\^28"):
        map_index.CropPlan(_fake_index(4096, 4096, 1.0), 1 << 12, 10, 10, 1e6)
    assert map_index.max_window_cells(ix, 1.5) == 2 * 2 and map_index.max_window_cells(ix, 40.0) == mc.NX * mc.NY
    assert map_index.max_window_cells(ix, 5.0) == 4 * 4                     # floor(10 / 4) + 2 cells per axis at most


def test_raw_plan_argument_errors_need_no_device():
    ix = _fake_index()
    with pytest.raises(ValueError, match="kitti"):
        map_index.MapRawPlan(ix, _opt(), 2, 100, 50, 5.0, (128, 256), dataset="kitti")
    with pytest.raises(ValueError, match="max_frame_points"):
        map_index.MapRawPlan(ix, _opt(), 2, 100, 1 << 21, 5.0, (128, 256))
    T, r = mc.grid_frames(1)
    img = np.zeros((4, 128, 256, 3), np.uint8)
    K = np.tile(np.eye(3), (4, 1, 1))
    with pytest.raises(ValueError, match="kitti"):
        map_index.prepare_map_raw(ix, T, r, img, K, T, _opt(), 100, dataset="kitti")
    with pytest.raises(ValueError, match="T_map_prior"):
        map_index.prepare_map_raw(ix, T[0], r, img, K, T, _opt(), 100)
    with pytest.raises(ValueError, match="radius"):
        map_index.prepare_map_raw(ix, T, r[:2], img, K, T, _opt(), 100)
    with pytest.raises(ValueError, match="MapIndex"):
        map_index.prepare_map_raw(None, T, r, img, K, T, _opt(), 100)


def test_host_map_frames_rejects_and_stages():
    B, hw = 2, (128, 256)
    world = mc.street()
    hb = dict(mc.street_batches(world)[0], image=np.zeros((B,) + hw + (3,), np.uint8), K_raw=np.tile(np.eye(3), (B, 1, 1)))
    T, r, image, K_raw, P_cam_pc, gt, seed = host_map_frames(hb, B, hw, mc.STREET_RADIUS)
    assert T.shape == (B, 16) and T.dtype == torch.float64 and r.shape == (B,) and seed == 90
    want = np.linalg.inv(hb["T_map_cam_gt"]) @ hb["T_map_prior"]
    assert np.abs(P_cam_pc.numpy() - want).max() < 1e-12 and gt.dtype == torch.float64
    none = host_map_frames({k: v for k, v in hb.items() if k != "T_map_cam_gt"}, B, hw)
    assert none[5] is None and np.array_equal(none[4].numpy(), np.tile(np.eye(4), (B, 1, 1)))
    skew = hb["T_map_prior"].copy()
    skew[1, :3, :3] *= 1.001
    nan = hb["T_map_prior"].copy()
    nan[0, 0, 3] = np.nan
    assert host_map_frames(dict(hb, T_map_prior=nan), B, hw)[0].isnan().any()   # a non-finite prior is the device's to reject
    for bad, match in ((dict(T_map_prior=skew), "rigid"), (dict(T_map_prior=hb["T_map_prior"][:1]), "T_map_prior"),
                       (dict(T_map_prior=hb["T_map_prior"].astype(np.int32)), "T_map_prior"), (dict(radius=np.ones(3)), "radius"),
                       (dict(radius=mc.STREET_RADIUS + 1.0), "max_radius"), (dict(image=hb["image"][:, :100]), "image"),
                       (dict(image=hb["image"].astype(np.float32)), "image"), (dict(K_raw=hb["K_raw"][:1]), "K_raw"),
                       (dict(T_map_cam_gt=skew), "rigid"), (dict(T_map_cam_gt=nan), "finite"), (dict(radius=None), "no 'radius'")):
        with pytest.raises(ValueError, match=match):
            host_map_frames(dict(hb, **bad), B, hw, mc.STREET_RADIUS)


# ---------------------------------------------------------------------------------------------------------------- the street
def test_make_map_is_deterministic_and_street_like():
    a, b = mc.street(), mc.street()
    assert a["points"].dtype == np.float32 and a["points"].shape == (mc.STREET_ROWS, 4) and a["points"].tobytes() == b["points"].tobytes()
    assert a["poses"].tobytes() == b["poses"].tobytes() and a["poses"].shape == (16, 4, 4)
    p = a["points"]
    assert np.all(np.diff(p[::64, 2]) > 0) and 290 < p[:, 2].max() - p[:, 2].min() < 310          # scan order along a path of 300 m
    assert np.isfinite(p).all() and p[:, 3].min() >= 0 and p[:, 3].max() <= 1
    for T in a["poses"]:
        assert np.abs(T[:3, :3].T @ T[:3, :3] - np.eye(3)).max() < 1e-12 and T[1, 3] == 0.0
    other = synthetic.make_map(np.random.default_rng(22), 1000)
    assert other["points"].shape == (1000, 4)


def test_street_frames_fit_the_executor_tests_capacities():
    """every frame of the GPU tests' batches keeps more than the network's 2048 points and fewer than STREET_MFP rows, except the one a test
    puts off the map on purpose, which keeps none"""
    world = mc.street()
    origin, nx, ny = oracle.default_grid(world["points"], mc.STREET_CELL, 1)
    ix = oracle.build(world["points"], mc.STREET_CELL, 1, origin, nx, ny)
    assert ix["status"] == 0
    cells = map_index.max_window_cells(_fake_index(nx, ny, mc.STREET_CELL), mc.STREET_RADIUS)
    for hb in mc.street_batches(world, off_map=[(1, 1)]):
        r = np.broadcast_to(np.asarray(hb["radius"], np.float64), (mc.STREET_B,))
        assert r.max() <= mc.STREET_RADIUS
        _, off, _, status = oracle.crop(ix, hb["T_map_prior"], r, mc.STREET_CAP, mc.STREET_MFP, cells)
        for f in range(mc.STREET_B):
            if hb["T_map_prior"][f, 0, 3] == mc.OFF_MAP[0]:
                assert status[f] == oracle.ST_EMPTY and off[f + 1] == off[f]
            else:
                assert status[f] == 0 and 2048 < off[f + 1] - off[f] < mc.STREET_MFP, (f, np.diff(off))
