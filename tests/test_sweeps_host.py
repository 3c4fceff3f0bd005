"""CPU: the nuScenes sweep stage (deepi2p_amd.sweeps, sweep_pipeline, csrc/sweeps.hip) without a device -- sweep_picks against the reference's
own walk, tests/sweeps_oracle.py against the reference's own functions (tests/golden/sweeps_golden.npz, written by
tests/golden/make_sweeps_golden.py), the exports, the argument errors (all raised before anything touches a device), the executor's batch
validation and the synthetic sweeps."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from scipy.spatial.transform import Rotation

from deepi2p_amd import _lib, sweep_pipeline, sweeps, synthetic
from tests import sweeps_oracle as swo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "sweeps_golden.npz"))
NEW = ["di2p_sweep_workspace_bytes", "di2p_pose_matrices", "di2p_sweep_transforms", "di2p_sweep_accumulate"]
RECORD_KEYS = ("ego", "lidar_calib", "cam_pose", "cam_calib")
MATRIX_KEYS = ("P_ego", "P_vehicle_lidar", "P_ego_cam", "P_vehicle_cam")


def scipy_matrices(records):
    """what the generator's Quaternion stub and get_P_from_Rt give: float32 rotation and translation in a float64 4x4"""
    rec = np.asarray(records, dtype=np.float64)
    P = np.tile(np.eye(4), (len(rec), 1, 1))
    P[:, :3, :3] = Rotation.from_quat(rec[:, [1, 2, 3, 0]]).as_matrix().astype(np.float32)
    P[:, :3, 3] = rec[:, 4:].astype(np.float32)
    return P


def f32_ulp(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


def test_sweep_picks_follow_the_reference_walk():
    table = G["walk_picks"]
    for w, (num, skip) in enumerate(G["walks"]):
        for length in range(table.shape[1]):
            want = [int(v) for v in table[w, length] if v > 0]
            nxt, prv = sweeps.sweep_picks(length, table.shape[1] - 1 - length, int(num), int(skip))
            assert nxt == want, (num, skip, length)
            assert prv == [int(v) for v in table[w, table.shape[1] - 1 - length] if v > 0]
            assert swo.sweep_picks(length, int(num), int(skip)) == want
    assert table.shape[1] == 15 and len(G["walks"]) >= 4
    assert sweeps.sweep_picks(13, 12) == ([4, 8, 12], [4, 8, 12]) and sweeps.sweep_picks(0, 0) == ([], []) and sweeps.sweep_picks(9, 3) == ([4, 8], [])
    for b, (n_next, n_prev) in enumerate(G["available"]):          # the picks the reference made for the golden frames
        nxt, prv = sweeps.sweep_picks(int(n_next), int(n_prev), int(G["frame_num"]), int(G["frame_skip"]))
        assert nxt == [int(v) for v in G["picks_next"][b] if v > 0] and prv == [int(v) for v in G["picks_prev"][b] if v > 0]
        assert 1 + len(nxt) + len(prv) == np.diff(G["frame_offsets"])[b]
    for bad in ((1, 1, -1, 4), (1, 1, 3, 0), (-1, 0, 3, 4), (0, -2, 3, 4)):
        with pytest.raises(ValueError, match="sweeps:"):
            sweeps.sweep_picks(*bad)


def test_the_golden_cases_are_the_ones_promised():
    assert list(np.diff(G["frame_offsets"])) == [7, 1, 3, 2]
    rows = np.diff(G["sweep_offsets"])
    assert {0, 1, 63, 64, 65, 255, 256, 257} <= set(rows.tolist()) and G["rows"].shape[1] == 5 and G["rows"].dtype == np.float32
    kept, counts = G["kept"], np.diff(G["offsets"])
    assert kept[6] == 0 and rows[6] > 0                                   # a sweep wholly inside the ego box
    assert counts[3] == 0 and rows[-2:].min() > 0                         # the last frame wholly inside it
    assert counts[0] > 2 * int(G["input_pt_num"]) > counts[1] > 0 and 2 * int(G["input_pt_num"]) > counts[2] > 0
    assert 1500 < np.abs(G["ego"][:, 4:6]).min()
    x, y = G["rows"][:, 0], G["rows"][:, 1]
    for edge, col, other in ((0.8, x, np.abs(y) < 2.7), (2.7, y, np.abs(x) < 0.8)):
        e = np.float32(edge)
        for v in (e, np.nextafter(e, np.float32(0)), np.nextafter(e, np.float32(10))):
            assert np.any((col == v) & other) and np.any((col == -v) & other), (edge, v)
    assert np.any((np.abs(x) < 0.8) & (np.abs(y) > 2.7)) and np.any((np.abs(x) > 0.8) & (np.abs(y) < 2.7))
    # the float32 comparison: a row exactly on an edge is kept, its neighbour towards zero is removed
    edge = np.array([[np.float32(0.8), 0.5, 0, 0], [np.nextafter(np.float32(0.8), np.float32(0)), 0.5, 0, 0]], np.float32)
    assert list(swo.keep_mask(edge)) == [True, False]


def test_oracle_poses_against_the_reference():
    for rk, mk in zip(RECORD_KEYS, MATRIX_KEYS):
        got, want = swo.pose_matrices(G[rk]), G[mk]
        assert np.array_equal(want, scipy_matrices(G[rk]))                # the stored matrices are what the stub gives
        assert np.array_equal(got[:, :, 3], want[:, :, 3]) and np.array_equal(got[:, 3], want[:, 3])          # translation, last row: exact
        err = np.abs(got - want)
        print("%s: %d of %d rotation entries differ, largest %.3f ulp" % (rk, np.count_nonzero(err), 9 * len(got), (err / f32_ulp(want)).max()))
        assert np.all(err <= f32_ulp(want))
        assert np.array_equal(got, got.astype(np.float32).astype(np.float64))


def test_oracle_transforms_against_the_reference():
    """fed the reference's own P matrices, so the quaternion step does not enter: within sweeps_oracle.chain_bounds, gamma_38 times the product
    of the absolute matrices, of the reference's result"""
    fo = G["frame_offsets"]
    T, Pcp = swo.sweep_transforms(G["P_ego"], fo, G["P_vehicle_lidar"], G["P_ego_cam"], G["P_vehicle_cam"])
    k, bT, bP = swo.chain_bounds(G["P_ego"], fo, G["P_vehicle_lidar"], G["P_ego_cam"], G["P_vehicle_cam"])
    assert k == 38
    eT, eP = np.abs(T - G["T"]), np.abs(Pcp - G["P_cam_pc"])
    ratio = lambda e, b: (e[b > 0] / b[b > 0]).max()
    print("T: largest |difference| %.3e, largest ratio to gamma_%d . product %.4f; P_cam_pc: %.3e, %.4f" % (eT.max(), k, ratio(eT, bT), eP.max(), ratio(eP, bP)))
    assert np.all(eT <= bT) and np.all(eP <= bP)
    for b in range(len(fo) - 1):
        assert np.array_equal(T[fo[b]], np.eye(4))                        # the key sweep: the exact identity


def test_oracle_cloud_against_the_reference():
    got = swo.accumulate(G["rows"], G["sweep_offsets"], G["frame_offsets"], G["T"])
    assert np.array_equal(got["kept"], G["kept"]) and np.array_equal(got["offsets"], G["offsets"])          # counts and order: exact
    assert list(got["status"]) == [0, 0, 0, 4]
    assert np.array_equal(got["points"][:, 3], G["intensity"])
    err = np.abs(got["points"][:, :3].astype(np.float64) - G["cloud64"])
    print("cloud: largest error %.3f float32 ulp" % (err / f32_ulp(G["cloud64"])).max())
    assert np.all(err <= f32_ulp(G["cloud64"]))
    # the key sweeps are the input's rows bit for bit; cols = 4 gives the same result
    so, fo, off = G["sweep_offsets"], G["frame_offsets"], G["offsets"]
    for b in range(3):
        key = G["rows"][so[fo[b]]:so[fo[b] + 1], :4]
        key = key[swo.keep_mask(key)]
        assert got["points"][off[b]:off[b] + len(key)].tobytes() == np.ascontiguousarray(key).tobytes()
    again = swo.accumulate(np.ascontiguousarray(G["rows"][:, :4]), so, fo, G["T"])
    assert again["points"].tobytes() == got["points"].tobytes()
    # with the oracle's own matrices from the records, end to end
    P = [swo.pose_matrices(G[k]) for k in RECORD_KEYS]
    T, _ = swo.sweep_transforms(P[0], fo, P[1], P[2], P[3])
    own = swo.accumulate(G["rows"], so, fo, T)
    d = np.abs(own["points"][:, :3].astype(np.float64) - G["cloud64"]).max()
    print("cloud from the records: largest |difference| %.3e m" % d)
    assert np.array_equal(own["offsets"], G["offsets"]) and d < 1e-3          # a float32 ulp of a rotation entry times 2000 m is 1.2e-4 m


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
    assert "sweeps.hip" in build.SOURCES and build.PER_FILE_FLAGS["sweeps.hip"] == ["-ffp-contract=off"]
    l = _lib.load()
    assert l.di2p_version() == 9
    assert l.di2p_sweep_workspace_bytes(32, 448) > l.di2p_sweep_workspace_bytes(32, 224) >= 2 * 4 * 32 * 224
    assert l.di2p_sweep_workspace_bytes(-1, 10) == 0 and l.di2p_sweep_workspace_bytes(1, (1 << 24) + 1) == 0


def _cpu_batch():
    return dict(rows=torch.zeros((10, 4), dtype=torch.float32), sweep_offsets=np.array([0, 2, 5, 5, 10]), frame_offsets=np.array([0, 1, 4]),
                T=torch.eye(4, dtype=torch.float64).repeat(4, 1, 1))


def test_argument_errors_are_raised_on_the_host():
    """every tensor below lives on the CPU: an error that needed the device would surface as another exception"""
    b = _cpu_batch()
    acc = lambda **kw: sweeps.accumulate_sweeps(**dict(b, **kw))
    with pytest.raises(ValueError, match="max_frame_points"):
        acc(max_frame_points=(1 << 20) + 1)
    with pytest.raises(ValueError, match="box"):
        acc(box=(0.8,))
    with pytest.raises(ValueError, match="box"):
        acc(box=(float("nan"), 2.7))
    with pytest.raises(ValueError, match="rows"):
        acc(rows=b["rows"].double())
    with pytest.raises(ValueError, match="rows"):
        acc(rows=torch.zeros((10, 3), dtype=torch.float32))
    with pytest.raises(ValueError, match="T must"):
        acc(T=b["T"].float())
    with pytest.raises(ValueError, match="T must"):
        acc(T=b["T"][:, :3])
    with pytest.raises(ValueError, match="frame_offsets"):
        acc(frame_offsets=np.array([0, 3, 2]))
    with pytest.raises(ValueError, match="frame_offsets"):
        acc(frame_offsets=np.array([1, 2, 4]))
    with pytest.raises(ValueError, match="sweep_offsets"):
        acc(sweep_offsets=np.array([0, 5, 2, 5, 10]))
    with pytest.raises(ValueError, match="sweep_offsets"):
        acc(sweep_offsets=np.array([0, 2, 5, 10]))
    with pytest.raises(ValueError, match="sweep_offsets"):
        acc(sweep_offsets=np.array([0.0, 2, 5, 5, 10]))
    with pytest.raises(ValueError, match="cap"):
        acc(cap=-1)
    with pytest.raises(ValueError, match="records"):
        sweeps.pose_matrices(np.zeros((3, 6)))
    with pytest.raises(ValueError, match="records"):
        sweeps.pose_matrices(None)
    one = np.array([[1.0, 0, 0, 0, 0, 0, 0]])
    for bad in (torch.zeros((1, 4, 4)), torch.zeros((2, 4, 4), dtype=torch.float64), torch.zeros((1, 4, 8), dtype=torch.float64)[:, :, ::2], np.zeros((1, 4, 4))):
        with pytest.raises(ValueError, match="out must"):
            sweeps.pose_matrices(one, out=bad)
    P = torch.eye(4, dtype=torch.float64).repeat(4, 1, 1)
    with pytest.raises(ValueError, match="P_ego"):
        sweeps.sweep_transforms(P.float(), np.array([0, 1, 4]), P[:2], P[:2], P[:2])
    with pytest.raises(ValueError, match="P_ego_cam"):
        sweeps.sweep_transforms(P, np.array([0, 1, 4]), P[:2], P[:3], P[:2])
    with pytest.raises(ValueError, match="frame_offsets"):
        sweeps.sweep_transforms(P, np.array([0, 3, 2]), P[:2], P[:2], P[:2])
    # the plans: before any buffer is allocated
    with pytest.raises(ValueError, match="max_frame_points"):
        sweeps.SweepPlan(2, 10, 100, 100, (1 << 20) + 1)
    with pytest.raises(ValueError, match="cols"):
        sweeps.SweepPlan(2, 10, 100, 100, 100, cols=3)
    with pytest.raises(ValueError, match=">= 0"):
        sweeps.SweepPlan(2, -1, 100, 100, 100)
    with pytest.raises(ValueError, match="box"):
        sweeps.SweepPlan(2, 10, 100, 100, 100, box=(-1.0, 2.0))
    with pytest.raises(ValueError, match="max_frame_points"):
        sweeps.NuScenesRawPlan(SimpleNamespace(), 2, 10, 100, 100, (1 << 20) + 1)
    with pytest.raises(ValueError, match="img_scale"):
        sweeps.NuScenesRawPlan(SimpleNamespace(img_scale=0.3), 2, 10, 100, 100, 100)
    with pytest.raises(ValueError, match="cols"):
        sweeps.NuScenesRawPlan(SimpleNamespace(), 2, 10, 100, 100, 100, cols=6)


def test_pack_and_convenience_errors():
    with pytest.raises(ValueError, match="float32"):
        sweeps.pack_sweeps([[np.zeros((3, 4))]], device="cpu")
    with pytest.raises(ValueError, match="float32"):
        sweeps.pack_sweeps([[np.zeros((3, 3), np.float32)]], device="cpu")
    with pytest.raises(ValueError, match="same number of columns"):
        sweeps.pack_sweeps([[np.zeros((3, 4), np.float32), np.zeros((3, 5), np.float32)]], device="cpu")
    with pytest.raises(ValueError, match="list of sweeps"):
        sweeps.pack_sweeps([np.zeros((3, 4), np.float32)], device="cpu")
    # the host form packs without a device: ragged on both levels
    rows, so, fo = sweeps.pack_sweeps([[np.ones((3, 5), np.float32), np.zeros((0, 5), np.float32)], [], [2 * np.ones((2, 5), np.float32)]], device="cpu")
    assert so.tolist() == [0, 3, 3, 5] and fo.tolist() == [0, 2, 2, 3] and tuple(rows.shape) == (5, 5) and rows.dtype == torch.float32
    assert so.dtype == fo.dtype == torch.int32
    frames = [[np.zeros((3, 4), np.float32)]]
    rec = np.array([[1.0, 0, 0, 0, 0, 0, 0]])
    img = np.zeros((1, 140, 170, 3), np.uint8)
    opt = SimpleNamespace(crop_original_top_rows=10, img_H=24, img_W=32)
    conv = lambda **kw: sweeps.prepare_nuscenes_raw(**dict(dict(frames=frames, ego=[rec], lidar_calib=rec, cam_pose=rec, cam_calib=rec, images=img,
                                                                K_raw=np.eye(3)[None], opt=opt), **kw))
    with pytest.raises(ValueError, match="images"):
        conv(images=None)
    with pytest.raises(ValueError, match="one image per frame"):
        conv(images=np.zeros((2, 140, 170, 3), np.uint8))
    with pytest.raises(ValueError, match="img_scale"):
        conv(opt=SimpleNamespace(img_scale=0.3))
    with pytest.raises(ValueError, match="box"):
        conv(box=None)
    with pytest.raises(ValueError, match="ego"):
        conv(ego=[np.tile(rec, (2, 1))])
    with pytest.raises(ValueError, match="cam_calib"):
        conv(cam_calib=np.zeros((1, 6)))
    with pytest.raises(ValueError, match="lidar_calib"):
        conv(lidar_calib=None)


def _host_batch():
    s = synthetic.make_nuscenes_sweeps(np.random.default_rng(3), 2, [3, 1], 20)
    return dict(sweeps=s["frames"], ego=s["ego"], lidar_calib=s["lidar_calib"], cam_pose=s["cam_pose"], cam_calib=s["cam_calib"],
                image=np.zeros((2, 140, 170, 3), np.uint8), K_raw=np.tile(np.eye(3), (2, 1, 1)), seed=7)


def test_executor_batch_validation_needs_no_device():
    hb = _host_batch()
    check = lambda batch, **kw: sweep_pipeline.host_sweep_frames(batch, **dict(dict(B=2, S_cap=6, cap_raw=100, raw_hw=(140, 170), cols=5), **kw))
    parts, so, fo, ego, recs, image, K_raw, seed, cols = check(hb)
    assert cols == 5 and check(hb, cols=None)[-1] == 5
    assert so.tolist() == [0, 20, 40, 60, 80] and fo.tolist() == [0, 3, 4] and so.dtype == fo.dtype == torch.int32
    assert len(parts) == 4 and tuple(ego.shape) == (4, 7) and ego.dtype == torch.float64 and [tuple(r.shape) for r in recs] == [(2, 7)] * 3 and seed == 7
    # the flat form is the same batch; host rows past the last offset are ignored
    flat = dict(hb, sweeps=np.concatenate([s for f in hb["sweeps"] for s in f] + [np.full((3, 5), np.nan, np.float32)]), sweep_offsets=so.numpy(),
                frame_offsets=fo.numpy(), ego=np.concatenate(hb["ego"]))
    p2, so2, fo2, ego2 = check(flat)[:4]
    assert torch.equal(so2, so) and torch.equal(fo2, fo) and torch.equal(ego2, ego) and torch.equal(p2[0], torch.cat(parts))
    for key in ("sweeps", "ego", "lidar_calib", "cam_pose", "cam_calib", "image", "K_raw"):
        with pytest.raises(ValueError, match=key):
            check({k: v for k, v in hb.items() if k != key})
    with pytest.raises(ValueError, match="B = 2"):
        check(dict(hb, sweeps=hb["sweeps"][:1], ego=hb["ego"][:1]))
    with pytest.raises(ValueError, match="S_cap"):
        check(hb, S_cap=3)
    with pytest.raises(ValueError, match="cap_raw"):
        check(hb, cap_raw=79)
    with pytest.raises(ValueError, match="float32"):
        check(dict(hb, sweeps=[[s.astype(np.float64) for s in f] for f in hb["sweeps"]]))
    with pytest.raises(ValueError, match="columns"):
        check(hb, cols=4)
    with pytest.raises(ValueError, match="ego"):
        check(dict(hb, ego=hb["ego"][:1]))
    with pytest.raises(ValueError, match="cam_pose"):
        check(dict(hb, cam_pose=hb["cam_pose"][:1]))
    with pytest.raises(ValueError, match="image"):
        check(dict(hb, image=hb["image"][:, :100]))
    with pytest.raises(ValueError, match="K_raw"):
        check(dict(hb, K_raw=np.eye(3)))
    with pytest.raises(ValueError, match="sweep_offsets"):
        check({k: v for k, v in flat.items() if k != "sweep_offsets"})
    with pytest.raises(ValueError, match="sweep_offsets"):
        check(dict(flat, sweep_offsets=np.array([0, 20, 10, 60, 80])))
    with pytest.raises(ValueError, match="frame_offsets"):
        check(dict(flat, frame_offsets=np.array([0, 3, 5])))
    with pytest.raises(ValueError, match="float32"):
        check(dict(flat, sweeps=flat["sweeps"].astype(np.float64)))


def test_synthetic_sweeps():
    a = synthetic.make_nuscenes_sweeps(np.random.default_rng(5), 3, [7, 1, 3], 200)
    b = synthetic.make_nuscenes_sweeps(np.random.default_rng(5), 3, [7, 1, 3], 200)
    c = synthetic.make_nuscenes_sweeps(np.random.default_rng(6), 3, [7, 1, 3], 200)
    assert [len(f) for f in a["frames"]] == [7, 1, 3] and [e.shape for e in a["ego"]] == [(7, 7), (1, 7), (3, 7)]
    for fa, fb in zip(a["frames"], b["frames"]):          # deterministic per seed
        assert all(np.array_equal(x, y) for x, y in zip(fa, fb))
    assert not np.array_equal(a["frames"][0][0], c["frames"][0][0])
    s = a["frames"][0][0]
    assert s.dtype == np.float32 and s.shape == (200, 5)
    inside = ~swo.keep_mask(s)
    assert 0 < inside.sum() < 30                                              # returns on the ego car, and only a few
    assert s[:, 2].min() < -1.5 and s[:, 2].max() > 1.0                       # z-up: a road below the sensor, walls above it
    ego = np.concatenate(a["ego"])
    assert np.allclose(np.linalg.norm(ego[:, :4], axis=1), 1.0) and np.abs(ego[:, 4:6]).min() > 1000.0
    assert np.any(ego[:, 4:].astype(np.float32).astype(np.float64) != ego[:, 4:])          # the float32 rounding of the poses matters
    for k in ("lidar_calib", "cam_pose", "cam_calib"):
        assert a[k].shape == (3, 7) and np.allclose(np.linalg.norm(a[k][:, :4], axis=1), 1.0)
    # the sweeps of a frame see one static scene: accumulated with the oracle, the road stays a plane
    P = [swo.pose_matrices(r) for r in (ego, a["lidar_calib"], a["cam_pose"], a["cam_calib"])]
    fo = np.array([0, 7, 8, 11])
    T, Pcp = swo.sweep_transforms(P[0], fo, P[1], P[2], P[3])
    rows = np.concatenate([s for f in a["frames"] for s in f])
    acc = swo.accumulate(rows, np.arange(12) * 200, fo, T)
    first = acc["points"][:acc["offsets"][1]]
    world = first[:, :3].astype(np.float64) @ (P[0][0] @ P[1][0])[:3, :3].T + (P[0][0] @ P[1][0])[:3, 3]
    road = world[np.abs(world[:, 2]) < 0.5, 2]                               # the road is z = 0 in the map's frame, in every sweep of the frame
    assert len(road) > 600 and np.percentile(np.abs(road), 90) < 0.05          # (the rest are the feet of the walls)
    assert np.allclose(Pcp[0][3], [0, 0, 0, 1]) and abs(np.linalg.det(Pcp[0][:3, :3]) - 1) < 1e-6
    # an int gives every frame the same number of sweeps, a list of rows one count per sweep
    d = synthetic.make_nuscenes_sweeps(np.random.default_rng(1), 2, 2, [5, 0, 7, 1])
    assert [[len(s) for s in f] for f in d["frames"]] == [[5, 0], [7, 1]]
