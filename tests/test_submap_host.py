"""CPU: the Oxford sub-map stage (deepi2p_amd.submap, csrc/submap.hip) without a device -- tests/submap_oracle.py against the reference's own
my_build_pointcloud / downsample (tests/golden/submap_golden.npz, written by tests/golden/make_submap_golden.py), the exports, the argument
errors (all raised before anything touches a device), the synthetic traversal, and raw_prep's unchanged Oxford refusal."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from deepi2p_amd import _lib, raw_prep, submap, synthetic
from tests import submap_oracle as smo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "submap_golden.npz"))
NEW = ["di2p_submap_workspace_bytes", "di2p_submap_build", "di2p_submap_to_camera", "di2p_scan_prep_centroids_offset"]
GROUNDS = {"gnone": None, "gm1": -1, "g0p1": float(G["ground"])}
SKIPS = {"snone": None, "s16": float(G["skip"])}
CASES = [(g, s) for g in GROUNDS for s in SKIPS]
U24, U53 = 2.0 ** -24, 2.0 ** -53


def golden_case(g, s):
    """the arrays of one case; the big arrays of the -1 cases are stored under gnone (the generator asserted that they are equal)"""
    assert bool(G["gm1_equals_gnone"])
    big = "gnone" if g == "gm1" else g
    out = {k: G["%s_%s_%s" % (g, s, k)] for k in ("kept", "skip_count", "raised", "raw_offsets", "record_offsets")}
    out.update({k: G["%s_%s_%s" % (big, s, k)] for k in ("raw64", "raw_refl", "record")})
    return out


def oracle_case(g, s):
    return (smo.build_raw(G["scan_xyr"], G["scan_offsets"], G["submap_offsets"], G["poses"], G["present"], G["G_posesource_laser"], SKIPS[s], GROUNDS[g]),
            smo.build_submaps(G["scan_xyr"], G["scan_offsets"], G["submap_offsets"], G["poses"], G["present"], G["G_posesource_laser"], G["G_cam"],
                              SKIPS[s], GROUNDS[g], voxel=float(G["voxel"])))


def raw_bound(g, kept):
    """8 * 2^-53 * (|M| . |p|) per surviving row, M = pose . G_posesource_laser: the reference's product may order or fuse the four-term dots
    differently (and so may its pose . G)"""
    xyr, so = G["scan_xyr"], G["scan_offsets"]
    out = []
    for s in np.nonzero(kept == 1)[0]:
        rows = xyr[so[s]:so[s + 1]]
        if GROUNDS[g] is not None and GROUNDS[g] > -1:
            rows = rows[rows[:, 0] < GROUNDS[g]]
        M = np.abs(G["poses"][s]) @ np.abs(G["G_posesource_laser"])
        out.append(np.abs(rows[:, :1]) * M[:3, 0] + np.abs(rows[:, 1:2]) * M[:3, 1] + M[:3, 3])
    return 8 * U53 * np.concatenate(out)


@pytest.mark.parametrize("g,s", CASES)
def test_oracle_against_the_reference(g, s):
    want = golden_case(g, s)
    raw, rec = oracle_case(g, s)
    # counts and flags: exact
    assert np.array_equal(raw["kept"], want["kept"]) and np.array_equal(rec["kept"], want["kept"])
    assert np.array_equal(raw["skip_count"], want["skip_count"])
    assert np.array_equal(raw["offsets"], want["raw_offsets"])
    assert np.array_equal(rec["offsets"], want["record_offsets"])
    assert np.array_equal(rec["voxel_counts"], np.diff(want["record_offsets"]))
    assert np.array_equal(raw["status"], 4 * want["raised"].astype(np.int32))          # the reference raises IOError exactly where status is 4
    assert list(want["raised"]) == [0, 0, 0, 1]
    # raw cloud in fp64, the reflectance exactly
    diff = np.abs(raw["points64"] - want["raw64"])
    bound = raw_bound(g, want["kept"])
    print("%s %s raw: largest |difference| %.3e, largest bound %.3e" % (g, s, diff.max(), bound.max()))
    assert np.all(diff <= bound)
    assert np.array_equal(raw["points"][:, 3], want["raw_refl"].astype(np.float32))
    # the record: (sqrt 3 + 1) 2^-24 R on the coordinates (input rounding carried through a rigid transform + the final rounding), R the
    # largest point norm of the case; 2 * 2^-24 * max reflectance on the intensity
    R = max(np.linalg.norm(want["raw64"], axis=1).max(), np.linalg.norm(want["record"][:, :3].astype(np.float64), axis=1).max())
    dc = np.abs(rec["record"][:, :3].astype(np.float64) - want["record"][:, :3].astype(np.float64)).max()
    di = np.abs(rec["record"][:, 3].astype(np.float64) - want["record"][:, 3].astype(np.float64)).max()
    print("%s %s record: coordinates %.3e (bound %.3e), intensity %.3e (bound %.3e)" % (g, s, dc, (3 ** 0.5 + 1) * U24 * R, di,
                                                                                         2 * U24 * want["raw_refl"].max()))
    assert dc <= (3 ** 0.5 + 1) * U24 * R
    assert di <= 2 * U24 * want["raw_refl"].max()


def test_the_golden_cases_are_the_ones_promised():
    assert list(G["counts"]) == [37, 66, 5, 3] and list(np.diff(G["submap_offsets"])) == [37, 66, 5, 3]
    rows = np.diff(G["scan_offsets"])
    assert rows.min() == 0 and rows.max() == 130 and np.sort(rows)[-2] == 128 and {0, 1, 63, 64, 65, 70} <= set(rows.tolist())
    pres, kept = G["present"], G["gnone_s16_kept"]
    assert np.all(pres[-3:] == 0) and pres[37] == 0 and kept[37] == -1 and kept[38] == 1          # a missing first profile
    assert list(kept[10:13]) == [0, 0, 1]                          # "last kept", not "previous profile"
    assert kept[20] == 1 and kept[21] == 0                          # the emptied profile is kept and is the next "previous"
    so = G["scan_offsets"]
    assert np.all(G["scan_xyr"][so[20]:so[21], 0] >= float(G["ground"])) and so[21] > so[20]
    assert np.all(G["gnone_snone_kept"][pres != 0] == 1)
    for g, s in CASES:
        assert np.array_equal(G["%s_%s_kept" % (g, s)], G["gnone_%s_kept" % s])          # the ground filter never changes the keep rule


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
    assert "submap.hip" in build.SOURCES and build.PER_FILE_FLAGS["submap.hip"] == ["-ffp-contract=off"]
    l = _lib.load()
    assert l.di2p_version() == 9
    assert l.di2p_submap_workspace_bytes(8, 20000) > l.di2p_submap_workspace_bytes(8, 10000) >= 3 * 4 * 10000
    assert l.di2p_submap_workspace_bytes(-1, 10) == 0
    assert 0 < l.di2p_scan_prep_centroids_offset(4, 1000) < l.di2p_scan_prep_workspace_bytes(4, 1000) - 24 * 1000
    assert l.di2p_scan_prep_centroids_offset(4, 1000) % 256 == 0 and l.di2p_scan_prep_centroids_offset(-1, 5) == -1


def _cpu_batch(S=4, P=10, B=2):
    return dict(scan_xyr=torch.zeros((P, 3), dtype=torch.float64), scan_offsets=np.array([0, 2, 5, 5, 10][:S + 1]), submap_offsets=np.array([0, 1, S][:B + 1]),
                poses=torch.eye(4, dtype=torch.float64).repeat(S, 1, 1), present=torch.ones(S, dtype=torch.uint8), G_posesource_laser=np.eye(4))


def test_argument_errors_are_raised_on_the_host():
    """every tensor below lives on the CPU: an error that needed the device would surface as another exception"""
    b = _cpu_batch()
    raw = lambda **kw: submap.build_raw(**dict(b, **kw))
    with pytest.raises(ValueError, match="max_frame_points"):
        raw(max_frame_points=(1 << 20) + 1)
    with pytest.raises(ValueError, match="skip_threshold"):
        raw(skip_threshold=-0.5)
    with pytest.raises(ValueError, match="skip_threshold"):
        raw(skip_threshold=float("nan"))
    with pytest.raises(ValueError, match="ground_threshold"):
        raw(ground_threshold=float("nan"))
    with pytest.raises(ValueError, match="scan_xyr"):
        raw(scan_xyr=b["scan_xyr"].float())
    with pytest.raises(ValueError, match="scan_xyr"):
        raw(scan_xyr=torch.zeros((10, 4), dtype=torch.float64))
    with pytest.raises(ValueError, match="poses"):
        raw(poses=b["poses"][:, :3])
    with pytest.raises(ValueError, match="poses"):
        raw(poses=b["poses"].float())
    with pytest.raises(ValueError, match="present"):
        raw(present=torch.ones(3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="present"):
        raw(present=torch.ones(4, dtype=torch.bool))
    with pytest.raises(ValueError, match="submap_offsets"):
        raw(submap_offsets=np.array([0, 3, 2]))                          # decreasing
    with pytest.raises(ValueError, match="submap_offsets"):
        raw(submap_offsets=np.array([1, 2, 4]))                          # does not start at 0
    with pytest.raises(ValueError, match="scan_offsets"):
        raw(scan_offsets=np.array([0, 5, 2, 5, 10]))
    with pytest.raises(ValueError, match="scan_offsets"):
        raw(scan_offsets=np.array([0, 2, 5, 10]))                        # S + 1 entries are needed
    with pytest.raises(ValueError, match="scan_offsets"):
        raw(scan_offsets=np.array([0.0, 2, 5, 5, 10]))
    with pytest.raises(ValueError, match="G_posesource_laser"):
        submap.build_raw(**dict(b, scan_offsets=torch.tensor([0, 2, 5, 5, 10], dtype=torch.int32), submap_offsets=torch.tensor([0, 1, 4], dtype=torch.int32),
                                G_posesource_laser=np.eye(3)))
    sub = lambda **kw: submap.build_submaps(**dict(b, **kw))
    with pytest.raises(ValueError, match="G_cam"):
        sub()
    with pytest.raises(ValueError, match="voxel"):
        sub(G_cam=np.eye(4), voxel=0.0)
    with pytest.raises(ValueError, match="max_frame_points"):
        sub(G_cam=np.eye(4), max_frame_points=1 << 21)
    with pytest.raises(ValueError, match="G_cam"):
        submap.build_submaps(**dict(b, scan_offsets=torch.tensor([0, 2, 5, 5, 10], dtype=torch.int32), submap_offsets=torch.tensor([0, 1, 4], dtype=torch.int32),
                                    G_cam=np.zeros((3, 4, 4))))
    # the plans: before any buffer is allocated
    with pytest.raises(ValueError, match="max_frame_points"):
        submap.SubmapPlan(2, 10, 100, 100, (1 << 20) + 1)
    with pytest.raises(ValueError, match="skip_threshold"):
        submap.SubmapPlan(2, 10, 100, 100, 100, skip_threshold=-1.0)
    with pytest.raises(ValueError, match="voxel"):
        submap.SubmapPlan(2, 10, 100, 100, 100, voxel=-0.1)
    with pytest.raises(ValueError, match=">= 0"):
        submap.SubmapPlan(2, -1, 100, 100, 100)
    with pytest.raises(ValueError, match="max_frame_points"):
        submap.OxfordRawPlan(SimpleNamespace(), 2, 10, 100, 100, (1 << 20) + 1)
    with pytest.raises(ValueError, match="img_scale"):
        submap.OxfordRawPlan(SimpleNamespace(img_scale=0.3), 2, 10, 100, 100, 100)


def test_pack_and_convenience_errors():
    pose = np.eye(4)[None]
    with pytest.raises(ValueError, match="scans and"):
        submap.pack_scans([([np.zeros((3, 3))], np.tile(pose, (2, 1, 1)))], device="cpu")
    with pytest.raises(ValueError, match=r"\[n, 3\]"):
        submap.pack_scans([([np.zeros((3, 4))], pose)], device="cpu")
    with pytest.raises(ValueError, match="float64"):
        submap.pack_scans([([np.zeros((3, 3), np.float32)], pose)], device="cpu")
    # the host form packs without a device: ragged on both levels, a missing profile takes no rows
    xyr, so, mo, poses, present = submap.pack_scans([([np.ones((3, 3)), None, np.zeros((0, 3))], np.tile(pose, (3, 1, 1))), ([], np.zeros((0, 4, 4))),
                                                     ([2 * np.ones((2, 3))], pose)], device="cpu")
    assert so.tolist() == [0, 3, 3, 3, 5] and mo.tolist() == [0, 3, 3, 4] and present.tolist() == [1, 0, 1, 1]
    assert xyr.dtype == torch.float64 and tuple(xyr.shape) == (5, 3) and tuple(poses.shape) == (4, 4, 4) and so.dtype == mo.dtype == torch.int32
    sm = [([np.zeros((3, 3))], pose)]
    img = np.zeros((1, 72, 96, 3), np.uint8)
    conv = lambda **kw: submap.prepare_oxford_raw(**dict(dict(submaps=sm, G_posesource_laser=np.eye(4), G_cam=np.eye(4), images=img, K_raw=np.eye(3)[None],
                                                              P_cam_pc=pose, opt=SimpleNamespace(img_H=24, img_W=32)), **kw))
    with pytest.raises(ValueError, match="images"):
        conv(images=None)
    with pytest.raises(ValueError, match="one image per sub-map"):
        conv(images=np.zeros((2, 72, 96, 3), np.uint8))
    with pytest.raises(ValueError, match="img_scale"):
        conv(opt=SimpleNamespace(img_scale=0.3))
    with pytest.raises(ValueError, match="skip_threshold"):
        conv(skip_threshold=-2.0)
    with pytest.raises(ValueError, match="G_cam"):
        conv(G_cam=np.eye(3))
    with pytest.raises(ValueError, match="G_posesource_laser"):
        conv(G_posesource_laser=None)


def test_ground_and_skip_arguments_follow_the_reference():
    assert submap._ground_args(None) == (0.0, 0) and submap._ground_args(-1) == (0.0, 0) and submap._ground_args(-1.5) == (0.0, 0)
    assert submap._ground_args(0.1) == (0.1, 1) and submap._ground_args(-0.5) == (-0.5, 1)
    assert submap._skip_arg(None) == -1.0 and submap._skip_arg(0.0) == 0.0 and submap._skip_arg(0.1 / 16) == 0.1 / 16


def test_synthetic_traversal():
    a = synthetic.make_lms_traversal(np.random.default_rng(5), 3, [120, 40, 7], 90)
    b = synthetic.make_lms_traversal(np.random.default_rng(5), 3, [120, 40, 7], 90)
    c = synthetic.make_lms_traversal(np.random.default_rng(6), 3, [120, 40, 7], 90)
    assert [len(s) for s, _ in a["submaps"]] == [120, 40, 7]
    for (sa, pa), (sb, pb) in zip(a["submaps"], b["submaps"]):          # deterministic per seed
        assert np.array_equal(pa, pb) and len(sa) == len(sb)
        assert all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(sa, sb))
    assert not np.array_equal(a["submaps"][0][1], c["submaps"][0][1])
    scans, poses = a["submaps"][0]
    rows = [len(s) for s in scans if s is not None]
    assert max(rows) <= 90 and len(set(rows)) > 5 and all(s.dtype == np.float64 and s.shape[1] == 3 for s in scans if s is not None)
    assert np.allclose(poses[60], np.eye(4)) and np.allclose(poses[:, 3], [0, 0, 0, 1])
    R = poses[:, :3, :3]
    assert np.allclose(R @ R.transpose(0, 2, 1), np.eye(3), atol=1e-12)
    present = np.array([s is not None for s in scans], np.uint8)
    kept, skipped = smo.keep_chain(poses, present, 0.1 / 16)
    assert set(kept.tolist()) == {1, 0, -1} and skipped == int(np.sum(kept == 0)) > 0          # all three kept values
    x = np.concatenate([s[:, 0] for s in scans if s is not None])
    assert x.max() > 1.0 and x.min() < 0.5                                   # a road below (x points to the ground) and walls above it
    assert a["G_posesource_laser"].shape == (4, 4) and a["G_cam"].shape == (4, 4)
    # an int gives every sub-map the same number of profiles
    d = synthetic.make_lms_traversal(np.random.default_rng(1), 2, 9, 20)
    assert [len(s) for s, _ in d["submaps"]] == [9, 9]


@pytest.mark.parametrize("dataset", ["oxford", "nuscenes"])
def test_raw_prep_still_refuses_oxford(dataset):
    """the KITTI raw-frame plan keeps its refusal: the Oxford raw stage is deepi2p_amd.submap, a module of its own"""
    with pytest.raises(ValueError, match="raw-scan stage"):
        raw_prep.RawFramePlan(SimpleNamespace(), 1, 100, 100, dataset=dataset)
    with pytest.raises(ValueError, match="raw-scan stage"):
        raw_prep.prepare_raw([np.zeros((4, 4), np.float32)], np.zeros((1, 370, 1226, 3), np.uint8), np.eye(3)[None], np.eye(4)[None],
                             SimpleNamespace(), dataset=dataset)
