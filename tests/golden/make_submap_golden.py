"""Generates tests/golden/submap_golden.npz (arrays only):   python tests/golden/make_submap_golden.py

From the reference's own my_build_pointcloud and downsample (data/oxford/build_dataset.py), extracted with ``ast`` at generation time as
tests/golden/make_sample_prep_ds_golden.py does (no reference text is stored), run against
  os.path.isfile      a fake that makes the profiles of the `present` mask missing
  np.fromfile         a fake that serves the generated rows (x, y, reflectance) of a profile
  vo_manager          a stub whose interpolate_vo_poses returns the generated poses as np.matrix (the SDK's type)
  open3d              a stub whose voxel_down_sample is tests/scan_prep_oracle.voxel_down_sample (the voxel stage stays pinned by
                      restatement only): points = its fp64 means, colors = its averaged fake colour
The camera transform of save_pc_img_for_traversal (:310) and the float32 record (:319-321) are restated in run_reference().

Cases: 4 sub-maps of 37, 66, 5 and 3 profiles; 0 .. 70 rows per profile (mostly few: the file stays small) and one of 130; every profile of the last sub-map missing (IOError);
a missing first profile; three moves below the skip threshold whose sum passes it; a kept profile the ground filter empties, followed by a
move below the threshold from IT; ground thresholds None, -1, 0.1; skip thresholds None, 0.1 / 16.

Asserted, redrawing until they hold: every delta-translation norm the reference computes lies at least 1e-9 m from the skip threshold, and
every fp64 cloud coordinate at least 1e-4 m from a voxel face (measured from the fp64 min_bound), in every case."""
import ast
import math
import os
import sys
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import ref_network as rn  # noqa: E402
from tests import scan_prep_oracle as spo  # noqa: E402

REF = rn.REF
COUNTS = (37, 66, 5, 3)
VOXEL = 0.1
SKIP = VOXEL / 16.0
GROUNDS = {"gnone": None, "gm1": -1, "g0p1": 0.1}
SKIPS = {"snone": None, "s16": SKIP}
BIG = ("raw64", "raw_refl", "record")
EMPTIED = 20          # profile of sub-map 0 whose rows all lie below the ground threshold's plane (x >= 0.5)


def _functions(path, names, ns):
    for node in ast.parse(open(path).read()).body:
        if isinstance(node, ast.FunctionDef) and node.name in names:
            exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), ns)


def _rot(axis, a):
    c, s = math.cos(a), math.sin(a)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.eye(4)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def make_poses(rng):
    """per sub-map f64[S,4,4], relative to the middle profile; steps of about 0.2 m, the special moves of the module docstring"""
    out = []
    for b, S in enumerate(COUNTS):
        step = rng.uniform(0.15, 0.25, S)
        if b == 0:
            step[10:13] = 0.003                      # 0.003, 0.006 (skipped), 0.009 from the last KEPT profile (kept)
            step[EMPTIED + 1] = 0.002                # below the threshold from the emptied (but kept) profile
            step[30] = 1e-4
        if b == 1:
            step[[5, 6, 7, 40, 41]] = [2e-3, 1e-3, 5e-3, 6.0e-3, 1e-3]
            step[1] = 0.004                          # profile 0 is missing: profile 1 has no previous profile and is kept
        yaw = 0.1 * np.sin(np.cumsum(step) / 4.0 + b)
        T = np.tile(np.eye(4), (S, 1, 1))
        pos = np.zeros(3)
        for i in range(S):
            pos = pos + step[i] * np.array([math.cos(yaw[i]), math.sin(yaw[i]), 0.01 * math.sin(i)])
            T[i] = _rot(2, yaw[i]) @ _rot(1, 0.01 * math.sin(i / 3.0)) @ _rot(0, 0.005 * math.cos(i / 5.0))
            T[i, :3, 3] = pos
        inv0 = np.linalg.inv(T[S // 2])
        out.append(np.stack([inv0 @ T[i] for i in range(S)]))
    return out


def make_present():
    present = [np.ones(S, np.uint8) for S in COUNTS]
    present[0][[4, 17]] = 0
    present[1][[0, 33, 34]] = 0
    present[3][:] = 0
    return present


def draw_rows(rng, n, emptied):
    x = rng.uniform(0.5, 1.5, n) if emptied else rng.uniform(-3.0, 1.5, n)
    y = rng.uniform(-8.0, 8.0, n)
    h = n // 3          # a third of the rows next to another row of the profile: voxels with several members
    if h:
        x[-h:], y[-h:] = x[:h] + rng.uniform(-0.03, 0.03, h), y[:h] + rng.uniform(-0.03, 0.03, h)
    return np.stack([x, y, rng.integers(0, 256, n).astype(np.float64)], 1)


def make_scans(rng):
    forced = {(0, 2): 0, (0, 3): 1, (0, 5): 63, (0, 6): 64, (0, 7): 65, (0, 8): 70, (1, 12): 130, (1, 13): 128, (0, EMPTIED): 24}
    scans = []
    for b, S in enumerate(COUNTS):
        scans.append([draw_rows(rng, forced.get((b, i), int(71 * rng.random() ** 2.5)), (b, i) == (0, EMPTIED)) for i in range(S)])
    return scans


class _Recorder:
    """numpy with a fake fromfile and a linalg.norm that records what it returns"""

    def __init__(self, rows_of):
        self.rows_of, self.norms, self.read = rows_of, [], []
        self.linalg = SimpleNamespace(inv=np.linalg.inv, norm=self._norm)

    def _norm(self, a):
        v = np.linalg.norm(a)
        self.norms.append(float(v))
        return v

    def fromfile(self, path, dtype):
        assert dtype is np.double
        i = int(os.path.basename(path)[:-4])
        self.read.append(i)
        return self.rows_of(i).reshape(-1).copy()

    def __getattr__(self, name):
        return getattr(np, name)


class _PointCloud:
    points = colors = None

    def voxel_down_sample(self, voxel_size):
        pts4 = np.concatenate([np.asarray(self.points), np.asarray(self.colors)[:, :1]], 1)
        v = spo.voxel_down_sample(pts4, voxel_size)
        out = _PointCloud()
        out.points = v["cen"]
        out.colors = np.concatenate([v["intensity"].astype(np.float64)[:, None], np.zeros((len(v["cen"]), 2))], 1)
        return out


OPEN3D = SimpleNamespace(geometry=SimpleNamespace(PointCloud=_PointCloud), utility=SimpleNamespace(Vector3dVector=lambda a: np.asarray(a)))


def run_reference(scans, poses, present, G, G_cam, ground, skip):
    """every sub-map through the reference -> (dict of arrays, norms, surviving-row map [(sub-map, profile, row)] per cloud column)"""
    kept_all, skips, raised, raw, refl_all, recs, where, norms = [], [], [], [], [], [], [], []
    for b, S in enumerate(COUNTS):
        fake_np = _Recorder(lambda i, b=b: scans[b][i])
        ns = {"np": fake_np, "open3d": OPEN3D,
              "os": SimpleNamespace(path=SimpleNamespace(join=os.path.join, isfile=lambda p, b=b: bool(present[b][int(os.path.basename(p)[:-4])])))}
        _functions(os.path.join(REF, "data", "oxford", "build_dataset.py"), {"my_build_pointcloud", "downsample"}, ns)
        vo = SimpleNamespace(interpolate_vo_poses=lambda ts, origin, b=b: [np.matrix(poses[b][i]) for i in ts])
        kept = np.where(present[b] != 0, 0, -1).astype(np.int32)
        try:
            pc, refl, skipped = ns["my_build_pointcloud"](np.matrix(G), "lms_front", vo, list(range(S)), S // 2, skip_threshold=skip,
                                                          remove_ground_threshold=ground)
        except IOError:
            kept[fake_np.read] = 1
            kept_all.append(kept); skips.append(0); raised.append(1); norms += fake_np.norms
            raw.append(np.zeros((0, 3))); refl_all.append(np.zeros(0)); recs.append(np.zeros((0, 4), np.float32))
            continue
        kept[fake_np.read] = 1
        assert skipped == int(np.sum(kept == 0))
        pc = np.asarray(pc)
        for i in fake_np.read:
            rows = scans[b][i]
            idx = np.nonzero(rows[:, 0] < ground)[0] if (ground is not None and ground > -1) else np.arange(len(rows))
            where += [(b, i, int(r)) for r in idx]
        pc2, refl2 = ns["downsample"](pc, refl, VOXEL)
        cam = np.dot(G_cam, pc2)                                                            # build_dataset.py:310
        rec = np.concatenate((np.asarray(cam)[0:3, :], np.expand_dims(refl2, axis=0)), axis=0).astype(np.float32)          # :319-321
        kept_all.append(kept); skips.append(skipped); raised.append(0); norms += fake_np.norms
        raw.append(pc[0:3].T.copy()); refl_all.append(np.asarray(refl, dtype=np.float64)); recs.append(rec.T.copy())
    off = lambda parts: np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int32)
    out = dict(kept=np.concatenate(kept_all), skip_count=np.array(skips, np.int32), raised=np.array(raised, np.uint8), raw64=np.concatenate(raw),
               raw_refl=np.concatenate(refl_all), raw_offsets=off(raw), record=np.concatenate(recs), record_offsets=off(recs))
    assert len(where) == len(out["raw64"])
    return out, norms, where


def face_violations(raw64, offsets):
    """cloud rows with a coordinate closer than 1e-4 m to a voxel face"""
    bad = []
    for b in range(len(offsets) - 1):
        p = raw64[offsets[b]:offsets[b + 1]]
        if len(p) == 0:
            continue
        f = (p - (p.min(0) - VOXEL * 0.5)) / VOXEL
        frac = f - np.floor(f)
        d = np.minimum(frac, 1.0 - frac) * VOXEL
        bad += list(offsets[b] + np.nonzero(np.any(d < 1e-4, 1))[0])
    return bad


def main():
    rng = np.random.default_rng(2026)
    G = np.array([[0.0, 0.0, -1.0, 1.6], [0.0, 1.0, 0.0, 0.05], [1.0, 0.0, 0.0, -1.1], [0.0, 0.0, 0.0, 1.0]]) @ _rot(0, 0.02) @ _rot(1, -0.015)
    G_cam = np.array([[0.0, 1.0, 0.0, 0.1], [0.0, 0.0, 1.0, 1.2], [1.0, 0.0, 0.0, -1.4], [0.0, 0.0, 0.0, 1.0]]) @ _rot(2, 0.01)
    present = make_present()
    while True:
        poses = make_poses(rng)
        scans = make_scans(rng)
        _, norms, _ = run_reference(scans, poses, present, G, G_cam, None, SKIP)
        if len(norms) and min(abs(n - SKIP) for n in norms) >= 1e-9:
            break
    for sweep in range(200):
        results, redraw = {}, set()
        for gname, ground in GROUNDS.items():
            for sname, skip in SKIPS.items():
                res, norms, where = run_reference(scans, poses, present, G, G_cam, ground, skip)
                assert skip is None or min(abs(n - SKIP) for n in norms) >= 1e-9
                redraw |= {where[j] for j in face_violations(res["raw64"], res["raw_offsets"])}
                results[gname + "_" + sname] = res
        if not redraw:
            break
        for b, i, r in sorted(redraw):
            scans[b][i][r, :2] = draw_rows(rng, 1, (b, i) == (0, EMPTIED))[0, :2]
    else:
        raise AssertionError("the voxel-face condition did not settle")
    print("settled after %d sweeps" % sweep)
    # the cases are what the module docstring says they are
    k = results["gnone_s16"]["kept"]
    off = np.concatenate([[0], np.cumsum(COUNTS)])
    assert list(k[10:13]) == [0, 0, 1] and k[EMPTIED] == 1 and k[EMPTIED + 1] == 0 and k[off[1]] == -1 and k[off[1] + 1] == 1
    assert np.all(results["gnone_snone"]["kept"][present_flat(present) != 0] == 1)
    assert np.all(scans[0][EMPTIED][:, 0] >= 0.1) and list(results["g0p1_s16"]["raised"]) == [0, 0, 0, 1]
    assert max(np.abs(r["raw64"]).max() for r in results.values()) < 64.0
    for sname in SKIPS:          # -1 disables the ground filter exactly as None does
        for key in results["gnone_" + sname]:
            assert np.array_equal(results["gnone_" + sname][key], results["gm1_" + sname][key]), key
    out = dict(counts=np.array(COUNTS, np.int32), voxel=np.float64(VOXEL), skip=np.float64(SKIP), ground=np.float64(0.1),
               G_posesource_laser=G, G_cam=G_cam, poses=np.concatenate(poses), present=present_flat(present),
               scan_xyr=np.concatenate([s for sub in scans for s in sub]),
               scan_offsets=np.concatenate([[0], np.cumsum([len(s) for sub in scans for s in sub])]).astype(np.int32),
               submap_offsets=off.astype(np.int32))
    out["gm1_equals_gnone"] = np.bool_(True)          # asserted above: the big arrays of the -1 cases are stored once, under gnone
    for case, res in results.items():
        for key, a in res.items():
            if not (case.startswith("gm1") and key in BIG):
                out[case + "_" + key] = a
    path = os.path.join(HERE, "submap_golden.npz")
    np.savez_compressed(path, **out)
    print("submap_golden.npz written: %d arrays, %d bytes" % (len(out), os.path.getsize(path)))


def present_flat(present):
    return np.concatenate(present)


if __name__ == "__main__":
    assert os.path.isdir(REF), "needs the reference checkout"
    main()
