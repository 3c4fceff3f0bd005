"""Generates tests/golden/sweeps_golden.npz (arrays only):   python tests/golden/make_sweeps_golden.py

From the reference's own functions (data/nuscenes_pc_img_pose_loader.py), extracted with ``ast`` at generation time as
tests/golden/make_submap_golden.py does (no reference text is stored): the module-level get_sample_data_ego_pose_P, get_calibration_P,
get_P_from_Rt and transform_pc_np, the methods get_lidar_pc_intensity_by_token, lidar_frame_accumulation and accumulate_lidar_points, and
the assignments of __getitem__ that lead to P_cam_pc.  They run against
  nusc                        a fake whose get() serves generated sample_data / ego_pose / calibrated_sensor records with next / prev links
  LidarPointCloud.from_file   a fake that serves the generated rows of a sweep as the devkit does (4 x N float32; the ring dropped) and
                              records which sweeps were read
  Quaternion                  a stub on scipy.spatial.transform.Rotation (which takes x, y, z, w).  pyquaternion is not installed where this
                              was written, so the quaternion-to-matrix step of the reference is pinned by restatement only.

Cases: 4 frames of 7, 1, 3 and 2 sweeps (all picks; a list that ends at once; a list that ends early on both sides; one pick); rows per
sweep 0, 1, 63, 64, 65, 255, 256, 257 and a few dozen; a sweep wholly inside the ego box; the last frame wholly inside it; rows exactly on the
four box edges and on the neighbouring floats; ego translations around 2000 m.  Asserted here: frame 0 keeps more than 2 * 256 rows (the
loader's voxel pass runs for input_pt_num = 256), frames 1 and 2 fewer (it does not); and no rotation entry of any pose or calibration is
within 1e-6 of zero (every sensor has a small mounting error about all three axes, as real calibrations have): two fp64 evaluations of a
rotation matrix differ by about 1e-16 absolutely, which next to zero is any number of float32 ulps, so "within one float32 ulp of the
reference's matrix" can only be asked of entries away from zero."""
import ast
import math
import os
import sys
from types import SimpleNamespace

import numpy as np
from scipy.spatial.transform import Rotation

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import ref_network as rn  # noqa: E402

REF = rn.REF
LOADER = os.path.join(REF, "data", "nuscenes_pc_img_pose_loader.py")
FRAME_NUM, FRAME_SKIP, N_INPUT = 3, 4, 256
AVAILABLE = [(13, 12), (0, 0), (9, 3), (4, 0)]          # sweeps after / before the key sweep of each frame
ROWS = [[257, 256, 255, 65, 64, 63, 40], [48], [None, 0, 1], [20, 12]]          # key | next picks | prev picks; None: the edge rows
INSIDE = {(0, 6), (3, 0), (3, 1)}                        # sweeps with every row inside the ego box
WALKS = [(3, 4), (1, 1), (2, 5), (4, 3), (0, 2), (3, 1)]          # (frame_num, frame_skip) of the stored pick table
MAX_LEN = 14


class Quaternion:
    def __init__(self, wxyz):
        w, x, y, z = wxyz
        self.rotation_matrix = Rotation.from_quat([x, y, z, w]).as_matrix()


def _module_functions(names, ns):
    for node in ast.parse(open(LOADER).read()).body:
        if isinstance(node, ast.FunctionDef) and node.name in names:
            exec(compile(ast.Module(body=[node], type_ignores=[]), LOADER, "exec"), ns)


def _class_body():
    for node in ast.parse(open(LOADER).read()).body:
        if isinstance(node, ast.ClassDef) and node.name == "nuScenesLoader":
            return node.body
    raise AssertionError("nuScenesLoader not found")


def _methods(names, ns):
    out = {}
    for sub in _class_body():
        if isinstance(sub, ast.FunctionDef) and sub.name in names:
            g = dict(ns)
            exec(compile(ast.Module(body=[sub], type_ignores=[]), LOADER, "exec"), g)
            out[sub.name] = g[sub.name]
    assert set(out) == set(names)
    return out


def _p_cam_pc_statements():
    """the assignments of __getitem__ to the seven names on the way to P_cam_pc, in source order"""
    names = {"lidar_calib_P", "lidar_pose_P", "camera_calib_P", "camera_pose_P", "camera_pose_P_inv", "camera_calib_P_inv", "P_cam_pc"}
    for sub in _class_body():
        if isinstance(sub, ast.FunctionDef) and sub.name == "__getitem__":
            body = [n for n in sub.body if isinstance(n, ast.Assign) and len(n.targets) == 1 and isinstance(n.targets[0], ast.Name)
                    and n.targets[0].id in names]
            assert [n.targets[0].id for n in body] == ["lidar_calib_P", "lidar_pose_P", "camera_calib_P", "camera_pose_P", "camera_pose_P_inv",
                                                       "camera_calib_P_inv", "P_cam_pc"]
            return compile(ast.Module(body=body, type_ignores=[]), LOADER, "exec")
    raise AssertionError("__getitem__ not found")


class FakeNusc:
    dataroot = ""

    def __init__(self):
        self.tables = {"sample_data": {}, "ego_pose": {}, "calibrated_sensor": {}}

    def get(self, table, token):
        return self.tables[table][token]

    def add_chain(self, name, n_prev, n_next, ego_records, calib_token):
        """sample_data records name:-n_prev .. name:+n_next, linked; ego_records: position -> (w, x, y, z, tx, ty, tz)"""
        tok = lambda i: "%s:%d" % (name, i)
        for i in range(-n_prev, n_next + 1):
            self.tables["sample_data"][tok(i)] = dict(token=tok(i), next=tok(i + 1) if i < n_next else "", prev=tok(i - 1) if i > -n_prev else "",
                                                      ego_pose_token="ego:" + tok(i), calibrated_sensor_token=calib_token, filename=tok(i))
            r = ego_records[i]
            self.tables["ego_pose"]["ego:" + tok(i)] = dict(rotation=list(r[:4]), translation=list(r[4:]))
        return tok(0)

    def add_calib(self, token, record):
        self.tables["calibrated_sensor"][token] = dict(rotation=list(record[:4]), translation=list(record[4:]))


def _quat(yaw, pitch, roll):
    x, y, z, w = (Rotation.from_euler("z", yaw) * Rotation.from_euler("y", pitch) * Rotation.from_euler("x", roll)).as_quat()
    return np.array([w, x, y, z])


def ego_record(rng, origin, heading, time):
    d = 8.0 * time
    yaw = heading + 0.2 * math.sin(d / 40.0)
    pos = origin + d * np.array([math.cos(heading), math.sin(heading), 0.0]) + [0.0, 0.0, 0.02 * math.sin(d / 3.0)]
    q = _quat(yaw, 0.004 * math.sin(d / 7.0), 0.003 * math.cos(d / 5.0))
    return np.concatenate([np.round(q, 16), pos])


def edge_rows(rng):
    """rows on the four box edges, on both neighbouring floats of each, and inside in one coordinate only"""
    out = []
    for edge, axis in ((0.8, 0), (2.7, 1)):
        e = np.float32(edge)
        for v in (e, np.nextafter(e, np.float32(0)), np.nextafter(e, np.float32(10))):
            for sign in (1, -1):
                xy = [np.float32(0.1), np.float32(0.5)]
                xy[axis] = np.float32(sign) * v
                out.append(xy)
    out += [[0.1, 3.5], [0.1, -3.5], [1.5, 0.3], [-1.5, 0.3], [0.0, 0.0], [0.79, 2.69], [-0.8, -2.7], [0.8, 2.7]]
    xy = np.asarray(out, dtype=np.float32)
    return np.concatenate([xy, rng.uniform(-1.5, 0.5, (len(xy), 1)).astype(np.float32)], 1)


def draw_rows(rng, n, inside):
    if inside:
        xyz = np.stack([rng.uniform(-0.79, 0.79, n), rng.uniform(-2.69, 2.69, n), rng.uniform(-1.6, -0.4, n)], 1)
    else:
        r, az = 2.0 + 50.0 * rng.random(n) ** 1.5, rng.uniform(0, 2 * math.pi, n)
        xyz = np.stack([r * np.cos(az), r * np.sin(az), rng.uniform(-2.0, 4.0, n)], 1)
        m = max(n // 12, 0)          # returns on the ego car among the others
        xyz[:m] = np.stack([rng.uniform(-0.79, 0.79, m), rng.uniform(-2.69, 2.69, m), rng.uniform(-1.6, -0.4, m)], 1)
        xyz = xyz[rng.permutation(n)]
    return xyz.astype(np.float32)


def picks(available, num, skip):
    return [k * skip for k in range(1, num + 1) if k * skip <= available]


def reference_walks(methods):
    """lidar_frame_accumulation itself on chains of every length, with a stub in place of the sweep reader -> [len(WALKS), MAX_LEN + 1, 4]
    distances from the key sweep (0: no pick)"""
    table = np.zeros((len(WALKS), MAX_LEN + 1, max(n for n, _ in WALKS)), np.int32)
    for w, (num, skip) in enumerate(WALKS):
        for length in range(MAX_LEN + 1):
            nusc = FakeNusc()
            key = nusc.add_chain("walk", 0, length, {i: np.array([1.0, 0, 0, 0, 0, 0, 0]) for i in range(length + 1)}, "c")
            read = []

            def reader(token, read=read):
                read.append(int(token.split(":")[1]))
                return np.zeros((3, 1), np.float32), np.zeros((1, 1), np.float32), np.eye(4)

            self = SimpleNamespace(nusc=nusc, opt=SimpleNamespace(accumulation_frame_num=num, accumulation_frame_skip=skip),
                                   get_lidar_pc_intensity_by_token=reader)
            methods["lidar_frame_accumulation"](self, nusc.get("sample_data", key), np.eye(4), np.eye(4), np.eye(4), "next", [], [])
            assert read == picks(length, num, skip), (num, skip, length, read)
            table[w, length, :len(read)] = read
    return table


def main():
    rng = np.random.default_rng(2027)
    nusc = FakeNusc()
    sweeps = {}          # filename -> f32[n,5]
    read = []

    class LidarPointCloud:
        def __init__(self, points):
            self.points = points

        @classmethod
        def from_file(cls, path):
            read.append(path)
            return cls(np.ascontiguousarray(sweeps[path][:, :4].T))

    recorded = []          # (P_ij_trans, kept rows) of every transformed sweep

    ns = {"np": np, "os": os, "Quaternion": Quaternion, "LidarPointCloud": LidarPointCloud}
    _module_functions({"get_sample_data_ego_pose_P", "get_calibration_P", "get_P_from_Rt", "transform_pc_np"}, ns)
    ref_transform = ns["transform_pc_np"]

    def transform_pc_np(P, pc_np):
        recorded.append((np.array(P), pc_np.shape[1]))
        return ref_transform(P, pc_np)

    ns["transform_pc_np"] = transform_pc_np
    methods = _methods({"get_lidar_pc_intensity_by_token", "lidar_frame_accumulation", "accumulate_lidar_points"}, ns)
    p_cam_pc_code = _p_cam_pc_statements()
    B = len(AVAILABLE)
    lidar_calib = np.stack([np.concatenate([np.round(_quat(-math.pi / 2 + 0.004 + 0.001 * b, 0.003, -0.002), 16), [0.943713, 0.0, 1.84023]]) for b in range(B)])
    cam_calib = np.stack([np.concatenate([np.round(np.roll(Rotation.from_matrix(np.array([[0.0, 0, 1], [-1, 0, 0], [0, -1, 0]])
                                                                              @ Rotation.from_euler("zyx", [0.004, 0.006 + 0.002 * b, -0.003]).as_matrix()).as_quat(), 1), 16),
                                          [1.70079, 0.0159, 1.51095]]) for b in range(B)])
    rows_all, sweep_counts, ego_all, cam_pose = [], [], [], []
    out = dict(P_ego=[], T=[], kept=[], cloud64=[], intensity=[], P_cam_pc=[], P_vehicle_lidar=[], P_ego_cam=[], P_vehicle_cam=[])
    offsets, picks_next, picks_prev = [0], np.zeros((B, FRAME_NUM), np.int32), np.zeros((B, FRAME_NUM), np.int32)
    for b, (n_next, n_prev) in enumerate(AVAILABLE):
        origin = np.array([2100.0 - 100.0 * b, 1650.0 + 170.0 * b, 3.0])
        heading = rng.uniform(0, 2 * math.pi)
        ego = {i: ego_record(rng, origin, heading, 5.0 + i / 20.0) for i in range(-n_prev, n_next + 1)}
        nusc.add_calib("lidar_calib:%d" % b, lidar_calib[b])
        nusc.add_calib("cam_calib:%d" % b, cam_calib[b])
        key = nusc.add_chain("lidar%d" % b, n_prev, n_next, ego, "lidar_calib:%d" % b)
        cam_rec = ego_record(rng, origin, heading, 5.0 + 0.012)
        cam_key = nusc.add_chain("cam%d" % b, 0, 0, {0: cam_rec}, "cam_calib:%d" % b)
        order = [0] + picks(n_next, FRAME_NUM, FRAME_SKIP) + [-d for d in picks(n_prev, FRAME_NUM, FRAME_SKIP)]
        assert len(order) == len(ROWS[b])
        picks_next[b, :len(picks(n_next, FRAME_NUM, FRAME_SKIP))] = picks(n_next, FRAME_NUM, FRAME_SKIP)
        picks_prev[b, :len(picks(n_prev, FRAME_NUM, FRAME_SKIP))] = picks(n_prev, FRAME_NUM, FRAME_SKIP)
        for j, (pos, n) in enumerate(zip(order, ROWS[b])):
            xyz = edge_rows(rng) if n is None else draw_rows(rng, n, (b, j) in INSIDE)
            if (b, j) == (0, 1):          # the edge rows in a transformed sweep too
                e = edge_rows(rng)
                xyz[:len(e)] = e
            full = np.concatenate([xyz, np.rint(rng.uniform(0, 255, (len(xyz), 1))).astype(np.float32),
                                   rng.integers(0, 32, (len(xyz), 1)).astype(np.float32)], 1).astype(np.float32)
            sweeps["lidar%d:%d" % (b, pos)] = full
            rows_all.append(full)
            ego_all.append(ego[pos])
        sweep_counts.append(len(order))
        cam_pose.append(cam_rec)
        # ---- the reference
        self = SimpleNamespace(nusc=nusc, opt=SimpleNamespace(accumulation_frame_num=FRAME_NUM, accumulation_frame_skip=FRAME_SKIP))
        for name, fn in methods.items():
            setattr(self, name, fn.__get__(self))
        lidar = nusc.get("sample_data", key)
        del read[:], recorded[:]
        pc_np, intensity_np = self.accumulate_lidar_points(lidar)
        assert read == ["lidar%d:%d" % (b, pos) for pos in order], (read, order)          # the picks and their order
        assert pc_np.shape[0] == 3 and intensity_np.shape == (1, pc_np.shape[1])
        kept_other = [n for _, n in recorded]
        out["kept"] += [pc_np.shape[1] - sum(kept_other)] + kept_other
        out["T"] += [np.eye(4)] + [P for P, _ in recorded]
        out["cloud64"].append(np.asarray(pc_np, dtype=np.float64).T.copy())
        out["intensity"].append(np.asarray(intensity_np[0], dtype=np.float32).copy())
        offsets.append(offsets[-1] + pc_np.shape[1])
        out["P_ego"] += [ns["get_sample_data_ego_pose_P"](nusc, nusc.get("sample_data", "lidar%d:%d" % (b, pos))) for pos in order]
        g = dict(ns, self=self, lidar=lidar, camera=nusc.get("sample_data", cam_key))
        exec(p_cam_pc_code, g)
        out["P_cam_pc"].append(g["P_cam_pc"])
        out["P_vehicle_lidar"].append(g["lidar_calib_P"])
        out["P_ego_cam"].append(g["camera_pose_P"])
        out["P_vehicle_cam"].append(g["camera_calib_P"])
        assert np.array_equal(g["lidar_pose_P"], out["P_ego"][-len(order)])
    counts = np.diff(offsets)
    assert counts[0] > 2 * N_INPUT and 0 < counts[1] < 2 * N_INPUT and 0 < counts[2] < 2 * N_INPUT and counts[3] == 0, counts
    kept = np.asarray(out["kept"], np.int32)
    so = np.concatenate([[0], np.cumsum([len(r) for r in rows_all])]).astype(np.int32)
    fo = np.concatenate([[0], np.cumsum(sweep_counts)]).astype(np.int32)
    assert kept[6] == 0 and np.all(kept[fo[3]:] == 0) and set(np.diff(so).tolist()) >= {0, 1, 63, 64, 65, 255, 256, 257}
    ego_all = np.stack(ego_all)
    assert 1500.0 < np.abs(ego_all[:, 4:6]).min() and np.abs(ego_all[:, 4:6]).max() < 2500.0
    for P in out["P_ego"] + out["P_vehicle_lidar"] + out["P_ego_cam"] + out["P_vehicle_cam"]:          # float32 values in a float64 matrix
        assert P.dtype == np.float64 and np.array_equal(P, P.astype(np.float32).astype(np.float64))
        assert np.abs(P[:3, :3]).min() > 1e-6          # see the module docstring: "one float32 ulp" means nothing next to zero
    data = dict(frame_num=np.int32(FRAME_NUM), frame_skip=np.int32(FRAME_SKIP), input_pt_num=np.int32(N_INPUT),
                available=np.asarray(AVAILABLE, np.int32), picks_next=picks_next, picks_prev=picks_prev,
                walks=np.asarray(WALKS, np.int32), walk_picks=reference_walks(methods),
                rows=np.concatenate(rows_all), sweep_offsets=so, frame_offsets=fo,
                ego=ego_all, lidar_calib=lidar_calib, cam_pose=np.stack(cam_pose), cam_calib=cam_calib,
                P_ego=np.stack(out["P_ego"]), P_vehicle_lidar=np.stack(out["P_vehicle_lidar"]), P_ego_cam=np.stack(out["P_ego_cam"]),
                P_vehicle_cam=np.stack(out["P_vehicle_cam"]), T=np.stack(out["T"]), P_cam_pc=np.stack(out["P_cam_pc"]),
                cloud64=np.concatenate(out["cloud64"]), intensity=np.concatenate(out["intensity"]), kept=kept,
                offsets=np.asarray(offsets, np.int32))
    path = os.path.join(HERE, "sweeps_golden.npz")
    np.savez_compressed(path, **data)
    print("sweeps_golden.npz written: %d arrays, %d bytes; kept rows per frame %s" % (len(data), os.path.getsize(path), counts.tolist()))


if __name__ == "__main__":
    assert os.path.isdir(REF), "needs the reference checkout"
    main()
