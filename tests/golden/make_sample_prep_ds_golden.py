"""Generates tests/golden/sample_prep_ds_golden.npz (arrays only):   python tests/golden/make_sample_prep_ds_golden.py

From the reference's own functions, extracted with ``ast`` at generation time as tests/golden/make_golden.py does (no reference text is
stored): camera_matrix_cropping / camera_matrix_scaling in each loader's crop / scale / crop order, angles2rotation_matrix, and
OxfordLoader / nuScenesLoader.generate_random_transform under a ``random`` that replays a recorded sequence, with both loaders' option
values (train) and their val_random_Ry calls; P = P_cam_pc . inv(Pr) as the loaders assemble it (Pr is float32 there)."""
import ast
import math
import os
import random as pyrandom
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import ref_network as rn  # noqa: E402

REF = rn.REF


class _Replay:
    """random.uniform from a recorded sequence of unit uniforms"""

    def __init__(self, unit):
        self.unit, self.k = list(unit), 0

    def uniform(self, a, b):
        v = a + (b - a) * self.unit[self.k]
        self.k += 1
        return v


def _functions(path, names, ns):
    for node in ast.parse(open(path).read()).body:
        if isinstance(node, ast.FunctionDef) and node.name in names:
            exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), ns)


def _method(path, cls, name, ns):
    for node in ast.parse(open(path).read()).body:
        if isinstance(node, ast.ClassDef) and node.name == cls:
            for sub in node.body:
                if isinstance(sub, ast.FunctionDef) and sub.name == name:
                    g = dict(ns)
                    exec(compile(ast.Module(body=[sub], type_ignores=[]), path, "exec"), g)
                    return g
    raise KeyError(name)


def main():
    rng = np.random.default_rng(2025)
    ns = {"np": np, "math": math}
    _functions(os.path.join(REF, "data", "kitti_helper.py"), {"camera_matrix_cropping", "camera_matrix_scaling"}, ns)
    _functions(os.path.join(REF, "data", "augmentation.py"), {"angles2rotation_matrix"}, ns)
    crop, scale = ns["camera_matrix_cropping"], ns["camera_matrix_scaling"]
    from types import SimpleNamespace
    ns["augmentation"] = SimpleNamespace(angles2rotation_matrix=ns["angles2rotation_matrix"])
    out = {}
    # K': Oxford scales, then crops the window (the bottom crop does not touch K); nuScenes crops the top rows, scales, crops the window
    K_ox = np.asarray([[964.828979, 0, 643.788025], [0, 964.828979, 484.407990], [0, 0, 1]], dtype=np.float32)
    K_nu = np.asarray([[1266.417203046554, 0.0, 816.2670197447984], [0.0, 1266.417203046554, 491.50706579294757], [0.0, 0.0, 1.0]]).astype(np.float32)
    win_ox = np.array([[0, 0], [0, 96], [0, 48], [0, 17], [8, 5]], dtype=np.int64)          # (dx, dy); 640-wide windows leave dx = 0
    win_nu = np.array([[0, 0], [0, 0], [3, 1], [1, 2], [4, 0]], dtype=np.int64)
    out["ox_K_raw"], out["ox_scale"], out["ox_windows"] = K_ox, np.float64(0.5), win_ox
    out["ox_K_out"] = np.stack([crop(scale(K_ox, 0.5), dx=int(w[0]), dy=int(w[1])) for w in win_ox])
    out["nu_K_raw"], out["nu_scale"], out["nu_top"], out["nu_windows"] = K_nu, np.float64(0.2), np.int64(100), win_nu
    out["nu_K_out"] = np.stack([crop(scale(crop(K_nu, dx=0, dy=100), 0.2), dx=int(w[0]), dy=int(w[1])) for w in win_nu])
    # Pr and P
    amps = {"ox": (10.0, 5.0, 10.0, 0.0, 2.0 * math.pi, 0.0), "nu": (0.0, 0.0, 0.0, 0.0, 0.0, 2.0 * math.pi),
            "ox_val": (0, 0, 0, 0, math.pi * 2, 0), "nu_val": (0, 0, 0, 0, 0, math.pi * 2)}
    loaders = {"ox": ("oxford_pc_img_pose_loader.py", "OxfordLoader"), "nu": ("nuscenes_pc_img_pose_loader.py", "nuScenesLoader")}
    for name, amp in amps.items():
        fname, cls = loaders[name[:2]]
        units, Prs, Ps, Pcs = [], [], [], []
        for _ in range(4):
            unit = rng.random(6)
            g = _method(os.path.join(REF, "data", fname), cls, "generate_random_transform", dict(ns, random=_Replay(unit)))
            Pr = g["generate_random_transform"](None, *amp)
            Pcp = np.identity(4)
            Pcp[:3, :3] = ns["angles2rotation_matrix"](rng.uniform(-0.1, 0.1, 3))
            Pcp[:3, 3] = rng.uniform(-6, 6, 3)
            Pcp = Pcp.astype(np.float32)          # the loaders' poses are float32 arrays
            units.append(unit); Prs.append(Pr); Pcs.append(Pcp); Ps.append(np.dot(Pcp, np.linalg.inv(Pr)))
        out[name + "_amp"], out[name + "_unit"] = np.array(amp, dtype=np.float64), np.stack(units)
        out[name + "_Pr"], out[name + "_P_cam_pc"], out[name + "_P"] = np.stack(Prs), np.stack(Pcs), np.stack(Ps)
    path = os.path.join(HERE, "sample_prep_ds_golden.npz")
    np.savez_compressed(path, **out)
    print("sample_prep_ds_golden.npz written: %d arrays, %d bytes" % (len(out), os.path.getsize(path)))


if __name__ == "__main__":
    assert os.path.isdir(REF), "needs the reference checkout"
    main()
