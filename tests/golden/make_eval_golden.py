"""Generates tests/golden/eval_golden.npz from the REFERENCE's own evaluation functions (run where the reference checkout exists):

    python tests/golden/make_eval_golden.py

`get_P_diff` and `enu2cam` (with `transform_pc_np`, which it calls) are extracted from evaluation/registration_lsq.py with `ast` at
generation time, the way make_golden.py takes its functions, and run in fp64 on 67 seeded pairs of rigid transforms.  The file holds arrays
only:

  P_pred, P_gt f64[67,4,4]     the pairs; gt_is3[i] marks the pairs whose ground truth went to the reference as a 3-row matrix and got its
                               fourth row the way registration_lsq.py:298-300 appends it
  cost f64[67]                 some entries 0 and 1e-7 (invalid under registration_result_analysis.py:22), the rest >= 1e-3
  rte, rre                     get_P_diff(P_pred, P_gt)
  rte_enu, rre_enu             get_P_diff(P_pred P_convert^-1, enu2cam(., P_gt)[1]): both poses taken into the converted frame
  pc, pc_enu2cam               a few points and enu2cam's image of them
  <frame>_{n_valid, rte_mean, rte_sigma, rre_mean, rre_sigma, success_rate, rte_hist, rre_hist, rte_over, rre_over}
                               registration_result_analysis.py:22-47,59,63 restated (the script body cannot be executed: it uses the
                               removed np.float and reads files): np.mean, sqrt(np.var), np.histogram(range=..., bins=60) over the
                               frames with cost > 1e-6, for frame in ("cam", "enu")

Pairs: five fixed ones (identity against identity; translation only; pure yaw of 179.9 and of -179.9 degrees; a pair 1 cm / 0.01 degree
apart), then 62 drawn ones.  Every rotation is an Euler triple 'xzy' whose middle (z) angle lies within +-80 degrees; P_gt has a
translation of up to 20 m per axis, and P_pred = P_gt D^-1 for a drawn difference D of one of three sizes (small: a success; medium:
inside the histogram ranges; large: up to 20 m and any x / y angle).  67 is not a multiple of 64.

The draw is repeated with the next seed until, in BOTH frames: the middle angle of the measured difference is within +-80 degrees; no
rte is within 1e-6 of 2 m and no rre within 1e-6 of 5 degrees; no rte or rre is within 1e-6 of a histogram bin edge (the edge at 0 apart:
the errors are not negative, and the identity pair sits on it by construction); the valid frames hold at least one success, one failure and one value in each overflow bucket.  Flags and bins are then defined without a tolerance.
"""
import ast
import os
import sys

import numpy as np
from scipy.spatial.transform import Rotation

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle import ref_network as rn  # noqa: E402

N_PAIRS, N_FIXED = 67, 5
BINS, RTE_RANGE, RRE_RANGE = 60, 15.0, 30.0
T_THRESH, R_THRESH = 2.0, 5.0
INVALID = {3: 0.0, 10: 1e-7, 20: 0.0, 33: 1e-7, 47: 0.0, 60: 1e-7, 66: 0.0}


def reference_functions():
    path = os.path.join(rn.REF, "evaluation", "registration_lsq.py")
    ns = {"np": np, "Rotation": Rotation}
    for node in ast.parse(open(path).read()).body:
        if isinstance(node, ast.FunctionDef) and node.name in ("get_P_diff", "enu2cam", "transform_pc_np"):
            exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), ns)
    return ns["get_P_diff"], ns["enu2cam"]


def rigid(angles_xzy_deg, t):
    P = np.identity(4)
    P[:3, :3] = Rotation.from_euler("xzy", angles_xzy_deg, degrees=True).as_matrix()
    P[:3, 3] = t
    return P


def draw(seed):
    rng = np.random.default_rng(seed)
    P_pred, P_gt = np.zeros((N_PAIRS, 4, 4)), np.zeros((N_PAIRS, 4, 4))
    eye = np.identity(4)
    fixed = [(eye, eye),
             (rigid([0, 0, 0], [0.5, -0.25, 1.0]), rigid([0, 0, 0], [-1.5, 0.75, 3.1])),
             (eye, rigid([0, 0, 179.9], [0, 0, 0])),
             (eye, rigid([0, 0, -179.9], [0, 0, 0])),
             (rigid([10, 20, 30], [1, 2, 3]), rigid([10.004, 20.003, 30.003], [1.006, 2.006, 3.005]))]
    for i, (a, b) in enumerate(fixed):
        P_pred[i], P_gt[i] = a, b
    for i in range(N_FIXED, N_PAIRS):
        size = (i - N_FIXED) % 3
        t_amp, xy_amp, z_amp = [(0.9, 1.5, 1.5), (7.0, 9.0, 9.0), (20.0, 180.0, 80.0)][size]
        D = rigid([rng.uniform(-xy_amp, xy_amp), rng.uniform(-z_amp, z_amp), rng.uniform(-xy_amp, xy_amp)], rng.uniform(-t_amp, t_amp, 3))
        P_gt[i] = rigid([rng.uniform(-180, 180), rng.uniform(-80, 80), rng.uniform(-180, 180)], rng.uniform(-20, 20, 3))
        P_pred[i] = P_gt[i] @ np.linalg.inv(D)
    cost = rng.uniform(1e-3, 50.0, N_PAIRS)
    for i, v in INVALID.items():
        cost[i] = v
    gt_is3 = (np.arange(N_PAIRS) % 3 == 1)
    pc = rng.uniform(-30, 30, (3, 16))
    return P_pred, P_gt, cost, gt_is3, pc


def away(v, marks, eps=1e-6):
    return np.all(np.abs(np.asarray(v)[:, None] - np.asarray(marks)[None, :]) > eps)


def statistics(rte, rre, cost):
    valid = cost > 1e-6                                                        # registration_result_analysis.py:22
    t, r = rte[valid], rre[valid]
    success = np.logical_and(t < T_THRESH, r < R_THRESH)                       # :37
    return dict(n_valid=np.int64(valid.sum()), rte_mean=np.mean(t), rte_sigma=np.sqrt(np.var(t)), rre_mean=np.mean(r),
                rre_sigma=np.sqrt(np.var(r)), success_rate=np.mean(success.astype(np.float64)), n_success=np.int64(success.sum()),
                rte_hist=np.histogram(t, range=[0, RTE_RANGE], bins=BINS)[0].astype(np.int64),      # :59
                rre_hist=np.histogram(r, range=[0, RRE_RANGE], bins=BINS)[0].astype(np.int64),      # :63
                rte_over=np.int64((t > RTE_RANGE).sum()), rre_over=np.int64((r > RRE_RANGE).sum()))


def main():
    get_P_diff, enu2cam = reference_functions()
    P_convert_inv = np.linalg.inv(np.asarray([[1, 0, 0, 0], [0, 0, -1, 0], [0, 1, 0, 0], [0, 0, 0, 1]], dtype=np.float64))
    for seed in range(2024, 2124):
        P_pred, P_gt, cost, gt_is3, pc = draw(seed)
        out = {k: np.zeros(N_PAIRS) for k in ("rte", "rre", "rte_enu", "rre_enu")}
        middle = []
        for i in range(N_PAIRS):
            gt = P_gt[i]
            if gt_is3[i]:
                gt = gt[:3]
                gt = np.concatenate((gt, np.identity(4)[3:4, :]), axis=0)      # registration_lsq.py:298-300
            out["rte"][i], out["rre"][i] = get_P_diff(P_pred[i], gt)
            _, gt_cam = enu2cam(pc, gt)
            pred_cam = np.dot(P_pred[i], P_convert_inv)                        # the pose of the converted points
            out["rte_enu"][i], out["rre_enu"][i] = get_P_diff(pred_cam, gt_cam)
            for a, b in ((P_pred[i], gt), (pred_cam, gt_cam)):
                D = np.dot(np.linalg.inv(a), b)
                middle.append(abs(Rotation.from_matrix(D[:3, :3]).as_euler("xzy", degrees=True)[1]))
        ok = max(middle) <= 80.0
        stats = {}
        for frame, suffix in (("cam", ""), ("enu", "_enu")):
            t, r = out["rte" + suffix], out["rre" + suffix]
            ok = ok and away(t, [T_THRESH]) and away(r, [R_THRESH])
            ok = ok and away(t, np.linspace(0, RTE_RANGE, BINS + 1)[1:]) and away(r, np.linspace(0, RRE_RANGE, BINS + 1)[1:])
            s = statistics(t, r, cost)
            ok = ok and 0 < s["n_success"] < s["n_valid"] and s["rte_over"] > 0 and s["rre_over"] > 0
            stats.update({"%s_%s" % (frame, k): v for k, v in s.items()})
        if ok:
            break
    else:
        raise SystemExit("no seed met the conditions")
    pc_cam, _ = enu2cam(pc, np.identity(4))
    path = os.path.join(HERE, "eval_golden.npz")
    np.savez(path, P_pred=P_pred, P_gt=P_gt, cost=cost, gt_is3=gt_is3, pc=pc, pc_enu2cam=pc_cam, seed=np.int64(seed), **out, **stats)
    print("eval_golden.npz written: seed %d, valid %d, successes %d / %d (cam / enu), overflow rte %d rre %d, largest middle angle %.2f deg"
          % (seed, stats["cam_n_valid"], stats["cam_n_success"], stats["enu_n_success"], stats["cam_rte_over"], stats["cam_rre_over"],
             max(middle)))


if __name__ == "__main__":
    main()
