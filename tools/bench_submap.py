#!/usr/bin/env python3
"""Oxford sub-map building on one MI355X (deepi2p_amd.submap): HIP-event times of stages A-C (di2p_submap_build: keep rule, counts and
offsets, transform and write), of the 0.1 m voxel pass, of the camera transform, and of OxfordRawPlan.run (LMS profiles + camera frames ->
the Oxford loader's sample) eagerly and as a graph replay; and the bytes per second of stages A-C against their compulsory traffic, 24 B in +
16 B out per surviving row + 128 B of pose per kept profile.
    python tools/bench_submap.py [--B 8] [--scans 1800] [--rows 541] [--reps 10] [--warmup 3] [--no-graph]
The default shape is 8 sub-maps x 1800 profiles x 541 rows (974 k rows each, under the 2^20 limit of a sub-map).
"""
import argparse
import json
import os
import sys
from types import SimpleNamespace

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[_v] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from deepi2p_amd import _lib, sample_prep, submap, synthetic  # noqa: E402

K_RAW = np.array([[964.828979, 0.0, 643.788025], [0.0, 964.828979, 484.407990], [0.0, 0.0, 1.0]])
STAGES = {"A-C keep / count / write": "di2p_submap_build", "D voxel 0.1": "di2p_voxel_down_sample", "E camera frame": "di2p_submap_to_camera"}


def _ms(fn, reps, warmup):
    out = []
    for i in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(i)
        e1.record()
        torch.cuda.synchronize()
        if i >= warmup:
            out.append(e0.elapsed_time(e1))
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--scans", type=int, default=1800)
    ap.add_argument("--rows", type=int, default=541)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-graph", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    B = a.B
    trav = synthetic.make_lms_traversal(np.random.default_rng(0), B, a.scans, a.rows)
    xyr, scan_off, sub_off, poses, present = submap.pack_scans(trav["submaps"], dev)
    S, P = int(poses.shape[0]), int(xyr.shape[0])
    Gl = torch.from_numpy(trav["G_posesource_laser"]).to(dev)
    Gc = torch.from_numpy(np.tile(trav["G_cam"], (B, 1, 1))).to(dev)
    H0, W0 = sample_prep.RAW_HW["oxford"]
    one = [synthetic.make_camera_image(np.random.default_rng(200 + i), H0, W0) for i in range(min(B, 2))]
    images = torch.from_numpy(np.stack([one[i % len(one)] for i in range(B)])).to(dev)
    K = torch.from_numpy(np.tile(K_RAW, (B, 1, 1))).to(dev)
    Pcp = torch.from_numpy(np.tile(np.eye(4), (B, 1, 1))).to(dev)
    plan = submap.OxfordRawPlan(SimpleNamespace(), B, S, P, P, submap.MAX_FRAME_POINTS, (H0, W0), "train", skip_threshold=submap.VOXEL / 16.0, device=dev)
    sub_args = (xyr, scan_off, sub_off, poses, present, Gl, Gc)
    args = sub_args + (images, K, Pcp)
    per_stage = {k: [] for k in STAGES}
    for i in range(a.warmup + a.reps):
        _lib.TIMED = {n: [] for n in STAGES.values()}
        plan.submap.run(*sub_args)
        torch.cuda.synchronize()
        if i >= a.warmup:
            for k, n in STAGES.items():
                per_stage[k].append(sum(s.elapsed_time(e) for s, e, _ in _lib.TIMED[n]))
        _lib.TIMED = None
    med = {k: float(np.median(v)) for k, v in per_stage.items()}
    status = plan.submap.status[:B].cpu().numpy()
    kept = plan.submap.kept[:S].cpu().numpy()
    raw_rows = int(plan.submap.raw_off[-1])
    rec_rows = int(plan.submap.v_off[-1])
    nbytes = 40 * raw_rows + 128 * int(np.sum(kept == 1))
    eager = _ms(lambda i: plan.run(*args, seed=i), a.reps, a.warmup)
    submap.check_status(plan.status[:B])
    replay = None
    if not a.no_graph:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            plan.run(*args, seed=None)

        def one_replay(i):
            plan.seed.fill_(i)
            g.replay()
        replay = _ms(one_replay, a.reps, a.warmup)
        submap.check_status(plan.status[:B])
    print("%d sub-maps x %d profiles x up to %d rows: %d rows read, %d profiles kept / %d skipped / %d missing, %d surviving rows, %d record rows, status %s"
          % (B, a.scans, a.rows, P, int(np.sum(kept == 1)), int(np.sum(kept == 0)), int(np.sum(kept == -1)), raw_rows, rec_rows, status.tolist()))
    for k, v in med.items():
        print("  %-26s %8.3f ms (eager, per-call events)" % (k, v))
    ac = med["A-C keep / count / write"]
    print("  stages A-C: %.1f MB compulsory traffic = %.1f GB/s = %.2f %% of 8 TB/s" % (nbytes / 1e6, nbytes / (ac * 1e-3) / 1e9, 100.0 * nbytes / (ac * 1e-3) / 8e12))
    print("  %-26s %8.3f ms (eager; %.3f ms per sub-map)" % ("OxfordRawPlan.run", eager, eager / B))
    if replay is not None:
        print("  %-26s %8.3f ms (graph replay; %.3f ms per sub-map)" % ("OxfordRawPlan.run", replay, replay / B))
    print(json.dumps(dict(metric="submap_ms", B=B, scans=a.scans, rows=a.rows, rows_read=P, surviving_rows=raw_rows, record_rows=rec_rows, stages_ms=med,
                          stage_ac_bytes=nbytes, stage_ac_bytes_per_s=nbytes / (ac * 1e-3), oxford_raw_plan_eager_ms=eager,
                          oxford_raw_plan_replay_ms=replay)))


if __name__ == "__main__":
    main()
