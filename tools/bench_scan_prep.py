#!/usr/bin/env python3
"""Raw-scan preparation on one MI355X: per-stage and total ms for a batch of synthetic HDL-64 scans (default 32), from the raw
f32[total,4] batch in HBM to the network input (voxel 0.1 -> normals -> 1-NN intensity -> the loader's 0.3 m pass -> ragged
down-sample -> node sampling), plus, for context, the CPU restatement (tests/scan_prep_oracle.py: numpy + scipy cKDTree) per frame
on one host thread.
    python tools/bench_scan_prep.py [--B 32] [--reps 10] [--warmup 3] [--cpu-frames 2] [--normals {query,cells}] [--alternate]
--normals: the normals kernel (scan_prep.estimate_normals' method): one wave per query point, or one workgroup per grid cell.
--alternate: both kernels in this one process, in turn within every repetition; a line and a JSON line per kernel.
"""
import argparse
import json
import os
import sys
import time

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[_v] = "1"          # the CPU reference runs on one host thread
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from deepi2p_amd import _lib, scan_prep, synthetic  # noqa: E402

STAGES = {"voxel 0.1": ["di2p_voxel_down_sample@0.1"], "normals": ["di2p_estimate_normals", "di2p_estimate_normals_cells"], "1-NN": ["di2p_nearest_raw"],
          "voxel 0.3": ["di2p_voxel_down_sample@0.3"], "down-sample": ["di2p_random_choice_ragged", "di2p_gather_ragged"],
          "nodes": ["di2p_random_choice", "di2p_gather_points", "di2p_farthest_point_sampling"]}


def run(points, offsets, cap, max_frame, plan, seed, method="query"):
    _lib.TIMED_TAG = "0.1"
    st = scan_prep.voxel_down_sample(points, offsets, 0.1, cap=cap)
    normals = scan_prep.estimate_normals(st, 0.6, 30, method=method)
    _, inten, _ = scan_prep.nearest_raw(st, points, offsets)
    rec4 = torch.cat((st.points, inten[:, None]), 1)          # the record, still ragged in HBM (not timed as a stage)
    _lib.TIMED_TAG = "0.3"
    return plan.run(rec4, normals, st.offsets, seed)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-frames", type=int, default=2)
    ap.add_argument("--normals", choices=("query", "cells"), default="query")
    ap.add_argument("--alternate", action="store_true", help="time both normals kernels alternately in this process")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    scans = [synthetic.make_velodyne_scan(np.random.default_rng(100 + i)) for i in range(a.B)]
    points, offsets, host = scan_prep.pack(scans, dev)
    cap, max_frame = int(points.shape[0]), int(np.diff(host).max())
    plan = scan_prep.BatchPlan(a.B, cap, max_frame, 20480, 128, device=dev)
    # --alternate: both normals kernels in ONE process, query / cells in turn within every repetition (same box, same clocks)
    methods = ["query", "cells"] if a.alternate else [a.normals]
    for i in range(a.warmup):
        for m in methods:
            run(points, offsets, cap, max_frame, plan, i, m)
    torch.cuda.synchronize()
    names = sorted({n.split("@")[0] for v in STAGES.values() for n in v})
    totals, per_stage = {m: [] for m in methods}, {m: {k: [] for k in STAGES} for m in methods}
    for i in range(a.reps):
        for m in methods:
            _lib.TIMED = {n: [] for n in names}
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(points, offsets, cap, max_frame, plan, i, m)
            e1.record()
            torch.cuda.synchronize()
            totals[m].append(e0.elapsed_time(e1))
            for stage, keys in STAGES.items():
                ms = 0.0
                for key in keys:
                    name, _, tag = key.partition("@")
                    ms += sum(s.elapsed_time(e) for s, e, t in _lib.TIMED[name] if not tag or t == tag)
                per_stage[m][stage].append(ms)
            _lib.TIMED = None
    scan_prep.check_status(plan.status)
    for m in methods[:-1]:          # the other method of an alternated run: its own lines, then the last method as before
        print("normals %s: normals %.3f ms (min %.3f, max %.3f), total %.3f ms" % (
            m, float(np.median(per_stage[m]["normals"])), min(per_stage[m]["normals"]), max(per_stage[m]["normals"]), float(np.median(totals[m]))))
        print(json.dumps(dict(metric="scan_prep_ms", normals=m, B=a.B, total_ms=float(np.median(totals[m])),
                              stages_ms={k: float(np.median(v)) for k, v in per_stage[m].items()}, normals_ms_all=per_stage[m]["normals"])))
    a.normals = methods[-1]
    med = {k: float(np.median(v)) for k, v in per_stage[a.normals].items()}
    total = float(np.median(totals[a.normals]))
    nrm = per_stage[a.normals]["normals"]
    print("normals %s: normals %.3f ms (min %.3f, max %.3f), total %.3f ms" % (a.normals, med["normals"], min(nrm), max(nrm), total))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import scan_prep_oracle as spo
    cpu = []
    for s in scans[:a.cpu_frames]:
        t = time.perf_counter()
        spo.preprocess_velodyne(s)
        cpu.append((time.perf_counter() - t) * 1e3)
    pts_per_frame = float(np.mean(np.diff(host)))
    print("batch %d scans, %.0f points per scan (total %d), normals: %s" % (a.B, pts_per_frame, cap, a.normals))
    for k, v in med.items():
        print("  %-12s %8.3f ms" % (k, v))
    print("  %-12s %8.3f ms  (%.3f ms per frame; stage sum %.3f)" % ("total", total, total / a.B, sum(med.values())))
    cpu_ms = float(np.mean(cpu)) if cpu else None
    if cpu:
        print("  CPU restatement (numpy + cKDTree, one thread): %.1f ms per frame (voxel + normals + 1-NN only)" % cpu_ms)
    print(json.dumps(dict(metric="scan_prep_ms", normals=a.normals, B=a.B, points_per_scan=pts_per_frame, total_ms=total, per_frame_ms=total / a.B, stages_ms=med,
                          cpu_oracle_ms_per_frame=cpu_ms)))


if __name__ == "__main__":
    main()
