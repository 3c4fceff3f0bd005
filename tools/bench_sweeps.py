#!/usr/bin/env python3
"""nuScenes sweep accumulation on one MI355X (deepi2p_amd.sweeps): HIP-event times of the eager stages (di2p_pose_matrices,
di2p_sweep_transforms, di2p_sweep_accumulate), of NuScenesRawPlan.run (raw sweeps + records + camera frames -> the nuScenes loader's sample)
eagerly and as a graph replay, the host numpy time of tests/sweeps_oracle.py for the same batch (context only), and the bytes per second of
di2p_sweep_accumulate against its algorithmic traffic: 4 * cols B in per row read, 16 B out per surviving row, 128 B of T per sweep.
    python tools/bench_sweeps.py [--B 32] [--sweeps 7] [--rows 34720] [--cols 5] [--reps 10] [--warmup 3] [--no-graph] [--no-host]
The default shape is the reference's: 32 frames x 7 sweeps (accumulation_frame_num 3 on both sides) x 34 720 rows.
"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[_v] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from deepi2p_amd import _lib, sample_prep, sweeps, synthetic  # noqa: E402

K_RAW = np.array([[1266.417203, 0.0, 816.2670197], [0.0, 1266.417203, 491.5070657], [0.0, 0.0, 1.0]])
STAGES = {"pose matrices (4 calls)": "di2p_pose_matrices", "sweep transforms": "di2p_sweep_transforms", "accumulate": "di2p_sweep_accumulate"}


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
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--sweeps", type=int, default=7)
    ap.add_argument("--rows", type=int, default=34720)
    ap.add_argument("--cols", type=int, default=5, choices=(4, 5))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    B = a.B
    s = synthetic.make_nuscenes_sweeps(np.random.default_rng(0), B, a.sweeps, a.rows)
    frames = s["frames"] if a.cols == 5 else [[np.ascontiguousarray(x[:, :4]) for x in f] for f in s["frames"]]
    rows, sweep_off, frame_off = sweeps.pack_sweeps(frames, dev)
    S, P = int(sweep_off.shape[0]) - 1, int(rows.shape[0])
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    recs = (t(np.concatenate(s["ego"])), t(s["lidar_calib"]), t(s["cam_pose"]), t(s["cam_calib"]))
    H0, W0 = sample_prep.RAW_HW["nuscenes"]
    one = [synthetic.make_camera_image(np.random.default_rng(200 + i), H0, W0) for i in range(min(B, 2))]
    images = torch.from_numpy(np.stack([one[i % len(one)] for i in range(B)])).to(dev)
    K = torch.from_numpy(np.tile(K_RAW, (B, 1, 1))).to(dev)
    per_frame = a.sweeps * a.rows
    plan = sweeps.NuScenesRawPlan(SimpleNamespace(), B, S, P, P, min(per_frame, sweeps.MAX_FRAME_POINTS), (H0, W0), "train", cols=a.cols, device=dev)
    sweep_args = (rows, sweep_off, frame_off) + recs
    args = sweep_args + (images, K)
    per_stage = {k: [] for k in STAGES}
    for i in range(a.warmup + a.reps):
        _lib.TIMED = {n: [] for n in STAGES.values()}
        plan.sweeps.run(*sweep_args)
        torch.cuda.synchronize()
        if i >= a.warmup:
            for k, n in STAGES.items():
                per_stage[k].append(sum(b.elapsed_time(e) for b, e, _ in _lib.TIMED[n]))
        _lib.TIMED = None
    med = {k: float(np.median(v)) for k, v in per_stage.items()}
    status = plan.sweeps.status[:B].cpu().numpy()
    kept_rows = int(plan.sweeps.offsets[-1])
    nbytes = 4 * a.cols * P + 16 * kept_rows + 128 * S
    eager = _ms(lambda i: plan.run(*args, seed=i), a.reps, a.warmup)
    sweeps.check_status(plan.status[:B])
    replay = None
    if not a.no_graph:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            plan.run(*args, seed=None)

        def one_replay(i):
            plan.seed.fill_(i)
            g.replay()
        replay = _ms(one_replay, a.reps, a.warmup)
        sweeps.check_status(plan.status[:B])
    host = None
    if not a.no_host:
        from tests import sweeps_oracle as swo
        h_rows, so, fo = rows.cpu().numpy(), sweep_off.cpu().numpy(), frame_off.cpu().numpy()
        t0 = time.perf_counter()
        Pm = [swo.pose_matrices(r.cpu().numpy()) for r in recs]
        T, _ = swo.sweep_transforms(Pm[0], fo, Pm[1], Pm[2], Pm[3])
        acc = swo.accumulate(h_rows, so, fo, T)
        host = (time.perf_counter() - t0) * 1e3
        assert int(acc["offsets"][-1]) == kept_rows
    print("%d frames x %d sweeps x %d rows (%d columns): %d rows read, %d surviving rows, status %s"
          % (B, a.sweeps, a.rows, a.cols, P, kept_rows, sorted(set(status.tolist()))))
    for k, v in med.items():
        print("  %-26s %8.3f ms (eager, per-call events)" % (k, v))
    acc_ms = med["accumulate"]
    rate = nbytes / (acc_ms * 1e-3)
    print("  accumulate: %.1f MB algorithmic traffic = %.1f GB/s = %.2f %% of the 8 TB/s HBM peak" % (nbytes / 1e6, rate / 1e9, 100.0 * rate / 8e12))
    print("  %-26s %8.3f ms (eager; %.3f ms per frame)" % ("NuScenesRawPlan.run", eager, eager / B))
    if replay is not None:
        print("  %-26s %8.3f ms (graph replay; %.3f ms per frame)" % ("NuScenesRawPlan.run", replay, replay / B))
    if host is not None:
        print("  %-26s %8.3f ms (numpy, one thread; context only)" % ("tests/sweeps_oracle.py", host))
    print(json.dumps(dict(metric="sweeps_ms", B=B, sweeps=a.sweeps, rows=a.rows, cols=a.cols, rows_read=P, surviving_rows=kept_rows, stages_ms=med,
                          accumulate_bytes=nbytes, accumulate_bytes_per_s=rate, nuscenes_raw_plan_eager_ms=eager, nuscenes_raw_plan_replay_ms=replay,
                          host_oracle_ms=host)))


if __name__ == "__main__":
    main()
