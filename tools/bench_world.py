#!/usr/bin/env python3
"""Synthetic worlds on one MI355X (deepi2p_amd.world): HIP-event times per batch of the camera render (di2p_world_render_camera, 32 x 370 x 1226)
and of the scan (di2p_world_render_scan, 32 x 64 x 1800, four launches), of WorldPlan.run eagerly and as a graph replay, and the host numpy
time of tests/world_oracle.py for ONE frame (context only).  The camera kernel against its bounds: fp64 operations counted from the scene
(rays x primitives x operations per hit test, from world.hip's code: box 20, cylinder 23, ground 3, each division and square root counted
as one) over the fp64 vector peak, and the bytes it stores over the HBM peak.
    python tools/bench_world.py [--B 32] [--H0 370] [--W0 1226] [--beams 64] [--azimuths 1800] [--reps 10] [--warmup 3] [--no-graph] [--no-host]
"""
import argparse
import json
import os
import sys
import time

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[_v] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from deepi2p_amd import _lib, world  # noqa: E402

K_RAW = np.array([[718.856, 0.0, 607.1928], [0.0, 718.856, 185.2157], [0.0, 0.0, 1.0]])          # a KITTI odometry camera
PC = np.array([[0.0, -1, 0, 0.06], [0, 0, -1, -0.08], [1, 0, 0, -0.27], [0, 0, 0, 1]])
OPS = {world.GROUND: 3, world.BOX: 20, world.CYLINDER: 23}          # fp64 operations of one hit test + 2 for the nearest-hit select
FP64_PEAK, HBM_PEAK = 78.6e12, 8e12
STAGES = {"camera render": "di2p_world_render_camera", "scan": "di2p_world_render_scan"}


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
    ap.add_argument("--H0", type=int, default=370)
    ap.add_argument("--W0", type=int, default=1226)
    ap.add_argument("--beams", type=int, default=64)
    ap.add_argument("--azimuths", type=int, default=1800)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    B = a.B
    rng = np.random.default_rng(0)
    pattern = world.hdl64_pattern(rng, B, a.beams, a.azimuths)
    w = world.make_world(rng, B)
    K, Pc = np.tile(K_RAW, (B, 1, 1)), np.tile(PC, (B, 1, 1))
    plan = world.WorldPlan(B, a.H0, a.W0, a.beams, a.azimuths, dev)
    plan.set_pattern(pattern)
    plan.run(w, K, Pc, seed=0)
    per_stage = {k: [] for k in STAGES}
    for i in range(a.warmup + a.reps):
        _lib.TIMED = {n: [] for n in STAGES.values()}
        plan.run(seed=i)
        torch.cuda.synchronize()
        if i >= a.warmup:
            for k, n in STAGES.items():
                per_stage[k].append(sum(b.elapsed_time(e) for b, e, _ in _lib.TIMED[n]))
        _lib.TIMED = None
    med = {k: float(np.median(v)) for k, v in per_stage.items()}
    eager = _ms(lambda i: plan.run(seed=i), a.reps, a.warmup)
    replay = None
    if not a.no_graph:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            plan.run()

        def one_replay(i):
            plan.seed.fill_(i)
            g.replay()
        replay = _ms(one_replay, a.reps, a.warmup)
    kept = int(plan.offsets[-1])
    pixels, rays = B * a.H0 * a.W0, B * a.beams * a.azimuths
    per_ray = [sum(OPS[int(k)] + 2 for k in w[0][b, :w[1][b], 0]) for b in range(B)]
    cam_flop = float(sum(per_ray)) * a.H0 * a.W0
    cam_bytes = 3 * pixels
    bound = max(cam_flop / FP64_PEAK, cam_bytes / HBM_PEAK) * 1e3
    host = None
    if not a.no_host:
        from tests import world_oracle as wo
        M = world.camera_pose(Pc)
        t0 = time.perf_counter()
        wo.render_camera(w[0][0], int(w[1][0]), K[0], M[0], a.H0, a.W0)
        host_cam = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        wo.render_scan(w[0][0], int(w[1][0]), pattern[0], pattern[1][0], 0, 0)
        host = dict(camera_ms=host_cam, scan_ms=(time.perf_counter() - t0) * 1e3)
    print("%d frames: %d x %d pixels = %.1f M camera rays, %d x %d = %.2f M LiDAR rays (%d kept), %.1f primitives per frame"
          % (B, a.H0, a.W0, pixels / 1e6, a.beams, a.azimuths, rays / 1e6, kept, float(np.mean(w[1]))))
    for k, v in med.items():
        print("  %-22s %8.3f ms (eager, per-call events)" % (k, v))
    cam = med["camera render"]
    print("  camera: %.2e fp64 operations of hit tests = %.2f TFLOP/s = %.1f %% of the %.1f TF fp64 vector peak; %.1f MB stored = %.1f GB/s; bound %.3f ms (%s)"
          % (cam_flop, cam_flop / cam / 1e9, 100.0 * cam_flop / (cam * 1e-3) / FP64_PEAK, FP64_PEAK / 1e12, cam_bytes / 1e6, cam_bytes / cam / 1e6, bound,
             "operations" if cam_flop / FP64_PEAK > cam_bytes / HBM_PEAK else "bytes"))
    print("  %-22s %8.3f ms (eager)" % ("WorldPlan.run", eager))
    if replay is not None:
        print("  %-22s %8.3f ms (graph replay)" % ("WorldPlan.run", replay))
    if host is not None:
        print("  tests/world_oracle.py, ONE frame: camera %.1f ms, scan %.1f ms (numpy, one thread; context only)" % (host["camera_ms"], host["scan_ms"]))
    print(json.dumps(dict(metric="world_ms", B=B, H0=a.H0, W0=a.W0, beams=a.beams, azimuths=a.azimuths, stages_ms=med, camera_flop=cam_flop,
                          camera_bytes=cam_bytes, camera_bound_ms=bound, kept_rows=kept, world_plan_eager_ms=eager, world_plan_replay_ms=replay,
                          host_oracle_one_frame_ms=host)))


if __name__ == "__main__":
    main()
