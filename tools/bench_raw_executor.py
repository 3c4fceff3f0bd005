#!/usr/bin/env python3
"""Frames/s of raw_pipeline.RawFrameExecutor (raw scans + camera frames in, poses out) next to pipeline.RegistrationExecutor on the
SAME frames already prepared, on one MI355X, at the shapes of BASELINE config 2 (B = 64 frames, 20480 points, 160 x 512 images).
Both executors copy their inputs host -> device in every step.  The two are timed alternately in one process (wall time of --steps steps
between two full synchronisations: RegistrationExecutor.throughput); the medians over --rounds rounds are reported.
    python tools/bench_raw_executor.py [--B 64] [--streams 3] [--steps 6] [--warmup 3] [--rounds 10] [--normals cells] [--pnp]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from deepi2p_amd import raw_prep, scan_prep, synthetic  # noqa: E402
from deepi2p_amd.pipeline import RegistrationExecutor  # noqa: E402
from deepi2p_amd.raw_pipeline import RawFrameExecutor  # noqa: E402

N, H, W = 20480, 160, 512
NAMES = ("pc", "intensity", "sn", "node_a", "node_b", "img")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--streams", type=int, default=3)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--distinct", type=int, default=8, help="distinct synthetic scans (repeated over the batch)")
    ap.add_argument("--normals", choices=("query", "cells"), default="cells")
    ap.add_argument("--pnp", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    from deepi2p_amd.networks import MMClassifer, MMClassiferCoarse
    opt = synthetic.OptLike(N, H, W, a.pnp)
    opt.device = dev
    mm = (MMClassifer if a.pnp else MMClassiferCoarse)(opt)
    mm.detector.load_state_dict(synthetic.synthetic_state_dict(opt))
    if a.pnp:
        from deepi2p_amd.registration_pnp import PnPPipeline
        pipe = PnPPipeline(H, W, iterations=500, seed=0)
    else:
        from deepi2p_amd.registration import RegistrationPipeline
        pipe = RegistrationPipeline(H, W, seed=0)
    draws = pipe.draw(a.B, dev)
    kw = dict(samples=draws) if a.pnp else dict(restarts=draws)
    base = [synthetic.make_velodyne_scan(np.random.default_rng(100 + i)) for i in range(a.distinct)]
    scans = [base[b % a.distinct] for b in range(a.B)]
    image = torch.from_numpy(np.stack([synthetic.make_camera_image(np.random.default_rng(b % a.distinct)) for b in range(a.B)]))
    K_raw = np.tile(np.array([[718.856, 0, 607.1928], [0, 718.856, 185.2157], [0, 0, 1]]), (a.B, 1, 1))
    Pc = np.tile(np.array([[0, -1, 0, 0], [0, 0, -1, 0], [1, 0, 0, 0], [0, 0, 0, 1]], np.float64), (a.B, 1, 1))       # velodyne -> camera axes
    hb = dict(scans=scans, image=image, K_raw=torch.from_numpy(K_raw), Pc=torch.from_numpy(Pc), seed=1)
    total, mfp = sum(len(s) for s in scans), max(len(s) for s in scans)
    raw_ex = RawFrameExecutor(mm, pipe, opt, hb, total, mfp, n_streams=a.streams, normals_method=a.normals, **kw)
    plan = raw_prep.RawFramePlan(opt, a.B, total, mfp, tuple(image.shape[1:3]), "val", "kitti", a.normals, dev)
    points, offsets, _ = scan_prep.pack(scans, dev)
    prepared = plan.run(points, offsets, image.to(dev), torch.from_numpy(K_raw).to(dev), torch.from_numpy(Pc).to(dev), seed=1)
    host = {k: prepared[j].cpu() for j, k in enumerate(NAMES[:5])}
    host["img"] = prepared[6].cpu()
    ref_ex = RegistrationExecutor(mm, pipe, prepared[7].cpu(), host, n_streams=a.streams, **kw)
    del plan, points
    rates = {"raw": [], "prepared": []}
    for r in range(a.rounds + 1):                    # round 0 warms both up and is dropped
        for name, ex in (("raw", raw_ex), ("prepared", ref_ex)):
            dt, _, _ = ex.throughput(a.steps, a.warmup, True)
            if r:
                rates[name].append(a.B * a.steps / dt)
    assert raw_ex.use_graph and ref_ex.use_graph, (raw_ex.graph_error, ref_ex.graph_error)
    med = {k: float(np.median(v)) for k, v in rates.items()}
    spread = {k: (float(np.min(v)), float(np.max(v))) for k, v in rates.items()}
    for k in rates:
        print("%-9s %8.1f frames/s (median of %d rounds; min %.1f, max %.1f)" % (k, med[k], a.rounds, spread[k][0], spread[k][1]))
    print(json.dumps(dict(metric="raw_executor_frames_per_s", B=a.B, streams=a.streams, normals=a.normals, pnp=a.pnp, raw=med["raw"],
                          prepared=med["prepared"], ratio=med["raw"] / med["prepared"], raw_points_per_frame=total / a.B)))


if __name__ == "__main__":
    main()
