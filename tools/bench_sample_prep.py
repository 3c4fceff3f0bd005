#!/usr/bin/env python3
"""Training-sample preparation on one MI355X: SamplePlan.run (draws -> 0.3 m voxel pass -> jittered down-sample -> node sampling -> image
path) for a batch of records and 370 x 1226 camera frames, as one captured graph (total) and eagerly with per-launch events (stages);
the algorithmic bytes over the total as a fraction of 8 TB/s; and, for context, the numpy oracle's image path per sample on one host thread.
    python tools/bench_sample_prep.py [--B 8] [--reps 10] [--warmup 3] [--cpu-frames 2]
--dataset oxford / nuscenes: the same plan at that loader's own shapes (Oxford 960 x 1280 -> 384 x 640 with the range filter and shuffle,
nuScenes 900 x 1600 -> 160 x 320; 0.2 m voxel pass, intensity jitter), e.g. --dataset oxford --B 32 --points 60000.
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

from deepi2p_amd import _lib, sample_prep, scan_prep, synthetic  # noqa: E402

STAGES = {"draws": ["di2p_sample_draws"], "voxel 0.3": ["di2p_voxel_down_sample"],
          "down-sample + jitter": ["di2p_random_choice_ragged_dseed", "di2p_gather_ragged_aug"],
          "nodes": ["di2p_random_choice_dseed", "di2p_gather_points", "di2p_farthest_point_sampling"], "image": ["di2p_image_prepare"]}
STAGES_DS = {"draws": ["di2p_sample_draws_ds"], "filter + shuffle": ["di2p_range_shuffle"], "voxel 0.2": ["di2p_voxel_down_sample"],
             "down-sample + jitter": ["di2p_random_choice_ragged_dseed", "di2p_gather_ragged_aug_intensity"], "nodes": STAGES["nodes"],
             "image": ["di2p_image_prepare_ds"]}
K_RAW = np.array([[718.856, 0.0, 607.1928], [0.0, 718.856, 185.2157], [0.0, 0.0, 1.0]])
PC = np.array([[0, -1, 0, 0], [0, 0, -1, -0.05], [1, 0, 0, -0.3], [0, 0, 0, 1]], dtype=np.float64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-frames", type=int, default=2)
    ap.add_argument("--points", type=int, default=60000, help="points per record (above 2 * 20480: the voxel pass runs)")
    ap.add_argument("--dataset", choices=sorted(sample_prep.DATASETS), default="kitti")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, rng = a.B, np.random.default_rng(0)
    stages = STAGES if a.dataset == "kitti" else STAGES_DS
    recs = []
    for i in range(B):
        if a.dataset == "oxford":
            recs.append(synthetic.make_oxford_submap(np.random.default_rng(100 + i), a.points).T)
            continue
        s = synthetic.make_velodyne_scan(np.random.default_rng(100 + i))[:a.points]
        sn = rng.standard_normal((s.shape[0], 3)).astype(np.float32)
        recs.append(np.concatenate([s.T, sn.T], 0) if a.dataset == "kitti" else s)
    H0, W0 = sample_prep.RAW_HW[a.dataset]
    one = [synthetic.make_camera_image(np.random.default_rng(200 + i), H0, W0) for i in range(min(B, 4))]
    raw = np.stack([one[i % len(one)] for i in range(B)])
    if a.dataset == "kitti":
        points, normals, offsets, host = scan_prep.pack_records(recs, dev)
    else:
        (points, offsets, host), normals = scan_prep.pack(recs, dev), None
    images = torch.from_numpy(raw).to(dev)
    K, Pc = [torch.from_numpy(np.tile(m, (B, 1, 1))).to(dev) for m in (K_RAW, PC)]
    opt = SimpleNamespace()
    plan = sample_prep.SamplePlan(opt, B, points.shape[0], int(np.diff(host).max()), raw.shape[1:3], "train", dev, dataset=a.dataset)
    args = (points, normals, offsets, images, K, Pc, None)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for i in range(a.warmup):
            plan.run(*args, seed=i)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        plan.run(*args, seed=None)
    totals = []
    for i in range(a.warmup + a.reps):
        plan.seed.fill_(i)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        if i >= a.warmup:
            totals.append(e0.elapsed_time(e1))
    names = sorted({n for v in stages.values() for n in v})
    per_stage = {k: [] for k in stages}
    for i in range(a.reps):
        _lib.TIMED = {n: [] for n in names}
        plan.run(*args, seed=i)
        torch.cuda.synchronize()
        for stage, keys in stages.items():
            per_stage[stage].append(sum(s.elapsed_time(e) for k in keys for s, e, _ in _lib.TIMED[k]))
        _lib.TIMED = None
    scan_prep.check_status(plan.status[:B])
    med = {k: float(np.median(v)) for k, v in per_stage.items()}
    total = float(np.median(totals))
    H, W, n = plan.optb.img_H, plan.optb.img_W, plan.points.n
    nbytes = raw.size + 12 * B * H * W + int(points.shape[0]) * 28 + B * n * 28
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from tests import sample_prep_oracle as spo
    ints, fac = plan.table.ints.cpu().numpy(), plan.table.factors.cpu().numpy()
    cpu = []
    for b in range(min(a.cpu_frames, B) if a.dataset == "kitti" else 0):
        t = time.perf_counter()
        spo.prepare_image(raw[b], 50, 0.5, H, W, ints[b], fac[b])
        cpu.append((time.perf_counter() - t) * 1e3)
    print("%s, batch %d: %d x %d images, %.0f points per record" % (a.dataset, B, raw.shape[1], raw.shape[2], float(np.mean(np.diff(host)))))
    for k, v in med.items():
        print("  %-22s %8.3f ms (eager, per-launch events)" % (k, v))
    print("  %-22s %8.3f ms (graph replay; %.3f ms per sample; %.1f MB algorithmic = %.2f %% of 8 TB/s)"
          % ("total", total, total / B, nbytes / 1e6, 100.0 * nbytes / (total * 1e-3) / 8e12))
    cpu_ms = float(np.mean(cpu)) if cpu else None
    if cpu:
        print("  numpy oracle, image path only, one thread: %.1f ms per sample" % cpu_ms)
    print(json.dumps(dict(metric="sample_prep_ms", dataset=a.dataset, B=B, total_ms=total, per_sample_ms=total / B, stages_ms=med, algorithmic_bytes=nbytes,
                          fraction_of_8TBs=nbytes / (total * 1e-3) / 8e12, cpu_oracle_image_ms_per_sample=cpu_ms)))


if __name__ == "__main__":
    main()
