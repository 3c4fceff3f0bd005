"""BASELINE configs[2] (coarse + fine head + PnP, B = 64, 20480 points, 160 x 512, 500 EPnP RANSAC samples) through the stream / graph
executor in PnP mode, at 1 and 8 streams (GT labels through labels_override: random-init weights predict nothing; the network part --
predict_labels -- runs in full).  Then the fine head's tail alone, old against new, alternating in the same process with device events:
  old  layer 1 (bf16x3 pointwise kernel) + layer 2 (fp32 pointwise kernel, score tensor in HBM) + two argmax_channels
  new  di2p_point_head_labels_x3 (layers 1-2 + both argmaxes, no score tensor)
at B = 64 / KITTI (20480 points, L = 80) and at the configs[3] shard (B = 16, 30000 points, 896 x 1600: L = 1400).
Prints one JSON line.  Per-kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/bench_pnp_executor.py --tail-only`."""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from deepi2p_amd import ops, prep, synthetic  # noqa: E402

NAMES = ("pc", "intensity", "sn", "node_a", "node_b", "img")


def executor_rate(dev, streams, steps, warmup):
    from deepi2p_amd.networks import MMClassifer
    from deepi2p_amd.pipeline import RegistrationExecutor
    from deepi2p_amd.registration import get_P_diff
    from deepi2p_amd.registration_pnp import PnPPipeline
    B, N, H, W = 64, 20480, 160, 512
    opt = synthetic.OptLike(N, H, W, True)
    opt.device = dev
    mm = MMClassifer(opt)
    mm.detector.load_state_dict(synthetic.synthetic_state_dict(opt))
    b = synthetic.make_batch(5, B, N=N, H=H, W=W)
    host = {k: torch.from_numpy(b[k]) for k in NAMES}
    pc = host["pc"].to(dev)
    gt = prep.project_labels(pc, torch.from_numpy(b["P_gt"][:, :3, :]).float().to(dev), torch.from_numpy(b["K"]).float().to(dev), H, W, 32)
    pipe = PnPPipeline(H, W, iterations=500, method="epnp", seed=0)
    ex = RegistrationExecutor(mm, pipe, torch.from_numpy(b["K"]), host, n_streams=streams, labels_override=gt)
    dt, last, lat = ex.throughput(steps, warmup, with_h2d=False)
    P = last["P"].cpu().numpy()
    ok = sum(1 for i in range(B) if (lambda tr: tr[0] < 2.0 and tr[1] < 8.0)(get_P_diff(P[i], b["P_gt"][i])))
    return {"streams": streams, "frames_per_s": round(steps * B / dt, 1), "ms_per_step": round(dt / steps * 1e3, 3),
            "latency_ms_median": round(float(np.median(lat)), 3), "graph": ex.use_graph, "within_2m_8deg": ok, "frames": B}


def tail_times(dev, B, N, L, reps):
    g = torch.Generator().manual_seed(1)
    P = 2 + L
    y0 = torch.relu(torch.randn(B, 256, N, generator=g)).to(dev)
    W1 = (torch.randn(256, 256, generator=g) / 16).to(dev)
    W2 = (torch.randn(256, P, generator=g) / 16).to(dev)
    sc1, sh1, sh2 = (torch.rand(256, generator=g) + 0.5).to(dev), (torch.randn(256, generator=g) * 0.1).to(dev), (torch.randn(P, generator=g) * 0.1).to(dev)
    packed = {"W1p": ops.head_labels_pack(W1), "W2p": ops.head_labels_pack(W2), "P": P, "sc1": sc1, "sh1": sh1, "relu1": True, "sc2": None, "sh2": sh2}

    def old():
        # what KeypointDetector.forward + two argmax_channels launch after layer 0 (_run_pn with the automatic bf16x3 rule)
        y1 = ops.pointwise_gemm([ops.Src(y0)], W1, 256, N, scale=sc1, shift=sh1, relu=True)
        s = ops.pointwise_gemm([ops.Src(y1)], W2, P, N, shift=sh2)
        return ops.argmax_channels(s[:, 0:2]), ops.argmax_channels(s[:, 2:])

    def new():
        return ops.point_head_labels(y0, packed, N)

    for f in (old, new, old, new):
        f()
    torch.cuda.synchronize()
    t = {"old": [], "new": []}
    for _ in range(reps):
        for name, f in (("old", old), ("new", new)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            torch.cuda.synchronize()
            t[name].append(e0.elapsed_time(e1))
    co, fo = old()
    cn, fn = new()
    torch.cuda.synchronize()
    return {"B": B, "N": N, "L": L, "old_ms_median": round(float(np.median(t["old"])), 3), "new_ms_median": round(float(np.median(t["new"])), 3),
            "old_ms_min": round(min(t["old"]), 3), "new_ms_min": round(min(t["new"]), 3),
            "label_agreement": [round(float((co == cn).float().mean()), 6), round(float((fo == fn).float().mean()), 6)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--tail-only", action="store_true", help="only the old-vs-new tail timing (the profiler pass)")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"config": "configs[2] PnP executor", "hw_queues": int(os.environ.get("GPU_MAX_HW_QUEUES", "4"))}
    res["tail"] = [tail_times(dev, 64, 20480, 80, a.reps), tail_times(dev, 16, 30000, 1400, a.reps)]
    if not a.tail_only:
        res["executor"] = [executor_rate(dev, s, a.steps, a.warmup) for s in (1, 8)]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
