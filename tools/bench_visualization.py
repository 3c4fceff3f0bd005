#!/usr/bin/env python3
"""What the result overlays cost, at the configuration bench.py times (BASELINE configs[1]: 32 frames of 20480 points, 160 x 512 images,
60 restarts, synthetic labels into the solver, 8 streams, one captured graph per slot, inputs resident):

    python tools/bench_visualization.py [--steps 48] [--warmup 8] [--repeats 2] [--parent DIR]

1. Per-overlay device time: each of the three eager calls (clear + stamp + compose, whole batch) between two device events, 20 warm-up
   calls, then `--overlay-repeats` timed batches of 20 calls; median, minimum and maximum of the per-call time in microseconds, next to the
   bytes the three kernels move at least (keys written, read and atomically updated; image read; canvas written).
2. The executor's step: visualize off, "registration", and -- under evaluate=True, which "both" needs -- off and "both"; with --parent DIR (a
   built checkout of the parent commit) the parent's plain step too.  Every measurement runs in a fresh child process, one after the other,
   `--repeats` times each, interleaved, so that the run-to-run spread is there to compare the differences with.  Milliseconds per step:
   wall time of `steps` submits between two synchronisations, over steps.

Prints one line per run and one JSON line."""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
B, N, H, W, R, STREAMS = 32, 20480, 160, 512, 60, 8
NAMES = ("pc", "intensity", "sn", "node_a", "node_b", "img")
# (name, evaluate, visualize)
STEPS = [("evaluate off, visualize off", False, None), ("evaluate off, registration", False, "registration"),
         ("evaluate on, visualize off", True, None), ("evaluate on, both", True, "both")]


def overlay_bytes(n_points):
    """the least the three launches of one overlay move: keys cleared, five atomics per point at most, keys read, image read, canvas written"""
    pixels = B * (H + 200) * (W + 200)
    return 4 * pixels + 5 * 4 * B * n_points + 4 * pixels + 3 * B * H * W * 4 + 3 * pixels


def child_overlays(root, repeats):
    sys.path.insert(0, root)
    import torch
    from deepi2p_amd import prep, synthetic, visualization
    dev = torch.device("cuda", 0)
    b = synthetic.make_batch(1000, B, N=N, H=H, W=W)
    pc, img, labels = (torch.from_numpy(b[k]).to(dev) for k in ("pc", "img", "labels"))
    P64, K64 = torch.from_numpy(b["P_gt"]).to(dev), torch.from_numpy(b["K"]).to(dev).double()
    if K64.dim() == 2:
        K64 = K64.unsqueeze(0).expand(B, 3, 3).contiguous()
    gt = prep.project_labels(pc, P64.float(), K64.float(), H, W, 32, want_pxpy=True)
    pred = labels.to(torch.int32).contiguous()
    fine_pred = torch.roll(gt[1], 1, dims=1).contiguous()
    canvas, ws = visualization.buffers(B, H, W, dev)
    calls = {"registration": lambda: visualization.registration_overlay_into(pc, P64, K64, pred, img, canvas, ws),
             "classification_coarse": lambda: visualization.classification_overlay_coarse_into(gt[2], pred, gt[0], img, canvas, ws),
             "classification_fine": lambda: visualization.classification_overlay_into(gt[2], pred, gt[0], fine_pred, gt[1], img, canvas, ws)}
    res = {}
    for name, fn in calls.items():
        for _ in range(20):
            fn()
        torch.cuda.synchronize(dev)
        us = []
        for _ in range(repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                fn()
            e1.record()
            e1.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3 / 20)
        res[name] = dict(median_us=statistics.median(us), min_us=min(us), max_us=max(us), painted_pixels=int((canvas != 255).any(-1).sum()))
    print("RESULT " + json.dumps(res), flush=True)


def child_step(root, evaluate, visualize, steps, warmup):
    sys.path.insert(0, root)
    import torch
    from deepi2p_amd import synthetic
    from deepi2p_amd.networks import MMClassiferCoarse
    from deepi2p_amd.pipeline import RegistrationExecutor
    from deepi2p_amd.registration import RegistrationPipeline
    dev = torch.device("cuda", 0)
    opt = synthetic.OptLike(N, H, W, False)
    opt.device = dev
    mm = MMClassiferCoarse(opt)
    mm.detector.load_state_dict(synthetic.synthetic_state_dict(opt))
    batch = synthetic.make_batch(1000, B, N=N, H=H, W=W)
    host = {k: torch.from_numpy(batch[k]).pin_memory() for k in NAMES}
    pipe = RegistrationPipeline(H, W, R=R, seed=0)
    kw = {}                           # the keywords do not exist on the parent commit
    if evaluate:
        kw["evaluate"] = True
        host["P"] = torch.from_numpy(batch["P_gt"])
    if visualize:
        kw["visualize"] = visualize
    ex = RegistrationExecutor(mm, pipe, torch.from_numpy(batch["K"]).to(dev), host, n_streams=STREAMS, restarts=pipe.draw(B, dev),
                              labels_override=torch.from_numpy(batch["labels"]).to(dev), **kw)
    dt, out, _ = ex.throughput(steps, warmup, False)
    print("RESULT " + json.dumps(dict(ms_per_step=dt / steps * 1e3, frames_per_s=B * steps / dt, graph=bool(ex.use_graph))), flush=True)


def run_child(args):
    cmd = [sys.executable, os.path.abspath(__file__)] + [str(a) for a in args]
    out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    for line in out.stdout.splitlines():
        if line.startswith("RESULT "):
            return json.loads(line[7:])
    raise SystemExit("child %s failed (%d):\n%s" % (cmd, out.returncode, out.stdout[-4000:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--overlay-repeats", type=int, default=9)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: its plain step is timed too")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--root", default=os.path.dirname(HERE), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child == "overlays":
        child_overlays(a.root, a.overlay_repeats)
        return
    if a.child is not None:
        _, evaluate, visualize = STEPS[int(a.child)]
        child_step(a.root, evaluate, visualize, a.steps, a.warmup)
        return
    overlays = run_child(["--child", "overlays", "--root", a.root, "--overlay-repeats", a.overlay_repeats])
    for name, r in overlays.items():
        r["min_bytes"] = overlay_bytes(N)
        print("%-24s %8.1f us per call (min %.1f, max %.1f over %d batches of 20), %d painted pixels, at least %.1f MB moved"
              % (name, r["median_us"], r["min_us"], r["max_us"], a.overlay_repeats, r["painted_pixels"], r["min_bytes"] / 1e6), flush=True)
    variants = ([("parent, plain step", os.path.abspath(a.parent), 0)] if a.parent else []) + [(name, a.root, i) for i, (name, _, _) in enumerate(STEPS)]
    runs = {name: [] for name, _, _ in variants}
    for rep in range(a.repeats):
        for name, root, i in variants:
            r = run_child(["--child", i, "--root", root, "--steps", a.steps, "--warmup", a.warmup])
            assert r["graph"], "the step was not captured"
            runs[name].append(r["ms_per_step"])
            print("%-30s run %d: %8.3f ms per step (%7.1f frames/s)" % (name, rep, r["ms_per_step"], r["frames_per_s"]), flush=True)
    print(json.dumps(dict(metric="visualization_cost", config=dict(B=B, N=N, H=H, W=W, R=R, streams=STREAMS, steps=a.steps, warmup=a.warmup),
                          overlays_us=overlays, ms_per_step=runs, spread_ms={k: max(v) - min(v) for k, v in runs.items()})))


if __name__ == "__main__":
    main()
