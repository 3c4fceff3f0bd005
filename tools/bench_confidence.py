#!/usr/bin/env python3
"""What the confidence stage costs a step of the executor, and whether its measures separate good poses from bad ones, at the configuration
bench.py times (BASELINE configs[1]: 32 frames of 20480 points, 160 x 512 images, 60 restarts, synthetic labels into the solver, 8 streams,
one captured graph per slot, inputs resident):

    python tools/bench_confidence.py [--steps 48] [--warmup 8] [--repeats 2] [--parent DIR] [--calib-batches 4] [--flips 0.05,0.2,0.35]

Every measurement runs in a fresh child process, one after the other: the executor with confidence off and with confidence on from this
tree, and -- with --parent DIR, a built checkout of the parent commit -- the same step from THAT tree, `--repeats` times each, interleaved,
so that the run-to-run spread is there to compare the difference with.  Prints one line per run and one JSON line: milliseconds per step
(wall time of `steps` submits between two synchronisations, over steps) and the spread per variant.

Calibration (--calib-batches > 0): synthetic scenes (synthetic.make_batch: exact frustum labels with a share `flip` of them flipped, the
ground-truth pose known) through an executor with evaluate=True and confidence=True, `--calib-batches` batches per flip rate.  Prints the
success rate (rte < 2 m and rre < 5 degrees, evaluation mode's flag) per flip rate, per bin of agree / finite, per quartile of sigma_t and
per quartile of gap / cost, and puts the table into a second JSON line.  The frames of all flip rates are pooled: a measure is useful when
the rate rises with agree / finite and falls with sigma_t.
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
B, N, H, W, R, STREAMS = 32, 20480, 160, 512, 60, 8
NAMES = ("pc", "intensity", "sn", "node_a", "node_b", "img")
AGREE_BINS = (0.0, 0.02, 0.04, 0.07, 0.1, 0.25, 1.0)      # (lo, hi] but for the first, which takes 0 too; of 60 restarts: 1 | 2 | 3-4 | 5-6 | 7-15 | 16+


def _executor(root, n_streams, **kw):
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
    if kw.get("evaluate"):
        host["P"] = torch.from_numpy(batch["P_gt"])
    pipe = RegistrationPipeline(H, W, R=R, seed=0)
    labels = torch.from_numpy(batch["labels"]).to(dev)
    ex = RegistrationExecutor(mm, pipe, torch.from_numpy(batch["K"]).to(dev), host, n_streams=n_streams, restarts=pipe.draw(B, dev),
                              labels_override=labels, **kw)
    return ex, labels, host


def child_time(root, confidence, steps, warmup):
    ex, _, _ = _executor(root, STREAMS, **({"confidence": True} if confidence else {}))      # the keyword does not exist on the parent commit
    dt, out, _ = ex.throughput(steps, warmup, False)
    res = dict(ms_per_step=dt / steps * 1e3, frames_per_s=B * steps / dt, graph=bool(ex.use_graph))
    if confidence:
        res.update(cov_ok=int((out["cov_status"] == 0).sum()), agree_mean=float(out["agree"].double().mean()))
    print("RESULT " + json.dumps(res), flush=True)


def _rate(ok, sel):
    n = int(sel.sum())
    return dict(frames=n, success_rate=(float(ok[sel].mean()) if n else None))


def child_calibrate(root, batches, flips):
    import numpy as np
    import torch
    ex, labels, host = _executor(root, 1, evaluate=True, confidence=True)
    from deepi2p_amd import synthetic
    keys = ("flags", "agree", "finite", "sigma_t", "sigma_r", "cov_status", "gap", "cost", "rte", "rre")
    rows = {k: [] for k in keys}
    frame_flip = []
    seed = 2000
    for flip in flips:
        for _ in range(batches):
            b = synthetic.make_batch(seed, B, N=N, H=H, W=W, flip=flip)
            seed += 1
            labels.copy_(torch.from_numpy(b["labels"]))          # the graph reads the override where it lies
            hb = {k: torch.from_numpy(b[k]) for k in NAMES}
            hb["P"], hb["K"] = torch.from_numpy(b["P_gt"]), torch.from_numpy(b["K"])
            out = ex.result(ex.submit(hb))
            for k in keys:
                rows[k].append(out[k].cpu().numpy())
            frame_flip += [flip] * B
    assert ex.use_graph, ex.graph_error
    v = {k: np.concatenate(rows[k]) for k in keys}
    ok = (v["flags"] & 2) != 0
    share = v["agree"] / np.maximum(v["finite"], 1)
    table = dict(frames=int(ok.size), success_rate=float(ok.mean()), flips=list(flips), cov_status_counts=np.bincount(v["cov_status"], minlength=3).tolist(),
                 by_flip=[], by_agree_share=[], by_sigma_t=[], by_gap=[])
    frame_flip = np.asarray(frame_flip)
    for flip in flips:
        table["by_flip"].append(dict(bin="flip %.2f" % flip, **_rate(ok, frame_flip == flip)))
    for lo, hi in zip(AGREE_BINS[:-1], AGREE_BINS[1:]):
        sel = (share > lo) & (share <= hi) if lo > 0 else (share <= hi)
        table["by_agree_share"].append(dict(bin="(%.2f, %.2f]" % (lo, hi) if lo > 0 else "[0, %.2f]" % hi, **_rate(ok, sel)))
    good = v["cov_status"] == 0
    if good.any():
        q = np.quantile(v["sigma_t"][good], [0.25, 0.5, 0.75])
        edges = [-np.inf] + list(q) + [np.inf]
        for i in range(4):
            sel = good & (v["sigma_t"] > edges[i]) & (v["sigma_t"] <= edges[i + 1])
            table["by_sigma_t"].append(dict(bin="quartile %d (sigma_t <= %.4g)" % (i + 1, edges[i + 1]), **_rate(ok, sel)))
    table["by_sigma_t"].append(dict(bin="cov_status != 0", **_rate(ok, ~good)))
    rel = v["gap"] / v["cost"]                                   # the gap as a share of the winning cost
    fin = np.isfinite(rel)
    if fin.any():
        q = np.quantile(rel[fin], [0.25, 0.5, 0.75])
        edges = [-np.inf] + list(q) + [np.inf]
        for i in range(4):
            sel = fin & (rel > edges[i]) & (rel <= edges[i + 1])
            table["by_gap"].append(dict(bin="quartile %d (gap / cost <= %.4g)" % (i + 1, edges[i + 1]), **_rate(ok, sel)))
    table["by_gap"].append(dict(bin="all agree (gap = inf)", **_rate(ok, np.isinf(v["gap"]))))
    print("RESULT " + json.dumps(table), flush=True)


def run_child(args, timeout=900):
    cmd = [sys.executable, os.path.abspath(__file__)] + args
    out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout)
    for line in out.stdout.splitlines():
        if line.startswith("RESULT "):
            return json.loads(line[7:])
    raise SystemExit("child %s failed (%d):\n%s" % (cmd, out.returncode, out.stdout[-4000:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: its step is timed too")
    ap.add_argument("--calib-batches", type=int, default=4, help="batches of 32 frames per flip rate for the calibration table (0: none)")
    ap.add_argument("--flips", default="0.05,0.2,0.35", help="label flip rates of the calibration scenes")
    ap.add_argument("--child", choices=("on", "off", "calib"), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--root", default=os.path.dirname(HERE), help=argparse.SUPPRESS)
    a = ap.parse_args()
    flips = [float(x) for x in a.flips.split(",") if x]
    if a.child == "calib":
        child_calibrate(a.root, a.calib_batches, flips)
        return
    if a.child:
        child_time(a.root, a.child == "on", a.steps, a.warmup)
        return
    variants = ([("parent", os.path.abspath(a.parent), False)] if a.parent else []) + \
               [("this tree, confidence off", a.root, False), ("this tree, confidence on", a.root, True)]
    runs = {name: [] for name, _, _ in variants}
    for rep in range(a.repeats):
        for name, root, confidence in variants:
            r = run_child(["--child", "on" if confidence else "off", "--root", root, "--steps", str(a.steps), "--warmup", str(a.warmup)])
            assert r["graph"], "the step was not captured"
            runs[name].append(r["ms_per_step"])
            print("%-27s run %d: %8.3f ms per step (%7.1f frames/s)" % (name, rep, r["ms_per_step"], r["frames_per_s"]), flush=True)
    if a.repeats > 0:
        print(json.dumps(dict(metric="confidence_step_ms", config=dict(B=B, N=N, H=H, W=W, R=R, streams=STREAMS, steps=a.steps, warmup=a.warmup),
                              ms_per_step=runs, spread_ms={k: max(v) - min(v) for k, v in runs.items()})))
    if a.calib_batches > 0:
        t = run_child(["--child", "calib", "--root", a.root, "--calib-batches", str(a.calib_batches), "--flips", a.flips])
        print("calibration: %d frames, success rate %.3f, cov_status counts %s" % (t["frames"], t["success_rate"], t["cov_status_counts"]))
        for key, title in (("by_flip", "labels"), ("by_agree_share", "agree / finite"), ("by_sigma_t", "sigma_t"), ("by_gap", "gap")):
            for row in t[key]:
                rate = "   -  " if row["success_rate"] is None else "%6.3f" % row["success_rate"]
                print("  %-14s %-34s %4d frames, success rate %s" % (title, row["bin"], row["frames"], rate))
        print(json.dumps(dict(metric="confidence_calibration", config=dict(B=B, N=N, H=H, W=W, R=R), table=t)))


if __name__ == "__main__":
    main()
