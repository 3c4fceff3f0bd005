#!/usr/bin/env python3
"""What evaluation mode costs a step of the executor, at the configuration bench.py times (BASELINE configs[1]: 32 frames of 20480 points,
160 x 512 images, 60 restarts, synthetic labels into the solver, 8 streams, one captured graph per slot, inputs resident):

    python tools/bench_evaluation.py [--steps 48] [--warmup 8] [--repeats 2] [--parent DIR]

Every measurement runs in a fresh child process, one after the other: the executor with evaluate off and with evaluate on from this tree,
and -- with --parent DIR, a built checkout of the parent commit -- the same step with evaluate off from THAT tree, `--repeats` times each,
interleaved, so that the parent's own run-to-run spread is there to compare the difference with.  Prints one line per run and one JSON
line: milliseconds per step (wall time of `steps` submits between two synchronisations, over steps) and the spread per variant.
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
B, N, H, W, R, STREAMS = 32, 20480, 160, 512, 60, 8
NAMES = ("pc", "intensity", "sn", "node_a", "node_b", "img")


def child(root, evaluate, steps, warmup):
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
    kw = {}
    if evaluate:                      # the keyword does not exist on the parent commit
        kw["evaluate"] = True
        host["P"] = torch.from_numpy(batch["P_gt"])
    ex = RegistrationExecutor(mm, pipe, torch.from_numpy(batch["K"]).to(dev), host, n_streams=STREAMS, restarts=pipe.draw(B, dev),
                              labels_override=torch.from_numpy(batch["labels"]).to(dev), **kw)
    dt, out, _ = ex.throughput(steps, warmup, False)
    res = dict(ms_per_step=dt / steps * 1e3, frames_per_s=B * steps / dt, graph=bool(ex.use_graph))
    if evaluate:
        s = ex.eval_state().summary()
        res.update(frames_evaluated=s["n"], line=ex.eval_state().line())
    print("RESULT " + json.dumps(res), flush=True)


def run_child(root, evaluate, steps, warmup):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "on" if evaluate else "off", "--root", root, "--steps", str(steps),
           "--warmup", str(warmup)]
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
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: its evaluate-off step is timed too")
    ap.add_argument("--child", choices=("on", "off"), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--root", default=os.path.dirname(HERE), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.root, a.child == "on", a.steps, a.warmup)
        return
    variants = ([("parent, evaluate off", os.path.abspath(a.parent), False)] if a.parent else []) + \
               [("this tree, evaluate off", a.root, False), ("this tree, evaluate on", a.root, True)]
    runs = {name: [] for name, _, _ in variants}
    for rep in range(a.repeats):
        for name, root, evaluate in variants:
            r = run_child(root, evaluate, a.steps, a.warmup)
            assert r["graph"], "the step was not captured"
            runs[name].append(r["ms_per_step"])
            print("%-26s run %d: %8.3f ms per step (%7.1f frames/s)%s" % (name, rep, r["ms_per_step"], r["frames_per_s"],
                                                                          "   " + r["line"] if evaluate else ""), flush=True)
    print(json.dumps(dict(metric="evaluation_step_ms", config=dict(B=B, N=N, H=H, W=W, R=R, streams=STREAMS, steps=a.steps, warmup=a.warmup),
                          ms_per_step=runs, spread_ms={k: max(v) - min(v) for k, v in runs.items()})))


if __name__ == "__main__":
    main()
