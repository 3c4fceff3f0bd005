#!/usr/bin/env python3
"""The Oxford raw front end on one MI355X, fed by a rendered traversal (deepi2p_amd.world.TraversalPlan): HIP-event times of
TraversalPlan.run eagerly and as a graph replay, of the push-broom render alone (di2p_world_render_profiles, next to di2p_world_render_scan
at the same ray count: the same trace with a pose per profile instead of per frame), and frames/s of submap_pipeline.OxfordFrameExecutor
with the batch resident and with the H2D copy in the step, next to the route without it: submap.OxfordRawPlan.run eagerly, its outputs
brought to the host and submitted to pipeline.RegistrationExecutor.  The two routes are timed alternately in one process; the medians over
--rounds rounds and their spread are reported.
    python tools/bench_oxford_executor.py [--B 32] [--profiles 500] [--beams 541] [--streams 2] [--steps 20] [--warmup 3] [--rounds 3]
                                          [--reps 10] [--render-warmup 3] [--coarse]
The default shapes are 32 sub-maps of 500 profiles x 541 beams and the reference's Oxford options: 960 x 1280 frames, 384 x 640 images,
20480 points, the fine head with the PnP back end (--coarse: the coarse head and the Gauss-Newton back end)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from deepi2p_amd import _lib, sample_prep, submap, synthetic, world  # noqa: E402
from deepi2p_amd.pipeline import RegistrationExecutor  # noqa: E402
from deepi2p_amd.submap_pipeline import OxfordFrameExecutor  # noqa: E402

N, H, W = 20480, 384, 640
NAMES = ("pc", "intensity", "sn", "node_a", "node_b")
K_RAW = np.array([[964.828979, 0.0, 643.788025], [0.0, 964.828979, 484.40799], [0.0, 0.0, 1.0]])          # a Robotcar stereo-centre camera
INPUTS = ("scan_xyr", "scan_offsets", "submap_offsets", "poses", "present", "G_posesource_laser", "G_cam", "image", "K_raw", "P_cam_pc")
SKIP = submap.VOXEL / 16.0


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
    ap.add_argument("--profiles", type=int, default=500)
    ap.add_argument("--beams", type=int, default=541)
    ap.add_argument("--streams", type=int, default=2)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--render-warmup", type=int, default=3)
    ap.add_argument("--coarse", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, S, beams = a.B, a.profiles, a.beams
    H0, W0 = sample_prep.RAW_HW["oxford"]
    rng = np.random.default_rng(0)
    cal = synthetic.make_lms_traversal(rng, 1, 1, 1)
    Gl, Gc = cal["G_posesource_laser"], cal["G_cam"]
    tp = world.TraversalPlan(B, S, beams, H0, W0, dev)
    street = world.make_street(rng, B, 0.2 * S + 20.0)
    tp.set_world(street)
    tp.set_calibration(Gl, Gc)
    tp.set_camera(np.tile(K_RAW, (B, 1, 1)))
    tp.set_traversal(*world.traversal_inputs(world.make_trajectory(rng, B, S), S // 2, S // 2, Gl, Gc))
    # ---- the renders
    stages = {"camera render": "di2p_world_render_camera", "profile render": "di2p_world_render_profiles"}
    per_stage = {k: [] for k in stages}
    for i in range(a.render_warmup + a.reps):
        _lib.TIMED = {n: [] for n in stages.values()}
        tp.run(seed=i)
        torch.cuda.synchronize()
        if i >= a.render_warmup:
            for k, n in stages.items():
                per_stage[k].append(sum(b.elapsed_time(e) for b, e, _ in _lib.TIMED[n]))
        _lib.TIMED = None
    med = {k: float(np.median(v)) for k, v in per_stage.items()}
    eager = _ms(lambda i: tp.run(seed=i), a.reps, a.render_warmup)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        tp.run()

    def one_replay(i):
        tp.seed.fill_(i)
        g.replay()
    replay = _ms(one_replay, a.reps, a.render_warmup)
    # di2p_world_render_scan at the same ray count: B frames of beams x S rays in the same scenes, the sensor at the first laser pose
    wp = world.WorldPlan(B, 4, 4, beams, S, dev)
    wp.set_pattern(world.hdl64_pattern(rng, B, beams, S))
    wp.set_world(street)
    wp.pose.copy_(tp.laser_to_world.view(B, S, 4, 4)[:, 0])
    _lib.TIMED = {"di2p_world_render_scan": []}
    for i in range(a.render_warmup + a.reps):
        wp.run(seed=i)
    torch.cuda.synchronize()
    scan = float(np.median([b.elapsed_time(e) for b, e, _ in _lib.TIMED["di2p_world_render_scan"]][a.render_warmup:]))
    _lib.TIMED = None
    rays, kept = B * S * beams, int(tp.scan_offsets[-1])
    print("%d sub-maps x %d profiles x %d beams = %.2f M rays (%d kept), %d x %d frames, %.1f primitives per scene"
          % (B, S, beams, rays / 1e6, kept, H0, W0, float(np.mean(street[1]))))
    for k, v in med.items():
        print("  %-26s %8.3f ms (eager, per-call events)" % (k, v))
    print("  %-26s %8.3f ms = %.3f ns per ray; di2p_world_render_scan at the same ray count %8.3f ms = %.3f ns per ray: ratio %.2f"
          % ("profile render", med["profile render"], 1e6 * med["profile render"] / rays, scan, 1e6 * scan / rays, med["profile render"] / scan))
    print("  %-26s %8.3f ms (eager)   %8.3f ms (graph replay)" % ("TraversalPlan.run", eager, replay))
    del wp, g
    # ---- the executor and the route without it
    from deepi2p_amd.networks import MMClassifer, MMClassiferCoarse
    opt = synthetic.OptLike(N, H, W, not a.coarse)
    opt.device = dev
    mm = (MMClassiferCoarse if a.coarse else MMClassifer)(opt)
    mm.detector.load_state_dict(synthetic.synthetic_state_dict(opt))
    if a.coarse:
        from deepi2p_amd.registration import RegistrationPipeline
        pipe = RegistrationPipeline(H, W, seed=0)
    else:
        from deepi2p_amd.registration_pnp import PnPPipeline
        pipe = PnPPipeline(H, W, iterations=500, seed=0)
    draws = pipe.draw(B, dev)
    kw = dict(restarts=draws) if a.coarse else dict(samples=draws)
    outs = tp.run(seed=1)
    torch.cuda.synchronize()
    mfp = min(S * beams, submap.MAX_FRAME_POINTS)
    hb = dict(zip(INPUTS, (t.cpu() for t in outs)), seed=1)
    ex = OxfordFrameExecutor(mm, pipe, opt, hb, tp.S_cap, tp.P_cap, tp.P_cap, mfp, n_streams=a.streams, skip_threshold=SKIP, **kw)
    plan = submap.OxfordRawPlan(opt, B, tp.S_cap, tp.P_cap, tp.P_cap, mfp, (H0, W0), "val", skip_threshold=SKIP, device=dev)
    d_in = [t.to(dev) for t in (hb[k] for k in INPUTS)]

    def prepared_host():
        p = plan.run(*d_in, seed=1)
        host = {k: p[j].cpu() for j, k in enumerate(NAMES)}
        host["img"], host["K"] = p[6].cpu(), p[7].cpu()
        return host
    first = prepared_host()
    ref_ex = RegistrationExecutor(mm, pipe, first["K"], first, n_streams=a.streams, **kw)

    def route(steps):
        """OxfordRawPlan.run eagerly on resident inputs, its outputs to the host, RegistrationExecutor.submit: frames/s over `steps` batches"""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tickets = [ref_ex.submit(prepared_host()) for _ in range(steps)]
        for t in tickets:
            ref_ex.result(t)
        torch.cuda.synchronize()
        return B * steps / (time.perf_counter() - t0)
    rates = {"executor, resident": [], "executor, with H2D": [], "plan + RegistrationExecutor": []}
    for r in range(a.rounds + 1):                    # round 0 warms everything up and is dropped
        vals = {"executor, resident": B * a.steps / ex.throughput(a.steps, a.warmup, False)[0],
                "executor, with H2D": B * a.steps / ex.throughput(a.steps, a.warmup, True)[0], "plan + RegistrationExecutor": route(a.steps)}
        if r:
            for k, v in vals.items():
                rates[k].append(v)
    assert ex.use_graph and ref_ex.use_graph, (ex.graph_error, ref_ex.graph_error)
    status = sorted(set(ex.slots[0].prepared[9].cpu().numpy().tolist()))
    res = {k: float(np.median(v)) for k, v in rates.items()}
    for k, v in rates.items():
        print("  %-28s %8.1f frames/s (median of %d rounds; min %.1f, max %.1f)" % (k, res[k], a.rounds, min(v), max(v)))
    print("  status %s" % status)
    print(json.dumps(dict(metric="oxford_executor", B=B, profiles=S, beams=beams, rays=rays, kept_rows=kept, streams=a.streams, coarse=a.coarse,
                          stages_ms=med, render_scan_same_rays_ms=scan, traversal_plan_eager_ms=eager, traversal_plan_replay_ms=replay,
                          frames_per_s=res, spread={k: (min(v), max(v)) for k, v in rates.items()}, status=status)))


if __name__ == "__main__":
    main()
