#!/usr/bin/env python3
"""Map localisation on one MI355X: HIP-event times of the index build (map_index.MapIndex.build) and of the crop (map_index.CropPlan.run,
eager and as a graph replay) at M = 2^22 and 2^24 map rows, B = 32 priors, r = 50 m, 8 m cells, next to what a user without the index would
run on the device: B passes of scan_prep.range_shuffle (the Oxford loader's range filter) over the WHOLE map, the map cut into frames of
2^20 rows because that is the filter's limit per frame.  Then frames/s of map_pipeline.MapFrameExecutor next to
submap_pipeline.OxfordFrameExecutor at the same B and N, timed alternately in one process.
--normals adds, at both sizes, map_index.estimate_normals (radius 0.6, max_nn 30) next to scan_prep.estimate_normals(method="cells") on the
same rows cut into frames of 2^20 (it loses the neighbours across the cuts: context, not a target), and the crop that carries normals
(CropPlan(want_normals=True)) next to the plain crop.  --dataset kitti adds MapFrameExecutor(dataset="kitti") with the KITTI model (20480
points, 160 x 512 images from 370 x 1226 frames) on the same map with normals.
    python tools/bench_map.py [--B 32] [--radius 50] [--cell 8] [--sizes 22 24] [--reps 20] [--warmup 3] [--streams 2] [--steps 20]
                              [--rounds 3] [--no-executor] [--coarse] [--normals] [--dataset kitti]
The street (synthetic.make_map) is as long as it takes for a 50 m disc to hold about 2^18 of the map's rows: 1.6 km at 2^22, 6.4 km at 2^24.
Bytes: the rows of the window cells a crop visits x 16, counted on the host from cell_start; the count and the write pass each read them."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from deepi2p_amd import map_index, sample_prep, scan_prep, submap, synthetic, world  # noqa: E402

N, H, W = 20480, 384, 640
K_RAW = np.array([[964.828979, 0.0, 643.788025], [0.0, 964.828979, 484.40799], [0.0, 0.0, 1.0]])
HBM_PEAK = 8.0e12          # bytes/s, the MI355X's specified peak
FILTER_FRAME = 1 << 20     # rows of one frame of di2p_range_shuffle


def _ms(fn, reps, warmup):
    out = []
    for i in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if i >= warmup:
            out.append(e0.elapsed_time(e1))
    return float(np.median(out)), float(min(out)), float(max(out))


def priors_along(world_map, B, rng):
    """B priors: poses of the street moved by up to 2 m and turned by up to 0.1 rad"""
    picks = rng.integers(0, len(world_map["poses"]), B)
    T = world_map["poses"][picks].copy()
    for b in range(B):
        D = np.eye(4)
        D[:3, :3] = synthetic.ry_matrix(float(rng.uniform(-0.1, 0.1)))
        D[0, 3], D[2, 3] = rng.uniform(-2.0, 2.0, 2)
        T[b] = T[b] @ D
    return T


def window_rows(index, T, radius):
    """rows of the window cells of every frame, from cell_start on the host"""
    cs = index.cell_start.cpu().numpy().astype(np.int64)
    a, b = map_index.ground_axes(index.up_axis)
    total = 0
    for P in T:
        lo = [int(max(0, np.floor((P[k, 3] - radius - o) / index.cell))) for k, o in ((a, index.origin[0]), (b, index.origin[1]))]
        hi = [int(min(n - 1, np.floor((P[k, 3] + radius - o) / index.cell))) for k, o, n in ((a, index.origin[0], index.nx), (b, index.origin[1], index.ny))]
        for iy in range(lo[1], hi[1] + 1):          # the cells of one window row are one span of `sorted`
            total += cs[iy * index.nx + hi[0] + 1] - cs[iy * index.nx + lo[0]]
    return int(total)


def bench_size(log2m, a, dev):
    M, B = 1 << log2m, a.B
    rng = np.random.default_rng(log2m)
    length = 2.0 * a.radius * M / float(1 << 18)
    wm = synthetic.make_map(rng, M, length=length, poses=64)
    pts = torch.from_numpy(wm["points"]).to(dev)
    build = _ms(lambda: map_index.MapIndex.build(pts, a.cell, up_axis=1), max(a.reps // 4, 3), 1)
    index = map_index.MapIndex.build(pts, a.cell, up_axis=1)
    Th = priors_along(wm, B, rng)
    T = torch.from_numpy(Th).to(dev)
    r = torch.full((B,), float(a.radius), dtype=torch.float64, device=dev)
    mfp = map_index.MAX_FRAME_POINTS
    plan = map_index.CropPlan(index, B, B * (1 << 19), mfp, a.radius)
    eager = _ms(lambda: plan.run(T, r), a.reps, a.warmup)
    status = plan.status.cpu().numpy()
    kept = int(plan.offsets[-1])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        plan.run(T, r)
    replay = _ms(g.replay, a.reps, a.warmup)
    visited = window_rows(index, Th, a.radius)
    # the route without the index: the loader's filter over the whole map, once per prior
    frames = M // FILTER_FRAME
    off = torch.arange(0, frames + 1, dtype=torch.int32, device=dev) * FILTER_FRAME
    ws = scan_prep.workspace(frames, M, dev)
    out = (torch.zeros((M, 4), dtype=torch.float32, device=dev), torch.zeros((frames + 1,), dtype=torch.int32, device=dev),
           torch.zeros((frames,), dtype=torch.int32, device=dev))

    def passes():
        for _ in range(B):
            scan_prep.range_shuffle(pts, off, a.radius, max_frame_points=FILTER_FRAME, cap=M, out=out, ws=ws)
    whole = _ms(passes, max(a.reps // 4, 3), 1)
    res = dict(M=M, B=B, radius=a.radius, cell=a.cell, street_m=length, grid=(index.nx, index.ny), max_cells=plan.max_cells, kept_rows=kept,
               status=sorted(set(status.tolist())), window_rows=visited, build_ms=build, crop_eager_ms=eager, crop_replay_ms=replay,
               window_bytes_per_s=16.0 * visited / (replay[0] * 1e-3), share_of_hbm_peak=16.0 * visited / (replay[0] * 1e-3) / HBM_PEAK,
               whole_map_passes_ms=whole, whole_map_over_crop=whole[0] / replay[0])
    print("M = 2^%d rows, street %.0f m, grid %d x %d, B = %d, r = %.0f m: %d rows kept (status %s), window cells hold %.2f M rows"
          % (log2m, length, index.nx, index.ny, B, a.radius, kept, res["status"], visited / 1e6))
    print("  build                       %9.3f ms (min %.3f, max %.3f)" % build)
    print("  crop, eager                 %9.3f ms (min %.3f, max %.3f)" % eager)
    print("  crop, graph replay          %9.3f ms (min %.3f, max %.3f) = %.2f TB/s of window-cell rows read once (%.1f %% of 8 TB/s; both passes read them)"
          % (replay + (res["window_bytes_per_s"] / 1e12, 100 * res["share_of_hbm_peak"])))
    print("  %d whole-map filter passes  %9.3f ms (min %.3f, max %.3f) = %.1f x the crop" % ((B,) + whole + (res["whole_map_over_crop"],)))
    if a.normals or a.dataset == "kitti":
        del out, ws
        torch.cuda.empty_cache()
        index = bench_normals(a, dev, pts, index, T, r, frames, off, res)
    return res, index, wm


def bench_normals(a, dev, pts, index, T, r, frames, off, res):
    """-> the index with normals; fills res with the times of estimate_normals, of the per-frame cells kernel and of the two crops"""
    M, B = int(pts.shape[0]), a.B
    reps = max(a.reps // 4, 3)
    est = _ms(lambda: map_index.estimate_normals(pts, up_axis=1, orient=-1), reps, 1)
    normals = map_index.estimate_normals(pts, up_axis=1, orient=-1)
    index = map_index.MapIndex(index.sorted, index.cell_start, index.order, index.origin, index.cell, index.nx, index.ny, index.up_axis, normals)
    res.update(normals_ms=est, normals_rows_per_s=M / (est[0] * 1e-3))
    print("  estimate_normals            %9.3f ms (min %.3f, max %.3f) = %.1f M rows/s" % (est + (res["normals_rows_per_s"] / 1e6,)))
    if a.normals:
        # what there was before: the per-frame kernel on frames of 2^20 rows, every row a voxel of its own (2 mm voxels)
        st = scan_prep.voxel_down_sample(pts, off, 0.002, max_frame_points=FILTER_FRAME)
        cells = _ms(lambda: scan_prep.estimate_normals(st, method="cells"), reps, 1)
        voxels = int(st.offsets[-1])
        res.update(frame_cells_ms=cells, frame_cells_voxels=voxels, frame_cells_status=sorted(set(st.status.cpu().numpy().tolist())))
        print("  per-frame cells kernel      %9.3f ms (min %.3f, max %.3f) on %d frames of 2^20 rows (%d voxels, status %s): neighbours lost at the cuts"
              % (cells + (frames, voxels, res["frame_cells_status"])))
        del st
        torch.cuda.empty_cache()
        mfp = map_index.MAX_FRAME_POINTS
        for name, want in (("crop", False), ("crop_normals", True)):          # the plain crop again, in the same minute as the one with normals
            plan = map_index.CropPlan(index, B, B * (1 << 19), mfp, a.radius, want_normals=want)
            plan.run(T, r)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                plan.run(T, r)
            res[name + "_again_replay_ms" if not want else name + "_replay_ms"] = t = _ms(g.replay, a.reps, a.warmup)
            print("  %-27s %9.3f ms (min %.3f, max %.3f), graph replay, %d rows kept" % (("crop with normals" if want else "crop without normals",) + t
                                                                                       + (int(plan.offsets[-1]),)))
            del g, plan
    return index


def bench_executors(a, dev, index, wm):
    from deepi2p_amd.map_pipeline import MapFrameExecutor
    from deepi2p_amd.networks import MMClassifer, MMClassiferCoarse
    from deepi2p_amd.submap_pipeline import OxfordFrameExecutor
    B = a.B
    H0, W0 = sample_prep.RAW_HW["oxford"]
    opt = synthetic.OptLike(N, H, W, not a.coarse)
    opt.device = dev
    mm = (MMClassiferCoarse if a.coarse else MMClassifer)(opt)
    mm.detector.load_state_dict(synthetic.synthetic_state_dict(opt))
    from deepi2p_amd.registration import RegistrationPipeline
    from deepi2p_amd.registration_pnp import PnPPipeline
    pipe = RegistrationPipeline(H, W, seed=0) if a.coarse else PnPPipeline(H, W, iterations=500, seed=0)
    draws = pipe.draw(B, dev)
    kw = dict(restarts=draws) if a.coarse else dict(samples=draws)
    rng = np.random.default_rng(1)
    image = torch.from_numpy(np.stack([synthetic.make_camera_image(np.random.default_rng(b), H0, W0) for b in range(B)]))
    hb = dict(T_map_prior=priors_along(wm, B, rng), radius=a.radius, image=image, K_raw=np.tile(K_RAW, (B, 1, 1)), seed=1)
    mex = MapFrameExecutor(mm, pipe, opt, index, hb, B * (1 << 19), map_index.MAX_FRAME_POINTS, a.radius, n_streams=a.streams, **kw)
    # the Oxford executor as tools/bench_oxford_executor.py feeds it: 500 profiles x 541 beams per sub-map from a rendered traversal
    S, beams = 500, 541
    cal = synthetic.make_lms_traversal(rng, 1, 1, 1)
    Gl, Gc = cal["G_posesource_laser"], cal["G_cam"]
    tp = world.TraversalPlan(B, S, beams, H0, W0, dev)
    tp.set_world(world.make_street(rng, B, 0.2 * S + 20.0))
    tp.set_calibration(Gl, Gc)
    tp.set_camera(np.tile(K_RAW, (B, 1, 1)))
    tp.set_traversal(*world.traversal_inputs(world.make_trajectory(rng, B, S), S // 2, S // 2, Gl, Gc))
    outs = tp.run(seed=1)
    torch.cuda.synchronize()
    names = ("scan_xyr", "scan_offsets", "submap_offsets", "poses", "present", "G_posesource_laser", "G_cam", "image", "K_raw", "P_cam_pc")
    ohb = dict(zip(names, (t.cpu() for t in outs)), seed=1)
    oex = OxfordFrameExecutor(mm, pipe, opt, ohb, tp.S_cap, tp.P_cap, tp.P_cap, min(S * beams, submap.MAX_FRAME_POINTS), n_streams=a.streams,
                              skip_threshold=submap.VOXEL / 16.0, **kw)
    rates = {"map, resident": [], "map, with H2D": [], "oxford, resident": [], "oxford, with H2D": []}
    kex = None
    if a.dataset == "kitti":          # the KITTI model on the same map, which carries normals (bench_normals)
        kH0, kW0 = sample_prep.RAW_HW["kitti"]
        kopt = synthetic.OptLike(N, 160, 512, not a.coarse)
        kopt.device = dev
        kmm = (MMClassiferCoarse if a.coarse else MMClassifer)(kopt)
        kmm.detector.load_state_dict(synthetic.synthetic_state_dict(kopt))
        kpipe = RegistrationPipeline(160, 512, seed=0) if a.coarse else PnPPipeline(160, 512, iterations=500, seed=0)
        kdraws = kpipe.draw(B, dev)
        kimage = torch.from_numpy(np.stack([synthetic.make_camera_image(np.random.default_rng(b), kH0, kW0) for b in range(B)]))
        khb = dict(hb, image=kimage)
        kex = MapFrameExecutor(kmm, kpipe, kopt, index, khb, B * (1 << 19), map_index.MAX_FRAME_POINTS, a.radius, n_streams=a.streams,
                               dataset="kitti", **(dict(restarts=kdraws) if a.coarse else dict(samples=kdraws)))
        rates.update({"map kitti, resident": [], "map kitti, with H2D": []})
    for rnd in range(a.rounds + 1):                  # round 0 warms everything up and is dropped
        vals = {"map, resident": B * a.steps / mex.throughput(a.steps, a.warmup, False)[0],
                "oxford, resident": B * a.steps / oex.throughput(a.steps, a.warmup, False)[0],
                "map, with H2D": B * a.steps / mex.throughput(a.steps, a.warmup, True)[0],
                "oxford, with H2D": B * a.steps / oex.throughput(a.steps, a.warmup, True)[0]}
        if kex is not None:
            vals.update({"map kitti, resident": B * a.steps / kex.throughput(a.steps, a.warmup, False)[0],
                         "map kitti, with H2D": B * a.steps / kex.throughput(a.steps, a.warmup, True)[0]})
        if rnd:
            for k, v in vals.items():
                rates[k].append(v)
    assert mex.use_graph and oex.use_graph, (mex.graph_error, oex.graph_error)
    assert kex is None or kex.use_graph, kex.graph_error
    res = {k: float(np.median(v)) for k, v in rates.items()}
    for k, v in rates.items():
        print("  %-20s %8.1f frames/s = %7.3f ms per step of %d (median of %d rounds; min %.1f, max %.1f)"
              % (k, res[k], 1e3 * B / res[k], B, a.rounds, min(v), max(v)))
    print("  status map %s, oxford %s" % (sorted(set(mex.slots[0].prepared[9].cpu().numpy().tolist())),
                                          sorted(set(oex.slots[0].prepared[9].cpu().numpy().tolist()))))
    if kex is not None:
        print("  status map kitti %s" % sorted(set(kex.slots[0].prepared[9].cpu().numpy().tolist())))
    return dict(frames_per_s=res, spread={k: (min(v), max(v)) for k, v in rates.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--radius", type=float, default=50.0)
    ap.add_argument("--cell", type=float, default=8.0)
    ap.add_argument("--sizes", type=int, nargs="+", default=[22, 24])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--streams", type=int, default=2)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-executor", action="store_true")
    ap.add_argument("--coarse", action="store_true")
    ap.add_argument("--normals", action="store_true", help="time estimate_normals and the crop with normals at every size")
    ap.add_argument("--dataset", choices=["oxford", "kitti"], default="oxford", help="kitti: add the MapFrameExecutor(dataset='kitti') row")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_map.py measures on the GPU; there is none here")
    dev = torch.device("cuda", 0)
    out = dict(metric="map", sizes=[])
    first = None
    for log2m in a.sizes:
        res, index, wm = bench_size(log2m, a, dev)
        out["sizes"].append(res)
        first = first or (index, wm)
        torch.cuda.empty_cache()
    if not a.no_executor:
        out["executors"] = bench_executors(a, dev, *first)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
