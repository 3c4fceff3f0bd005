#!/usr/bin/env python3
"""Map localisation end to end on a synthetic street (one MI355X): a push-broom traversal of one scene (deepi2p_amd.world.TraversalPlan,
one sub-map of --profiles LMS profiles) is built into a map in camera convention (submap.build_submaps: the frame of the traversal's origin
profile, y down), indexed (map_index.MapIndex.build) and kept on the device; camera frames are rendered along the traversal, their true poses
perturbed into priors, and map_pipeline.MapFrameExecutor localises them with evaluate=True.  The solver is fed the ground-truth frustum
labels of the prepared points (synthetic weights predict nothing), so the printed EvalState.line() says what the registration back end makes
of a crop around a rough prior, not what a trained network would.
    python tools/localize_synthetic.py [--frames 8] [--profiles 1500] [--beams 541] [--radius 40] [--shift 2.0] [--yaw 0.1] [--cell 8]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from deepi2p_amd import map_index, prep, submap, synthetic, world  # noqa: E402
from deepi2p_amd.map_pipeline import MapFrameExecutor, host_map_frames  # noqa: E402

N, H, W = 20480, 384, 640
RAW_HW = (960, 1280)
K_RAW = np.array([[964.828979, 0.0, 643.788025], [0.0, 964.828979, 484.40799], [0.0, 0.0, 1.0]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--profiles", type=int, default=1500)
    ap.add_argument("--beams", type=int, default=541)
    ap.add_argument("--radius", type=float, default=40.0)
    ap.add_argument("--shift", type=float, default=2.0)
    ap.add_argument("--yaw", type=float, default=0.1)
    ap.add_argument("--cell", type=float, default=8.0)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("localize_synthetic.py runs on the GPU; there is none here")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(a.seed)
    F, S = a.frames, a.profiles
    cal = synthetic.make_lms_traversal(rng, 1, 1, 1)
    Gl, Gc = cal["G_posesource_laser"], cal["G_cam"]
    street = world.make_street(rng, 1, 0.2 * S + 20.0)
    T_wv = world.make_trajectory(rng, 1, S)                                  # [1,S,4,4] vehicle poses in the world
    tp = world.TraversalPlan(1, S, a.beams, RAW_HW[0], RAW_HW[1], dev)
    tp.set_world(street)
    tp.set_calibration(Gl, Gc)
    tp.set_camera(K_RAW[None])
    tp.set_traversal(*world.traversal_inputs(T_wv, S // 2, S // 2, Gl, Gc))
    outs = tp.run(seed=a.seed)
    record, offsets, status = submap.build_submaps(*outs[:6], skip_threshold=submap.VOXEL / 16.0, G_cam=Gc)
    submap.check_status(status)
    M = int(offsets[-1])
    index = map_index.MapIndex.build(record[:M].contiguous(), a.cell, up_axis=1)
    # the map frame is the camera-convention frame of the origin profile: X_map = G_cam . inv(T_wv[origin]) . X_world
    T_map_world = Gc @ np.linalg.inv(T_wv[0, S // 2])
    at = np.linspace(0.15 * S, 0.85 * S, F).astype(np.int64)
    cam_to_world = T_wv[0, at] @ np.linalg.inv(Gc)
    gt = T_map_world @ cam_to_world                                          # T_map_cam_gt [F,4,4]
    scene = (np.repeat(np.asarray(street[0]), F, axis=0), np.repeat(np.asarray(street[1]), F))
    images = world.render_camera(scene, np.tile(K_RAW, (F, 1, 1)), np.linalg.inv(cam_to_world), RAW_HW[0], RAW_HW[1], device=dev)
    priors = gt.copy()
    for f in range(F):
        D = np.eye(4)
        D[:3, :3] = synthetic.ry_matrix(float(rng.uniform(-a.yaw, a.yaw)))
        D[0, 3], D[2, 3] = rng.uniform(-a.shift, a.shift, 2)
        priors[f] = gt[f] @ D
    hb = dict(T_map_prior=priors, radius=a.radius, image=images.cpu(), K_raw=np.tile(K_RAW, (F, 1, 1)), T_map_cam_gt=gt, seed=a.seed)
    from deepi2p_amd.networks import MMClassiferCoarse
    from deepi2p_amd.registration import RegistrationPipeline
    opt = synthetic.OptLike(N, H, W, False)
    opt.device = dev
    mm = MMClassiferCoarse(opt)
    mm.detector.load_state_dict(synthetic.synthetic_state_dict(opt))
    pipe = RegistrationPipeline(H, W, seed=0)
    mfp, cap = map_index.MAX_FRAME_POINTS, F * (1 << 19)
    # the labels the solver is fed: the frustum labels of the prepared points under the prepared sample's own pose
    plan = map_index.MapRawPlan(index, opt, F, cap, mfp, a.radius, RAW_HW, "val")
    T, r, image, K_raw, P_cam_pc, _, seed = host_map_frames(hb, F, RAW_HW, a.radius)
    prepared = plan.run(T.view(F, 4, 4).to(dev), r.to(dev), image.to(dev), K_raw.to(dev), P_cam_pc.to(dev), seed=seed)
    map_index.check_status(prepared[9])
    labels = prep.project_labels(prepared[0], prepared[5], prepared[7], H, W, 32)[0].clone()
    ex = MapFrameExecutor(mm, pipe, opt, index, hb, cap, mfp, a.radius, n_streams=1, restarts=pipe.draw(F, dev), labels_override=labels, evaluate=True)
    ex.eval_reset()
    out = ex.result(ex.submit(hb))
    torch.cuda.synchronize()
    kept = np.diff(plan.crop.offsets.cpu().numpy())
    print("map: %d rows (%d x %d cells of %.0f m), %d frames, r = %.0f m, priors off by up to %.1f m / %.2f rad; rows per crop %d .. %d; labels inside %.1f %%"
          % (M, index.nx, index.ny, a.cell, F, a.radius, a.shift, a.yaw, kept.min(), kept.max(), 100.0 * float(labels.float().mean())))
    rte, rre = out["rte"].cpu().numpy(), out["rre"].cpu().numpy()
    for f in range(F):
        prior_err = np.linalg.norm(priors[f, :3, 3] - gt[f, :3, 3])
        print("  frame %2d: prior off by %.2f m -> RTE %.3f m, RRE %.3f deg (status %d)" % (f, prior_err, rte[f], rre[f], int(out["status"][f])))
    print(ex.eval_state().line())


if __name__ == "__main__":
    main()
