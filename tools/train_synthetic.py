#!/usr/bin/env python3
"""Training on rendered synthetic worlds: per step B fresh scenes (world.make_world) -> WorldPlan (camera frames + LiDAR scans of the same
scenes, on the device) -> raw_prep.RawFramePlan(mode="train") (the KITTI raw stage and the loader's augmentation) -> ClassifierTrainer.optimize.

    python tools/train_synthetic.py [--steps 300] [--batch 8] [--points 20480] [--height 160] [--width 512] [--coarse] [--seed 0] [--every 25] [--blind]
                                    [--dataset oxford [--profiles 300] [--lms-beams 541]]

--dataset oxford is the same loop on a push-broom traversal: per step B fresh streets and drives (world.make_street, make_trajectory) ->
TraversalPlan (camera frames + LMS profiles of the same scenes) -> submap.OxfordRawPlan(mode="train") (the Oxford raw stage and the loader's
augmentation) -> ClassifierTrainer.optimize, on 960 x 1280 frames (--height 384 --width 640 is the reference's Oxford image).

Every `--every` steps one line: the loss and the coarse / fine accuracy of the step's own batch (train-mode forward, before the update), and
the share of inside points of that batch -- 1 minus it is the accuracy of the classifier that answers "outside" for every point.
--blind is the control: the rendered frames are overwritten with uniform noise bytes before the raw stage, so whatever is learnt then is learnt
from the cloud alone.  The defaults are the reference's training shapes (batch 8, 20480 points, 160 x 512 images, fine resolution).  A record, not a
test: nothing is asserted."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--points", type=int, default=20480)
    ap.add_argument("--height", type=int, default=160)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--coarse", action="store_true", help="train the coarse head alone")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--every", type=int, default=25)
    ap.add_argument("--blind", action="store_true", help="control: uniform-noise frames instead of the rendered ones")
    ap.add_argument("--beams", type=int, default=64)
    ap.add_argument("--azimuths", type=int, default=1800)
    ap.add_argument("--dataset", choices=("kitti", "oxford"), default="kitti")
    ap.add_argument("--profiles", type=int, default=300, help="oxford: LMS profiles per sub-map")
    ap.add_argument("--lms-beams", type=int, default=541, help="oxford: beams per profile")
    a = ap.parse_args()
    import numpy as np
    import torch
    from deepi2p_amd import raw_prep, scan_prep, synthetic, world
    from deepi2p_amd.networks import KeypointDetector
    from deepi2p_amd.training import ClassifierTrainer
    dev = torch.device("cuda", 0)
    B, N, H, W = a.batch, a.points, a.height, a.width
    raw_hw = (370, 1226)
    opt = synthetic.OptLike(N, H, W, not a.coarse)
    opt.lr, opt.coarse_loss_alpha = 1e-3, 50.0
    det = KeypointDetector(opt)
    det.load_state_dict(synthetic.random_state_dict(opt, a.seed))
    tr = ClassifierTrainer(det.to(dev), opt, seed=a.seed)
    rng = np.random.default_rng(a.seed)
    if a.dataset == "oxford":
        from deepi2p_amd import submap
        S, raw_hw = a.profiles, (960, 1280)
        cal = synthetic.make_lms_traversal(np.random.default_rng(0), 1, 1, 1)          # the mounting of the laser and of the camera
        Gl, Gc = cal["G_posesource_laser"], cal["G_cam"]
        raw = submap.OxfordRawPlan(opt, B, B * S, B * S * a.lms_beams, B * S * a.lms_beams, min(S * a.lms_beams, submap.MAX_FRAME_POINTS), raw_hw,
                                   "train", skip_threshold=submap.VOXEL / 16.0, device=dev)
        tp = world.TraversalPlan(B, S, a.lms_beams, raw_hw[0], raw_hw[1], dev, seed_slot=raw.seed)
        tp.set_calibration(Gl, Gc)
        tp.set_camera(np.tile(np.array([[964.828979, 0.0, 643.788025], [0.0, 964.828979, 484.40799], [0.0, 0.0, 1.0]]), (B, 1, 1)))

        def one_batch(step):
            tp.set_world(world.make_street(rng, B, 0.2 * S + 20.0))
            tp.set_traversal(*world.traversal_inputs(world.make_trajectory(rng, B, S), S // 2, S // 2, Gl, Gc))
            outs = tp.run(seed=a.seed * 1000003 + step)
            if a.blind:
                outs[7].random_(0, 256)
            return raw.run(*outs, seed=None)
    else:
        raw = raw_prep.RawFramePlan(opt, B, B * a.beams * a.azimuths, min(a.beams * a.azimuths, scan_prep.MAX_FRAME_POINTS), raw_hw, "train", "kitti", "cells", dev)
        wp = world.WorldPlan(B, raw_hw[0], raw_hw[1], a.beams, a.azimuths, dev, seed_slot=raw.seed)
        K = np.tile(np.array([[718.856, 0.0, 607.1928], [0.0, 718.856, 185.2157], [0.0, 0.0, 1.0]]), (B, 1, 1))
        Pc = np.tile(np.array([[0.0, -1, 0, 0.06], [0, 0, -1, -0.08], [1, 0, 0, -0.27], [0, 0, 0, 1]]), (B, 1, 1))
        wp.set_cameras(K, Pc)

        def one_batch(step):
            wp.set_pattern(world.hdl64_pattern(rng, B, a.beams, a.azimuths))
            points, offsets, images = wp.run(world.make_world(rng, B), seed=a.seed * 1000003 + step)
            if a.blind:
                images.random_(0, 256)
            return raw.run(points, offsets, images, wp.K_raw, wp.Pc, seed=None)
    curve, window = [], []
    t0 = time.perf_counter()
    for step in range(a.steps):
        out = one_batch(step)
        pc, intensity, sn, node_a, node_b, P, img, Kf = out[:8]
        L = tr.optimize(pc, intensity, sn, node_a, node_b, img, Kf, P)
        window.append(torch.stack([L["loss"], L["coarse_accuracy"], L["fine_accuracy"], L["inside"] / float(B * N)]))
        if (step + 1) % a.every == 0 or step + 1 == a.steps:
            status = raw.status[:B].cpu().numpy()
            last = window[-1].cpu().numpy()
            mean = torch.stack(window).mean(0).cpu().numpy()
            window = []
            rec = dict(step=step + 1, loss=float(last[0]), coarse_accuracy=float(last[1]), fine_accuracy=float(last[2]), inside_share=float(last[3]),
                       all_outside_accuracy=1.0 - float(last[3]), mean_loss=float(mean[0]), mean_coarse_accuracy=float(mean[1]),
                       mean_fine_accuracy=float(mean[2]), mean_inside_share=float(mean[3]))
            curve.append(rec)
            print("step %4d  loss %8.4f  coarse acc %.4f  fine acc %.4f  inside %.4f (all-outside acc %.4f) | mean of the last %d steps: loss %8.4f  coarse %.4f  "
                  "fine %.4f  all-outside %.4f | status %s | %.1f s"
                  % (step + 1, last[0], last[1], last[2], last[3], 1.0 - last[3], a.every, mean[0], mean[1], mean[2], 1.0 - mean[3],
                     sorted(set(status.tolist())), time.perf_counter() - t0), flush=True)
    print(json.dumps(dict(metric="train_synthetic", batch=B, points=N, height=H, width=W, fine=not a.coarse, blind=a.blind, steps=a.steps, curve=curve)))


if __name__ == "__main__":
    main()
