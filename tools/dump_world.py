#!/usr/bin/env python3
"""A few synthetic worlds rendered on the device (deepi2p_amd.world), written as PNG files (PIL):

    python tools/dump_world.py [--out worlds] [--frames 4] [--height 370] [--width 1226] [--seed 0]

Per frame <out>/<i>_image.png (the camera frame), <out>/<i>_depth.png (the camera-frame depth, white = near, black = sky or beyond max_range)
and <out>/<i>_scan.png (the LiDAR returns of the same scene projected into the image, coloured by intensity)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="worlds")
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--height", type=int, default=370)
    ap.add_argument("--width", type=int, default=1226)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    import numpy as np
    import torch
    from PIL import Image
    from deepi2p_amd import world
    dev = torch.device("cuda", 0)
    B, H0, W0 = a.frames, a.height, a.width
    rng = np.random.default_rng(a.seed)
    pattern = world.hdl64_pattern(rng, B)
    w = world.make_world(rng, B)
    f = 0.586 * W0
    K = np.tile(np.array([[f, 0, (W0 - 1) / 2.0], [0, f, (H0 - 1) / 2.0], [0, 0, 1.0]]), (B, 1, 1))
    Pc = np.tile(np.array([[0.0, -1, 0, 0.06], [0, 0, -1, -0.08], [1, 0, 0, -0.27], [0, 0, 0, 1]]), (B, 1, 1))
    img, depth = (t.cpu().numpy() for t in world.render_camera(w, K, Pc, H0, W0, depth=True, device=dev))
    pts, off, _ = (t.cpu().numpy() for t in world.render_scan(w, pattern, a.seed, device=dev))
    os.makedirs(a.out, exist_ok=True)
    for b in range(B):
        Image.fromarray(img[b]).save(os.path.join(a.out, "%02d_image.png" % b))
        near = np.where(depth[b] > 0, 1.0 - np.minimum(depth[b] / world.MAX_RANGE, 1.0), 0.0)
        Image.fromarray(np.rint(255.0 * near).astype(np.uint8)).save(os.path.join(a.out, "%02d_depth.png" % b))
        p = pts[off[b]:off[b + 1]]
        cam = p[:, :3].astype(np.float64) @ Pc[b, :3, :3].T + Pc[b, :3, 3]
        front = cam[:, 2] > 0.1
        u = np.rint(K[b, 0, 0] * cam[front, 0] / cam[front, 2] + K[b, 0, 2]).astype(int)
        v = np.rint(K[b, 1, 1] * cam[front, 1] / cam[front, 2] + K[b, 1, 2]).astype(int)
        ok = (u >= 0) & (u < W0) & (v >= 0) & (v < H0)
        canvas = (img[b] // 3).copy()
        inten = p[front, 3][ok]
        canvas[v[ok], u[ok]] = np.stack([255.0 * inten, 255.0 * (1.0 - inten), np.full_like(inten, 64.0)], 1).astype(np.uint8)
        Image.fromarray(canvas).save(os.path.join(a.out, "%02d_scan.png" % b))
    print("%d frames: %d files in %s; %d returns, %.1f %% of the pixels are sky" % (B, 3 * B, a.out, int(off[-1]), 100.0 * float(np.mean(depth == 0))))


if __name__ == "__main__":
    main()
