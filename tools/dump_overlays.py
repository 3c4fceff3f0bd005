#!/usr/bin/env python3
"""A few synthetic frames through the executor with visualize="both", the canvases written as PNG files (PIL):

    python tools/dump_overlays.py [--out overlays] [--frames 4] [--points 20480] [--height 160] [--width 512] [--fine]

Per frame <out>/<i>_registration.png and <out>/<i>_classification.png, and <out>/grid.png: all registration canvases on one sheet
(visualization.overlay_grid, two columns).  The solver is fed the synthetic labels (random-init weights predict nothing), the overlays show
the network's own prediction, as the executor documents."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
NAMES = ("pc", "intensity", "sn", "node_a", "node_b", "img")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="overlays")
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--points", type=int, default=20480)
    ap.add_argument("--height", type=int, default=160)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--restarts", type=int, default=60)
    ap.add_argument("--fine", action="store_true", help="a model with the fine head: the classification overlay with its grid")
    a = ap.parse_args()
    import torch
    from PIL import Image
    from deepi2p_amd import synthetic, visualization
    from deepi2p_amd.networks import MMClassifer, MMClassiferCoarse
    from deepi2p_amd.pipeline import RegistrationExecutor
    from deepi2p_amd.registration import RegistrationPipeline
    dev = torch.device("cuda", 0)
    B, N, H, W = a.frames, a.points, a.height, a.width
    opt = synthetic.OptLike(N, H, W, a.fine)
    opt.device = dev
    mm = (MMClassifer if a.fine else MMClassiferCoarse)(opt)
    mm.detector.load_state_dict(synthetic.synthetic_state_dict(opt))
    batch = synthetic.make_batch(1000, B, N=N, H=H, W=W)
    host = {k: torch.from_numpy(batch[k]) for k in NAMES}
    host["P"] = torch.from_numpy(batch["P_gt"])
    pipe = RegistrationPipeline(H, W, R=a.restarts, seed=0)
    ex = RegistrationExecutor(mm, pipe, torch.from_numpy(batch["K"]).to(dev), host, n_streams=1, restarts=pipe.draw(B, dev),
                              labels_override=torch.from_numpy(batch["labels"]).to(dev), evaluate=True, visualize="both")
    out = ex.result(ex.submit(host))
    os.makedirs(a.out, exist_ok=True)
    for kind in ("registration", "classification"):
        for i, canvas in enumerate(out["vis_" + kind].cpu().numpy()):
            Image.fromarray(canvas).save(os.path.join(a.out, "%02d_%s.png" % (i, kind)))
    Image.fromarray(visualization.overlay_grid(out["vis_registration"]).cpu().numpy()).save(os.path.join(a.out, "grid.png"))
    print("%d frames: %d files in %s (graph: %s); %s" % (B, 2 * B + 1, a.out, ex.use_graph, ex.eval_state().line()))


if __name__ == "__main__":
    main()
