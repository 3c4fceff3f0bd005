"""Generates tests/golden/vis_golden.npz from the REFERENCE's own drawing functions (run where the reference checkout exists):

    python tests/golden/make_vis_golden.py

`get_registration_visualization`, `get_classification_visualization_coarse`, `get_classification_visualization` and
`visualization_list_to_grid` are extracted from util/vis_tools.py with `ast` at generation time and run against a stub `cv2` (OpenCV is not
installed): `circle` paints the five pixels of a filled circle of radius 1 -- OpenCV's midpoint loop for that radius makes one pass with
dx = 1, dy = 0, after which dx drops to 0 and the loop ends: the centre row from cx - 1 to cx + 1 and the centre column from cy - 1 to
cy + 1, clipped -- and `line` paints an axis-aligned run of one-pixel width, ends included.  Both assert the arguments they were restated for.
Control flow, rounding, skip tests, colour rules and paint order are therefore the reference's own; only the two rasters are restated.

The file holds arrays only, per case `<kind><i>_<name>` with kind `cls` or `reg`:

  cls<i>_dims     H, W, H_delta, W_delta, N, cell size
  cls<i>_img      u8 [H,W,3];  _pxpy f32 [2,N];  _coarse_pred, _coarse_gt, _fine_pred, _fine_gt i32 [N]
  cls<i>_fine, cls<i>_coarse      the two functions' canvases, u8 [H + 2 H_delta, W + 2 W_delta, 3]
  reg<i>_dims     H, W, H_delta, W_delta, N, exact (1: P = [I | t] and K in dyadic numbers)
  reg<i>_img, _pc f32 [3,N], _P f64 [4,4], _K f64 [3,3], _labels i32 [N], _canvas
  grid_in u8 [3,h,w,3], grid_out  visualization_list_to_grid(list(grid_in), col=2)

Classification inputs: coordinates uniform over the canvas and three pixels beyond; three in ten are exact .5 values (both parities of the
integer part occur); from N = 63 on the first slots hold inf, -inf, NaN, 1e30 and -1e30 in either coordinate and centres at -1, 0,
side - 2 and side - 1 of both axes; from N = 300 on the last two points share a centre, the earlier one drawn and the later one of the
"nothing drawn" class.  Registration inputs: `exact` cases project through P = [I | t], K = [[16, 0, cx], [0, 16, cy], [0, 0, 1]] and hold
points with z == 0 exactly, points with z == -1 whose projection lies inside the canvas, and the same eight edge centres (computed without
rounding: z == 1); the other cases use a drawn rotation.  Any registration point whose fp64 projection is within 1e-6 px of a half-integer
(every skip boundary is one) or has 0 < |z| < 1e-6 is redrawn (tests/vis_oracle.py:near_tie): the device's dot products and numpy's may
differ in the last place and that ordering cannot be pinned.  Everything else is compared exactly.
"""
import ast
import math
import os
import sys
import types

import numpy as np
from scipy.spatial.transform import Rotation

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle import ref_network as rn  # noqa: E402
from tests import vis_oracle  # noqa: E402

NAMES = ("get_registration_visualization", "get_classification_visualization_coarse", "get_classification_visualization",
         "visualization_list_to_grid")
# H, W, H_delta, W_delta, N, cell size
CLS_CASES = [(24, 40, 6, 6, 3000, 16), (24, 40, 0, 0, 300, 8), (16, 32, 6, 6, 65, 8), (16, 32, 0, 0, 64, 16), (16, 32, 100, 100, 63, 8),
             (24, 40, 6, 0, 1, 8)]
# H, W, H_delta, W_delta, N, exact
REG_CASES = [(24, 40, 6, 6, 3000, 0), (16, 32, 0, 0, 300, 1), (16, 32, 6, 6, 65, 0), (24, 40, 6, 6, 64, 1), (24, 40, 0, 0, 63, 0),
             (16, 32, 6, 0, 1, 0)]


def stub_cv2():
    def circle(img, center, radius, color, thickness):
        assert radius == 1 and thickness == -1, (radius, thickness)
        cx, cy = center
        H, W = img.shape[:2]
        for dx, dy in ((0, 0), (-1, 0), (1, 0), (0, -1), (0, 1)):
            x, y = cx + dx, cy + dy
            if 0 <= x < W and 0 <= y < H:
                img[y, x] = color
        return img

    def line(img, p0, p1, color, thickness):
        assert thickness == 1 and (p0[0] == p1[0] or p0[1] == p1[1]), (p0, p1, thickness)
        H, W = img.shape[:2]
        for x in range(min(p0[0], p1[0]), max(p0[0], p1[0]) + 1):
            for y in range(min(p0[1], p1[1]), max(p0[1], p1[1]) + 1):
                if 0 <= x < W and 0 <= y < H:
                    img[y, x] = color
        return img

    return types.SimpleNamespace(circle=circle, line=line)


def reference_functions():
    path = os.path.join(rn.REF, "util", "vis_tools.py")
    ns = {"np": np, "math": math, "cv2": stub_cv2()}
    for node in ast.parse(open(path).read()).body:
        if isinstance(node, ast.FunctionDef) and node.name in NAMES:
            exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), ns)
    return [ns[n] for n in NAMES]


def edge_centres(H, W, H_delta, W_delta):
    """(px, py) whose centres are -1, 0, side - 2, side - 1 along x (y mid-image) and then along y (x mid-image)"""
    HL, WL = H + 2 * H_delta, W + 2 * W_delta
    out = [(c - W_delta, H // 2) for c in (-1, 0, WL - 2, WL - 1)]
    return out + [(W // 2, c - H_delta) for c in (-1, 0, HL - 2, HL - 1)]


def classification_inputs(rng, H, W, H_delta, W_delta, N):
    lo = np.array([-W_delta - 3.0, -H_delta - 3.0])[:, None]
    hi = np.array([W + W_delta + 3.0, H + H_delta + 3.0])[:, None]
    pxpy = rng.uniform(lo, hi, (2, N))
    half = rng.random((2, N)) < 0.3
    pxpy[half] = np.floor(pxpy[half]) + 0.5
    pxpy = pxpy.astype(np.float32)
    labels = [(rng.random(N) < p).astype(np.int32) for p in (0.6, 0.6)] + [rng.integers(0, 3, N).astype(np.int32) for _ in range(2)]
    if N >= 63:
        specials = [(np.inf, 3), (3, np.inf), (-np.inf, 3), (3, -np.inf), (np.nan, 3), (3, np.nan), (1e30, 3), (3, 1e30), (-1e30, 3), (3, -1e30),
                    (0.5, 1.5), (1.5, 0.5), (2.5, 2.5)] + edge_centres(H, W, H_delta, W_delta)
        for j, (x, y) in enumerate(specials):
            pxpy[:, j] = (x, y)
            labels[0][j] = labels[1][j] = 1            # they would be drawn if their coordinates let them
    if N >= 300:
        pxpy[:, N - 2] = pxpy[:, N - 1] = (W // 2 + 1, H // 2 + 1)
        labels[0][N - 2], labels[1][N - 2] = 0, 1      # red ...
        labels[0][N - 1], labels[1][N - 1] = 0, 0      # ... and a later point of the class that draws nothing, which must not cover it
    return pxpy, labels


def registration_inputs(rng, H, W, H_delta, W_delta, N, exact):
    HL, WL = H + 2 * H_delta, W + 2 * W_delta
    P = np.identity(4)
    if exact:
        P[:3, 3] = (0.5, -0.25, 2.0)
        K = np.array([[16.0, 0, W / 2], [0, 16.0, H / 2], [0, 0, 1]])
    else:
        P[:3, :3] = Rotation.from_euler("xyz", rng.uniform(-25, 25, 3), degrees=True).as_matrix()
        P[:3, 3] = rng.uniform(-1, 1, 3)
        K = np.array([[W * 0.6, 0, W / 2 + 0.3], [0, W * 0.6, H / 2 - 0.2], [0, 0, 1]])

    def draw(n):
        # camera-frame points over a frustum wider than the canvas, a tenth of them behind the camera; back to the cloud's frame, as f32
        z = rng.uniform(1.0, 12.0, n) * np.where(rng.random(n) < 0.1, -1.0, 1.0)
        px, py = rng.uniform(-W_delta - 3, W + W_delta + 3, n), rng.uniform(-H_delta - 3, H + H_delta + 3, n)
        cam = np.stack([(px - K[0, 2]) / K[0, 0] * z, (py - K[1, 2]) / K[1, 1] * z, z, np.ones(n)])
        return np.dot(np.linalg.inv(P), cam)[:3].astype(np.float32)

    pc = draw(N)
    if exact:
        t = P[:3, 3]
        j = 0
        for x, y in edge_centres(H, W, H_delta, W_delta):                      # z == 1 after the translation: px = 16 X + cx without rounding
            pc[:, j] = ((x - K[0, 2]) / 16.0 - t[0], (y - K[1, 2]) / 16.0 - t[1], 1.0 - t[2])
            j += 1
        for x in (0.0, 1.0, -3.0):                                             # z == 0 exactly: the projection is inf or NaN
            pc[:, j] = (x - t[0], 0.25 - t[1], -t[2])
            j += 1
        for x, y in ((W // 2, H // 2), (3, 2)):                                # z == -1 with a finite projection inside the canvas
            pc[:, j] = (-(x - K[0, 2]) / 16.0 - t[0], -(y - K[1, 2]) / 16.0 - t[1], -1.0 - t[2])
            j += 1
    fixed = 13 if exact else 0
    for _ in range(100):
        bad = vis_oracle.near_tie(pc, P, K)
        bad[:fixed] = False
        if not bad.any():
            break
        pc[:, bad] = draw(int(bad.sum()))
    else:
        raise SystemExit("could not move every point off the ties")
    labels = (rng.random(N) < 0.5).astype(np.int32)
    return pc, P, K, labels


def main():
    registration, coarse, fine, to_grid = reference_functions()
    rng = np.random.default_rng(2025)
    out = {}
    for i, (H, W, H_delta, W_delta, N, s) in enumerate(CLS_CASES):
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        pxpy, (cp, cg, fp, fg) = classification_inputs(rng, H, W, H_delta, W_delta, N)
        k = "cls%d_" % i
        out.update({k + "dims": np.array([H, W, H_delta, W_delta, N, s]), k + "img": img, k + "pxpy": pxpy, k + "coarse_pred": cp,
                    k + "coarse_gt": cg, k + "fine_pred": fp, k + "fine_gt": fg,
                    k + "fine": fine(pxpy, cp, fp, cg, fg, img, s, H_delta=H_delta, W_delta=W_delta),
                    k + "coarse": coarse(pxpy, cp, cg, img, H_delta=H_delta, W_delta=W_delta)})
    for i, (H, W, H_delta, W_delta, N, exact) in enumerate(REG_CASES):
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        pc, P, K, labels = registration_inputs(rng, H, W, H_delta, W_delta, N, exact)
        k = "reg%d_" % i
        out.update({k + "dims": np.array([H, W, H_delta, W_delta, N, exact]), k + "img": img, k + "pc": pc, k + "P": P, k + "K": K,
                    k + "labels": labels,
                    k + "canvas": registration(pc.astype(np.float64), P, K, labels, img, H_delta=H_delta, W_delta=W_delta)})
    grid_in = rng.integers(0, 256, (3, 5, 7, 3), dtype=np.uint8)
    out["grid_in"], out["grid_out"] = grid_in, to_grid(list(grid_in), col=2)
    assert to_grid([], col=2).shape == (3, 3)
    path = os.path.join(HERE, "vis_golden.npz")
    np.savez_compressed(path, **out)
    print("vis_golden.npz written: %d classification and %d registration cases, %d bytes" % (len(CLS_CASES), len(REG_CASES), os.path.getsize(path)))


if __name__ == "__main__":
    main()
