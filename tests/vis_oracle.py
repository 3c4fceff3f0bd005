"""numpy restatement of the result overlays (deepi2p_amd/visualization.py, csrc/vis.hip) in the max-key form: a canvas pixel shows the colour
of the LARGEST point index whose five-pixel stamp covers it, otherwise the base (white margin, image, white grid lines).  Vectorised; one
frame per call.  tests/golden/vis_golden.npz holds what the reference's own loops give, and test_vis_host.py requires this file to equal
every golden canvas exactly; the GPU tests use it where the golden has no case (batches, N = 1, executor outputs)."""
import numpy as np

RED, BLUE, GREEN, YELLOW = 1, 2, 3, 4
COLOURS = np.array([[0, 0, 0], [255, 0, 0], [0, 0, 255], [0, 255, 0], [255, 255, 0]], np.uint8)
STAMP = ((0, 0), (-1, 0), (1, 0), (0, -1), (0, 1))          # (dx, dy) of cv2.circle(radius 1, filled)


def image_u8(img):
    """u8 [H,W,3] as it is; f32 [3,H,W] -> round half to even, clamp to 0..255, HWC"""
    img = np.asarray(img)
    if img.dtype == np.uint8:
        return img
    return np.clip(np.rint(img.astype(np.float32)), 0, 255).astype(np.uint8).transpose(1, 2, 0)


def grid_lines(H, W, s):
    return max(int(round(H / s)) - 1, 0), max(int(round(W / s)) - 1, 0)


def base_canvas(img, H_delta, W_delta, grid_s=0):
    img = image_u8(img)
    H, W = img.shape[:2]
    canvas = np.full((H + 2 * H_delta, W + 2 * W_delta, 3), 255, np.uint8)
    canvas[H_delta:H_delta + H, W_delta:W_delta + W] = img
    if grid_s:
        n_rows, n_cols = grid_lines(H, W, grid_s)
        for h in range(1, n_rows + 1):
            canvas[h * grid_s + H_delta, W_delta:W_delta + W] = 255
        for w in range(1, n_cols + 1):
            canvas[H_delta:H_delta + H, w * grid_s + W_delta] = 255
    return canvas


def paint(canvas, px, py, code, H_delta, W_delta):
    """px, py float arrays [N]; code int [N] (0: not drawn).  In place, -> canvas"""
    HL, WL = canvas.shape[:2]
    with np.errstate(invalid="ignore"):
        rx, ry = np.rint(px), np.rint(py)
        ok = np.isfinite(px) & np.isfinite(py) & (code > 0)
        ok &= (rx >= -W_delta) & (rx < WL - 1 - W_delta) & (ry >= -H_delta) & (ry < HL - 1 - H_delta)
    n = np.nonzero(ok)[0]
    cx, cy = rx[n].astype(np.int64) + W_delta, ry[n].astype(np.int64) + H_delta
    keys = np.zeros((HL, WL), np.int64)
    key = ((n + 1) << 3) | code[n]
    for dx, dy in STAMP:
        x, y = cx + dx, cy + dy
        inside = (x >= 0) & (x < WL) & (y >= 0) & (y < HL)
        np.maximum.at(keys, (y[inside], x[inside]), key[inside])
    drawn = keys > 0
    canvas[drawn] = COLOURS[keys[drawn] & 7]
    return canvas


def classification(pxpy, coarse_pred, coarse_gt, fine_pred, fine_gt, img, grid_s, H_delta, W_delta):
    """pxpy f32 [2,N]; fine_pred / fine_gt None and grid_s 0: the coarse variant"""
    pred, gt = np.asarray(coarse_pred) == 1, np.asarray(coarse_gt) == 1
    code = np.zeros(pred.shape, np.int64)
    code[pred & gt] = GREEN
    if fine_pred is not None:
        code[pred & gt & (np.asarray(fine_pred) != np.asarray(fine_gt))] = YELLOW
    code[~pred & gt] = RED
    code[pred & ~gt] = BLUE
    pxpy = np.asarray(pxpy, np.float32)
    return paint(base_canvas(img, H_delta, W_delta, grid_s), pxpy[0], pxpy[1], code, H_delta, W_delta)


def project(pc, P, K):
    """get_registration_visualization's projection (util/vis_tools.py:104-109) in fp64 -> (px, py, z)"""
    pc = np.asarray(pc, np.float32).astype(np.float64)
    homo = np.concatenate((pc, np.ones((1, pc.shape[1]))), axis=0)
    k = np.dot(np.asarray(K, np.float64), np.dot(np.asarray(P, np.float64), homo)[0:3])
    with np.errstate(divide="ignore", invalid="ignore"):
        return k[0] / k[2], k[1] / k[2], k[2]


def registration(pc, P, K, labels, img, H_delta, W_delta):
    px, py, z = project(pc, P, K)
    code = np.where(np.asarray(labels) == 1, RED, BLUE).astype(np.int64)
    code[z < 0] = 0
    return paint(base_canvas(img, H_delta, W_delta), px, py, code, H_delta, W_delta)


def near_tie(pc, P, K, eps=1e-6):
    """Points whose fp64 projection the device's dot products and numpy's may round to different pixels or skip differently: px or py
    within eps of a half-integer (every skip boundary of the centre test is one), or 0 < |z| < eps.  Exact z == 0 is not a tie."""
    px, py, z = project(pc, P, K)
    with np.errstate(invalid="ignore"):
        bad = (z != 0) & (np.abs(z) < eps)
        for p in (px, py):
            near = np.isfinite(p) & (np.abs(p) < 1e7)
            frac = np.abs(p - np.floor(p) - 0.5)
            bad |= near & (frac < eps)
    return bad
