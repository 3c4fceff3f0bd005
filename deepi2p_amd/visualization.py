"""Result overlays on the device: the images the reference writes for every evaluated frame (csrc/vis.hip).

get_registration_visualization              util/vis_tools.py:96-145        registration_overlay / registration_overlay_into
get_classification_visualization_coarse     util/vis_tools.py:147-228       classification_overlay_coarse / ..._into
get_classification_visualization            util/vis_tools.py:231-339       classification_overlay / ..._into
visualization_list_to_grid                  util/vis_tools.py:70-93         overlay_grid

A canvas is u8 [B, H + 2 H_delta, W + 2 W_delta, 3] (RGB): white, the frame's image in the middle, the points of the frame stamped over it
in index order as cv2.circle(radius 1, filled) -- five pixels -- with the reference's skip tests, roundings and colours (the header,
include/deepi2p_hip.h, has them in full).  The image is u8 [B,H,W,3] or the network's f32 [B,3,H,W] (img.round().to(uint8); values outside
0..255 are clamped, which torch leaves unspecified).  The reference's optional caption (t_ij_np, cv2.putText) is not reproduced: these
functions have no such parameter.  circle_size other than 1 raises: the five-pixel stamp is the only raster restated from OpenCV.

The `*_into` forms take the canvas and the workspace (`buffers`), launch three kernels on the current stream and allocate nothing: they
are what pipeline.RegistrationExecutor(visualize=...) captures into its step.  Argument errors are ValueErrors raised before any device work.
"""
import operator

import torch

from . import _lib
from ._lib import call, ptr, require_cuda, stream

MAX_POINTS = 1 << 28          # the key of a stamp is ((n + 1) << 3) | colour code in 32 bits


def _count(name, v, least):
    try:
        i = operator.index(v)
    except TypeError:
        raise ValueError("%s must be an integer, got %r" % (name, v)) from None
    if isinstance(v, bool) or i < least:
        raise ValueError("%s must be an integer >= %d, got %r" % (name, least, v))
    return i


def _geometry(who, img, H_delta, W_delta, circle_size):
    """-> (B, H, W, img_is_u8, H_delta, W_delta) of a checked image and margins"""
    if circle_size != 1:
        raise ValueError("%s: circle_size must be 1 (the only cv2.circle raster this port restates), got %r" % (who, circle_size))
    H_delta, W_delta = _count(who + ": H_delta", H_delta, 0), _count(who + ": W_delta", W_delta, 0)
    if not isinstance(img, torch.Tensor) or img.dim() != 4:
        raise ValueError("%s: img must be u8 [B,H,W,3] or f32 [B,3,H,W]" % who)
    if img.dtype == torch.uint8 and img.shape[3] == 3:
        B, H, W, u8 = int(img.shape[0]), int(img.shape[1]), int(img.shape[2]), 1
    elif img.dtype == torch.float32 and img.shape[1] == 3:
        B, H, W, u8 = int(img.shape[0]), int(img.shape[2]), int(img.shape[3]), 0
    else:
        raise ValueError("%s: img must be u8 [B,H,W,3] or f32 [B,3,H,W], got %s %s" % (who, img.dtype, tuple(img.shape)))
    if H < 1 or W < 1:
        raise ValueError("%s: empty image %s" % (who, tuple(img.shape)))
    return B, H, W, u8, H_delta, W_delta


def _labels(who, name, t, B, N):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or tuple(t.shape) != (B, N):
        raise ValueError("%s: %s must be i32 [%d,%d]" % (who, name, B, N))


def _buffers(who, canvas, workspace, B, H, W, H_delta, W_delta):
    want = (B, H + 2 * H_delta, W + 2 * W_delta, 3)
    if not isinstance(canvas, torch.Tensor) or canvas.dtype != torch.uint8 or tuple(canvas.shape) != want:
        raise ValueError("%s: canvas must be u8 %s" % (who, want))
    need = workspace_bytes(B, H, W, H_delta, W_delta)
    if not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.uint8 or workspace.dim() != 1 or workspace.numel() < need:
        raise ValueError("%s: workspace must be u8 [>= %d] (workspace_bytes)" % (who, need))


def workspace_bytes(B, H, W, H_delta=100, W_delta=100):
    """Bytes of the u32 key plane [B, H + 2 H_delta, W + 2 W_delta], rounded up to 256 (di2p_vis_workspace_bytes; host arithmetic)."""
    return (4 * B * (H + 2 * H_delta) * (W + 2 * W_delta) + 255) // 256 * 256


def buffers(B, H, W, device, H_delta=100, W_delta=100):
    """-> (canvas u8 [B, H + 2 H_delta, W + 2 W_delta, 3], workspace u8) for the `*_into` forms"""
    return (torch.empty((B, H + 2 * H_delta, W + 2 * W_delta, 3), dtype=torch.uint8, device=device),
            torch.empty((workspace_bytes(B, H, W, H_delta, W_delta),), dtype=torch.uint8, device=device))


def grid_lines(H, W, fine_scale):
    """The number of grid rows and columns the fine variant draws: round(H / s) - 1, round(W / s) - 1 with Python's round (half to even)"""
    return max(int(round(H / fine_scale)) - 1, 0), max(int(round(W / fine_scale)) - 1, 0)


def _classification(who, pxpy, coarse_pred, coarse_gt, fine_pred, fine_gt, img, canvas, workspace, fine_scale, H_delta, W_delta, circle_size):
    B, H, W, u8, H_delta, W_delta = _geometry(who, img, H_delta, W_delta, circle_size)
    fine = fine_pred is not None
    s = _count(who + ": fine_scale", fine_scale, 1) if fine else 0
    if not isinstance(pxpy, torch.Tensor) or pxpy.dtype != torch.float32 or pxpy.dim() != 3 or pxpy.shape[0] != B or pxpy.shape[1] != 2:
        raise ValueError("%s: pxpy must be f32 [%d,2,N]" % (who, B))
    N = int(pxpy.shape[2])
    if N > MAX_POINTS:
        raise ValueError("%s: at most 2^28 points per frame" % who)
    named = [("coarse_pred", coarse_pred), ("coarse_gt", coarse_gt)] + ([("fine_pred", fine_pred), ("fine_gt", fine_gt)] if fine else [])
    for name, t in named:
        _labels(who, name, t, B, N)
    if canvas is None:
        require_cuda(img)
        canvas, workspace = buffers(B, H, W, img.device, H_delta, W_delta)
    _buffers(who, canvas, workspace, B, H, W, H_delta, W_delta)
    require_cuda(pxpy, coarse_pred, coarse_gt, fine_pred, fine_gt, img, canvas, workspace)
    n_rows, n_cols = grid_lines(H, W, s) if fine else (0, 0)
    call("di2p_vis_classification", ptr(pxpy), ptr(coarse_pred), ptr(coarse_gt), ptr(fine_pred), ptr(fine_gt), ptr(img), u8, B, N, H, W, H_delta,
         W_delta, s, n_rows, n_cols, ptr(canvas), ptr(workspace), stream())
    return canvas


def classification_overlay_into(pxpy, coarse_pred, coarse_gt, fine_pred, fine_gt, img, canvas, workspace, fine_scale=32, H_delta=100,
                                W_delta=100, circle_size=1):
    """classification_overlay into `canvas` with `workspace` (buffers()): three launches, no allocation -- the form graphs capture."""
    if fine_pred is None or fine_gt is None:
        raise ValueError("classification_overlay: fine_pred and fine_gt are required (classification_overlay_coarse takes none)")
    return _classification("classification_overlay", pxpy, coarse_pred, coarse_gt, fine_pred, fine_gt, img, canvas, workspace, fine_scale,
                           H_delta, W_delta, circle_size)


def classification_overlay(pxpy, coarse_pred, coarse_gt, fine_pred, fine_gt, img, fine_scale=32, H_delta=100, W_delta=100, circle_size=1):
    """get_classification_visualization for a batch.  pxpy f32[B,2,N] (prep.project_labels(..., want_pxpy=True); no z test: a point behind
    the camera with a finite projection is drawn, as in the reference), coarse / fine predictions and labels i32[B,N], img u8 [B,H,W,3] or
    f32 [B,3,H,W], fine_scale the integer cell size in pixels.  Over the image: white grid lines between the cells; green = true positive in
    the right cell, yellow = true positive in a wrong cell, red = false negative, blue = false positive; true negatives are not drawn.
    -> u8 [B, H + 2 H_delta, W + 2 W_delta, 3].  Allocates canvas and workspace (the eager convenience)."""
    if fine_pred is None or fine_gt is None:
        raise ValueError("classification_overlay: fine_pred and fine_gt are required (classification_overlay_coarse takes none)")
    return _classification("classification_overlay", pxpy, coarse_pred, coarse_gt, fine_pred, fine_gt, img, None, None, fine_scale, H_delta,
                           W_delta, circle_size)


def classification_overlay_coarse_into(pxpy, coarse_pred, coarse_gt, img, canvas, workspace, H_delta=100, W_delta=100, circle_size=1):
    """classification_overlay_coarse into `canvas` with `workspace`: three launches, no allocation."""
    return _classification("classification_overlay_coarse", pxpy, coarse_pred, coarse_gt, None, None, img, canvas, workspace, 0, H_delta, W_delta,
                           circle_size)


def classification_overlay_coarse(pxpy, coarse_pred, coarse_gt, img, H_delta=100, W_delta=100, circle_size=1):
    """get_classification_visualization_coarse for a batch: as classification_overlay without the grid and without yellow."""
    return _classification("classification_overlay_coarse", pxpy, coarse_pred, coarse_gt, None, None, img, None, None, 0, H_delta, W_delta,
                           circle_size)


def _registration(pc, P, K, labels, img, canvas, workspace, H_delta, W_delta, circle_size):
    who = "registration_overlay"
    B, H, W, u8, H_delta, W_delta = _geometry(who, img, H_delta, W_delta, circle_size)
    if not isinstance(pc, torch.Tensor) or pc.dtype != torch.float32 or pc.dim() != 3 or pc.shape[0] != B or pc.shape[1] != 3:
        raise ValueError("%s: pc must be f32 [%d,3,N]" % (who, B))
    N = int(pc.shape[2])
    if N > MAX_POINTS:
        raise ValueError("%s: at most 2^28 points per frame" % who)
    if not isinstance(P, torch.Tensor) or P.dtype != torch.float64 or tuple(P.shape) != (B, 4, 4):
        raise ValueError("%s: P must be f64 [%d,4,4]" % (who, B))
    if not isinstance(K, torch.Tensor) or K.dtype != torch.float64 or tuple(K.shape) != (B, 3, 3):
        raise ValueError("%s: K must be f64 [%d,3,3]" % (who, B))
    _labels(who, "labels", labels, B, N)
    if canvas is None:
        require_cuda(img)
        canvas, workspace = buffers(B, H, W, img.device, H_delta, W_delta)
    _buffers(who, canvas, workspace, B, H, W, H_delta, W_delta)
    require_cuda(pc, P, K, labels, img, canvas, workspace)
    call("di2p_vis_registration", ptr(pc), ptr(P), ptr(K), ptr(labels), ptr(img), u8, B, N, H, W, H_delta, W_delta, ptr(canvas), ptr(workspace),
         stream())
    return canvas


def registration_overlay_into(pc, P, K, labels, img, canvas, workspace, H_delta=100, W_delta=100, circle_size=1):
    """registration_overlay into `canvas` with `workspace` (buffers()): three launches, no allocation -- the form graphs capture."""
    return _registration(pc, P, K, labels, img, canvas, workspace, H_delta, W_delta, circle_size)


def registration_overlay(pc, P, K, labels, img, H_delta=100, W_delta=100, circle_size=1):
    """get_registration_visualization for a batch: pc f32[B,3,N] projected in fp64 with the pose P f64[B,4,4] and the camera K f64[B,3,3],
    red where labels i32[B,N] is 1 and blue elsewhere; points with z < 0 are not drawn.  img u8 [B,H,W,3] or f32 [B,3,H,W].
    -> u8 [B, H + 2 H_delta, W + 2 W_delta, 3].  Allocates canvas and workspace (the eager convenience)."""
    return _registration(pc, P, K, labels, img, None, None, H_delta, W_delta, circle_size)


def overlay_grid(canvases, col=2):
    """visualization_list_to_grid: canvases u8 [B,h,w,3] (a tensor on any device, or a list of [h,w,3] tensors) laid out row-major in `col`
    columns on a white sheet u8 [ceil(B / col) h, col w, 3]; an empty list gives the reference's zeros of shape (3, 3).  Torch indexing only."""
    col = _count("overlay_grid: col", col, 1)
    if isinstance(canvases, (list, tuple)):
        if len(canvases) == 0:
            return torch.zeros((3, 3), dtype=torch.uint8)
        canvases = torch.stack(list(canvases))
    if canvases.dim() != 4 or canvases.dtype != torch.uint8:
        raise ValueError("overlay_grid: canvases must be u8 [B,h,w,c]")
    B, h, w, c = canvases.shape
    if B == 0:
        return torch.zeros((3, 3), dtype=torch.uint8, device=canvases.device)
    rows = -(-B // col)
    sheet = torch.full((rows * col, h, w, c), 255, dtype=torch.uint8, device=canvases.device)
    sheet[:B] = canvases
    return sheet.view(rows, col, h, w, c).permute(0, 2, 1, 3, 4).reshape(rows * h, col * w, c)


def library_workspace_bytes(B, H, W, H_delta=100, W_delta=100):
    """The library's own count (tests compare it with workspace_bytes)."""
    return int(_lib.load().di2p_vis_workspace_bytes(B, H, W, H_delta, W_delta))
