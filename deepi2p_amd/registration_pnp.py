"""PnP registration front-end (BASELINE config 3) on the HIP RANSAC kernel.

solve_PnP                evaluation/registration_pnp.py:95-148   (same signature, same return pair)
camera_matrix_scaling    evaluation/registration_pnp.py:58-61

cv2.solvePnPRansac's sampling is internal and unseeded; here the RANSAC draws are an explicit input (or come from a
seeded numpy Generator), like the solver's restart list.  OpenCV is absent: parity unpinned.
"""
import numpy as np
import torch

from . import _lib
from ._lib import call, ptr, require_cuda, stream

SAMPLE_SIZE = 6


def camera_matrix_scaling(K, s):
    K_scale = s * np.asarray(K, dtype=np.float64)
    K_scale[2, 2] = 1
    return K_scale


def draw_samples(rng, F, iters):
    """RANSAC draws: i32[F, iters, 6] INDEPENDENT uniform integers; the device reduces each modulo the frame's correspondence
    count.  A sample may therefore repeat a correspondence (likely only for frames with a handful of them); such samples are
    rejected as degenerate by the estimators, which lowers the effective iteration count for those frames but is never wrong."""
    return rng.integers(0, 2 ** 30, size=(F, iters, SAMPLE_SIZE), dtype=np.int64).astype(np.int32)


def pack_correspondences(pc, coarse, fine, W_fine, pixels=None):
    """What solve_PnP hands to cv2.solvePnPRansac (registration_pnp.py:97-110,125-127), packed on the device.
    pc f32[F,3,N], coarse/fine i32[F,N] -> (corr f32[F,N,8] = {x, y, z, u, v, 0, 0, 0}, n_corr i32[F]); the first n_corr[f] records are valid."""
    require_cuda(pc, coarse, fine, pixels)
    F, _, N = pc.shape
    corr = torch.zeros((F, N, 8), dtype=torch.float32, device=pc.device)
    n_corr = torch.empty((F,), dtype=torch.int32, device=pc.device)
    call("di2p_pnp_pack", ptr(pc), ptr(coarse), ptr(fine), ptr(pixels), int(W_fine), F, N, ptr(corr), ptr(n_corr), stream())
    return corr, n_corr


def _align256(n):
    return (n + 255) // 256 * 256


def workspace_views(ws, F, N, iters):
    """The intermediates both RANSAC entry points leave in their workspace (layout: include/deepi2p_hip.h, di2p_pnp_workspace_bytes), as
    VIEWS of `ws` u8[>= di2p_pnp_workspace_bytes(F, N, iters)], readable after the call (tests, debugging):
    corr f32[F,N,8] (the first n_corr[f] records of a frame valid), hyp f64[F,iters,13] = R (9, row-major), t (3), valid flag,
    inliers i32[F,iters] (-1: invalid hypothesis), mask u8[F,N] (inliers of the final round; written for frames with a model only)."""
    sizes = (F * N * 32, F * iters * 13 * 8, F * iters * 4, F * N)
    offs = [0]
    for s in sizes[:-1]:
        offs.append(offs[-1] + _align256(s))
    if ws.dtype != torch.uint8 or ws.dim() != 1 or ws.numel() < offs[3] + sizes[3]:
        raise ValueError("workspace must be a flat uint8 tensor of at least di2p_pnp_workspace_bytes(F, N, iters) bytes")
    part = [ws[o:o + s] for o, s in zip(offs, sizes)]
    return dict(corr=part[0].view(torch.float32).view(F, N, 8), hyp=part[1].view(torch.float64).view(F, iters, 13),
                inliers=part[2].view(torch.int32).view(F, iters), mask=part[3].view(F, N))


def pnp_ransac(pc, coarse, fine, K_scaled, W_fine, samples, reproj_err=0.6, refine_rounds=20, refine_iters=5, pixels=None,
               method="epnp", return_workspace=False):
    """Batched device entry.  pc f32[F,3,N], coarse/fine i32[F,N], K_scaled f64[F,3,3], samples i32[F,iters,6]
    -> dict(P f64[F,4,4], outlier_ratio f64[F], n_inliers, n_corr, best i32[F]).
    method "epnp" (default -- what the reference asks OpenCV for, registration_pnp.py:125-132): EPnP minimal-sample hypotheses (5 points,
    or 4 when a frame has only 4) + one EPnP re-fit on the inliers, the estimator of cv2.solvePnPRansac(flags=SOLVEPNP_EPNP);
    "dlt_lo": the builder's 6-point DLT hypotheses + locally optimised best model (more robust on cell-quantised observations, but not the
    reference's algorithm; refine_rounds / refine_iters apply to it only).
    return_workspace: add the stage intermediates corr, hyp, inliers, mask (workspace_views: views of the call's workspace, no copies)."""
    require_cuda(pc, coarse, fine, K_scaled, samples, pixels)
    F, _, N = pc.shape
    iters = samples.shape[1]
    dev = pc.device
    P = torch.empty((F, 4, 4), dtype=torch.float64, device=dev)
    ratio = torch.empty((F,), dtype=torch.float64, device=dev)
    n_in = torch.empty((F,), dtype=torch.int32, device=dev)
    n_corr = torch.empty((F,), dtype=torch.int32, device=dev)
    best = torch.empty((F,), dtype=torch.int32, device=dev)
    ws = torch.empty((_lib.load().di2p_pnp_workspace_bytes(F, N, iters),), dtype=torch.uint8, device=dev)
    if method == "epnp":
        call("di2p_pnp_ransac_epnp", ptr(pc), ptr(coarse), ptr(fine), ptr(pixels), ptr(K_scaled), int(W_fine), ptr(samples), iters,
             float(reproj_err), F, N, ptr(P), ptr(ratio), ptr(n_in), ptr(n_corr), ptr(best), ptr(ws), stream())
    elif method == "dlt_lo":
        call("di2p_pnp_ransac", ptr(pc), ptr(coarse), ptr(fine), ptr(pixels), ptr(K_scaled), int(W_fine), ptr(samples), iters,
             float(reproj_err), int(refine_rounds), int(refine_iters), F, N, ptr(P), ptr(ratio), ptr(n_in), ptr(n_corr), ptr(best), ptr(ws), stream())
    else:
        raise ValueError("method must be 'epnp' or 'dlt_lo'")
    out = dict(P=P, outlier_ratio=ratio, n_inliers=n_in, n_corr=n_corr, best=best)
    if return_workspace:
        out.update(workspace_views(ws, F, N, iters))
    return out


def solve_PnP(pc_np, coarse_predictions_np, fine_predictions_np, K_np, H, W, fine_resolution_scale, iterationsCount,
              method=None, rng=None, samples=None):
    """Reference signature (registration_pnp.py:95-96).  `fine_resolution_scale` is the reference's 1/32 factor
    (it multiplies H, W and K, :101-104).  `method`: None / cv2.SOLVEPNP_EPNP (the reference's choice) -> the EPnP RANSAC;
    the string "dlt_lo" selects the builder's 6-point DLT + locally optimised variant."""
    if not torch.cuda.is_available():
        raise RuntimeError("deepi2p_amd.registration_pnp needs a HIP device (there is no CPU fallback)")
    dev = torch.device("cuda", torch.cuda.current_device())
    Ws = W * fine_resolution_scale
    K_fine = camera_matrix_scaling(K_np, fine_resolution_scale)
    if int((np.asarray(coarse_predictions_np) == 1).sum()) < 4:          # :123 (points.shape[1] >= 4)
        return np.identity(4), 1
    if samples is None:
        rng = rng if rng is not None else np.random.default_rng()
        samples = draw_samples(rng, 1, int(iterationsCount))
    pc = torch.as_tensor(np.ascontiguousarray(pc_np, dtype=np.float32), device=dev).unsqueeze(0)
    co = torch.as_tensor(np.ascontiguousarray(coarse_predictions_np).astype(np.int32), device=dev).unsqueeze(0)
    fi = torch.as_tensor(np.ascontiguousarray(fine_predictions_np).astype(np.int32), device=dev).unsqueeze(0)
    Kt = torch.as_tensor(K_fine, device=dev).reshape(1, 3, 3)
    out = pnp_ransac(pc, co, fi, Kt, int(round(Ws)), torch.as_tensor(np.ascontiguousarray(samples, dtype=np.int32), device=dev),
                     method="dlt_lo" if method == "dlt_lo" else "epnp")
    ratio = float(out["outlier_ratio"][0])
    return out["P"][0].cpu().numpy(), (1 if ratio == 1.0 else ratio)


class PnPPipeline:
    """Device-resident labels -> pose by PnP for a batch of frames (the reference's second back end, registration_pnp.py:95-148): what
    RegistrationPipeline is for the Gauss-Newton solve, for pipeline.RegistrationExecutor.  Fixed per pipeline: the image size, the fine
    grid (fine_resolution_scale, the reference's 1/32), the RANSAC settings; per call: the frames, their labels, K and the draws.
    frame="enu" (z-up points): as in RegistrationPipeline -- the points are converted first, P_cam is the pose of the converted points and
    P = P_cam . P_convert that of the points as given."""

    def __init__(self, H, W, fine_resolution_scale=1 / 32, iterations=500, reproj_err=0.6, method="epnp", seed=0, frame="cam"):
        if method not in ("epnp", "dlt_lo"):
            raise ValueError("method must be 'epnp' or 'dlt_lo'")
        from . import evaluation
        self.enu, self.frame = bool(evaluation.check_frame(frame)), frame
        self._convert = {}
        self.H, self.W, self.scale = H, W, float(fine_resolution_scale)
        self.W_fine = int(round(W * self.scale))
        self.H_fine = int(round(H * self.scale))
        self.iterations, self.reproj_err, self.method = int(iterations), float(reproj_err), method
        self.rng = np.random.default_rng(seed)

    def draw(self, F, device):
        """RANSAC samples i32[F, iterations, 6] from the pipeline's seeded generator (draw_samples)."""
        return torch.as_tensor(draw_samples(self.rng, F, self.iterations), device=device)

    def scale_K(self, K):
        """camera_matrix_scaling of every frame's K f64[F,3,3], on the device (no host round trip; capture-safe)."""
        Ks = K.to(torch.float64) * self.scale
        Ks[:, 2, 2] = 1.0
        return Ks

    def __call__(self, pc, coarse, fine, K, samples, pixels=None):
        """pc f32[F,3,N], coarse / fine i32[F,N], K f64[F,3,3] (full-resolution camera), samples i32[F,iters,6]
        -> dict(P f64[F,4,4], outlier_ratio f64[F], n_inliers, n_corr, best i32[F]); a frame without an accepted pose comes back as identity
        with outlier ratio 1 (the reference's acceptance rules, registration_pnp.py:123-148, inside the kernels)."""
        if self.enu:
            from . import evaluation
            pc = evaluation.enu2cam_points(pc)
        out = pnp_ransac(pc, coarse, fine, self.scale_K(K), self.W_fine, samples, reproj_err=self.reproj_err, pixels=pixels,
                         method=self.method)
        if self.enu:
            from .registration import compose_convert
            out["P_cam"], out["P"] = out["P"], compose_convert(self._convert, out["P"])
        return out
