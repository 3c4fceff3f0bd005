"""Evaluation on the device: pose errors, success statistics, ENU frames (csrc/eval.hip).

get_P_diff                  evaluation/registration_lsq.py:87-95            pose_errors / pose_errors_into
enu2cam                     evaluation/registration_lsq.py:237-248          enu2cam_points, P_CONVERT, frame="enu"
summary statistics          evaluation/registration_result_analysis.py:22-47,59,63      EvalAccumulator -> EvalState.summary() / line()

`registration.get_P_diff` stays the per-frame host function (numpy + scipy); this module is the batched device path that
pipeline.RegistrationExecutor(evaluate=True) captures into its step, so that a test-set run leaves the device once, for the summary.
"""
import dataclasses
import math

import numpy as np
import torch

from . import _lib
from ._lib import call, ptr, require_cuda, stream

FRAMES = ("cam", "enu")
# the reference's P_convert (registration_lsq.py:244-247): z-up (ENU) coordinates -> the camera convention (y down, z forward)
P_CONVERT = np.asarray([[1, 0, 0, 0], [0, 0, -1, 0], [0, 1, 0, 0], [0, 0, 0, 1]], dtype=np.float64)
BINS, RTE_RANGE, RRE_RANGE = 60, 15.0, 30.0          # the reference's plots, registration_result_analysis.py:59,63
LINE = "RTE %.2f +- %.2f, RRE %.2f +- %.2f, success rate %.2f"      # registration_result_analysis.py:43
# the accumulator's 8-byte words (include/deepi2p_hip.h, di2p_eval_accumulate)
_COUNTS = ("n", "n_valid", "n_success", "n_coarse", "n_fine", "rte_over", "rre_over")
_SUMS = ("rte_sum", "rte_sq", "rre_sum", "rre_sq", "coarse_sum", "fine_sum")
_SUM0, _HIST0, _WORDS = 8, 16, 16 + 2 * BINS


def check_frame(frame):
    """"cam" (the solver's own convention) or "enu" (z-up clouds: nuScenes); anything else raises ValueError.  -> 0 / 1"""
    if frame not in FRAMES:
        raise ValueError("frame must be 'cam' or 'enu', got %r" % (frame,))
    return FRAMES.index(frame)


def _gt_rows(P_pred, P_gt):
    F = P_pred.shape[0]
    if P_pred.dtype != torch.float64 or tuple(P_pred.shape) != (F, 4, 4):
        raise ValueError("pose_errors: P_pred must be f64 [F,4,4]")
    if P_gt.dtype != torch.float64 or P_gt.dim() != 3 or P_gt.shape[0] != F or P_gt.shape[1] not in (3, 4) or P_gt.shape[2] != 4:
        raise ValueError("pose_errors: P_gt must be f64 [F,3,4] or [F,4,4]")
    return F, int(P_gt.shape[1])


def pose_errors_into(P_pred, P_gt, cost, rte, rre, flags, frame="cam", t_thresh=2.0, r_thresh=5.0):
    """pose_errors with the outputs supplied (rte, rre f64[F], flags i32[F]): one launch, no allocation -- the form graphs capture."""
    enu = check_frame(frame)
    require_cuda(P_pred, P_gt, cost, rte, rre, flags)
    F, rows = _gt_rows(P_pred, P_gt)
    if cost is not None and (cost.dtype != torch.float64 or cost.numel() != F):
        raise ValueError("pose_errors: cost must be f64 [F]")
    if rte.dtype != torch.float64 or rre.dtype != torch.float64 or flags.dtype != torch.int32 or min(rte.numel(), rre.numel(), flags.numel()) < F:
        raise ValueError("pose_errors: outputs must be rte, rre f64[F] and flags i32[F]")
    call("di2p_pose_errors", ptr(P_pred), ptr(P_gt), rows, ptr(cost), enu, F, float(t_thresh), float(r_thresh), ptr(rte), ptr(rre), ptr(flags),
         stream())
    return rte, rre, flags


def pose_errors(P_pred, P_gt, cost=None, frame="cam", t_thresh=2.0, r_thresh=5.0):
    """get_P_diff for a batch, on the device.  P_pred f64[F,4,4], P_gt f64[F,3,4] or [F,4,4], cost f64[F] or None
    -> (rte f64[F] metres, rre f64[F] degrees, flags i32[F]: bit 0 valid = cost > 1e-6 (set when cost is None), bit 1 success = rte <
    t_thresh and rre < r_thresh).  frame="enu": both poses are those of z-up points and are taken into the converted frame first, where
    the reference measures them.  Within about 1e-3 degree of gimbal lock (the middle angle at +-90 degrees) rre is finite and no more.
    Allocates its outputs (the eager convenience)."""
    F = P_pred.shape[0]
    dev = P_pred.device
    rte = torch.empty((F,), dtype=torch.float64, device=dev)
    rre = torch.empty((F,), dtype=torch.float64, device=dev)
    flags = torch.empty((F,), dtype=torch.int32, device=dev)
    return pose_errors_into(P_pred, P_gt, cost, rte, rre, flags, frame, t_thresh, r_thresh)


def enu2cam_points(pc, out=None):
    """(x, y, z) -> (x, -z, y) for pc f32[B,3,N] (transform_pc_np(P_convert, pc)); exact.  out may be pc."""
    require_cuda(pc, out)
    if pc.dtype != torch.float32 or pc.dim() != 3 or pc.shape[1] != 3:
        raise ValueError("enu2cam_points: pc must be f32 [B,3,N]")
    out = torch.empty_like(pc) if out is None else out
    call("di2p_enu2cam_points", ptr(pc), ptr(out), pc.shape[0], pc.shape[2], stream())
    return out


def convert_matrices(F, device):
    """P_convert repeated for F frames, f64[F,4,4] on the device (the constant operand of di2p_compose_poses in the frame="enu" pipelines)"""
    return torch.as_tensor(np.tile(P_CONVERT, (F, 1, 1)), device=device)


@dataclasses.dataclass
class EvalState:
    """Host copy of an accumulator: integer counts, fp64 sums, two 60-bin histograms.  Everything is a sum, so states of several slots, devices
    or runs merge by addition."""
    n: int = 0                    # frames seen (frame mask != 0)
    n_valid: int = 0              # ... with cost > 1e-6: the frames the error statistics are over
    n_success: int = 0            # ... of these with rte < t_thresh and rre < r_thresh
    n_coarse: int = 0             # frames seen that brought a coarse / fine label accuracy (NaN: not counted)
    n_fine: int = 0
    rte_over: int = 0             # valid frames above the histogram's range
    rre_over: int = 0
    rte_sum: float = 0.0
    rte_sq: float = 0.0
    rre_sum: float = 0.0
    rre_sq: float = 0.0
    coarse_sum: float = 0.0
    fine_sum: float = 0.0
    rte_hist: np.ndarray = dataclasses.field(default_factory=lambda: np.zeros(BINS, np.int64))
    rre_hist: np.ndarray = dataclasses.field(default_factory=lambda: np.zeros(BINS, np.int64))

    @classmethod
    def from_words(cls, raw):
        """raw: the accumulator's bytes as a uint8 / int64 array"""
        words = np.ascontiguousarray(raw).view(np.int64).reshape(-1)
        if words.shape[0] != _WORDS:
            raise ValueError("EvalState: an accumulator has %d words, got %d" % (_WORDS, words.shape[0]))
        sums = words[_SUM0:_SUM0 + len(_SUMS)].view(np.float64)
        kw = {k: int(words[i]) for i, k in enumerate(_COUNTS)}
        kw.update({k: float(sums[i]) for i, k in enumerate(_SUMS)})
        return cls(rte_hist=words[_HIST0:_HIST0 + BINS].copy(), rre_hist=words[_HIST0 + BINS:_HIST0 + 2 * BINS].copy(), **kw)

    @classmethod
    def from_errors(cls, rte, rre, flags=None, frame_mask=None, accuracy=None, t_thresh=2.0, r_thresh=5.0):
        """The same fold on the host, in numpy fp64 (lists of errors that are on the host already)."""
        rte, rre = np.asarray(rte, np.float64).reshape(-1), np.asarray(rre, np.float64).reshape(-1)
        if flags is None:
            flags = 1 | (np.logical_and(rte < t_thresh, rre < r_thresh).astype(np.int32) << 1)
        flags = np.asarray(flags).reshape(-1)
        seen = np.ones(rte.shape, bool) if frame_mask is None else np.asarray(frame_mask).reshape(-1) != 0
        valid = seen & ((flags & 1) != 0)
        t, r = rte[valid], rre[valid]
        s = cls(n=int(seen.sum()), n_valid=int(valid.sum()), n_success=int((valid & ((flags & 2) != 0)).sum()),
                rte_sum=float(np.sum(t)), rte_sq=float(np.sum(t * t)), rre_sum=float(np.sum(r)), rre_sq=float(np.sum(r * r)),
                rte_hist=np.histogram(t, range=[0, RTE_RANGE], bins=BINS)[0].astype(np.int64),
                rre_hist=np.histogram(r, range=[0, RRE_RANGE], bins=BINS)[0].astype(np.int64))
        s.rte_over, s.rre_over = s.n_valid - int(s.rte_hist.sum()), s.n_valid - int(s.rre_hist.sum())
        if accuracy is not None:
            a = np.asarray(accuracy, np.float64).reshape(-1, 2)[seen]
            ok_c, ok_f = ~np.isnan(a[:, 0]), ~np.isnan(a[:, 1])
            s.n_coarse, s.n_fine, s.coarse_sum, s.fine_sum = int(ok_c.sum()), int(ok_f.sum()), float(a[ok_c, 0].sum()), float(a[ok_f, 1].sum())
        return s

    def merge(self, other):
        """-> a new state: the sum of both (pure Python / numpy, fp64)"""
        kw = {k: getattr(self, k) + getattr(other, k) for k in _COUNTS + _SUMS}
        return EvalState(rte_hist=self.rte_hist + other.rte_hist, rre_hist=self.rre_hist + other.rre_hist, **kw)

    def summary(self):
        """The paper's numbers over the valid frames: mean and sigma (the square root of the population variance, np.var) of both errors,
        the success rate as a fraction, the mean label accuracies over the frames seen, the histograms.  Empty sets give nan."""
        nan = float("nan")
        nv = self.n_valid

        def mean_sigma(s, sq):
            if nv == 0:
                return nan, nan
            m = s / nv
            return m, math.sqrt(max(sq / nv - m * m, 0.0))

        rte_mean, rte_sigma = mean_sigma(self.rte_sum, self.rte_sq)
        rre_mean, rre_sigma = mean_sigma(self.rre_sum, self.rre_sq)
        return dict(n=self.n, n_valid=nv, rte_mean=rte_mean, rte_sigma=rte_sigma, rre_mean=rre_mean, rre_sigma=rre_sigma,
                    success_rate=self.n_success / nv if nv else nan,
                    coarse_accuracy=self.coarse_sum / self.n_coarse if self.n_coarse else nan,
                    fine_accuracy=self.fine_sum / self.n_fine if self.n_fine else nan,
                    rte_hist=self.rte_hist.copy(), rre_hist=self.rre_hist.copy(), rte_overflow=self.rte_over, rre_overflow=self.rre_over)

    def line(self):
        """The reference's print (registration_result_analysis.py:43-47); the success rate in per cent."""
        s = self.summary()
        return LINE % (s["rte_mean"], s["rte_sigma"], s["rre_mean"], s["rre_sigma"], s["success_rate"] * 100)


class EvalAccumulator:
    """A device accumulator (di2p_eval_acc_bytes() bytes).  update() is one launch on the current stream, without allocation or
    synchronisation (capturable); frames are added in index order, so the state depends on the sequence of updates alone.  One accumulator
    belongs to one stream at a time: concurrent steps each get their own and merge on the host (EvalState.merge)."""

    def __init__(self, device):
        self.device = torch.device(device)
        nbytes = int(_lib.load().di2p_eval_acc_bytes())
        if nbytes != 8 * _WORDS:
            raise _lib.DeepI2PHipError("the library's accumulator has %d bytes, this binding reads %d" % (nbytes, 8 * _WORDS))
        self.buf = torch.zeros((_WORDS,), dtype=torch.int64, device=self.device)

    def update(self, rte, rre, flags, frame_mask=None, accuracy=None):
        """rte, rre f64[F], flags i32[F] (pose_errors' outputs), frame_mask i32[F] | None (0: the frame is skipped entirely), accuracy
        f32[F,2] | None (prep.label_accuracy's output)"""
        require_cuda(rte, rre, flags, frame_mask, accuracy)
        F = rte.numel()
        if rte.dtype != torch.float64 or rre.dtype != torch.float64 or flags.dtype != torch.int32 or rre.numel() != F or flags.numel() != F:
            raise ValueError("EvalAccumulator.update: rte, rre must be f64[F] and flags i32[F]")
        if frame_mask is not None and (frame_mask.dtype != torch.int32 or frame_mask.numel() != F):
            raise ValueError("EvalAccumulator.update: frame_mask must be i32[F]")
        if accuracy is not None and (accuracy.dtype != torch.float32 or tuple(accuracy.shape) != (F, 2)):
            raise ValueError("EvalAccumulator.update: accuracy must be f32[F,2]")
        call("di2p_eval_accumulate", ptr(rte), ptr(rre), ptr(flags), ptr(frame_mask), ptr(accuracy), F, ptr(self.buf), stream())

    def reset(self):
        call("di2p_eval_acc_reset", ptr(self.buf), stream())

    def state(self):
        """-> EvalState, a host copy (synchronises with the current stream)"""
        return EvalState.from_words(self.buf.cpu().numpy())
