"""Host-side argument helpers of the ragged-batch front ends (scan_prep, submap, sweeps): one copy of what they check and allocate alike.
`prefix` is the module's name in its messages ("submap", "sweeps", "scan_prep"), `unit` its word for a batch entry ("sub-map", "frame")."""
import numpy as np
import torch

from . import _lib
from ._lib import DeepI2PHipError

MAX_FRAME_POINTS = 1 << 20          # rows of one batch entry: the voxel stage's limit (scan_prep.hip)


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def check_status(prefix, unit, table, status):
    """Raise DeepI2PHipError for a rejected entry (synchronises)."""
    st = status.cpu().numpy()
    bad = np.nonzero(st)[0]
    if len(bad):
        raise DeepI2PHipError("%s: %s %d rejected: %s" % (prefix, unit, int(bad[0]), table.get(int(st[bad[0]]), "status %d" % int(st[bad[0]]))))


def _check_max_frame_points(prefix, max_frame_points):
    if int(max_frame_points) < 0 or int(max_frame_points) > MAX_FRAME_POINTS:
        raise ValueError("%s: max_frame_points must be in [0, 2^20] (the voxel stage's limit)" % prefix)
    return int(max_frame_points)


def _offsets(prefix, x, name, length, dev):
    """device tensor: shape and dtype only (its values are checked on the device: status 3); host values: also non-decreasing from 0"""
    if torch.is_tensor(x) and x.is_cuda:
        return _check_tensor(prefix, x, name, torch.int32, (length,), "tensor")
    a = np.asarray(x.numpy() if torch.is_tensor(x) else x)
    if a.ndim != 1 or a.shape[0] != length or a.dtype.kind not in "iu":
        raise ValueError("%s: %s must be an integer array [%d]" % (prefix, name, length))
    if a[0] != 0 or np.any(np.diff(a.astype(np.int64)) < 0) or a[-1] >= 2 ** 31:
        raise ValueError("%s: %s must start at 0 and be non-decreasing (int32)" % (prefix, name))
    return torch.as_tensor(a.astype(np.int32)).to(dev or _dev())


def _check_tensor(prefix, t, name, dtype, shape, kind="device tensor"):
    """t must be a contiguous tensor of that dtype and shape; an entry of `shape` that is a string stands for any size"""
    if (not torch.is_tensor(t) or t.dtype != dtype or t.dim() != len(shape) or any(not isinstance(n, str) and m != n for m, n in zip(t.shape, shape))
            or not t.is_contiguous()):
        raise ValueError("%s: %s must be a contiguous %s %s [%s]" % (prefix, name, str(dtype).split(".")[1], kind, ", ".join(str(n) for n in shape)))
    return t


def workspace(entry, B, cap, device=None):
    """u8 device buffer of the bytes the C function `entry`(B, cap) asks for, at least 256"""
    return torch.empty((max(256, getattr(_lib.load(), entry)(B, cap)),), dtype=torch.uint8, device=device or _dev())
