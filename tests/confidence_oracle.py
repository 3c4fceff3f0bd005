"""Numpy fp64 references of the pose-confidence entry points (csrc/solver_aux.hip: di2p_pose_information, di2p_pose_covariance,
di2p_restart_consensus).  Helper of tests/test_confidence_host.py and tests/test_gpu_confidence.py; no tests here.

The residuals and Jacobians are the oracle's (oracle/frustum_lm.cpp, dual numbers: uncorrected rows in point order); this file only groups
them into blocks, weights them and sums."""
import numpy as np

from oracle import frustum_lm as flm

EPS = np.finfo(np.float64).eps


def npar(is_2d):
    return 4 if is_2d else 6


def information(points, labels, K, H, W, is_2d, params):
    """-> dict(A [np,np], g [np], g_abs [np] = sum of |terms| of g, cost, active [2]) at `params`; points [3,N] (any float type, widened)"""
    pts = np.asarray(points).astype(np.float64)
    lab = np.asarray(labels).astype(np.int32)
    n = npar(is_2d)
    r, J, cost = flm.residuals_and_jacobian(pts, lab, K, H, W, is_2d, params)
    used = lab[(lab == 0) | (lab == 1)]
    if used.size == 0:
        return dict(A=np.zeros((n, n)), g=np.zeros(n), g_abs=np.zeros(n), cost=0.0, active=np.zeros(2, np.int32))
    sizes = np.where(used == 1, 3, 1)                                   # a label-1 point is a block of 3 rows, a label-0 point of 1
    s = np.add.reduceat(r * r, np.r_[0, np.cumsum(sizes)[:-1]])
    w = np.repeat(1.0 / (1.0 + s), sizes)                               # rho'(s) of the row's block
    Jw = J * w[:, None]
    active = np.array([np.count_nonzero((s != 0) & (sizes == 3)), np.count_nonzero((s != 0) & (sizes == 1))], np.int32)
    return dict(A=Jw.T @ J, g=Jw.T @ r, g_abs=np.abs(Jw).T @ np.abs(r), cost=cost, active=active)


def covariance(info, params, lb, ub, is_2d, has_inside=1):
    """-> dict(cov [np,np], free_mask, status, sigma_t, sigma_r) by the rules of di2p_pose_covariance, the inverse by numpy.linalg.inv"""
    n, toff = npar(is_2d), (1 if is_2d else 3)
    info, params = np.asarray(info, np.float64), np.asarray(params, np.float64)
    free = np.ones(n, bool)
    for i in range(3):
        if params[toff + i] == lb[i] or params[toff + i] == ub[i]:
            free[toff + i] = False
    mask = int(sum(1 << i for i in range(n) if free[i]))
    idx = np.nonzero(free)[0]
    status = 0
    if has_inside == 0 or not np.all(np.isfinite(info)) or not np.all(np.isfinite(params)):
        status = 2
    elif idx.size == 0:
        status = 1
    else:
        Af = info[np.ix_(idx, idx)]
        tiny = n * EPS * np.max(np.diag(Af))
        L = np.zeros_like(Af)
        for i in range(idx.size):                                       # the pivots of the Cholesky factorisation, in order
            for j in range(i + 1):
                v = Af[i, j] - L[i, :j] @ L[j, :j]
                if i == j:
                    if not v > tiny:
                        status = 1
                    L[i, i] = np.sqrt(v) if v > 0 else np.nan
                else:
                    L[i, j] = v / L[j, j]
            if status:
                break
    nan = float("nan")
    if status:
        return dict(cov=np.full((n, n), nan), free_mask=mask, status=status, sigma_t=nan, sigma_r=nan)
    cov = np.zeros((n, n))
    cov[np.ix_(idx, idx)] = np.linalg.inv(Af)
    d = np.diag(cov)
    return dict(cov=cov, free_mask=mask, status=0, sigma_t=float(np.sqrt(d[toff:].sum())), sigma_r=float(np.sqrt(d[:toff].sum()) * 180.0 / np.pi))


def rotation(x, is_2d):
    """The solver's rotation of a parameter vector (angle-axis; [0, ry, 0] for the 2-D solver)"""
    from scipy.spatial.transform import Rotation
    w = np.array([0.0, x[0], 0.0]) if is_2d else np.asarray(x[0:3], np.float64)
    return Rotation.from_rotvec(w).as_matrix()


def pose(x, is_2d):
    P = np.eye(4)
    P[:3, :3] = rotation(x, is_2d)
    P[:3, 3] = x[1:4] if is_2d else x[3:6]
    return P


def consensus(params, cost, best, is_2d, t_tol, r_tol_deg, has_inside=1):
    """params [R,np], cost [R], best -> (finite, agree, gap) of one frame by flm.get_P_diff on P_r^-1 P_best"""
    if has_inside == 0 or best < 0:
        return 0, 0, float("nan")
    Pb = pose(params[best], is_2d)
    finite = agree = 0
    other = np.inf
    for r in range(cost.shape[0]):
        if not np.isfinite(cost[r]):
            continue
        finite += 1
        t, a = flm.get_P_diff(pose(params[r], is_2d), Pb)
        if t < t_tol and a < r_tol_deg:
            agree += 1
        else:
            other = min(other, cost[r])
    return finite, agree, other - cost[best]


def plane_margins(points, labels, K, params, H, W, is_2d=None):
    """The smallest |pix_x|, |pix_x - (W-1)|, |pix_y|, |pix_y - (H-1)| and |p2| over all points: how far the nearest point is from a plane
    at which its residual block switches.  is_2d defaults to what len(params) says."""
    params = np.asarray(params, np.float64)
    is_2d = (params.shape[0] == 4) if is_2d is None else is_2d
    pts = np.asarray(points).astype(np.float64)
    p = rotation(params, is_2d) @ pts + (params[1:4] if is_2d else params[3:6])[:, None]
    px = K[0, 0] * p[0] / p[2] + K[0, 2]
    py = K[1, 1] * p[1] / p[2] + K[1, 2]
    return float(min(np.abs(px).min(), np.abs(px - (W - 1)).min(), np.abs(py).min(), np.abs(py - (H - 1)).min(), np.abs(p[2]).min()))
