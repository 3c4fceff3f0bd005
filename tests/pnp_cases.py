"""Shared by tests/test_epnp_host.py (CPU) and tests/test_gpu_pnp_stages.py (GPU): csrc/epnp.h built for the host, the committed RANSAC case
with its "clean" samples, and the fp64 numpy restatements of the PnP stages that are well posed given the stage before them (squared
reprojection errors, the strict / loose inlier band, the pose distance).  TEST INFRASTRUCTURE ONLY."""
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALE = 32
K_FINE = np.array([[350.0 / SCALE, 0, 256.0 / SCALE], [0, 350.0 / SCALE, 80.0 / SCALE], [0, 0, 1]])
W_FINE, H_FINE = 16, 5
REPROJ = 0.6
BAND = 1e-9              # relative half-width of the threshold band: fp64 e2 carries ~1e-13 relative error, this leaves four decades
T_TOL, R_TOL = 1e-5, 1e-6                                # "the same pose" for minimal samples: metres, radians
CASE_SEED = 2024
PLANTED = (7, 64, 200, 300)                              # hypotheses of every frame of the case whose sample repeats an index
TIE_STRIDE, TIE_COPIES = 256, 32                         # hypotheses 256 .. 287 of the case repeat the samples of hypotheses 0 .. 31


# ------------------------------------------------------------------------------------------------------------ epnp.h on the host
def load_epnp_host(tmpdir):
    """Build tests/epnp_host.cpp (csrc/epnp.h as plain C++, no contraction) into `tmpdir` and load it.  No GPU is involved."""
    from deepi2p_amd import build
    so = os.path.join(str(tmpdir), "libepnp_host.so")
    cmd = [build.HIPCC, "-x", "c++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-I", build.CSRC,
           os.path.join(ROOT, "tests", "epnp_host.cpp"), "-o", so]
    subprocess.check_call(cmd)
    lib = ctypes.CDLL(so)
    lib.epnp_host_solve.restype = None
    lib.epnp_host_solve.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 5
    return lib


def epnp_host(lib, X, uv, K):
    """X f64[sets, n, 3], uv f64[sets, n, 2] -> (R [sets,3,3], t [sets,3], err [sets], ok bool[sets]); NaN where not accepted."""
    X = np.ascontiguousarray(X, np.float64)
    uv = np.ascontiguousarray(uv, np.float64)
    sets, n = X.shape[0], X.shape[1]
    cam = np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]], np.float64)
    R, t, err = np.full((sets, 3, 3), np.nan), np.full((sets, 3), np.nan), np.full((sets,), np.nan)
    ok = np.zeros((sets,), np.int32)
    lib.epnp_host_solve(X.ctypes.data, uv.ctypes.data, n, sets, cam.ctypes.data, R.ctypes.data, t.ctypes.data, err.ctypes.data, ok.ctypes.data)
    return R, t, err, ok.astype(bool)


# ------------------------------------------------------------------------------------------------------------------- point sets
def _rotation(w):
    th = np.linalg.norm(w)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def exact_set(rng, n, K=K_FINE, noise=0.0):
    """n points in front of a camera with a random pose; X and uv rounded to f32 (what a correspondence record holds), returned as f64:
    X [n,3], uv [n,2] (exact projections + N(0, noise) pixels), P 4x4."""
    R = _rotation(rng.normal(0, 0.5, 3))
    t = np.array([rng.uniform(-2, 2), rng.uniform(-1, 1), rng.uniform(-2, 2)])
    pc = np.stack([rng.uniform(-10, 10, n), rng.uniform(-2, 3, n), rng.uniform(4, 40, n)])
    X = (R.T @ (pc - t[:, None])).astype(np.float32).astype(np.float64)
    cam = R @ X + t[:, None]
    uv = np.stack([K[0, 0] * cam[0] / cam[2] + K[0, 2], K[1, 1] * cam[1] / cam[2] + K[1, 2]])
    if noise:
        uv = uv + rng.normal(0, noise, uv.shape)
    P = np.eye(4)
    P[:3, :3], P[:3, 3] = R, t
    return X.T.copy(), uv.astype(np.float32).astype(np.float64).T.copy(), P


def pose_diff(Ra, ta, Rb, tb):
    """(|ta - tb|, rotation angle between Ra and Rb); the angle from the chord |Ra - Rb|_F = 2 sqrt(2) |sin(angle / 2)|, accurate near 0"""
    chord = np.linalg.norm(np.asarray(Ra) - np.asarray(Rb)) / (2 * np.sqrt(2))
    return float(np.linalg.norm(np.asarray(ta) - np.asarray(tb))), float(2 * np.arcsin(min(chord, 1.0)))


def proper_rotation(R, tol=1e-9):
    R = np.asarray(R)
    return bool(np.all(np.isfinite(R)) and np.abs(R @ R.T - np.eye(3)).max() <= tol and np.linalg.det(R) > 0)


# --------------------------------------------------------------------------------------------------------------- the RANSAC case
def reduce_samples(samples, cnt):
    """the device's `s % cnt; if (s < 0) s += cnt` is numpy's floored modulo"""
    return np.asarray(samples, np.int64) % cnt


def make_case(seed=CASE_SEED, F=3, N=700, iters=301, outliers=0.2):
    """F frames of N points, about half of them correspondences (coarse = 1); exact projections rounded to f32, `outliers` of the
    correspondences replaced by uniform pixels; samples i32[F, iters, 6] over the full int32 range, the hypotheses PLANTED given a repeated
    index among their first five entries, hypotheses 256 .. 287 given the samples of 0 .. 31 (ties inside one thread of the strided argmax).  clean5 / clean6 [F, iters]: the first five / all six reduced indices distinct and true inliers."""
    rng = np.random.default_rng(seed)
    pc, px, co, Ps, inl = [], [], [], [], []
    for f in range(F):
        X, uv, P = exact_set(rng, N)
        c = (rng.random(N) < 0.5).astype(np.int32)
        bad = (rng.random(N) < outliers) & (c == 1)
        uv[bad] = np.stack([rng.uniform(0, W_FINE, int(bad.sum())), rng.uniform(0, H_FINE, int(bad.sum()))], axis=1)
        pc.append(X.T.astype(np.float32)), px.append(uv.T.astype(np.float32)), co.append(c), Ps.append(P)
        inl.append(~bad[c == 1])                                     # per packed record: a true inlier
    samples = rng.integers(-2 ** 31, 2 ** 31, size=(F, iters, 6), dtype=np.int64).astype(np.int32)
    for it in PLANTED:
        if it < iters:
            samples[:, it, 3] = samples[:, it, 1]
    if iters >= TIE_STRIDE + TIE_COPIES:         # equal samples one argmax stride apart: equal counts in ONE thread of the select kernels
        samples[:, TIE_STRIDE:TIE_STRIDE + TIE_COPIES] = samples[:, :TIE_COPIES]
    cnt = np.array([int(c.sum()) for c in co])
    clean5, clean6 = np.zeros((F, iters), bool), np.zeros((F, iters), bool)
    for f in range(F):
        idx = reduce_samples(samples[f], cnt[f])
        for it in range(iters):
            i5, i6 = idx[it, :5], idx[it]
            clean5[f, it] = len(set(i5.tolist())) == 5 and inl[f][i5].all()
            clean6[f, it] = len(set(i6.tolist())) == 6 and inl[f][i6].all()
    return dict(pc=np.stack(pc), pixels=np.stack(px), coarse=np.stack(co), K=np.stack([K_FINE] * F), samples=samples, P_gt=np.stack(Ps),
                inlier=inl, cnt=cnt, clean5=clean5, clean6=clean6, F=F, N=N, iters=iters)


def case_records(case, f):
    """what the pack stage leaves for frame f, computed on the host: X [cnt,3], uv [cnt,2] (f64 values of the f32 records)"""
    m = case["coarse"][f] == 1
    return case["pc"][f][:, m].T.astype(np.float64), case["pixels"][f][:, m].T.astype(np.float64)


# ---------------------------------------------------------------------------------------------------------- stages in fp64 numpy
def reproj_e2(X, uv, K, R, t):
    """squared reprojection errors and depths of records X [n,3], uv [n,2] under (R, t)"""
    p = X @ np.asarray(R).T + np.asarray(t)
    with np.errstate(divide="ignore", invalid="ignore"):
        du = K[0, 0] * p[:, 0] / p[:, 2] + K[0, 2] - uv[:, 0]
        dv = K[1, 1] * p[:, 1] / p[:, 2] + K[1, 2] - uv[:, 1]
    return du * du + dv * dv, p[:, 2]


def band_masks(X, uv, K, R, t, method, thr=REPROJ):
    """(strict, loose) inlier masks of each method's rule with the threshold moved by -/+ BAND: EPnP `e2 <= thr2`, no depth test;
    DLT `e2 < thr2` and depth > 1e-9.  A correct count lies between their sums."""
    e2, z = reproj_e2(X, uv, K, R, t)
    thr2 = thr * thr
    with np.errstate(invalid="ignore"):
        strict, loose = e2 <= thr2 * (1 - BAND), e2 <= thr2 * (1 + BAND)
        if method == "dlt_lo":
            strict, loose = (e2 < thr2 * (1 - BAND)) & (z > 1e-9 * (1 + BAND)), (e2 < thr2 * (1 + BAND)) & (z > 1e-9 * (1 - BAND))
    return strict, loose


# ------------------------------------------------------------------------- stage rules on the device's own intermediates (GPU tests)
# EPnP re-fit on the inliers of the winner, csrc/epnp.h compiled for the host vs oracle/epnp_np.epnp, measured on the CPU on the committed
# cases (the three frames of make_case(), 261-286 inliers, and the three N = 4096 frames of tests/test_pnp.py, 689-747 inliers):
# worst |dt| 2.21e-13 m, worst |dR| 4.32e-14 rad.  The device bound is 1000 x that: the margin covers the wave-butterfly summation order and
# FMA contraction of the device build.  It may not exceed 1e-8.
REFIT_MEASURED = (2.21e-13, 4.32e-14)
REFIT_BOUND = (1000 * REFIT_MEASURED[0], 1000 * REFIT_MEASURED[1])
# fewer than 50 inliers: the header-vs-oracle error grows as the system loses redundancy (n = 6: 2.52e-10 m measured, tests/test_epnp_host.py);
# there the cap itself is the bound (40 x that measurement)
REFIT_BOUND_SMALL = (1e-8, 1e-8)
assert max(REFIT_BOUND) <= 1e-8
MSIZE = {"epnp": 5, "dlt_lo": 6}


def run_device(dev, pc_, pixels, coarse, K, samples, method, fine=None, W_fine=W_FINE, reproj_err=REPROJ):
    """pnp_ransac(..., return_workspace=True) on numpy inputs -> every output and every intermediate as a numpy array"""
    import torch
    from deepi2p_amd import registration_pnp as rp
    F, _, N = pc_.shape
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    fi = torch.zeros((F, N), dtype=torch.int32, device=dev) if fine is None else t(fine)
    out = rp.pnp_ransac(t(pc_), t(coarse), fi, t(K), W_fine, t(samples), reproj_err=reproj_err, pixels=None if pixels is None else t(pixels),
                        method=method, return_workspace=True)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def min_sample(method, cnt):
    return 6 if method == "dlt_lo" else (5 if cnt >= 5 else 4)


def device_records(o, f):
    cnt = int(o["n_corr"][f])
    rec = o["corr"][f, :cnt].astype(np.float64)
    return rec[:, :3], rec[:, 3:5]


def check_hypothesis_rules(o, f, samples, method):
    """stage B without a reference: the valid flag is 0 where the rules say so; every valid hypothesis is a finite proper rotation"""
    cnt, iters = int(o["n_corr"][f]), samples.shape[0]
    hyp = o["hyp"][f]
    flag = hyp[:, 12]
    assert np.all((flag == 0.0) | (flag == 1.0))
    if cnt < (6 if method == "dlt_lo" else 4):
        assert not flag.any(), (method, f, cnt)
        return
    if method == "epnp":
        m = min_sample(method, cnt)
        idx = reduce_samples(samples[:, :m], cnt)
        repeated = np.array([len(set(r.tolist())) < m for r in idx])
        assert not flag[repeated].any(), (f, np.nonzero(repeated & (flag != 0))[0])
    for it in np.nonzero(flag)[0]:
        assert np.all(np.isfinite(hyp[it, :12])) and proper_rotation(hyp[it, :9].reshape(3, 3)), (method, f, it)


def check_score(o, f, K, method, thr=REPROJ):
    """stage C: every valid device hypothesis re-scored in fp64 on the device's records; -> (sum of band widths, sum of counts)"""
    X, uv = device_records(o, f)
    hyp, inl = o["hyp"][f], o["inliers"][f]
    width = total = 0
    for it in range(hyp.shape[0]):
        if hyp[it, 12] == 0.0:
            assert inl[it] == -1, (method, f, it, inl[it])
            continue
        strict, loose = band_masks(X, uv, K, hyp[it, :9].reshape(3, 3), hyp[it, 9:12], method, thr)
        lo, hi = int(strict.sum()), int(loose.sum())
        assert lo <= inl[it] <= hi, (method, f, it, lo, int(inl[it]), hi)
        width += hi - lo
        total += int(inl[it])
    return width, total


def check_select(o, f, method):
    """stage D: best = the lowest index among the maxima of the device's counts; no model -> identity, ratio 1, 0 inliers, best -1.
    -> True when the frame has a model"""
    cnt, inl = int(o["n_corr"][f]), o["inliers"][f]
    top = int(inl.max())
    if cnt < (6 if method == "dlt_lo" else 4) or top < min_sample(method, cnt):
        assert int(o["best"][f]) == -1 and int(o["n_inliers"][f]) == 0 and float(o["outlier_ratio"][f]) == 1.0, (method, f)
        assert np.array_equal(o["P"][f], np.eye(4)), (method, f)
        return False
    best = int(np.nonzero(inl == top)[0][0])
    assert int(o["best"][f]) == best, (method, f, int(o["best"][f]), best)
    if method == "epnp":
        assert int(o["n_inliers"][f]) == top, (f, int(o["n_inliers"][f]), top)
    else:
        assert int(o["n_inliers"][f]) >= top, (f, int(o["n_inliers"][f]), top)
    return True


def check_acceptance(o, f, R, t):
    """the last step of both select kernels, given the final model (R, t): |t| < 14.14 -> P = [R t], ratio = 1 - n_inliers / n_corr exactly
    (the same two fp64 operations); else identity and ratio 1.  -> accepted"""
    if np.linalg.norm(t) < 14.14:
        assert float(o["outlier_ratio"][f]) == 1.0 - int(o["n_inliers"][f]) / int(o["n_corr"][f]), f
        return True
    assert np.array_equal(o["P"][f], np.eye(4)) and float(o["outlier_ratio"][f]) == 1.0, f
    return False


def check_epnp_final(o, f, K):
    """stage E (EPnP), for a frame with a model: the mask between the strict and the loose mask of the winning device hypothesis, its sum
    within the band width of n_inliers, and P = oracle EPnP on the DEVICE's masked records (REFIT_BOUND; fewer than 6 masked records:
    the four eigenvectors are a null-space basis and only the invariants hold).  -> (|dt|, |dR|) or None when the pose was rejected"""
    from oracle import epnp_np
    X, uv = device_records(o, f)
    cnt, b = X.shape[0], int(o["best"][f])
    h = o["hyp"][f, b]
    assert h[12] == 1.0
    strict, loose = band_masks(X, uv, K, h[:9].reshape(3, 3), h[9:12], "epnp")
    mask = o["mask"][f, :cnt]
    assert np.all((mask == 0) | (mask == 1))
    mask = mask.astype(bool)
    assert np.all(strict <= mask) and np.all(mask <= loose), (f, int(strict.sum()), int(mask.sum()), int(loose.sum()))
    assert abs(int(mask.sum()) - int(o["n_inliers"][f])) <= int(loose.sum()) - int(strict.sum()), f
    P = o["P"][f]
    if np.array_equal(P, np.eye(4)):                 # rejected: the re-fit (or, should it fail, the winner) is 14.14 m or more away
        assert float(o["outlier_ratio"][f]) == 1.0
        sol = epnp_np.epnp(X[mask].T, uv[mask].T, K) if mask.sum() >= 6 else None
        if sol is not None:
            assert np.linalg.norm(sol[1]) >= 14.14 - 1e-6, (f, np.linalg.norm(sol[1]))
        return None
    assert proper_rotation(P[:3, :3]) and np.all(np.isfinite(P)) and np.array_equal(P[3], [0, 0, 0, 1])
    assert check_acceptance(o, f, P[:3, :3], P[:3, 3])
    if mask.sum() < 6:
        return None
    sol = epnp_np.epnp(X[mask].T, uv[mask].T, K)
    assert sol is not None, f
    dt, dr = pose_diff(P[:3, :3], P[:3, 3], sol[0], sol[1])
    bt, br = REFIT_BOUND if mask.sum() >= 50 else REFIT_BOUND_SMALL
    print("frame %d: %d masked records, P vs oracle re-fit |dt| %.3g m |dR| %.3g rad" % (f, int(mask.sum()), dt, dr))
    assert dt <= bt and dr <= br, (f, int(mask.sum()), dt, dr)
    return dt, dr


def dlt_refine_from(X, uv, K, R, t, nin, rounds=20, iters=5):
    """oracle/pnp_np.py's locally optimised loop started from (R, t, nin) -> (R, t, nin, ambiguous); ambiguous: in some round a record's
    error lay inside the threshold band, so the device may legitimately have taken the other branch"""
    from oracle import pnp_np
    Xc, uc = X.T, uv.T
    ambiguous = False
    for _ in range(rounds):
        strict, loose = band_masks(X, uv, K, R, t, "dlt_lo")
        ambiguous |= bool((strict != loose).any())
        R1, t1 = pnp_np.refine(Xc, uc, K, R, t, pnp_np.inlier_mask(Xc, uc, K, R, t, REPROJ), iters)
        strict, loose = band_masks(X, uv, K, R1, t1, "dlt_lo")
        ambiguous |= bool((strict != loose).any())
        c1 = int(pnp_np.inlier_mask(Xc, uc, K, R1, t1, REPROJ).sum())
        if c1 < nin:
            break
        R, t, nin = R1, t1, c1
    return R, t, nin, ambiguous


def check_dlt_final(o, f, K, rounds=20, iters=5):
    """stage E (DLT), for a frame with a model: n_inliers >= the winner's count and inside the band count of the returned pose; P = the
    oracle's refinement loop started from the DEVICE's winning hypothesis, within 1e-8.  -> False when the frame is left out (ambiguous)"""
    X, uv = device_records(o, f)
    b = int(o["best"][f])
    h = o["hyp"][f, b]
    assert h[12] == 1.0 and int(o["n_inliers"][f]) >= int(o["inliers"][f, b])
    R, t, nin, ambiguous = dlt_refine_from(X, uv, K, h[:9].reshape(3, 3), h[9:12].copy(), int(o["inliers"][f, b]), rounds, iters)
    if ambiguous:
        return False
    assert int(o["n_inliers"][f]) == nin, (f, int(o["n_inliers"][f]), nin)
    P = o["P"][f]
    if check_acceptance(o, f, R, t):
        strict, loose = band_masks(X, uv, K, P[:3, :3], P[:3, 3], "dlt_lo")
        assert int(strict.sum()) <= int(o["n_inliers"][f]) <= int(loose.sum()), f
        dt, dr = pose_diff(P[:3, :3], P[:3, 3], R, t)
        print("frame %d: P vs oracle refinement from the device's winner |dt| %.3g m |dR| %.3g rad" % (f, dt, dr))
        assert dt <= 1e-8 and dr <= 1e-8, (f, dt, dr)
    return True
