"""CPU: csrc/epnp.h compiled as plain C++ (tests/epnp_host.cpp; no contraction, no GPU) against oracle/epnp_np.py on the same points.

What can be compared and what cannot ("PnP: what is pinned"): with six or more noisy points M^T M has full rank, the four
smallest eigenvectors are determined and the two implementations agree to 1e-10; with five points two of the four span an exact null
space, the pose of EXACT data does not depend on the basis, the pose of noisy data does.  So the header is pinned here on n >= 6 noisy
points and on five-point samples of true inliers, and the GPU stage tests (tests/test_gpu_pnp_stages.py) compare device hypotheses with
the oracle on those "clean" samples only."""
import numpy as np
import pytest

from oracle import epnp_np
from tests import pnp_cases as pc

K = pc.K_FINE
# n -> (sets, seed, measured max |dt| [m], measured max |dR| [rad]) of header vs epnp_np.epnp on the committed seeds, 0.2 px noise
NOISY = {6: (200, 106, 2.52e-10, 3.8e-12), 7: (200, 107, 1.34e-12, 1.54e-13), 50: (50, 150, 8.13e-13, 4.67e-14),
         2000: (50, 1200, 6.79e-13, 6.79e-14)}


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return pc.load_epnp_host(tmp_path_factory.mktemp("epnp_host"))


def _versus_oracle(host, X, uv, check_err=False):
    """header vs oracle on point sets X [sets,n,3], uv [sets,n,2]: (|dt|, |dR|) per set; both must accept every set"""
    R, t, err, ok = pc.epnp_host(host, X, uv, K)
    d = np.empty((X.shape[0], 2))
    for s in range(X.shape[0]):
        o = epnp_np.epnp(X[s].T, uv[s].T, K)
        assert ok[s] and o is not None, s
        d[s] = pc.pose_diff(R[s], t[s], o[0], o[1])
        if check_err:                  # the mean reprojection error it reports (pixels; a pose shift of dt metres moves it by < 10 dt)
            assert abs(err[s] - o[2]) <= 1e-9 * o[2] + 10 * d[s, 0], (s, err[s], o[2])
    return d


@pytest.mark.parametrize("n", sorted(NOISY))
def test_header_matches_oracle_on_noisy_points(host, n):
    """n points, exact projections + N(0, 0.2 px), observations rounded to f32; the reference is oracle/epnp_np.epnp (numpy eigh / SVD /
    lstsq where the header has cyclic Jacobi / Newton polar iteration / Householder QR).
    Measured on the committed seeds, header vs oracle, max over the sets:
        n = 6 (200 sets)    |dt| 2.52e-10 m   |dR| 3.8e-12 rad
        n = 7 (200 sets)    |dt| 1.34e-12 m   |dR| 1.54e-13 rad
        n = 50 (50 sets)    |dt| 8.13e-13 m   |dR| 4.67e-14 rad
        n = 2000 (50 sets)  |dt| 6.79e-13 m   |dR| 6.79e-14 rad
    Asserted: 100 x the measured maximum of that n (margin for another LAPACK build behind numpy), never more than 1e-7."""
    sets, seed, dt_meas, dr_meas = NOISY[n]
    rng = np.random.default_rng(seed)
    S = [pc.exact_set(rng, n, noise=0.2) for _ in range(sets)]
    d = _versus_oracle(host, np.stack([s[0] for s in S]), np.stack([s[1] for s in S]), check_err=True)
    print("n = %d: max |dt| %.3g m, max |dR| %.3g rad" % (n, d[:, 0].max(), d[:, 1].max()))
    dt_bound, dr_bound = 100 * dt_meas, 100 * dr_meas
    assert dt_bound <= 1e-7 and dr_bound <= 1e-7
    assert d[:, 0].max() <= dt_bound and d[:, 1].max() <= dr_bound, (n, d.max(axis=0))


def test_header_recovers_the_pose_of_exact_points(host):
    """exact projections (f32-rounded observations), n = 5, 6, 50: the header alone finds the ground truth -- five exact points determine
    the pose whatever basis the eigen-solver returns for the null space (1e-3 m / 1e-4 rad: f32 pixels at 11 px focal length)"""
    rng = np.random.default_rng(8)
    for n in (5, 6, 50):
        S = [pc.exact_set(rng, n) for _ in range(40)]
        R, t, err, ok = pc.epnp_host(host, np.stack([s[0] for s in S]), np.stack([s[1] for s in S]), K)
        good = 0
        for s in range(len(S)):
            dt, dr = pc.pose_diff(R[s], t[s], S[s][2][:3, :3], S[s][2][:3, 3])
            good += bool(ok[s] and dt < 1e-3 and dr < 1e-4)
        assert good >= len(S) - 1, (n, good)        # one near-degenerate minimal sample in forty may miss


def test_case_generator_and_clean_samples(host):
    """The committed RANSAC case of the GPU stage tests: F = 3, N = 700, about half the points correspondences, 20 % of them uniform
    pixels, samples over the whole int32 range.  On its CLEAN samples (five distinct true inliers) header and oracle give the same pose
    (within 1e-5 m and 1e-6 rad) for all but at most 1.5 % -- measured on the committed seed: 0 of 270 differ (max 4.1e-7 m / 3.4e-9 rad);
    on 400 exact five-point sets 0.25 % differ by more than 1e-6 m.  This share, verified here for the oracle and the header alone, is
    what licenses the 3 % cap of the device comparison (twice this bound)."""
    case = pc.make_case()
    F, N, iters = case["F"], case["N"], case["iters"]
    assert (F, N, iters) == (3, 700, 301) and case["samples"].dtype == np.int32 and case["samples"].shape == (F, iters, 6)
    assert (case["samples"] < 0).mean() > 0.4 and case["samples"].min() < -2 ** 30 and case["samples"].max() > 2 ** 30
    assert all(0.4 * N < c < 0.6 * N and c % 64 != 0 for c in case["cnt"]) and len(set(case["cnt"].tolist())) == F
    for f in range(F):
        assert 0.15 < 1 - case["inlier"][f].mean() < 0.25
        idx = pc.reduce_samples(case["samples"][f], case["cnt"][f])
        for it in pc.PLANTED:
            assert len(set(idx[it, :5].tolist())) < 5 and not case["clean5"][f, it] and not case["clean6"][f, it]
    assert case["clean5"].sum() >= 100 and case["clean6"].sum() >= 100
    total = differ = 0
    worst = np.zeros(2)
    for f in range(F):
        X, uv = pc.case_records(case, f)
        idx = pc.reduce_samples(case["samples"][f], case["cnt"][f])
        its = np.nonzero(case["clean5"][f])[0]
        d = _versus_oracle(host, np.stack([X[idx[it, :5]] for it in its]), np.stack([uv[idx[it, :5]] for it in its]))
        differ += int(((d[:, 0] > pc.T_TOL) | (d[:, 1] > pc.R_TOL)).sum())
        total += len(its)
        worst = np.maximum(worst, d.max(axis=0))
    print("clean samples: %d, differing: %d, worst |dt| %.3g m |dR| %.3g rad" % (total, differ, worst[0], worst[1]))
    assert differ <= 0.015 * total, (differ, total)


def test_five_noisy_points_are_not_comparable(host):
    """DOCUMENTATION OF A FINDING, not a comparison.  With five points M (10 x 12) leaves M^T M a null space of dimension >= 2: two of the
    "four smallest eigenvectors" are an arbitrary basis of it, fixed only by the eigen-solver's rounding (cyclic Jacobi in the header, LAPACK
    behind numpy's eigh in the oracle).  On exact data every basis represents the same pose; with 0.2 px noise the betas fitted to the basis
    -- and so the pose -- depend on it.  Measured on 400 such sets: 60 % of the poses differ by more than 1e-6 m, median 1.9e-5 m, 90th
    percentile 0.63 m.  A RANSAC hypothesis from a five-point sample that holds an outlier is therefore NOT a function of the input that a
    restatement (or another compiler) reproduces.  What holds for any basis, and is asserted: both return finite proper rotations."""
    rng = np.random.default_rng(5)
    S = [pc.exact_set(rng, 5, noise=0.2) for _ in range(400)]
    X, uv = np.stack([s[0] for s in S]), np.stack([s[1] for s in S])
    R, t, err, ok = pc.epnp_host(host, X, uv, K)
    for s in range(len(S)):
        if ok[s]:
            assert pc.proper_rotation(R[s]) and np.all(np.isfinite(t[s])) and np.isfinite(err[s]), s
        o = epnp_np.epnp(X[s].T, uv[s].T, K)
        if o is not None:
            assert pc.proper_rotation(o[0]) and np.all(np.isfinite(o[1])), s
    assert ok.mean() > 0.9


def _collinear(rng, n, K):
    _, uv, P = pc.exact_set(rng, n)
    p0, d = rng.uniform(-3, 3, 3) + np.array([0, 0, 15.0]), rng.normal(0, 1, 3)
    X = p0 + rng.uniform(-4, 4, n)[:, None] * d
    cam = X @ P[:3, :3].T + P[:3, 3]
    return X, np.stack([K[0, 0] * cam[:, 0] / cam[:, 2] + K[0, 2], K[1, 1] * cam[:, 1] / cam[:, 2] + K[1, 2]], axis=1), uv


def test_degenerate_sets_are_refused(host):
    """fewer than four points, coincident points, collinear points (on a coordinate axis: exactly rank one; in general position: rank one
    to rounding, the case an absolute determinant test let through with an arbitrary pose): ok == false, and whatever IS accepted holds
    no NaN.  Near-degenerate sets (collinear only to f32 rounding) may be accepted; they must then be finite."""
    rng = np.random.default_rng(11)
    for n in (1, 2, 3):
        X, uv, _ = pc.exact_set(rng, n)
        assert not pc.epnp_host(host, X[None], uv[None], K)[3][0], n
    accepted = 0
    for n in (4, 5, 6, 50):
        Xs, uvs = [], []
        for trial in range(100):
            X, uv, _ = pc.exact_set(rng, n)
            Xs += [np.repeat(X[:1], n, axis=0)] * 2                     # coincident: one observation, and n different ones
            uvs += [np.repeat(uv[:1], n, axis=0), uv]
            Xl, uvl, uvo = _collinear(rng, n, K)                        # a line in general position: its own projections, and others
            Xs += [Xl, Xl]
            uvs += [uvl, uvo]
            Xa = np.zeros((n, 3))                                       # a line along x
            Xa[:, 0], Xa[:, 2] = rng.uniform(-4, 4, n), 10.0
            Xs.append(Xa), uvs.append(uv)
        R, t, err, ok = pc.epnp_host(host, np.stack(Xs), np.stack(uvs), K)
        assert not ok.any(), (n, np.nonzero(ok)[0])
        # collinear up to the f32 rounding of the coordinates: a (badly conditioned) 3-D configuration
        Xs, uvs = [], []
        for trial in range(100):
            Xl, uvl, _ = _collinear(rng, n, K)
            Xs.append(Xl.astype(np.float32).astype(np.float64)), uvs.append(uvl.astype(np.float32).astype(np.float64))
        R, t, err, ok = pc.epnp_host(host, np.stack(Xs), np.stack(uvs), K)
        for s in np.nonzero(ok)[0]:
            assert np.all(np.isfinite(R[s])) and np.all(np.isfinite(t[s])) and np.isfinite(err[s]), (n, s)
        accepted += int(ok.sum())
    assert accepted > 0              # the last loop is not vacuous
