"""GPU: the PnP back end (csrc/pnp.hip, csrc/epnp.h) stage by stage, each stage checked on the DEVICE's OWN input to it.

pack -> hypotheses -> score -> select (+ re-fit / refinement): both RANSAC entry points leave every intermediate in their workspace
(registration_pnp.workspace_views).  A hypothesis from a minimal EPnP sample that holds an outlier is not a function of the input that
a restatement reproduces (tests/test_epnp_host.py), so nothing here compares the pipeline's end with an oracle run of the
whole pipeline; instead every stage is recomputed in fp64 numpy from what the device handed to it:
  A  pack        bit for bit against oracle/pnp_np.correspondences, at the edges of the 256-wide scan
  B  hypotheses  validity rules, the modulo of negative draws, proper rotations; poses against the oracle on CLEAN samples only
  C  score       every device hypothesis re-scored on the device's records, inside a 1e-9 threshold band
  D  select      best = lowest index among the maxima of the device's counts; frames without a model
  E  final       EPnP: mask and re-fit of the device's winner; DLT: the oracle's refinement loop from the device's winner
  F  rejection (|t| >= 14.14) and one batch of frames with 0, 3, 4, 5, 6, 64, 65 correspondences
Shapes: F = 3, N = 700, 70 and 301 hypotheses (not multiples of 64 or 4; below and above the 256-thread argmax), counts that are no
multiple of 64; the measured figures behind every measured bound are in tests/pnp_cases.py and printed before they are asserted."""
import numpy as np
import pytest

from oracle import epnp_np, pnp_np
from tests import pnp_cases as pc

pytestmark = pytest.mark.gpu
METHODS = ("epnp", "dlt_lo")
K = pc.K_FINE


@pytest.fixture(scope="module")
def case():
    return pc.make_case()


@pytest.fixture(scope="module")
def runs(dev, case):
    """(method, iters) -> the device's outputs and intermediates on the committed case (its first `iters` hypotheses), computed once"""
    cache = {}

    def get(method, iters):
        if (method, iters) not in cache:
            cache[method, iters] = pc.run_device(dev, case["pc"], case["pixels"], case["coarse"], case["K"], case["samples"][:, :iters], method)
        return cache[method, iters]
    return get


# ----------------------------------------------------------------------------------------------------------------------- A. pack
@pytest.mark.parametrize("N", [1, 255, 256, 257, 700])
@pytest.mark.parametrize("use_pixels", [False, True])
def test_pack_at_the_scan_edges(dev, N, use_pixels):
    """frame 0 without a correspondence (labels 0 and 2 only), frame 1 with all of them, frame 2 mixed labels from {0, 1, 2}"""
    import torch
    from deepi2p_amd import registration_pnp as rp
    rng = np.random.default_rng(N)
    F = 3
    pts = rng.normal(0, 10, (F, 3, N)).astype(np.float32)
    coarse = np.stack([rng.choice([0, 2], N), np.ones(N, np.int64), rng.integers(0, 3, N)]).astype(np.int32)
    fine = rng.integers(0, pc.W_FINE * pc.H_FINE, (F, N)).astype(np.int32)
    pixels = rng.uniform(-3, 20, (F, 2, N)).astype(np.float32)
    t = lambda a: torch.from_numpy(a).to(dev)      # noqa: E731
    corr, n_corr = rp.pack_correspondences(t(pts), t(coarse), t(fine), pc.W_FINE, pixels=t(pixels) if use_pixels else None)
    corr, n_corr = corr.cpu().numpy(), n_corr.cpu().numpy()
    assert corr.shape == (F, N, 8) and corr.dtype == np.float32
    for f in range(F):
        X, uv = pnp_np.correspondences(pts[f], coarse[f], fine[f], pc.W_FINE, pixels[f] if use_pixels else None)
        cnt = X.shape[1]
        assert int(n_corr[f]) == cnt == int((coarse[f] == 1).sum())
        assert np.array_equal(corr[f, :cnt, :3].astype(np.float64), X.T) and np.array_equal(corr[f, :cnt, 3:5].astype(np.float64), uv.T)
        assert not corr[f, :cnt, 5:].any() and not corr[f, cnt:].any()
    assert int(n_corr[0]) == 0 and int(n_corr[1]) == N


# ----------------------------------------------------------------------------------------------------------------- B. hypotheses
@pytest.mark.parametrize("method", METHODS)
def test_hypothesis_rules_and_launch_geometry(runs, case, method):
    """301 hypotheses = four full blocks of 64 and one of 45; the run with 70 must reproduce the first 70 of them bit for bit (one thread per
    hypothesis: the result may not depend on the grid).  Valid flag 0 for a repeated index among the first five (EPnP; PLANTED and natural
    ones); every valid hypothesis a finite proper rotation (|R R^T - I| <= 1e-9, det > 0: holds for any null-space basis)."""
    o, o70 = runs(method, 301), runs(method, 70)
    for f in range(case["F"]):
        assert int(o["n_corr"][f]) == case["cnt"][f] == int(o70["n_corr"][f])
        pc.check_hypothesis_rules(o, f, case["samples"][f], method)
        pc.check_hypothesis_rules(o70, f, case["samples"][f, :70], method)
        flag = o["hyp"][f, :, 12]
        assert np.array_equal(o70["hyp"][f, :, 12], flag[:70])
        v = flag[:70] != 0
        assert np.array_equal(o70["hyp"][f, v], o["hyp"][f, :70][v]) and np.array_equal(o70["inliers"][f], o["inliers"][f, :70])
        if method == "epnp":
            assert not flag[list(pc.PLANTED)].any() and flag.sum() > 0.9 * (case["iters"] - len(pc.PLANTED) - 1)
        # the records the later stages read are the ones the pack stage is pinned to
        X, uv = pc.device_records(o, f)
        Xh, uvh = pc.case_records(case, f)
        assert np.array_equal(X, Xh) and np.array_equal(uv, uvh)


def test_epnp_hypotheses_on_clean_samples(runs, case):
    """Device pose vs oracle/epnp_np.epnp of the same five records (read from the device's corr at numpy's `% cnt` of the draws, more than
    40 % of them negative), on the samples of five distinct true inliers.  On exact data the pose does not depend on the null-space basis,
    up to near-degenerate samples: header vs oracle on these very samples differ (> 1e-5 m or > 1e-6 rad) in 0 of 270 on the CPU, asserted
    <= 1.5 % there (tests/test_epnp_host.py); the device, built with FMA contraction, may differ in at most 3 %, twice that.  An invalid
    device hypothesis on a clean sample counts as differing.  (Seen on an MI355X: 0 of 270 differ, the worst pair 1.5e-6 m / 6.5e-9 rad.)"""
    o = runs("epnp", 301)
    total = differ = 0
    worst = np.zeros(2)
    for f in range(case["F"]):
        X, uv = pc.device_records(o, f)
        idx = pc.reduce_samples(case["samples"][f], case["cnt"][f])
        for it in np.nonzero(case["clean5"][f])[0]:
            sol = epnp_np.epnp(X[idx[it, :5]].T, uv[idx[it, :5]].T, K)
            assert sol is not None
            total += 1
            h = o["hyp"][f, it]
            if h[12] == 0.0:
                differ += 1
                continue
            dt, dr = pc.pose_diff(h[:9].reshape(3, 3), h[9:12], sol[0], sol[1])
            bad = dt > pc.T_TOL or dr > pc.R_TOL
            differ += bad
            if not bad:
                worst = np.maximum(worst, (dt, dr))
    print("clean samples %d, differing %d; the others agree within |dt| %.3g m |dR| %.3g rad" % (total, differ, worst[0], worst[1]))
    assert total >= 100
    assert differ <= 0.03 * total, (differ, total)


def test_dlt_hypotheses_on_clean_samples(runs, case):
    """Device pose (Gaussian elimination, Newton polar iteration) vs oracle/pnp_np.dlt6 (SVD twice) on samples of six distinct true inliers.
    Left out: samples whose null vector is separated by s[10] / s[0] < 1e-6 in the oracle (or that the oracle refuses) -- decided by the
    oracle alone, at most 10 % of the samples (0 of 209 on the committed seed).  Bound for the rest: 1e-6 m / 1e-6 rad = unit round-off
    1e-16 x condition <= 1e6 x pivot growth 1e4.  (Seen on an MI355X: worst 1.4e-11 m / 2.5e-12 rad.)"""
    o = runs("dlt_lo", 301)
    total = left = 0
    worst = np.zeros(2)
    for f in range(case["F"]):
        X, uv = pc.device_records(o, f)
        idx = pc.reduce_samples(case["samples"][f], case["cnt"][f])
        for it in np.nonzero(case["clean6"][f])[0]:
            sol, gap = pnp_np.dlt6(X[idx[it]].T, uv[idx[it]].T, K, with_sv=True)
            total += 1
            if sol is None or gap < 1e-6:
                left += 1
                continue
            h = o["hyp"][f, it]
            assert h[12] == 1.0, (f, it)
            dt, dr = pc.pose_diff(h[:9].reshape(3, 3), h[9:12], sol[0], sol[1])
            worst = np.maximum(worst, (dt, dr))
            assert dt <= 1e-6 and dr <= 1e-6, (f, it, dt, dr, gap)
    print("six-inlier samples %d, left out %d, worst |dt| %.3g m |dR| %.3g rad" % (total, left, worst[0], worst[1]))
    assert total >= 100 and left <= 0.1 * total, (left, total)


# ---------------------------------------------------------------------------------------------------------------------- C. score
@pytest.mark.parametrize("iters", [70, 301])
@pytest.mark.parametrize("method", METHODS)
def test_score_of_every_device_hypothesis(runs, case, method, iters):
    """One wave per hypothesis, four per block: 70 = 17 blocks + 2 waves, 301 = 75 blocks + 1 wave; 358 / 351 / 335 records = five full
    strides of 64 and a partial one.  count(e2 within thr2 (1 - 1e-9)) <= inliers <= count(e2 within thr2 (1 + 1e-9)) with each method's rule;
    fp64 evaluation of e2 at the threshold carries ~1e-13 relative error, so the band leaves four decades -- and it may not hide a
    miscount: the summed width of all bands is at most 1e-3 of the summed counts.  Invalid hypotheses hold -1."""
    o = runs(method, iters)
    width = total = 0
    for f in range(case["F"]):
        assert case["cnt"][f] % 64 != 0
        w, t = pc.check_score(o, f, K, method)
        width, total = width + w, total + t
    print("%s, %d hypotheses: summed counts %d, summed band width %d" % (method, iters, total, width))
    assert total > 0 and width <= 1e-3 * total


@pytest.mark.parametrize("method", METHODS)
def test_score_rule_at_equality(dev, case, method):
    """`<=` (EPnP, as OpenCV's computeError test) against `<` (DLT) differ where e2 == thr2 exactly, which no finite threshold band can
    see.  The one equality IEEE arithmetic gives for certain: a record observed at u = +inf has e2 = +inf under every hypothesis, and
    reproj_err = 1e200 makes thr2 = +inf.  EPnP must count that record in every valid hypothesis, DLT must not; all finite records count."""
    px = case["pixels"][:, :, :].copy()
    planted = []
    for f in range(case["F"]):
        n = int(np.nonzero(case["coarse"][f] == 1)[0][10 + f])
        px[f, 0, n] = np.inf
        planted.append(n)
    iters = 70
    o = pc.run_device(dev, case["pc"], px, case["coarse"], case["K"], case["samples"][:, :iters], method, reproj_err=1e200)
    seen = 0
    for f in range(case["F"]):
        cnt = int(o["n_corr"][f])
        w, t = pc.check_score(o, f, K, method, thr=1e200)
        assert w == 0
        valid = o["hyp"][f, :, 12] != 0
        seen += int(valid.sum())
        X, uv = pc.device_records(o, f)
        assert np.isinf(uv[:, 0]).sum() == 1
        if method == "epnp":
            assert np.all(o["inliers"][f, valid] == cnt), (f, np.unique(o["inliers"][f, valid]), cnt)
        else:
            assert np.all(o["inliers"][f, valid] <= cnt - 1), (f, np.unique(o["inliers"][f, valid]), cnt)
    assert seen > 0.5 * iters * case["F"]


# --------------------------------------------------------------------------------------------------------------------- D. select
@pytest.mark.parametrize("iters", [70, 301])
@pytest.mark.parametrize("method", METHODS)
def test_select_lowest_index_among_the_maxima(runs, case, method, iters):
    """70 hypotheses: 186 argmax threads have none; 301: threads 0 .. 44 hold two.  Samples of true inliers all reach the true inlier
    count, so the maximum is tied many times over (asserted), and hypotheses 256 .. 287 repeat the samples of 0 .. 31: where the winner is
    below 32 its twin ties with it INSIDE one thread's stride (asserted for at least one frame)."""
    o = runs(method, iters)
    ties = twins = 0
    for f in range(case["F"]):
        assert pc.check_select(o, f, method)
        inl, b = o["inliers"][f], int(o["best"][f])
        ties += int((inl == inl.max()).sum() >= 2)
        if iters > pc.TIE_STRIDE and b < pc.TIE_COPIES:
            assert np.array_equal(case["samples"][f, b], case["samples"][f, b + pc.TIE_STRIDE])
            twins += int(inl[b + pc.TIE_STRIDE] == inl[b])
    assert ties >= 1
    if iters > pc.TIE_STRIDE:
        assert twins >= 1


# ---------------------------------------------------------------------------------------------------------------------- E. final
@pytest.mark.parametrize("iters", [70, 301])
def test_epnp_mask_and_refit(runs, case, iters):
    """EPnP: the mask lies between the strict and the loose mask of the winning device hypothesis, sum(mask) within the band width of
    n_inliers, outlier_ratio == 1 - n_inliers / n_corr exactly, and P = oracle/epnp_np.epnp on the device's masked records.
    Bound for P: csrc/epnp.h on the host vs that oracle on such inlier sets (261 - 747 inliers, the committed cases) measured at most
    2.21e-13 m and 4.32e-14 rad on the CPU; asserted 1000 x that = 2.21e-10 m / 4.32e-11 rad (pnp_cases.REFIT_BOUND; the margin covers the
    wave-butterfly summation order and FMA contraction; capped at 1e-8).  (Seen on an MI355X against the oracle: at most 1.4e-13 m / 2.9e-14 rad.)"""
    o = runs("epnp", iters)
    for f in range(case["F"]):
        assert pc.check_select(o, f, "epnp")
        assert pc.check_epnp_final(o, f, K) is not None
        dt, dr = pc.pose_diff(o["P"][f][:3, :3], o["P"][f][:3, 3], case["P_gt"][f][:3, :3], case["P_gt"][f][:3, 3])
        assert dt < 5e-2 and dr < 5e-3, (f, dt, dr)       # sanity only: a uniform pixel or two fall inside the threshold and join the fit


@pytest.mark.parametrize("iters", [70, 301])
def test_dlt_refinement_from_the_device_winner(runs, case, iters):
    """DLT: n_inliers >= inliers[best] and inside the band count of the returned P; outlier_ratio exact; P = oracle/pnp_np.py's refinement
    loop started from the DEVICE's winning hypothesis, within 1e-8 (Gauss-Newton contracts: both sides converge to the same minimum of the
    same inlier set).  A frame is left out when some record's error lies inside the 1e-9 threshold band in some round of the oracle's loop (the
    device may then keep another inlier set); at most one frame of the three."""
    o = runs("dlt_lo", iters)
    kept = 0
    for f in range(case["F"]):
        assert pc.check_select(o, f, "dlt_lo")
        kept += bool(pc.check_dlt_final(o, f, K))
        dt, dr = pc.pose_diff(o["P"][f][:3, :3], o["P"][f][:3, 3], case["P_gt"][f][:3, :3], case["P_gt"][f][:3, 3])
        assert dt < 5e-2 and dr < 5e-3, (f, dt, dr)       # sanity only, as for EPnP
    assert kept >= case["F"] - 1


# ------------------------------------------------------------------------------------------------- F. rejection and the edge batch
@pytest.mark.parametrize("method", METHODS)
def test_rejected_pose_and_frame_without_a_model(dev, case, method):
    """frame 0 shifted 100 m along z, its pixels unchanged: the pose that explains them has |t| ~ 100 >= 14.14 -> identity and ratio 1, but
    best and n_inliers are the winner's.  Frame 1: every sample is one index six times -> no valid hypothesis, every count -1 -> no
    model: identity, ratio 1, n_inliers 0, best -1.  Frame 2 unchanged."""
    pts, samples = case["pc"].copy(), case["samples"][:, :70].copy()
    pts[0, 2] += 100.0
    samples[1] = samples[1, :, :1]
    o = pc.run_device(dev, pts, case["pixels"], case["coarse"], case["K"], samples, method)
    for f in range(case["F"]):
        pc.check_hypothesis_rules(o, f, samples[f], method)
        pc.check_score(o, f, K, method)
    assert pc.check_select(o, 0, method) and pc.check_select(o, 2, method)
    b = int(o["best"][0])
    assert b >= 0 and int(o["inliers"][0, b]) > 0.7 * case["cnt"][0]
    assert np.array_equal(o["P"][0], np.eye(4)) and float(o["outlier_ratio"][0]) == 1.0
    if method == "epnp":
        assert int(o["n_inliers"][0]) == int(o["inliers"][0, b])
        assert pc.check_epnp_final(o, 0, K) is None and pc.check_epnp_final(o, 2, K) is not None
    else:
        assert int(o["n_inliers"][0]) >= int(o["inliers"][0, b])
        pc.check_dlt_final(o, 0, K), pc.check_dlt_final(o, 2, K)
    assert not o["hyp"][1, :, 12].any() and np.all(o["inliers"][1] == -1)
    assert not pc.check_select(o, 1, method)
    assert not np.array_equal(o["P"][2], np.eye(4)) and float(o["outlier_ratio"][2]) < 0.3


EDGE_COUNTS = (0, 3, 4, 5, 6, 64, 65)


@pytest.mark.parametrize("method", METHODS)
def test_edge_batch_of_small_counts(dev, method):
    """F = 7, N = 130, exact correspondences, 0 / 3 / 4 / 5 / 6 / 64 / 65 of them per frame, 70 samples (hypotheses 3 and 66 planted with six
    distinct indices, the second one through negative draws).  Per frame the stage rules above: EPnP has no model below 4 records, runs
    four-point samples on 4 (only the first four indices must differ) and five-point samples from 5 on; DLT has no model below 6.
    A re-fit on fewer than six records is compared with nothing (4 or 5 points: the eigenvectors are a null-space basis), on 6 .. 49
    records within 1e-8, from 50 on within pnp_cases.REFIT_BOUND."""
    rng = np.random.default_rng(77)
    F, N, iters = len(EDGE_COUNTS), 130, 70
    pts, px, co = np.zeros((F, 3, N), np.float32), np.zeros((F, 2, N), np.float32), np.zeros((F, N), np.int32)
    for f, cnt in enumerate(EDGE_COUNTS):
        X, uv, _ = pc.exact_set(rng, N)
        pts[f], px[f] = X.T, uv.T
        co[f, rng.permutation(N)[:cnt]] = 1
    samples = rng.integers(-2 ** 31, 2 ** 31, size=(F, iters, 6), dtype=np.int64).astype(np.int32)
    samples[:, 3] = np.arange(6)
    samples[:, 66] = -1 - np.arange(6)
    o = pc.run_device(dev, pts, px, co, np.stack([K] * F), samples, method)
    assert tuple(o["n_corr"]) == EDGE_COUNTS
    left = 0
    for f, cnt in enumerate(EDGE_COUNTS):
        pc.check_hypothesis_rules(o, f, samples[f], method)
        pc.check_score(o, f, K, method)
        model = pc.check_select(o, f, method)
        if cnt < (6 if method == "dlt_lo" else 4):
            assert not model and np.all(o["inliers"][f] == -1)
            continue
        assert o["hyp"][f, 3, 12] == 1.0 and o["hyp"][f, 66, 12] == 1.0, (method, cnt)     # the planted samples are distinct at every count
        assert model, (method, cnt)
        if method == "epnp":
            pc.check_epnp_final(o, f, K)
        else:
            left += not pc.check_dlt_final(o, f, K)
    assert left <= 1
