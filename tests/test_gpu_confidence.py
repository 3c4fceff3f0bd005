"""GPU: pose confidence (csrc/solver_aux.hip: di2p_pose_information, di2p_pose_covariance, di2p_restart_consensus; ops.py, the pipeline's and
the executors' confidence=True) against the numpy references of tests/confidence_oracle.py.

Bars.  Information matrix: |A_ab - ref| <= 1e-9 sqrt(A_aa A_bb) and |g_a - ref| <= 1e-9 sum |terms| (Cauchy-Schwarz bounds every sum of
products by these scales and both sides evaluate in fp64: the 1e-9 of test_residuals_match_oracle), cost 1e-9 relative, counts exact --
with every point more than 1e-6 from every frustum plane (asserted on the CPU), so that an ulp cannot flip a point's activity.
Covariance: 64 np eps cond(A) |cov|_max, the backward-error bound of a Cholesky inverse with a constant margin, cond(A) <= 1e8 asserted.
Consensus: counts exact, the gap bit for bit (a difference of two inputs), no perturbation within 1e-6 of a threshold (asserted)."""
import numpy as np
import pytest
import torch

from deepi2p_amd import ops, synthetic
from tests import confidence_oracle as co

pytestmark = pytest.mark.gpu
H, W = 160, 512
LB, UB = [-5, -0.1, -10], [5, 0.1, 10]
CHUNK = 1024                                                          # points per workgroup of the information kernel
PLAIN_KEYS = {"P", "cost", "best", "yaw0", "costs", "iters", "sweeps", "params", "labels_front", "pred"}
CONF_KEYS = {"info", "grad", "cov", "cov_status", "free_mask", "sigma_t", "sigma_r", "active", "agree", "finite", "gap"}
EPS = np.finfo(np.float64).eps


def _np(t):
    return t.detach().cpu().numpy()


def _bits(t):
    return _np(t).tobytes()


def _params(f, is_2d, d):
    """the frame's true pose moved by d = (rotation, translation) -- many points on the wrong side of a plane"""
    x = np.array([f["yaw_gt"] + d[0], f["t_gt"][0] + d[1], f["t_gt"][1], f["t_gt"][2] - d[1]])
    return x if is_2d else np.array([0.02 * d[0], x[0], -0.5 * d[0], x[1], x[2], x[3]])


def _generic(seed, N, is_2d):
    """F = 3 frames: their own K, labels with 5 % flips and some 2 and -1, parameters off the truth"""
    rng = np.random.default_rng(seed)
    frames = [synthetic.make_frame(rng, N=N, H=H, W=W, flip=0.05, with_image=False) for _ in range(3)]
    pc = np.stack([f["pc"] for f in frames])
    lab = np.stack([f["labels"] for f in frames]).astype(np.int32)
    lab[:, ::17] = 2
    lab[:, 5::23] = -1
    K = np.stack([f["K"] for f in frames])
    K[1, 0, 0] *= 1.1; K[1, 1, 1] *= 0.9; K[1, 0, 2] += 3.5           # noqa: E702
    K[2, 0, 0] *= 0.8; K[2, 1, 2] -= 2.25                             # noqa: E702
    params = np.stack([_params(f, is_2d, d) for f, d in zip(frames, ((0.05, 0.4), (-0.08, -0.7), (0.02, 1.1)))])
    return pc, lab, K, params


def _special(is_2d):
    """rotation exactly zero (the first-order branch) | no label-1 point | nothing active (exact labels at the evaluated pose)"""
    N = 777
    rng = np.random.default_rng(11)
    frames = [synthetic.make_frame(rng, N=N, H=H, W=W, flip=0.05, with_image=False) for _ in range(3)]
    pc = np.stack([f["pc"] for f in frames])
    lab = np.stack([f["labels"] for f in frames]).astype(np.int32)
    lab[:, ::17] = 2
    K = np.stack([f["K"] for f in frames])
    n = co.npar(is_2d)
    params = np.zeros((3, n))
    params[0, n - 3:] = [0.3, 0.02, 1.5]                               # rotation 0: theta^2 <= DBL_EPSILON
    lab[1][lab[1] == 1] = np.where(np.arange(int((lab[1] == 1).sum())) % 2 == 0, 0, -1)
    params[1] = _params(frames[1], is_2d, (0.05, 0.4))
    params[2] = _params(frames[2], is_2d, (0.0, 0.0))
    p = co.rotation(params[2], is_2d) @ pc[2].astype(np.float64) + params[2, n - 3:, None]
    px, py = K[2, 0, 0] * p[0] / p[2] + K[2, 0, 2], K[2, 1, 1] * p[1] / p[2] + K[2, 1, 2]
    lab[2] = ((px > 0) & (px < W - 1) & (py > 0) & (py < H - 1) & (p[2] > 0)).astype(np.int32)
    lab[2, ::17] = 2
    return pc, lab, K, params


def _information(dev, pc, lab, K, params, is_2d):
    return ops.pose_information(torch.from_numpy(pc).to(dev), torch.from_numpy(lab).to(dev), torch.from_numpy(K).to(dev),
                                torch.from_numpy(params).to(dev), H, W, is_2d)


def _check_information(dev, pc, lab, K, params, is_2d):
    refs = []
    for f in range(pc.shape[0]):
        assert co.plane_margins(pc[f], lab[f], K[f], params[f], H, W) > 1e-6, f      # the precondition, on the CPU
        refs.append(co.information(pc[f], lab[f], K[f], H, W, is_2d, params[f]))
    info, grad, cost, active = [_np(t) for t in _information(dev, pc, lab, K, params, is_2d)]
    pts64 = torch.from_numpy(pc.astype(np.float64)).to(dev)
    _, _, cost_res = ops.solver_residuals(pts64, torch.from_numpy(lab).to(dev), torch.from_numpy(K).to(dev), torch.from_numpy(params).to(dev),
                                          H, W, is_2d)
    cost_res = _np(cost_res)
    for f, ref in enumerate(refs):
        d = np.sqrt(np.diag(ref["A"]))
        errA = np.abs(info[f] - ref["A"])
        errg = np.abs(grad[f] - ref["g"])
        print("frame %d: active %s, max |dA| / bound %.3g, max |dg| / bound %.3g" % (
            f, list(active[f]), float(np.max(errA / np.maximum(1e-9 * np.outer(d, d), 1e-300))),
            float(np.max(errg / np.maximum(1e-9 * ref["g_abs"], 1e-300)))))
        assert np.array_equal(info[f], info[f].T), f
        assert np.all(errA <= 1e-9 * np.outer(d, d)), f
        assert np.all(errg <= 1e-9 * ref["g_abs"]), f
        assert abs(cost[f] - ref["cost"]) <= 1e-9 * abs(ref["cost"]), f
        assert abs(cost[f] - cost_res[f]) <= 1e-9 * abs(cost_res[f]), f
        assert np.array_equal(active[f], ref["active"]), f
    return refs, (info, grad, cost, active)


# ---------------------------------------------------------------------------------------------------------------- 1. information
@pytest.mark.parametrize("N", [50, 777, CHUNK + 1])                  # below a wave | ragged | two partials to combine
@pytest.mark.parametrize("is_2d", [True, False])
def test_information_matches_the_reference(dev, is_2d, N):
    pc, lab, K, params = _generic(100 + N, N, is_2d)
    refs, _ = _check_information(dev, pc, lab, K, params, is_2d)
    if N >= 777:
        assert all(r["active"].min() > 0 for r in refs)                # both kinds of block constrain every frame


@pytest.mark.parametrize("is_2d", [True, False])
def test_information_special_frames(dev, is_2d):
    pc, lab, K, params = _special(is_2d)
    assert not params[0, :co.npar(is_2d) - 3].any() and not (lab[1] == 1).any()
    refs, (info, grad, cost, active) = _check_information(dev, pc, lab, K, params, is_2d)
    assert refs[0]["active"].min() > 0                                 # the first-order branch with real work
    assert refs[1]["active"][0] == 0 and refs[1]["active"][1] > 0
    assert not refs[2]["active"].any()                                 # nothing active: exact zeros
    assert not info[2].any() and not grad[2].any() and cost[2] == 0.0 and not active[2].any()


@pytest.mark.parametrize("is_2d", [True, False])
def test_information_is_reproducible_and_independent_of_the_batch(dev, is_2d):
    pc, lab, K, params = _generic(100 + CHUNK + 1, CHUNK + 1, is_2d)
    a = _information(dev, pc, lab, K, params, is_2d)
    b = _information(dev, pc, lab, K, params, is_2d)
    alone = _information(dev, pc[2:], lab[2:], K[2:], params[2:], is_2d)
    for x, y, z in zip(a, b, alone):
        assert _bits(x) == _bits(y)
        assert _bits(x[2:]) == _bits(z)


def test_information_rejects_bad_arguments(dev):
    pc, lab, K, params = _generic(1, 50, True)
    t = [torch.from_numpy(v).to(dev) for v in (pc, lab, K, params)]
    with pytest.raises(RuntimeError, match="points"):
        ops.pose_information(t[0].double(), t[1], t[2], t[3], H, W, True)
    with pytest.raises(ValueError, match="params"):
        ops.pose_information(t[0], t[1], t[2], t[3], H, W, False)      # four parameters, asked for six
    with pytest.raises(ValueError, match="workspace"):
        ops.pose_information(t[0], t[1], t[2], t[3], H, W, True, workspace=torch.empty((8,), dtype=torch.uint8, device=dev))


# ---------------------------------------------------------------------------------------------------------------- 2. covariance
def _spd(n, seed, log_cond):
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    A = (Q * np.logspace(0, log_cond, n)) @ Q.T
    return (A + A.T) / 2


@pytest.mark.parametrize("is_2d", [True, False])
def test_covariance(dev, is_2d):
    n, toff = co.npar(is_2d), (1 if is_2d else 3)
    x0 = np.linspace(0.05, 0.09, n)                                    # inside the box
    cases = []                                                         # (info, params, has_inside)
    for seed, lc in ((1, 1), (2, 4), (3, 6)):
        cases.append((_spd(n, seed, lc), x0, 1))
    on = [(0,), (1,), (2,), (0, 1), (0, 2), (1, 2)]                    # one or two translation parameters on a bound
    for k, fixed in enumerate(on):
        x = x0.copy()
        for j, i in enumerate(fixed):
            x[toff + i] = (LB if (k + j) % 2 == 0 else UB)[i]
        cases.append((_spd(n, 10 + k, 3), x, 1))
    first_bad = len(cases)
    S = np.eye(n)
    S[0, 0], S[0, 1], S[1, 0], S[1, 1] = 4.0, 2.0, 2.0, 1.0            # row 1 = row 0 / 2: the second pivot is exactly 0
    cases.append((S, x0, 1))
    cases.append((np.zeros((n, n)), x0, 1))
    Nn = _spd(n, 20, 2)
    Nn[n - 1, 0] = np.nan
    cases.append((Nn, x0, 1))
    xi = x0.copy()
    xi[0] = np.inf
    cases.append((_spd(n, 21, 2), xi, 1))
    xb = x0.copy()
    xb[toff + 2] = UB[2]
    cases.append((_spd(n, 22, 2), xb, 0))                              # no inside point; the mask is written all the same
    want_status = [0] * first_bad + [1, 1, 2, 2, 2]
    info = np.stack([c[0] for c in cases])
    params = np.stack([c[1] for c in cases])
    has = np.array([c[2] for c in cases], np.int32)
    refs = [co.covariance(c[0], c[1], LB, UB, is_2d, c[2]) for c in cases]
    assert [r["status"] for r in refs] == want_status
    cov, mask, status, st, sr = [_np(t) for t in ops.pose_covariance(torch.from_numpy(info).to(dev), torch.from_numpy(params).to(dev), LB, UB,
                                                                     is_2d, has_inside=torch.from_numpy(has).to(dev))]
    assert list(status) == want_status
    assert list(mask) == [r["free_mask"] for r in refs]
    assert sorted(set(mask[3:first_bad])) == sorted(((1 << n) - 1) & ~sum(1 << (toff + i) for i in fx) for fx in on)
    for f, ref in enumerate(refs):
        if want_status[f]:
            assert np.all(np.isnan(cov[f])) and np.isnan(st[f]) and np.isnan(sr[f]), f
            continue
        cond = np.linalg.cond(info[f])
        assert cond <= 1e8, f
        tol = 64 * n * EPS * cond * np.abs(ref["cov"]).max()
        print("frame %d: cond %.3g, max |dcov| / bound %.3g" % (f, cond, float(np.abs(cov[f] - ref["cov"]).max() / tol)))
        assert np.all(np.abs(cov[f] - ref["cov"]) <= tol), f
        assert np.array_equal(cov[f], cov[f].T), f
        fixed = [i for i in range(n) if not (ref["free_mask"] >> i) & 1]
        assert not cov[f][fixed].any() and not cov[f][:, fixed].any(), f
        assert abs(st[f] ** 2 - ref["sigma_t"] ** 2) <= 3 * tol and abs((sr[f] * np.pi / 180) ** 2 - (ref["sigma_r"] * np.pi / 180) ** 2) <= 3 * tol, f
        assert abs(st[f] - np.sqrt(np.trace(cov[f][toff:, toff:]))) <= 4 * EPS * st[f], f
    # has_inside = NULL: the last frame is an ordinary frame with tz on its bound
    cov2, mask2, status2, _, _ = [_np(t) for t in ops.pose_covariance(torch.from_numpy(info).to(dev), torch.from_numpy(params).to(dev), LB, UB, is_2d)]
    assert list(status2) == want_status[:-1] + [0] and np.array_equal(mask2, mask)
    assert cov2[:first_bad].tobytes() == cov[:first_bad].tobytes()
    ref = co.covariance(cases[-1][0], cases[-1][1], LB, UB, is_2d)
    assert np.all(np.abs(cov2[-1] - ref["cov"]) <= 64 * n * EPS * np.linalg.cond(info[-1]) * np.abs(ref["cov"]).max())


# ---------------------------------------------------------------------------------------------------------------- 3. consensus
def _consensus_frames(R, is_2d, seed):
    """F = 4 frames: a mix | all agree | has_inside = 0 | ties and NaN costs -> params [4,R,np], cost [4,R], best [4], has_inside [4]"""
    rng = np.random.default_rng(seed)
    n, toff = co.npar(is_2d), (1 if is_2d else 3)
    params = np.zeros((4, R, n))
    cost = np.zeros((4, R))
    best = np.array([R // 2, 0, R // 3, R - 1], np.int32)
    t_steps, r_steps = (0.0, 0.3, 1.5, 1.9, 2.1, 3.0, 7.0), (0.0, 1.0, 4.0, 6.0, 12.0)      # metres, degrees
    for f in range(4):
        xb = np.concatenate([rng.uniform(-0.3, 0.3, toff), rng.uniform(-1, 1, 3) * [4, 0.09, 8]])
        for r in range(R):
            x = xb.copy()
            if r != best[f]:
                small = f == 1                                           # every restart of frame 1 stays within (2 m, 5 deg)
                d = rng.standard_normal(3)
                x[toff:] += d / np.linalg.norm(d) * (rng.choice(t_steps[:3]) if small else rng.choice(t_steps))
                x[toff - 1 if is_2d else rng.integers(0, 3)] += np.deg2rad(rng.choice(r_steps[:2]) if small else rng.choice(r_steps))
            params[f, r] = x
            cost[f, r] = 10.0 + rng.uniform(0.5, 5.0) * (r != best[f])
        cost[f, best[f]] = 10.0
    if R >= 8:
        far = [r for r in range(R) if r != best[3] and co.consensus(params[3, [r, best[3]]], np.ones(2), 1, is_2d, 2.0, 5.0)[1] == 1]
        near = [r for r in range(R) if r != best[3] and r not in far]
        cost[3, far[0]] = 10.0                                           # a tie with the best in another basin: the gap is 0
        cost[3, near[0]] = 10.0                                          # ... and one in the best's own
        cost[3, far[1]] = np.nan
        cost[3, near[1]] = np.nan
        cost[0, 1] = np.inf
    return params, cost, best, np.array([1, 1, 0, 1], np.int32)


@pytest.mark.parametrize("R", [1, 60, 130])
@pytest.mark.parametrize("is_2d", [True, False])
def test_restart_consensus(dev, is_2d, R):
    params, cost, best, has = _consensus_frames(R, is_2d, 40 + R)
    want = []
    for f in range(4):
        Pb = co.pose(params[f, best[f]], is_2d)
        for r in range(R):                                                # no perturbation sits on a threshold
            t, a = co.flm.get_P_diff(co.pose(params[f, r], is_2d), Pb)
            assert abs(t - 2.0) > 1e-6 and abs(a - 5.0) > 1e-6, (f, r, t, a)
        want.append(co.consensus(params[f], cost[f], int(best[f]), is_2d, 2.0, 5.0, int(has[f])))
    dv = [torch.from_numpy(v).to(dev) for v in (params, cost, best, has)]
    finite, agree, gap = [_np(t) for t in ops.restart_consensus(dv[0], dv[1], dv[2], is_2d, 2.0, 5.0, has_inside=dv[3])]
    print("R = %d: finite %s agree %s gap %s" % (R, list(finite), list(agree), list(gap)))
    assert list(finite) == [w[0] for w in want] and list(agree) == [w[1] for w in want]
    wgap = np.array([w[2] for w in want])
    assert np.array_equal(np.isnan(gap), np.isnan(wgap)) and gap[~np.isnan(gap)].tobytes() == wgap[~np.isnan(wgap)].tobytes()
    assert (finite[2], agree[2]) == (0, 0) and np.isnan(gap[2])           # has_inside = 0
    assert agree[1] == finite[1] == R and gap[1] == np.inf                # all agree
    if R >= 8:
        assert gap[3] == 0.0 and finite[3] == R - 2 and 1 < agree[3] < finite[3] and finite[0] == R - 1
    # has_inside = NULL: frame 2 is an ordinary frame; best = -1 (select_best's mark of a frame without inside points) is not
    b2 = best.copy()
    b2[0] = -1
    finite2, agree2, gap2 = [_np(t) for t in ops.restart_consensus(dv[0], dv[1], torch.from_numpy(b2).to(dev), is_2d, 2.0, 5.0)]
    w2 = co.consensus(params[2], cost[2], int(best[2]), is_2d, 2.0, 5.0)
    assert (finite2[2], agree2[2]) == w2[:2] and gap2[2] == w2[2]
    assert (finite2[0], agree2[0]) == (0, 0) and np.isnan(gap2[0])


# ---------------------------------------------------------------------------------------------------------------- 4. pipeline, executors
def _check_info_of_result(out, pc, K, pipe):
    x = ops.gather_best_params(out["params"], out["best"], pipe.is_2d)
    b = _np(out["best"]).astype(np.int64)
    assert np.array_equal(_np(x), _np(out["params"])[np.arange(len(b)), np.maximum(b, 0)])
    info, grad, _, active = ops.pose_information(pc, out["labels_front"], K, x, pipe.H, pipe.W, pipe.is_2d)
    assert _bits(info) == _bits(out["info"]) and _bits(grad) == _bits(out["grad"]) and _bits(active) == _bits(out["active"])


def test_executor_confidence(dev):
    """the smallest executor configuration of test_gpu_evaluation.py: off is the parent's executor; on adds the keys, moves no other
    bit, replays as it runs eagerly, and its matrix is pose_information at the returned params[best]"""
    from deepi2p_amd.pipeline import RegistrationExecutor
    from tests.test_gpu_pipeline import NAMES, _setup
    B = 2
    mm, pipe, K, restarts, batches, host = _setup(dev, B=B)
    labels = torch.from_numpy(batches[0]["labels"]).to(dev)
    runs = {}
    for name, kw in (("off", {}), ("graph", dict(confidence=True)), ("eager", dict(confidence=True, use_graph=False))):
        ex = RegistrationExecutor(mm, pipe, K, host[0], n_streams=1, restarts=restarts, labels_override=labels, **kw)
        got = []
        for i in (0, 1):
            out = ex.result(ex.submit(host[i]))
            got.append({k: v.clone() for k, v in out.items()})
        assert ex.use_graph == (name != "eager"), ex.graph_error
        runs[name] = got
    for i in (0, 1):
        off, g, e = runs["off"][i], runs["graph"][i], runs["eager"][i]
        assert set(off) == PLAIN_KEYS and set(g) == set(e) == PLAIN_KEYS | CONF_KEYS
        for k in PLAIN_KEYS:
            assert _bits(off[k]) == _bits(g[k]), k
        for k in PLAIN_KEYS | CONF_KEYS:
            assert _bits(g[k]) == _bits(e[k]), k
        _check_info_of_result(g, host[i]["pc"].to(dev), K, pipe)
        assert torch.all(g["best"] >= 0) and torch.all(g["finite"] >= g["agree"]) and torch.all(g["agree"] >= 1)
        assert torch.all(g["active"].sum(dim=1) > 0)
        ok = _np(g["cov_status"]) == 0
        assert np.all(np.isfinite(_np(g["sigma_t"])[ok])) and np.all(np.isnan(_np(g["sigma_t"])[~ok]))
    # the pipeline on its own, with its own setting, gives the executor's bits
    d = {k: host[0][k].to(dev) for k in NAMES}
    from deepi2p_amd.registration import RegistrationPipeline
    own = RegistrationPipeline(pipe.H, pipe.W, R=pipe.R, seed=3, confidence=True)(d["pc"], labels, K, restarts)
    for k in CONF_KEYS:
        assert _bits(own[k]) == _bits(runs["graph"][0][k]), k


def test_pipeline_confidence_in_the_enu_frame(dev):
    """test_enu_frame_gauss_newton's scene: the confidence of a frame="enu" pipeline is that of the converted points, i.e. P_cam's"""
    from deepi2p_amd import evaluation
    from deepi2p_amd.registration import RegistrationPipeline
    F, N = 2, 1000
    rng = np.random.default_rng(21)
    frames = [synthetic.make_frame(rng, N=N, H=H, W=W, flip=0.05, with_image=False) for _ in range(F)]
    pc = np.stack([f["pc"] for f in frames])
    pc_enu = np.ascontiguousarray(np.stack([pc[:, 0], pc[:, 2], -pc[:, 1]], axis=1))
    lab = torch.from_numpy(np.stack([f["labels"] for f in frames])).to(dev)
    K = torch.from_numpy(np.stack([f["K"] for f in frames])).to(dev)
    cam = RegistrationPipeline(H, W, R=4, max_iter=50, seed=1, confidence=True)
    restarts = cam.draw(F, dev)
    a = cam(torch.from_numpy(pc).to(dev), lab, K, restarts)
    enu = RegistrationPipeline(H, W, R=4, max_iter=50, seed=1, frame="enu")
    plain = enu(torch.from_numpy(pc_enu).to(dev), lab, K, restarts)
    b = enu(torch.from_numpy(pc_enu).to(dev), lab, K, restarts, confidence=True)
    assert set(plain) == PLAIN_KEYS - {"pred"} | {"P_cam"} and set(b) == set(plain) | CONF_KEYS == set(a) | {"P_cam"}
    for k in CONF_KEYS:
        assert _bits(a[k]) == _bits(b[k]), k
    for k in plain:
        assert _bits(plain[k]) == _bits(b[k]), k
    _check_info_of_result(b, evaluation.enu2cam_points(torch.from_numpy(pc_enu).to(dev)), K, enu)
    assert int((b["active"].sum(dim=1) > 0).sum()) == F


def test_raw_executor_confidence(dev):
    """the smallest configuration of test_gpu_raw_frames.py: the argument reaches the base executor through RawFrameExecutor"""
    from deepi2p_amd.raw_pipeline import RawFrameExecutor
    from deepi2p_amd.registration import RegistrationPipeline
    from tests.test_gpu_raw_frames import H as RH, W as RW, _KP, _mm, _opt
    B = 2
    scans = [synthetic.make_velodyne_scan(np.random.default_rng(60 + i), azimuths=300) for i in range(2)]
    raw = np.stack([synthetic.make_camera_image(np.random.default_rng(100 + i)) for i in range(2)])
    K, Pc = _KP(B)
    batch = dict(image=torch.from_numpy(raw), K_raw=torch.from_numpy(K), Pc=torch.from_numpy(Pc), seed=31, scans=scans)
    mm = _mm(dev, False)
    pipe = RegistrationPipeline(RH, RW, R=4, seed=3)
    restarts = pipe.draw(B, dev)
    cap, mfp = sum(len(s) for s in scans), max(len(s) for s in scans)
    outs = {}
    for on in (False, True):
        ex = RawFrameExecutor(mm, pipe, _opt(), batch, cap, mfp, n_streams=1, restarts=restarts, confidence=on)
        out = ex.result(ex.submit(batch))
        assert ex.use_graph, ex.graph_error
        outs[on] = {k: v.clone() for k, v in out.items() if torch.is_tensor(v)}
        if on:
            d = ex.slots[0].dev
            _check_info_of_result(out, d["pc"], d["K"], pipe)
    assert set(outs[True]) == set(outs[False]) | CONF_KEYS and not (set(outs[False]) & CONF_KEYS)
    for k in outs[False]:
        assert _bits(outs[False][k]) == _bits(outs[True][k]), k
