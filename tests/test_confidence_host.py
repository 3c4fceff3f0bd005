"""CPU: the pose-confidence references (tests/confidence_oracle.py) pinned on their own, the ABI additions, and the executor's argument
checks.  No device call."""
import os
import types

import numpy as np
import pytest

from deepi2p_amd import synthetic
from oracle import frustum_lm as flm
from tests import confidence_oracle as co

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 160, 512
LB, UB = [-5, -0.1, -10], [5, 0.1, 10]
NEW = ["di2p_pose_information_workspace_bytes", "di2p_pose_information", "di2p_gather_best_params", "di2p_pose_covariance",
       "di2p_restart_consensus"]


def test_exports():
    from deepi2p_amd import _lib
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for n in NEW:
        assert n in _lib.EXPORTS, n
        assert n in doc, n
    l = _lib.load()
    assert l.di2p_version() == 9                      # purely additive
    # C = ceil(N / 1024) partials of 32 fp64 words per frame; an empty cloud still has one
    assert l.di2p_pose_information_workspace_bytes(3, 1025) == 3 * 2 * 32 * 8
    assert l.di2p_pose_information_workspace_bytes(3, 1024) == 3 * 1 * 32 * 8
    assert l.di2p_pose_information_workspace_bytes(2, 0) == 2 * 32 * 8
    assert l.di2p_pose_information_workspace_bytes(-1, 5) == 0


@pytest.mark.parametrize("is_2d", [True, False])
def test_reference_gradient_is_the_central_difference_of_the_oracle_cost(is_2d):
    """g = sum rho'(s) J^T r is the gradient of 1/2 sum log1p(s): compared with (cost(x + e) - cost(x - e)) / 2e of the ORACLE's cost, e = 1e-6.
    Kink-free: a step of 1e-6 in a parameter moves a pixel by at most ~1e-6 * fx * (1 + range / depth) < 1e-3, so with every point more than
    1e-2 from every plane no residual block switches inside the difference.  Bar: truncation e^2 f''' / 6 is far below it; the cancellation
    error is ~ eps * cost / e = 2.2e-16 * 1e3 / 1e-6 ~ 2e-7 absolute, so 1e-5 * (1 + sum |terms|) leaves a factor of ten."""
    rng = np.random.default_rng(7)
    f = synthetic.make_frame(rng, N=400, H=H, W=W, with_image=False)
    pts, lab = f["pc"].astype(np.float64), f["labels"].copy()
    lab[::13] = 7
    params = np.array([0.4, 0.7, -0.03, 1.5]) if is_2d else np.array([0.05, 0.4, -0.03, 0.7, -0.03, 1.5])
    assert co.plane_margins(pts, lab, f["K"], params, H, W) > 1e-2
    ref = co.information(pts, lab, f["K"], H, W, is_2d, params)
    assert ref["active"].sum() > 20 and ref["cost"] > 1.0             # a real comparison
    eps = 1e-6
    for a in range(params.size):
        d = np.zeros_like(params)
        d[a] = eps
        cp = flm.residuals_and_jacobian(pts, lab, f["K"], H, W, is_2d, params + d)[2]
        cm = flm.residuals_and_jacobian(pts, lab, f["K"], H, W, is_2d, params - d)[2]
        assert abs((cp - cm) / (2 * eps) - ref["g"][a]) <= 1e-5 * (1 + ref["g_abs"][a]), a
    # the matrix is the symmetric Gauss-Newton matrix of the same rows
    assert np.array_equal(ref["A"], ref["A"].T) or np.allclose(ref["A"], ref["A"].T, rtol=1e-14, atol=0)
    assert np.all(np.linalg.eigvalsh(ref["A"]) > -1e-9 * np.abs(ref["A"]).max())


def test_reference_information_of_an_empty_problem():
    ref = co.information(np.zeros((3, 5)), np.full(5, 2, np.int32), synthetic.make_K(H, W), H, W, True, np.array([0.1, 0, 0, 1.0]))
    assert not ref["A"].any() and not ref["g"].any() and ref["cost"] == 0.0 and list(ref["active"]) == [0, 0]


def _spd(n, seed):
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((n, n))
    return B @ B.T + n * np.eye(n)


@pytest.mark.parametrize("is_2d", [True, False])
def test_covariance_reference_rules(is_2d):
    n, toff = co.npar(is_2d), (1 if is_2d else 3)
    A = _spd(n, 3)
    x = np.linspace(0.1, 0.6, n)                                     # inside the box
    full = co.covariance(A, x, LB, UB, is_2d)
    assert full["status"] == 0 and full["free_mask"] == (1 << n) - 1
    assert np.allclose(full["cov"] @ A, np.eye(n), atol=1e-12)
    assert np.isclose(full["sigma_t"], np.sqrt(np.trace(full["cov"][toff:, toff:])))
    assert np.isclose(full["sigma_r"], np.sqrt(np.trace(full["cov"][:toff, :toff])) * 180 / np.pi)
    # a translation on its bound: removed before the inversion, zeros in cov -- NOT the rows of the full inverse
    for i, bound in ((0, LB), (1, UB), (2, LB)):
        xb = x.copy()
        xb[toff + i] = bound[i]
        c = co.covariance(A, xb, LB, UB, is_2d)
        keep = [j for j in range(n) if j != toff + i]
        assert c["status"] == 0 and c["free_mask"] == ((1 << n) - 1) & ~(1 << (toff + i))
        assert not c["cov"][toff + i].any() and not c["cov"][:, toff + i].any()
        assert np.allclose(c["cov"][np.ix_(keep, keep)], np.linalg.inv(A[np.ix_(keep, keep)]), rtol=1e-12)
        assert not np.allclose(c["cov"][np.ix_(keep, keep)], full["cov"][np.ix_(keep, keep)], rtol=1e-6)
    # a rotation parameter equal to a bound's value is still free
    xr = x.copy()
    xr[0] = LB[0]
    assert co.covariance(A, xr, LB, UB, is_2d)["free_mask"] == (1 << n) - 1
    # rank deficient (row 1 = half of row 0, exactly): status 1, NaN outputs, the mask is still there
    S = np.eye(n)
    S[0, 0], S[0, 1], S[1, 0], S[1, 1] = 4.0, 2.0, 2.0, 1.0
    c = co.covariance(S, x, LB, UB, is_2d)
    assert c["status"] == 1 and c["free_mask"] == (1 << n) - 1 and np.all(np.isnan(c["cov"])) and np.isnan(c["sigma_t"]) and np.isnan(c["sigma_r"])
    assert co.covariance(np.zeros((n, n)), x, LB, UB, is_2d)["status"] == 1
    # non-finite input or no inside point: status 2
    N = A.copy()
    N[1, 0] = np.nan
    assert co.covariance(N, x, LB, UB, is_2d)["status"] == 2
    xn = x.copy()
    xn[-1] = np.inf
    assert co.covariance(A, xn, LB, UB, is_2d)["status"] == 2
    c = co.covariance(A, x, LB, UB, is_2d, has_inside=0)
    assert c["status"] == 2 and np.all(np.isnan(c["cov"])) and c["free_mask"] == (1 << n) - 1


def test_consensus_reference_rules():
    best = np.array([0.3, 1.0, 0.05, -2.0])
    params = np.stack([best, best + [0, 0.5, 0, 0], best + [0, 3.0, 0, 0], best + [0.2, 0, 0, 0], best])
    cost = np.array([5.0, 6.0, 7.5, 6.5, np.nan])
    # restart 1 agrees (0.5 m), 2 is 3 m off, 3 is 11.5 degrees off, 4 has no finite cost
    assert co.consensus(params, cost, 0, True, 2.0, 5.0) == (4, 2, 1.5)
    assert co.consensus(params[:2], cost[:2], 0, True, 2.0, 5.0) == (2, 2, np.inf)
    f, a, g = co.consensus(params, cost, -1, True, 2.0, 5.0)
    assert (f, a) == (0, 0) and np.isnan(g)
    f, a, g = co.consensus(params, cost, 0, True, 2.0, 5.0, has_inside=0)
    assert (f, a) == (0, 0) and np.isnan(g)


def test_plane_margins():
    K = synthetic.make_K(H, W)
    pts = np.array([[0.0, 1.0], [0.0, 0.0], [200.0, 200.0]])        # the principal point, and fx / 200 pixels to its right
    m = co.plane_margins(pts, np.array([1, 0]), K, np.zeros(4), H, W)
    assert np.isclose(m, min(K[1, 2], (H - 1) - K[1, 2]))
    assert np.isclose(co.plane_margins(pts, np.array([1, 0]), K, np.array([0, 0, 0, -199.5]), H, W), 0.5)      # p2 = 0.5 is the nearest plane


def test_executor_confidence_argument_errors():
    """the checks run before the executor touches the model or the device"""
    from deepi2p_amd.pipeline import RegistrationExecutor
    from deepi2p_amd.registration import RegistrationPipeline
    from deepi2p_amd.registration_pnp import PnPPipeline
    fine = types.SimpleNamespace(opt=types.SimpleNamespace(is_fine_resolution=True))
    with pytest.raises(ValueError, match="confidence=True.*step_fn"):
        RegistrationExecutor(fine, RegistrationPipeline(H, W), None, {}, step_fn=lambda slot, d: {}, confidence=True)
    with pytest.raises(ValueError, match="confidence=True.*PnPPipeline"):
        RegistrationExecutor(fine, PnPPipeline(64, 128), None, {}, confidence=True)
    pipe = RegistrationPipeline(H, W, confidence=True, agree_tol=(1, 3))
    assert pipe.confidence and pipe.agree_tol == (1.0, 3.0) and not RegistrationPipeline(H, W).confidence
    assert set(RegistrationPipeline.CONFIDENCE_KEYS) == {"info", "grad", "cov", "cov_status", "free_mask", "sigma_t", "sigma_r", "active",
                                                         "agree", "finite", "gap"}


def test_subclass_executors_take_the_argument():
    import inspect
    from deepi2p_amd import raw_pipeline, submap_pipeline, sweep_pipeline
    for cls in (raw_pipeline.RawFrameExecutor, submap_pipeline.OxfordFrameExecutor, sweep_pipeline.SweepFrameExecutor):
        assert inspect.signature(cls.__init__).parameters["confidence"].default is False, cls
