"""GPU: the LM lane of solver.hip against the oracle on the case table of tests/solver_lm_cases.py -- every exit the oracle can be driven into
through the public arguments, every line-search branch, both point types (float64 records and the float32 records the pipeline and the benchmark
run), and the wide second-tier kernels resuming parked hypotheses.  tests/test_solver_lm_cases_host.py (CPU) keeps the table honest.

Rules of comparison (the suite's, tests/test_gpu_solver.py): a hypothesis AGREES when its parameters are within 1e-3 m / 1e-3 rad of the oracle's AND
it got there in the same number of iterations and sweeps; the ones that do not are enumerated in KNOWN_FORKS and one more is a failure; where it
agrees, costs agree to 1e-6 relative + COST_ATOL = 1e-12 absolute, the rule test_small_and_ragged_frames already applies to flat problems.  The
absolute term is the precision of the objective as the reference library defines it: Ceres' CauchyLoss forms log(1 + s) from the rounded sum 1 + s,
an absolute error of 2^-53 per residual block whatever the size of s, i.e. up to N * 2^-54 = 1.1e-13 on the cost at N = 2048 (the kernel
accumulates the product of the 1 + s and has the same bound; the oracle uses log1p and is more accurate than either).  The frames with exact
labels converge to costs of 1e-27 .. 1e-11, which are made of rounding alone and have no digit to compare relatively.

Sweep identity (read off solver.hip: lm_decide increments nsweep once per sweep; the kernel sweeps the start once and then every line-search trial
point WITH its normal equations, so it has neither the oracle's cost-only evaluation of the candidate nor its re-evaluation of the accepted
iterate):  sweeps == 1 + oracle trial evaluations."""
import numpy as np
import pytest
import torch

from oracle import frustum_lm as flm
from tests import solver_lm_cases as lc

pytestmark = pytest.mark.gpu

DTYPES = [False, True]
_ids = lambda f32: "f32" if f32 else "f64"
_cid = lambda c: c.name
PROF_WORDS = 28
TIER_SWEEPS = 8

# (case name, f32[, "tier"]) -> hypotheses whose HIP trajectory is not the oracle's (another end point, or the same end point after another number
# of iterations or sweeps).  Measured on MI355X; everything not listed must agree.
#   face0-2d, hypothesis 2: the iterate creeps along the box face z = 0 where the planted point's depth vanishes and trial samples are not
#     finite; it ends 1e-7 from the oracle's end point after 35 instead of 33 iterations (costs 1e-12 and 2e-11).
#   scaled-2d float32, hypothesis 3: same 16 iterations, same end point (1e-11) and cost (1e-14 relative), two trials fewer: a search that the
#     oracle stops two trials later, both falling back to the same first trial point.
KNOWN_FORKS = {
    ("face0-2d", False): [2], ("face0-2d", True): [2],
    ("scaled-2d", True): [3],
}


def _check_forks(key, ok):
    bad = sorted(np.nonzero(~ok)[0].tolist())
    assert bad == KNOWN_FORKS.get(key, []), "hypotheses that disagree with the oracle on case %r: %s (expected %s)" % (key, bad, KNOWN_FORKS.get(key, []))


def _agreement(po, pg, is_2d):
    toff = 1 if is_2d else 3
    dt = np.linalg.norm(po[:, toff:] - pg[:, toff:], axis=1)
    dr = np.linalg.norm(po[:, :toff] - pg[:, :toff], axis=1)
    return (dt <= 1e-3) & (dr <= 1e-3)


COST_RTOL, COST_ATOL = 1e-6, 1e-12


def _args(dev, inps, f32, max_iter, is_2d):
    """one call over the frames `inps` (same N, R, image and box)"""
    pts = np.stack([i.points for i in inps])
    a = inps[0]
    return (torch.from_numpy(pts.astype(np.float32) if f32 else pts).to(dev), torch.from_numpy(np.stack([i.labels for i in inps])).to(dev),
            torch.from_numpy(np.stack([i.K for i in inps])).to(dev), torch.from_numpy(np.stack([i.ys for i in inps])).to(dev),
            torch.from_numpy(np.stack([i.Ts for i in inps])).to(dev), a.H, a.W, list(a.lb), list(a.ub), max_iter, is_2d)


class Result:
    def __init__(self, params, cost, iters, sweeps, prof=None):
        self.params, self.cost, self.iters, self.sweeps, self.prof = params, cost, iters, sweeps, prof

    def bytes(self, f=None):
        sel = (lambda a: a) if f is None else (lambda a: a[f])
        return [np.ascontiguousarray(sel(a)).tobytes() for a in (self.params, self.cost, self.iters, self.sweeps)]


def _solve(dev, args, profile=False, tier=0):
    from deepi2p_amd import _lib, ops
    F, R = args[3].shape
    sweeps = torch.zeros((F, R), dtype=torch.int32, device=dev)
    prof = torch.zeros((F * R, PROF_WORDS), dtype=torch.int64, device=dev) if profile else None
    if profile:
        _lib.load().di2p_solver_set_profile_buffer(prof.data_ptr())
    try:
        with _lib.option("solver_tier_sweeps", tier):
            params, cost, iters = ops.solve_batched(*args, sweeps=sweeps)
        torch.cuda.synchronize()
    finally:
        if profile:
            _lib.load().di2p_solver_set_profile_buffer(None)
    return Result(params.cpu().numpy(), cost.cpu().numpy(), iters.cpu().numpy(), sweeps.cpu().numpy(), prof.cpu().numpy() if profile else None)


_RUNS = {}


def _run(dev, case, f32):
    """the plain single-launch solve of a case: run once, shared (read-only) by the tests below"""
    key = (case.name, f32)
    if key not in _RUNS:
        r = _solve(dev, _args(dev, [lc.inputs(case, f32)], f32, case.max_iter, case.is_2d))
        for a in (r.params, r.cost, r.iters, r.sweeps):
            a.setflags(write=False)
        _RUNS[key] = r
    return _RUNS[key]


def _compare(case, f32, g, key, f=0):
    """the comparison every test shares: forks enumerated; iters, sweeps, cost where the iterates agree; translations inside the box"""
    inp, o = lc.inputs(case, f32), lc.oracle(case.name, f32)
    pg, cg, ig, sg = g.params[f], g.cost[f], g.iters[f], g.sweeps[f]
    print("%s %s\n  iters hip %s\n  iters ref %s\n  sweeps hip %s\n  1+evals   %s\n  cost hip %s\n  cost ref %s\n  |dparam| %s"
          % (key, o.terms, ig.tolist(), o.iters.tolist(), sg.tolist(), (1 + o.stats["trial_evals"]).tolist(), cg.tolist(), o.cost.tolist(),
             np.abs(pg - o.params).max(1).tolist()))
    assert np.all(np.isfinite(pg))
    ok = _agreement(o.params, pg, case.is_2d) & (ig == o.iters) & (sg == 1 + o.stats["trial_evals"])
    _check_forks(key, ok)
    fin = np.isfinite(o.cost)
    np.testing.assert_array_equal(np.isfinite(cg), fin)
    m = ok & fin
    assert np.all(np.abs(cg[m] - o.cost[m]) <= COST_RTOL * np.abs(o.cost[m]) + COST_ATOL), (cg[m], o.cost[m])
    toff = 1 if case.is_2d else 3
    assert np.all(pg[:, toff:] >= np.array(inp.lb)) and np.all(pg[:, toff:] <= np.array(inp.ub))
    return ok


@pytest.mark.parametrize("f32", DTYPES, ids=_ids)
@pytest.mark.parametrize("case", lc.CASES, ids=_cid)
def test_exit_matches_oracle(dev, case, f32):
    """Every case of the table: the hypothesis ends where the oracle's does, after the same number of iterations AND sweeps (the sweep identity of
    the module docstring), at the same cost, inside the box."""
    _compare(case, f32, _run(dev, case, f32), (case.name, f32))


@pytest.mark.parametrize("f32", DTYPES, ids=_ids)
@pytest.mark.parametrize("case", [c for c in lc.CASES if c.max_iter == 0], ids=_cid)
def test_max_iter_zero_returns_the_projected_start(dev, case, f32):
    inp, o, g = lc.inputs(case, f32), lc.oracle(case.name, f32), _run(dev, case, f32)
    assert g.params[0].tobytes() == lc.project_start(inp, case.is_2d).tobytes()
    assert np.all(g.iters[0] == 0) and np.all(g.sweeps[0] == 1)
    assert np.all(np.abs(g.cost[0] - o.cost) <= 1e-9 * np.abs(o.cost)), (g.cost[0], o.cost)      # the tolerance of test_residuals_match_oracle


@pytest.mark.parametrize("f32", DTYPES, ids=_ids)
@pytest.mark.parametrize("case", [c for c in lc.CASES if set(c.terms) == {"eval_fail"}], ids=_cid)
def test_eval_fail_at_the_start(dev, case, f32):
    inp, o, g = lc.inputs(case, f32), lc.oracle(case.name, f32), _run(dev, case, f32)
    assert np.all(o.iters == 0) and np.all(g.iters[0] == 0) and np.all(g.sweeps[0] == 1)
    assert not np.isfinite(o.cost).any() and not np.isfinite(g.cost[0]).any()
    assert g.params[0].tobytes() == lc.project_start(inp, case.is_2d).tobytes()


@pytest.mark.parametrize("f32", DTYPES, ids=_ids)
@pytest.mark.parametrize("case", [c for c in lc.CASES if c.name.startswith("gt_start")], ids=_cid)
def test_gradient_tol_at_the_start(dev, case, f32):
    inp, o, g = lc.inputs(case, f32), lc.oracle(case.name, f32), _run(dev, case, f32)
    assert o.terms == ("gradient_tol",) * 2 and np.all(o.iters == 0) and np.all(o.cost == 0.0)
    assert np.all(g.iters[0] == 0) and np.all(g.sweeps[0] == 1) and np.all(g.cost[0] == 0.0)
    assert g.params[0].tobytes() == lc.project_start(inp, case.is_2d).tobytes()


@pytest.mark.parametrize("f32", DTYPES, ids=_ids)
@pytest.mark.parametrize("case", lc.LADDER, ids=_cid)
def test_ladder_within_rounding_noise(dev, case, f32):
    """max_iter = 1, 2, 3, 5 from one set of starts: parameters and cost after EXACTLY that many iterations agree with the oracle to 16 x the
    oracle's own spread over point orders (the table's noise figures; floor 1e-12).  A wrong step, radius or scaling shows at the iteration where it
    happens, before convergence hides it."""
    o, g = lc.oracle(case.name, f32), _run(dev, case, f32)
    tol_p, tol_c = lc.ladder_tolerance(case)
    dp = np.abs(g.params[0] - o.params).max(1)
    dc = np.abs(g.cost[0] - o.cost) / np.abs(o.cost)
    print("%s %s: |dparam| %s (tolerance %.1e), relative |dcost| %s (tolerance %.1e)" % (case.name, _ids(f32), dp.tolist(), tol_p, dc.tolist(), tol_c))
    np.testing.assert_array_equal(g.iters[0], case.max_iter)
    assert np.all(dp <= tol_p) and np.all(dc <= tol_c)


@pytest.mark.parametrize("f32", DTYPES, ids=_ids)
@pytest.mark.parametrize("case", lc.CASES, ids=_cid)
def test_line_search_counters_match_oracle(dev, case, f32):
    """The PROFILE instantiation's own counters (profile word 7: trials beyond the first in bits 0-19, accepts at a trial other than the first in
    bits 20-39) equal the oracle's for every hypothesis whose iterate agrees; the profiled solve returns the bits of the plain one."""
    o, plain = lc.oracle(case.name, f32), _run(dev, case, f32)
    g = _solve(dev, _args(dev, [lc.inputs(case, f32)], f32, case.max_iter, case.is_2d), profile=True)
    assert g.bytes() == plain.bytes()
    w7 = g.prof[:, 7]
    extra, late = w7 & 0xFFFFF, (w7 >> 20) & 0xFFFFF
    ok = _agreement(o.params, g.params[0], case.is_2d) & (g.iters[0] == o.iters) & (g.sweeps[0] == 1 + o.stats["trial_evals"])
    _check_forks((case.name, f32), ok)
    print("%s %s: ls_extra hip %s ref %s, ls_late_accept hip %s ref %s" % (case.name, _ids(f32), extra.tolist(), o.stats["ls_extra"].tolist(),
                                                                         late.tolist(), o.stats["ls_late_accept"].tolist()))
    np.testing.assert_array_equal(extra[ok], o.stats["ls_extra"][ok])
    np.testing.assert_array_equal(late[ok], o.stats["ls_late_accept"][ok])


@pytest.mark.parametrize("f32", DTYPES, ids=_ids)
@pytest.mark.parametrize("case", lc.TIER, ids=_cid)
def test_resumed_hypotheses_match_oracle(dev, case, f32):
    """solver_tier_sweeps = 8: the first launch parks every hypothesis that needs more sweeps and the wide kernels (12 waves per hypothesis in 2-D,
    8 in 3-D) resume them from the parked LM state.  The RESUMED results against the oracle by the same rules: equal iteration and sweep counts,
    1e-3 / 1e-6.  N = 130 leaves most waves of the wide kernels without a cluster."""
    g = _solve(dev, _args(dev, [lc.inputs(case, f32)], f32, case.max_iter, case.is_2d), tier=TIER_SWEEPS)
    o = lc.oracle(case.name, f32)
    assert (1 + o.stats["trial_evals"] > TIER_SWEEPS).sum() >= 4              # the oracle says so, and ...
    ok = _compare(case, f32, g, (case.name, f32, "tier"))
    assert (g.sweeps[0][ok] > TIER_SWEEPS).sum() >= 4                          # ... hypotheses WERE parked and resumed


def test_frames_of_a_batch_are_independent(dev):
    """Three different frames (padded to one N with label-2 points) in one F = 3 call: every frame's parameters, costs, iteration and sweep counts
    are bit-identical to its own F = 1 call."""
    names = ("ordinary-2d", "n130-2d", "far5-2d")
    inps = [lc.inputs(lc.BY_NAME[n], True) for n in names]
    N = max(i.points.shape[1] for i in inps)
    padded = []
    for i in inps:
        n = i.points.shape[1]
        pts, lab = np.zeros((3, N)), np.full((N,), 2, np.int32)
        pts[:, :n], lab[:n] = i.points, i.labels
        padded.append(i._replace(points=pts, labels=lab))
    assert len({(i.H, i.W, i.lb, i.ub, i.ys.shape) for i in padded}) == 1
    both = _solve(dev, _args(dev, padded, True, 500, True))
    assert len(set(both.bytes(f)[0] for f in range(3))) == 3
    for f in range(3):
        alone = _solve(dev, _args(dev, [padded[f]], True, 500, True))
        assert alone.bytes(0) == both.bytes(f), names[f]
        assert alone.sweeps.max() > 8
