"""CPU: holds the oracle to the case table of tests/solver_lm_cases.py, so that what tests/test_gpu_solver_lm.py believes it exercises is what it
exercises: for both point precisions every hypothesis of every case takes exactly the declared exit, every declared branch counter is hit, the
table as a whole covers the exits and counters it lists, and the rounding-noise scale of every ladder rung -- measured on the oracle alone, over
point orders -- stays below the figure the GPU tolerance is derived from."""
import numpy as np
import pytest

from oracle import frustum_lm as flm
from tests import solver_lm_cases as lc

PRECISIONS = [False, True]
_ids = lambda f32: "f32" if f32 else "f64"


@pytest.mark.parametrize("f32", PRECISIONS, ids=_ids)
@pytest.mark.parametrize("case", lc.CASES, ids=lambda c: c.name)
def test_oracle_takes_the_declared_exit_and_branches(case, f32):
    inp = lc.inputs(case, f32)
    N, R = inp.points.shape[1], inp.ys.shape[0]
    assert N <= 2048 and R <= 8 and len(case.terms) == R
    o = lc.oracle(case.name, f32)
    assert o.terms == case.terms, (o.terms, o.iters.tolist())
    for name in case.counters:
        assert o.stats[name].max() > 0, name
    # the counters are consistent with each other and with n_eval's definition
    st = o.stats
    assert np.all(st["ls_extra"] <= st["trial_evals"]) and np.all(st["ls_late_accept"] <= st["ls_extra"])
    assert np.all(st["trial_evals"] - st["ls_extra"] + st["invalid"] == o.iters)       # one first trial per iteration with a valid step
    assert np.all(st["ls_giveup"] + st["ls_min_step"] + st["ls_late_accept"] <= o.iters)
    toff = 1 if case.is_2d else 3
    lb, ub = np.array(inp.lb), np.array(inp.ub)
    t = o.params[:, toff:]
    assert np.all((t >= lb) & (t <= ub))
    np.testing.assert_array_equal(st["on_bound"], ((t == lb) | (t == ub)).any(1).astype(np.int32))
    if case.max_iter == 0 or set(case.terms) <= {"eval_fail", "invalid_steps"}:          # nothing moved: the projected start
        np.testing.assert_array_equal(o.params, lc.project_start(inp, case.is_2d))


def test_table_covers_what_it_lists():
    exits, counters, late_gradient, early_gradient = set(), set(), False, False
    for case in lc.CASES:
        for f32 in PRECISIONS:
            o = lc.oracle(case.name, f32)
            exits |= set(case.terms)
            counters |= set(case.counters)
            for r, t in enumerate(case.terms):
                late_gradient |= t == "gradient_tol" and o.iters[r] > 0
                early_gradient |= t == "gradient_tol" and o.iters[r] == 0
    assert exits == set(lc.COVERED_EXITS)
    assert counters == set(lc.COVERED_COUNTERS)
    assert late_gradient and early_gradient                      # gradient_tol at iteration 0 and later
    assert set(lc.COVERED_EXITS) | set(lc.NOT_REACHED_EXITS) == set(flm.TERM_NAMES)
    assert set(lc.COVERED_COUNTERS) == set(flm.STAT_NAMES)
    assert {"max_iter", "gradient_tol", "parameter_tol", "function_tol", "eval_fail"} <= set(lc.COVERED_EXITS)
    # the ladder: max_iter 0, 1, 2, 3, 5 in both dimensions; the tier cases: N = 130, 1024, 2048 in both dimensions
    assert sorted((c.max_iter, c.is_2d) for c in lc.CASES if c.name.startswith("ladder")) == sorted((k, d) for k in (0, 1, 2, 3, 5) for d in (True, False))
    assert sorted((lc.inputs(c, False).points.shape[1], c.is_2d) for c in lc.TIER) == sorted((n, d) for n in (130, 1024, 2048) for d in (True, False))


@pytest.mark.parametrize("f32", PRECISIONS, ids=_ids)
@pytest.mark.parametrize("case", lc.LADDER, ids=lambda c: c.name)
def test_ladder_noise_scale(case, f32):
    """The oracle against itself on 8 other point orders: the spread is the rounding-noise scale of this rung.  The table's figure (which the GPU
    tolerance multiplies by 16) must not be below it, and a spread above 1e-6 means the rung sits on a discontinuity of the objective."""
    par, cost = lc.measure_noise(case, f32)
    print("%s %s: parameter spread %.3e, relative cost spread %.3e (table: %.0e, %.0e)" % ((case.name, _ids(f32), par, cost) + case.noise))
    assert par <= lc.NOISE_LIMIT and cost <= lc.NOISE_LIMIT
    assert par <= case.noise[0] and cost <= case.noise[1]
    assert all(t == "max_iter" for t in case.terms)


def test_stats_entry_returns_the_same_iterates():
    """solve_restarts(..., return_stats=True) goes through another C entry point: same bits as the plain one"""
    case = lc.BY_NAME["ordinary-2d"]
    inp = lc.inputs(case, False)
    a = flm.solve_restarts(inp.points, inp.labels, inp.K, inp.ys, inp.Ts, inp.H, inp.W, inp.lb, inp.ub, case.max_iter, True, nthreads=2)
    b = flm.solve_restarts(inp.points, inp.labels, inp.K, inp.ys, inp.Ts, inp.H, inp.W, inp.lb, inp.ub, case.max_iter, True, nthreads=2, return_stats=True)
    assert len(a) == 5 and len(b) == 6 and sorted(b[5]) == sorted(flm.STAT_NAMES)
    for u, v in zip(a, b):
        assert u.tobytes() == v.tobytes()
