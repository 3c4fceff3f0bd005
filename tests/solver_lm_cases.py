"""The solves that put every reachable exit and line-search branch of the LM lane of solver.hip under an oracle comparison.  No GPU code.

A case is a deterministic builder of one frame with its R start hypotheses, plus a DECLARATION of what the oracle (oracle/frustum_lm.cpp) does
on it: the exit of every hypothesis (`terms`, names of flm.TERM_NAMES) and the branch counters (names of flm.STAT_NAMES) that are > 0 for at
least one hypothesis.  tests/test_solver_lm_cases_host.py holds the oracle to the declarations for both point precisions, so the table cannot
drift away from what tests/test_gpu_solver_lm.py believes it exercises; a case whose declaration stops holding fails before a GPU is needed.

Point precision: the kernel has a float64 and a float32 record path.  `inputs(case, f32=True)` rounds the points to float32 and widens them
back, so the oracle and the float32 kernel are fed the SAME values.  (synthetic.make_frame already returns float32 coordinates: only the cases
that rescale points differ between the two precisions.)

Ladder cases (`ladder<k>`: max_iter = k from one fixed set of starts) carry the oracle's own rounding-noise scale: the largest spread of the
parameters and of the relative cost over the frame and 8 fixed permutations of its point order (same values, another summation order),
measured by the host test, which fails when the table's figure is below what it measures.  The GPU ladder tolerance is 16 x that figure."""
import functools
from collections import namedtuple

import numpy as np

from deepi2p_amd import synthetic
from oracle import frustum_lm as flm

H, W = 160, 512
LB, UB = (-5.0, -0.1, -10.0), (5.0, 0.1, 10.0)

Inputs = namedtuple("Inputs", "points labels K ys Ts H W lb ub")
# terms: one exit name per hypothesis; counters: branch counters that must be > 0 in some hypothesis; noise: (params, relative cost) of a ladder rung
Case = namedtuple("Case", "name is_2d max_iter build terms counters noise tier")

N_PERM = 8                  # point-order permutations of the noise measurement
NOISE_FACTOR = 16.0         # GPU ladder tolerance = NOISE_FACTOR x measured spread ...
NOISE_FLOOR = 1e-12         # ... with this floor, absolute (parameters) and relative (cost)
NOISE_LIMIT = 1e-6          # a rung whose spread exceeds this sits on a discontinuity of the objective: pick another start, do not widen


# ------------------------------------------------------------------------------------------------------------------------- builders
@functools.lru_cache(maxsize=None)
def _frame(seed, N, flip=0.0):
    f = synthetic.make_frame(np.random.default_rng(seed), N=N, H=H, W=W, flip=flip, with_image=False)
    return f


def _base(N=1024, seed=11):
    f = _frame(seed, N)
    return f["pc"].astype(np.float64), f["labels"].astype(np.int32), f["K"], f["yaw_gt"], f["P_gt"][:3, 3].copy()


def _starts(yg, tg, R=6):
    """hypothesis 0 starts 0.1 rad / 0.5 m off the ground truth, the others further out"""
    d = np.arange(R, dtype=np.float64)
    return yg + 0.1 + 0.02 * d, tg[None] + 0.5 + 0.1 * d[:, None]


def _mk(pts, lab, K, ys, Ts, lb=LB, ub=UB):
    return Inputs(np.ascontiguousarray(pts, np.float64), np.ascontiguousarray(lab, np.int32), np.ascontiguousarray(K, np.float64),
                  np.ascontiguousarray(ys, np.float64), np.ascontiguousarray(Ts, np.float64), H, W, tuple(lb), tuple(ub))


def b_ordinary(N=1024):
    pts, lab, K, yg, tg = _base(N)
    return _mk(pts, lab, K, *_starts(yg, tg))


def b_gt_start():
    pts, lab, K, yg, tg = _base()
    return _mk(pts, lab, K, np.full(2, yg), np.tile(tg, (2, 1)))


def b_all_outside():
    pts, lab, K, yg, tg = _base()
    return _mk(pts, np.zeros_like(lab), K, np.full(2, yg), np.tile(tg, (2, 1)))


def b_far5():
    pts, lab, K, yg, tg = _base()
    pts = pts.copy()
    pts[:, :5] *= 1e6
    return _mk(pts, lab, K, *_starts(yg, tg))


def b_origin():
    """point 0 at the origin, yaw 0, T 0: it lies in the camera centre, depth 0 -> the first evaluation is not finite"""
    pts, lab, K, yg, tg = _base()
    pts = pts.copy()
    pts[:, 0] = 0.0
    return _mk(pts, lab, K, np.zeros(2), np.zeros((2, 3)))


def b_tiny(n):
    pts, lab, K, yg, tg = _base()
    return _mk(pts[:, :n], np.array([1, 0], np.int32)[:n], K, *_starts(yg, tg))


def b_pinned():
    pts, lab, K, yg, tg = _base()
    return _mk(pts, lab, K, *_starts(yg, tg), lb=(0.0, 0.0, 0.0), ub=(0.0, 0.0, 0.0))


def b_scaled():
    pts, lab, K, yg, tg = _base()
    ys, Ts = _starts(yg, tg)
    return _mk(pts * 1e4, lab, K, ys, Ts * 1e4, lb=[v * 1e4 for v in LB], ub=[v * 1e4 for v in UB])


def b_outside_box():
    """every start lies outside the box in all three translation components: the solve begins at its projection"""
    pts, lab, K, yg, tg = _base()
    ys, Ts = _starts(yg, tg)
    return _mk(pts, lab, K, ys, Ts + np.array([20.0, -3.0, 30.0]))


def b_depth_face(seed, lab0):
    """Point 0 at the origin and the box face z >= 0: an iterate that a step pushes through the face is clamped ONTO it, where point 0 has depth
    0 and the evaluation is not finite -- an invalid line-search sample, which halves the step (the bisection fallback), and repeatedly so
    (a search abandoned after 20 trials)."""
    rng = np.random.default_rng(2000 + seed)
    f = synthetic.make_frame(rng, N=256, H=H, W=W, flip=0.0, with_image=False)
    pts, lab = f["pc"].astype(np.float64), f["labels"].astype(np.int32)
    pts[:, 0] = 0.0
    lab[0] = lab0
    R = 8
    ys = f["yaw_gt"] + rng.normal(0, 0.3, R)
    Ts = np.stack((rng.uniform(-3, 3, R), np.zeros(R), rng.uniform(0.5, 6, R)), 1)
    return _mk(pts, lab, f["K"], ys, Ts, lb=(-5.0, -0.1, 0.0), ub=(5.0, 0.1, 10.0))


def b_tiny_depth():
    """Point 0 (label 1) at the origin seen from T = (1e-20, 0, 1e-155 | 1e-160): its pixel is finite (5e137), every Jacobian entry is finite
    (5e292), but J^T J overflows.  The Jacobi scale of that column is 0, the scaled matrix holds 0 * inf = NaN, the Cholesky factorisation fails:
    five invalid steps in a row."""
    pts, lab, K, yg, tg = _base()
    pts = pts.copy()
    lab = lab.copy()
    pts[:, 0] = 0.0
    lab[0] = 1
    return _mk(pts, lab, K, np.zeros(2), np.array([[1e-20, 0.0, 1e-155], [1e-20, 0.0, 1e-160]]))


# --------------------------------------------------------------------------------------------------------------------------- the table
_MI, _G, _P, _F, _E, _I = "max_iter", "gradient_tol", "parameter_tol", "function_tol", "eval_fail", "invalid_steps"
CASES = []          # filled below


def _add(name, is_2d, max_iter, build, terms, counters=(), noise=None, tier=0):
    CASES.append(Case("%s-%s" % (name, "2d" if is_2d else "3d"), is_2d, max_iter, build, tuple(terms), tuple(counters), noise, tier))


# counters every converging frame of the family exercises
_LS = ("trial_evals", "ls_extra", "ls_late_accept", "ls_min_step", "rejected", "on_bound")

for _d in (True, False):
    _add("gt_start", _d, 500, b_gt_start, (_G,) * 2)                                # gradient_tol at iteration 0, cost 0
    _add("origin", _d, 500, b_origin, (_E,) * 2)                                    # eval_fail at iteration 0, cost NaN
    _add("tiny_depth", _d, 500, b_tiny_depth, (_I,) * 2, ("invalid",))              # five invalid steps: iters 5, no trial evaluation
    _add("ladder0", _d, 0, b_ordinary, (_MI,) * 6, ("on_bound",))
# ladder rungs: noise = (parameter spread, relative cost spread) over 1 + N_PERM point orders, measured values rounded UP to one digit
_add("ladder1", True, 1, b_ordinary, (_MI,) * 6, ("trial_evals", "on_bound"), noise=(4e-13, 2e-14))
_add("ladder1", False, 1, b_ordinary, (_MI,) * 6, ("trial_evals", "ls_extra", "ls_late_accept"), noise=(6e-13, 2e-13))
_add("ladder2", True, 2, b_ordinary, (_MI,) * 6, ("trial_evals", "on_bound"), noise=(4e-13, 2e-14))
_add("ladder2", False, 2, b_ordinary, (_MI,) * 6, ("trial_evals", "ls_extra", "ls_late_accept"), noise=(5e-11, 2e-12))
_add("ladder3", True, 3, b_ordinary, (_MI,) * 6, ("trial_evals", "ls_extra", "ls_late_accept"), noise=(2e-13, 4e-14))
_add("ladder3", False, 3, b_ordinary, (_MI,) * 6, ("trial_evals", "ls_extra", "ls_late_accept"), noise=(2e-10, 4e-12))
_add("ladder5", True, 5, b_ordinary, (_MI,) * 6, ("trial_evals", "ls_extra", "ls_late_accept"), noise=(2e-13, 3e-13))
_add("ladder5", False, 5, b_ordinary, (_MI,) * 6, ("trial_evals", "ls_extra", "ls_late_accept"), noise=(2e-9, 3e-11))
# the ordinary frame, N = 1024 / 130 (3 clusters: idle waves in the wide tier's reduction) / 2048; tier = 1: also run through the two-tier launch
_add("ordinary", True, 500, b_ordinary, (_G, _F, _F, _P, _G, _P), _LS, tier=1)
_add("ordinary", False, 500, b_ordinary, (_F,) * 6, _LS, tier=1)
_add("n130", True, 500, functools.partial(b_ordinary, 130), (_F, _F, _F, _P, _P, _F), _LS, tier=1)
_add("n130", False, 500, functools.partial(b_ordinary, 130), (_F, _P, _F, _P, _P, _P), _LS, tier=1)
_add("n2048", True, 500, functools.partial(b_ordinary, 2048), (_F, _F, _P, _F, _F, _F), _LS, tier=1)
_add("n2048", False, 500, functools.partial(b_ordinary, 2048), (_F,) * 6, _LS, tier=1)
# every label 0 from the ground truth: 3-D ends by gradient_tol after 3 iterations (gradient_tol AFTER iteration 0), 2-D by function_tol
_add("all_outside", True, 500, b_all_outside, (_F,) * 2, ("ls_extra", "ls_min_step", "rejected"))
_add("all_outside", False, 500, b_all_outside, (_G,) * 2, ("trial_evals",))
# five points 1e6 times further out: hypothesis 0 of the 2-D solve ends by gradient_tol after 11 iterations
_add("far5", True, 500, b_far5, (_G, _P, _P, _P, _G, _P), _LS)
_add("far5", False, 500, b_far5, (_F,) * 6, _LS)
# one point (label 1) / two points (labels 1, 0): rank-deficient, the steps shrink until parameter_tol
_add("n1", True, 500, functools.partial(b_tiny, 1), (_P,) * 6, ("trial_evals", "on_bound"))
_add("n1", False, 500, functools.partial(b_tiny, 1), (_P, _P, _F, _P, _P, _P), ("ls_extra", "ls_late_accept", "rejected"))
_add("n2", True, 500, functools.partial(b_tiny, 2), (_P,) * 6, ("trial_evals", "on_bound"))
_add("n2", False, 500, functools.partial(b_tiny, 2), (_P, _P, _F, _P, _P, _P), ("ls_extra", "ls_late_accept", "rejected"))
# lb = ub = 0: every translation pinned on its bound, only the rotation moves
_add("pinned", True, 500, b_pinned, (_P, _F, _F, _F, _F, _F), _LS)
_add("pinned", False, 500, b_pinned, (_F, _F, _F, _P, _F, _F), _LS)
# points, translations and box times 1e4
_add("scaled", True, 500, b_scaled, (_F, _P, _F, _P, _F, _F), ("ls_extra", "ls_late_accept", "rejected", "on_bound"))
_add("scaled", False, 500, b_scaled, (_F,) * 6, _LS)
# starts outside the box: the projected start
_add("outside_box", True, 500, b_outside_box, (_F, _G, _F, _F, _P, _P), ("ls_extra", "ls_late_accept", "ls_min_step", "on_bound"))
_add("outside_box", False, 500, b_outside_box, (_P, _F, _F, _F, _F, _F), _LS)
# invalid line-search samples on the box face z = 0 (b_depth_face): the bisection fallback and searches abandoned after 20 trials
_add("face0", True, 100, functools.partial(b_depth_face, 0, 0), (_F, _F, _P, _P, _P, _P, _F, _F), ("ls_bisect", "ls_min_step", "rejected"))
_add("face4", True, 100, functools.partial(b_depth_face, 4, 1), (_F,) * 8, ("ls_giveup", "ls_bisect", "rejected"))
_add("face10", False, 100, functools.partial(b_depth_face, 10, 0), (_F,) * 8, ("ls_giveup", "ls_bisect", "ls_min_step", "rejected"))

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
LADDER = [c for c in CASES if c.noise is not None]
TIER = [c for c in CASES if c.tier]
# what the table covers: the host test holds the oracle to it and fails if a case that carried an entry is dropped
COVERED_EXITS = (_MI, _G, _P, _F, _E, _I)
COVERED_COUNTERS = ("trial_evals", "ls_extra", "ls_late_accept", "ls_giveup", "ls_min_step", "ls_bisect", "rejected", "invalid", "on_bound")
# not reached through the public arguments ("LM exits and branches under test"): no case, no GPU test
NOT_REACHED_EXITS = ("min_radius",)


def inputs(case, f32):
    inp = case.build()
    if f32:
        inp = inp._replace(points=inp.points.astype(np.float32).astype(np.float64))
    return inp


Oracle = namedtuple("Oracle", "cost iters terms params stats")


def run_oracle(inp, is_2d, max_iter, perm=None):
    pts, lab = inp.points, inp.labels
    if perm is not None:
        pts, lab = np.ascontiguousarray(pts[:, perm]), np.ascontiguousarray(lab[perm])
    _, cost, iters, term, params, stats = flm.solve_restarts(pts, lab, inp.K, inp.ys, inp.Ts, inp.H, inp.W, inp.lb, inp.ub, max_iter, is_2d,
                                                             nthreads=4, return_stats=True)
    return Oracle(cost, iters, tuple(flm.TERM_NAMES[t] for t in term), params, stats)


@functools.lru_cache(maxsize=None)
def oracle(name, f32):
    """the oracle's result on a case, computed once per session and shared (read-only) by every test that needs it"""
    case = BY_NAME[name]
    out = run_oracle(inputs(case, f32), case.is_2d, case.max_iter)
    for a in (out.cost, out.iters, out.params) + tuple(out.stats.values()):
        a.setflags(write=False)
    return out


def permutations(N):
    rng = np.random.default_rng(777)
    return [rng.permutation(N) for _ in range(N_PERM)]


def measure_noise(case, f32):
    """(largest parameter spread, largest relative cost spread) of the oracle over the frame and N_PERM permutations of its point order"""
    inp = inputs(case, f32)
    outs = [run_oracle(inp, case.is_2d, case.max_iter)] + [run_oracle(inp, case.is_2d, case.max_iter, p) for p in permutations(inp.points.shape[1])]
    par = np.stack([o.params for o in outs])
    cost = np.stack([o.cost for o in outs])
    return float((par.max(0) - par.min(0)).max()), float(((cost.max(0) - cost.min(0)) / np.abs(cost).min(0)).max())


def ladder_tolerance(case):
    return max(NOISE_FACTOR * case.noise[0], NOISE_FLOOR), max(NOISE_FACTOR * case.noise[1], NOISE_FLOOR)


def project_start(inp, is_2d):
    """the start the solve begins at: rotation (0, yaw, 0) | yaw, translation clamped onto the box"""
    T = np.minimum(np.maximum(inp.Ts, np.array(inp.lb)), np.array(inp.ub))
    R = inp.ys.shape[0]
    rot = inp.ys[:, None] if is_2d else np.stack((np.zeros(R), inp.ys, np.zeros(R)), 1)
    return np.concatenate((rot, T), 1)
