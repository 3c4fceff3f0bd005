// The Levenberg-Marquardt lane of the pose solver (included by solver.hip only): what ONE lane -- for the polynomial minimiser, one wave --
// does between two sweeps of a hypothesis: damped Cholesky step, box projection, Armijo search with Ceres' cubic interpolation, accept /
// reject, termination tests.  It uses nothing of the sweep; tests/test_gpu_solver_lm.py compares it with the oracle exit by exit.
#pragma once
#include "solver_model.h"

namespace {

enum { T_MAX_ITER = 0, T_GRADIENT = 1, T_PARAMETER = 2, T_FUNCTION = 3, T_RADIUS = 4, T_INVALID = 5, T_EVAL_FAIL = 6 };

// Division and square root of the LM update's linear solve: reciprocal / reciprocal square root + Newton corrections (<= 1 ulp) instead of
// the IEEE sequences (~25 instructions each with their scaling and fix-up steps) -- 16 of them sit on the critical lane per LM iteration
// (finish + begin 5.8 k -> 4.9 k cycles per sweep).  The HIP-vs-oracle agreement is unchanged hypothesis for hypothesis, iteration
// counts included (tools/solver_oracle_agreement.py, tools/ab_fastdiv.sh); -DDI2P_SOLVER_IEEEDIV restores the IEEE forms.
#ifndef DI2P_SOLVER_IEEEDIV
#define DI2P_SOLVER_FASTDIV 1
#endif
__device__ __forceinline__ double lm_div(double a, double b) {
#ifdef DI2P_SOLVER_FASTDIV
    const double r = fast_rcp(b), q = a * r;
    return fma(fma(-b, q, a), r, q);
#else
    return a / b;
#endif
}
__device__ __forceinline__ double lm_sqrt(double a) {
#ifdef DI2P_SOLVER_FASTDIV
    const double y = __builtin_amdgcn_rsq(a);
    double g = a * y, h = 0.5 * y;
    const double r = fma(-h, g, 0.5);
    g = fma(g, r, g); h = fma(h, r, h);
    const double v = fma(fma(-g, g, a), h, g);
    return a == 0.0 ? 0.0 : v;              // rsq(0) = inf would turn sqrt(0) into NaN: a zero step / iterate norm must satisfy the parameter tolerance
#else
    return sqrt(a);
#endif
}

// Cholesky solve of M y = rhs IN PLACE: M (lower triangle, row-major) is overwritten by its factor L, y holds rhs on entry and the
// solution on return (forward substitution, then backward substitution, both in place).  Same operations in the same order as the
// oracle's chol_solve; written in place because the LM update runs on one lane of a kernel whose register budget is set by the sweep --
// separate M / L / z arrays pushed it into scratch.
template <int NP>
__device__ __forceinline__ bool chol_solve_inplace(double* M, double* y) {
#pragma unroll
    for (int i = 0; i < NP; ++i) {
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            double s = M[i * (i + 1) / 2 + j];
#pragma unroll
            for (int q = 0; q < j; ++q) s -= M[i * (i + 1) / 2 + q] * M[j * (j + 1) / 2 + q];
            if (i == j) {
                if (!(s > 0.0) || !isfinite(s)) return false;
                M[i * (i + 1) / 2 + i] = lm_sqrt(s);
            } else {
                M[i * (i + 1) / 2 + j] = lm_div(s, M[j * (j + 1) / 2 + j]);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        double s = y[i];
#pragma unroll
        for (int q = 0; q < i; ++q) s -= M[i * (i + 1) / 2 + q] * y[q];
        y[i] = lm_div(s, M[i * (i + 1) / 2 + i]);
    }
#pragma unroll
    for (int i = NP - 1; i >= 0; --i) {
        double s = y[i];
#pragma unroll
        for (int q = i + 1; q < NP; ++q) s -= M[q * (q + 1) / 2 + i] * y[q];
        y[i] = lm_div(s, M[i * (i + 1) / 2 + i]);
    }
    bool ok = true;
#pragma unroll
    for (int i = 0; i < NP; ++i) ok &= isfinite(y[i]);
    return ok;
}

template <int NP>
__device__ __forceinline__ void plus_proj(const double* x, const double* d, double t, const double* lb, const double* ub, double* out) {
#pragma unroll
    for (int i = 0; i < NP; ++i) out[i] = fmin(fmax(x[i] + t * d[i], lb[i]), ub[i]);
}

template <int NP>
__device__ __forceinline__ double grad_max_norm(const double* x, const double* g, const double* lb, const double* ub) {
    double m = 0.0;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const double pr = fmin(fmax(x[i] - g[i], lb[i]), ub[i]);
        m = fmax(m, fabs(x[i] - pr));
    }
    return m;
}


// ---------------------------------------------------------------------------------------------------------------------
// Ceres' ArmijoLineSearch with CUBIC interpolation (line_search.cc, polynomial.cc), same statement as the oracle's:
// the next step minimises, over [1e-3, 0.6] x current step, the polynomial interpolating value + directional derivative at
// step 0, at the current trial and (when valid) at the previous trial.  Fitted in u = step / current step with the two
// constraints at 0 eliminated; minimiser = best of {interval midpoint, ends, real critical points} (MinimizePolynomial).
// Runs on ONE lane between sweeps: loops are unrolled over compile-time indices so that everything stays in registers.
template <int DEG> __device__ __forceinline__ double poly_eval(const double* c, double u) {
    double v = c[DEG];
#pragma unroll
    for (int i = DEG - 1; i >= 0; --i) v = fma(v, u, c[i]);
    return v;
}

// ---- real critical points by the WHOLE wavefront (wave 0 runs this between sweeps; arguments are wave-uniform).
// Same statement as the oracle's real_roots_in(): the roots of q inside [a,b] are isolated between consecutive roots of q'
// (found the same way one degree down; degree 2 in closed form, as polynomial.cc's FindQuadraticPolynomialRoots), q is
// monotone on each piece, so a sign change pins exactly one root.  The oracle solves a piece by scalar Newton/bisection
// (~25 dependent fp64 divisions); here the 64 lanes sample the piece at 64 points, a ballot finds the sub-interval with the
// sign change (three rounds: 63^3 = 2.5e5 x narrower), and three Newton steps with a reciprocal finish it to rounding.
template <int DEG>
__device__ __forceinline__ double wave_bracket_root(const double* q, double l, double r, double ql) {
    const int lane = threadIdx.x & 63;
    const bool lneg = ql < 0.0;
#pragma unroll 1
    for (int round = 0; round < 3; ++round) {
        const double h = (r - l) * (1.0 / 63.0);
        const double u = fma((double)lane, h, l);
        const double v = poly_eval<DEG>(q, u);
        const unsigned long long same = __ballot(v != 0.0 && (v < 0.0) == lneg);       // monotone piece: a prefix of lanes
        const unsigned long long zero = __ballot(v == 0.0);
        if (zero) return fma((double)__builtin_ctzll(zero), h, l);                       // a sample hit the root exactly
        const int idx = same ? 63 - (int)__builtin_clzll(same) : 0;                      // last lane on the left side
        l = fma((double)idx, h, l);
        r = l + h;
    }
    double dq[DEG];
#pragma unroll
    for (int i = 1; i <= DEG; ++i) dq[i - 1] = i * q[i];
    double x = 0.5 * (l + r);
#pragma unroll
    for (int it = 0; it < 3; ++it) {
        const double qx = poly_eval<DEG>(q, x), d = poly_eval<DEG - 1>(dq, x);
        const double xn = fma(-qx, fast_rcp(d), x);
        x = (xn >= l && xn <= r) ? xn : x;         // NaN / runaway steps keep the bracketed iterate
    }
    return x;
}

template <int DEG> struct WaveRoots {
    __device__ __forceinline__ static void run(const double* q, double a, double b, bool* has, double* val) {
        if (q[DEG] == 0.0) {                                   // RemoveLeadingZeros (polynomial.cc)
            WaveRoots<DEG - 1>::run(q, a, b, has, val);
            has[DEG - 1] = false;
            return;
        }
        double dq[DEG], vc[DEG - 1];
        bool hc[DEG - 1];
#pragma unroll
        for (int i = 1; i <= DEG; ++i) dq[i - 1] = i * q[i];
        WaveRoots<DEG - 1>::run(dq, a, b, hc, vc);
        double l = a, ql = poly_eval<DEG>(q, a);
#pragma unroll
        for (int i = 0; i < DEG; ++i) {
            has[i] = false;
            const bool last = i == DEG - 1;
            if (last || hc[last ? 0 : i]) {                    // wave-uniform
                const double r = last ? b : vc[last ? 0 : i];
                const double qr = poly_eval<DEG>(q, r);
                if (ql == 0.0) { has[i] = true; val[i] = l; }
                else if (qr != 0.0 && (ql < 0.0) != (qr < 0.0)) { has[i] = true; val[i] = wave_bracket_root<DEG>(q, l, r, ql); }
                l = r; ql = qr;
            }
        }
    }
};
template <> struct WaveRoots<2> {      // closed form, the numerically stable pair of FindQuadraticPolynomialRoots; ascending, inside [a,b]
    __device__ __forceinline__ static void run(const double* q, double a, double b, bool* has, double* val) {
        has[0] = has[1] = false;
        if (q[2] == 0.0) {
            if (q[1] == 0.0) return;
            const double r = -q[0] / q[1];
            if (r >= a && r <= b) { has[0] = true; val[0] = r; }
            return;
        }
        const double D = q[1] * q[1] - 4.0 * q[2] * q[0];
        if (!(D >= 0.0)) return;
        const double sD = sqrt(D);
        const double t = q[1] >= 0.0 ? -q[1] - sD : -q[1] + sD;
        double r0 = t / (2.0 * q[2]), r1 = t != 0.0 ? (2.0 * q[0]) / t : r0;
        if (r0 > r1) { const double tmp = r0; r0 = r1; r1 = tmp; }
        if (r0 >= a && r0 <= b) { has[0] = true; val[0] = r0; }
        if (r1 >= a && r1 <= b && r1 != r0) { has[1] = true; val[1] = r1; }
        if (!has[0] && has[1]) { has[0] = true; val[0] = val[1]; has[1] = false; }
    }
};
template <> struct WaveRoots<1> {
    __device__ __forceinline__ static void run(const double* q, double a, double b, bool* has, double* val) {
        has[0] = false;
        if (q[1] == 0.0) return;
        const double r = -q[0] / q[1];
        if (r >= a && r <= b) { has[0] = true; val[0] = r; }
    }
};

// MinimizePolynomial (polynomial.cc): interval midpoint first, then both ends, then the critical points, strict "<".
// Called by every lane of wave 0 with the same arguments; returns the same value on every lane.
__device__ __forceinline__ double poly_min_on_wave(const double* p, double umin, double umax) {     // p: degree <= 5, ascending
    double best_u = 0.5 * (umin + umax), best_v = poly_eval<5>(p, best_u);
    const double vmin = poly_eval<5>(p, umin);
    if (vmin < best_v) { best_v = vmin; best_u = umin; }
    const double vmax = poly_eval<5>(p, umax);
    if (vmax < best_v) { best_v = vmax; best_u = umax; }
    double dp[5], val[4];
    bool has[4];
#pragma unroll
    for (int i = 1; i <= 5; ++i) dp[i - 1] = i * p[i];
    WaveRoots<4>::run(dp, umin, umax, has, val);
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (has[i]) {
            const double v = poly_eval<5>(p, val[i]);
            if (v < best_v) { best_v = v; best_u = val[i]; }
        }
    return best_u;
}

struct LsSample { double x, value, gradient; bool value_ok, grad_ok; };

// LineSearch::InterpolatingPolynomialMinimizingStepSize, CUBIC: p(u) = f0 + g0 xc u + u^2 (r0 + r1 u + r2 u^2 + r3 u^3) with one
// coefficient per valid constraint {cur value, cur gradient, prev value, prev gradient}; missing constraints pin the
// highest coefficients to zero (unit rows), so the 4x4 elimination below always runs on compile-time indices.
// -> true: p[0..5] holds the interpolant in u = step / cur.x, to be minimised over [min_step, max_step] / cur.x ; false: the next
// step is the bisection step (invalid current sample, or a non-finite fit).
__device__ __forceinline__ bool interpolating_fit(double f0, double g0, const LsSample& cur, const LsSample& prev, double* p) {
    if (!cur.value_ok) return false;
    const double xc = cur.x, G0 = g0 * xc;
    const double up = prev.value_ok ? lm_div(prev.x, xc) : 2.0;
    const bool valid[4] = {true, cur.grad_ok, prev.value_ok, prev.value_ok && prev.grad_ok};
    const int m = 1 + (valid[1] ? 1 : 0) + (valid[2] ? 1 : 0) + (valid[3] ? 1 : 0);
    double A[4][5];
    {
        const double us[4] = {1.0, 1.0, up, up};
        const double rhs[4] = {cur.value - f0 - G0, cur.gradient * xc - G0, prev.value - f0 - G0 * up, prev.gradient * xc - G0};
        int pad = m;                                           // next coefficient pinned to zero
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bool is_grad = (i & 1) != 0;
            double pw = is_grad ? us[i] : us[i] * us[i];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double e = is_grad ? (j + 2) * pw : pw;
                A[i][j] = valid[i] ? (j < m ? e : 0.0) : (j == pad ? 1.0 : 0.0);
                pw *= us[i];
            }
            A[i][4] = valid[i] ? rhs[i] : 0.0;
            if (!valid[i]) ++pad;
        }
    }
    // Gaussian elimination with partial pivoting
    bool singular = false;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        int piv = c;
        double pv = fabs(A[c][c]);
#pragma unroll
        for (int i = c + 1; i < 4; ++i) if (fabs(A[i][c]) > pv) { pv = fabs(A[i][c]); piv = i; }
        if (pv == 0.0) singular = true;
#pragma unroll
        for (int i = c + 1; i < 4; ++i)
            if (i == piv) {
#pragma unroll
                for (int j = 0; j < 5; ++j) { const double t = A[i][j]; A[i][j] = A[c][j]; A[c][j] = t; }
            }
        const double inv = singular ? 0.0 : lm_div(1.0, A[c][c]);
#pragma unroll
        for (int i = c + 1; i < 4; ++i) {
            const double f = A[i][c] * inv;
#pragma unroll
            for (int j = c; j < 5; ++j) A[i][j] -= f * A[c][j];
        }
    }
    double r[4] = {0.0, 0.0, 0.0, 0.0};
    if (!singular) {
#pragma unroll
        for (int c = 3; c >= 0; --c) {
            double v = A[c][4];
#pragma unroll
            for (int j = c + 1; j < 4; ++j) v -= A[c][j] * r[j];
            r[c] = lm_div(v, A[c][c]);
        }
    }
    p[0] = f0; p[1] = G0; p[2] = r[0]; p[3] = m > 1 ? r[1] : 0.0; p[4] = m > 2 ? r[2] : 0.0; p[5] = m > 3 ? r[3] : 0.0;
    bool fin = true;
#pragma unroll
    for (int j = 0; j < 6; ++j) if (!isfinite(p[j])) fin = false;
    return fin;
}

// Levenberg-Marquardt state of one hypothesis.  Lives ONCE per workgroup in LDS; thread 0 advances it between
// sweeps (a few hundred scalar flops), so the sweep's register budget is not shared with it.
enum { PH_INIT = 0, PH_TRIAL = 1 };
template <int NP>
struct LMState {
    double x[NP], g[NP], A[Tri<NP>::N], S[NP], diag[NP], delta[NP], xe[NP];
    double lb[NP], ub[NP];
    double cost, gmax, radius, decrease, gd, dmax, t, f1, model_change;
    int iter, nsweep, invalid_run, ls_it, phase, reuse_diag, ok1, done, max_iter;
    int want_j;        // what the NEXT sweep must produce: 2 = cost + gradient + normal equations, 1 = cost + gradient
    double g1[NP], A1[Tri<NP>::N];     // sums of the FIRST trial point (t = 1): the candidate when the line search fails
    double prev_t, prev_f, prev_g;     // previous line-search sample (step, cost, directional derivative)
    int prev_vok, prev_gok;
    double poly[6], tn;                // pending interpolant (u = step / t) for the wave-wide minimiser, and the step it returns
    int poly_req, pad_;
    int n_ls_extra, n_ls_late_accept, n_resweep;      // diagnostics: line-search trials beyond the first, accepted ones among them, re-sweeps
};

// Round 6: the LM stages fetch the state they work on from LDS IN ONE BATCH into registers (pinned: every load is issued, then one wait)
// instead of field by field between the arithmetic -- the update runs on one lane, so every LDS round trip it waits for (the copy loops
// alone were 14 read -> wait -> write pairs) is a round trip the whole workgroup waits for.  Same operations on the same values:
// bit-identical; finish + begin 8.5 k -> 7.5 k cycles per iteration (profiles/r06_c6_prepare.txt), no more scratch.
#ifdef DI2P_SOLVER_LMPROF
// variant build: cycles of the LM lane's sub-stages, summed over a hypothesis' iterations (tools/bench_solver.py LMPROF=1 prints them)
//   [0] finish_iteration  [1] begin: fetch + scaled matrix  [2] Cholesky solve  [3] model change  [4] begin: step, projection, stores
//   [5] decide without the fit  [6] interpolating fit  [7] trial_next_decide
__shared__ long long g_lmclk[8];
#define DI2P_LMSTAMP(t) long long t = clock64()                         // start a stamp
#define DI2P_LMRESTAMP(t) t = clock64()                                 // restart it
#define DI2P_LMCLK(i, t0) g_lmclk[i] += clock64() - (t0)                // add the time since a stamp to sub-stage i ...
#define DI2P_LMADD(field, t0) field += (int)(clock64() - (t0))          // ... or to a field of the LM state
#else
#define DI2P_LMSTAMP(t) ((void)0)
#define DI2P_LMRESTAMP(t) ((void)0)
#define DI2P_LMCLK(i, t0) ((void)0)
#define DI2P_LMADD(field, t0) ((void)0)
#endif
template <int N> __device__ __forceinline__ void pin_regs(double* v) {
#pragma unroll
    for (int i = 0; i < N; ++i) asm volatile("" : "+v"(v[i]));
}

template <int NP>
__device__ __forceinline__ void lm_begin_iteration(LMState<NP>& st) {
    constexpr int NT = Tri<NP>::N;
    const double kMinDiag = 1e-6, kMaxDiag = 1e32, kMinRadius = 1e-32, kGradTol = 1e-10;
    DI2P_LMSTAMP(tb0);
    double S[NP], A[NT], g[NP], diag[NP], sc[3];
#pragma unroll
    for (int a = 0; a < NP; ++a) { S[a] = st.S[a]; g[a] = st.g[a]; diag[a] = st.diag[a]; }
#pragma unroll
    for (int i = 0; i < NT; ++i) A[i] = st.A[i];
    sc[0] = st.gmax; sc[1] = st.radius; sc[2] = st.decrease;
    int iter = st.iter, reuse_diag = st.reuse_diag, invalid_run = st.invalid_run;
    const int max_iter = st.max_iter;
    pin_regs<NP>(S); pin_regs<NP>(g); pin_regs<NP>(diag); pin_regs<NT>(A); pin_regs<3>(sc);
    const double gmax = sc[0];
    double radius = sc[1], decrease = sc[2];
    auto scaled_A = [&](int a, int b) { const int hi = a >= b ? a : b, lo = a >= b ? b : a; return S[hi] * A[hi * (hi + 1) / 2 + lo] * S[lo]; };
    auto write_back = [&]() { st.iter = iter; st.radius = radius; st.decrease = decrease; st.reuse_diag = reuse_diag; st.invalid_run = invalid_run; };
    for (;;) {
        if (iter >= max_iter || gmax <= kGradTol || radius <= kMinRadius) { write_back(); st.done = 1; return; }
        ++iter;
        double M[NT], ds[NP];
#pragma unroll
        for (int a = 0; a < NP; ++a)
#pragma unroll
            for (int b = 0; b <= a; ++b) M[a * (a + 1) / 2 + b] = scaled_A(a, b);
        if (!reuse_diag) {
#pragma unroll
            for (int a = 0; a < NP; ++a) { diag[a] = fmin(fmax(M[a * (a + 1) / 2 + a], kMinDiag), kMaxDiag); st.diag[a] = diag[a]; }
        }
#pragma unroll
        for (int a = 0; a < NP; ++a) { M[a * (a + 1) / 2 + a] += lm_div(diag[a], radius); ds[a] = -(S[a] * g[a]); }
        DI2P_LMCLK(1, tb0);
        DI2P_LMSTAMP(tc0);
        bool valid = chol_solve_inplace<NP>(M, ds);
        DI2P_LMADD(st.n_resweep, tc0);
        DI2P_LMCLK(2, tc0);
        DI2P_LMSTAMP(tm0);
        double model_change = 0.0;
        if (valid) {
            double q = 0.0, l = 0.0;
#pragma unroll
            for (int a = 0; a < NP; ++a) {
                l += ds[a] * (S[a] * g[a]);
#pragma unroll
                for (int b = 0; b < NP; ++b) q += ds[a] * scaled_A(a, b) * ds[b];
            }
            model_change = -(l + 0.5 * q);
            valid = model_change > 0.0;
        }
        DI2P_LMCLK(3, tm0);
        DI2P_LMSTAMP(tp0);
        if (!valid) {
            if (++invalid_run >= 5) { write_back(); st.done = 1; return; }
            radius /= decrease; decrease *= 2.0; reuse_diag = 1;
            DI2P_LMRESTAMP(tb0);
            continue;
        }
        invalid_run = 0;
        write_back();
        st.model_change = model_change;
        double x[NP], lb[NP], ub[NP], delta[NP];
#pragma unroll
        for (int a = 0; a < NP; ++a) { x[a] = st.x[a]; lb[a] = st.lb[a]; ub[a] = st.ub[a]; }
        pin_regs<NP>(x); pin_regs<NP>(lb); pin_regs<NP>(ub);
        double gd = 0.0, dmax = 0.0;
#pragma unroll
        for (int a = 0; a < NP; ++a) {
            delta[a] = ds[a] * S[a];
            gd += g[a] * delta[a];
            dmax = fmax(dmax, fabs(delta[a]));
        }
        double xe[NP];
        plus_proj<NP>(x, delta, 1.0, lb, ub, xe);
#pragma unroll
        for (int a = 0; a < NP; ++a) { st.delta[a] = delta[a]; st.xe[a] = xe[a]; }
        st.gd = gd; st.dmax = dmax; st.t = 1.0; st.ls_it = 0;
        st.phase = PH_TRIAL; st.want_j = 2; st.prev_vok = 0; st.prev_gok = 0;
        DI2P_LMCLK(4, tp0);
        return;   // needs a sweep at xe
    }
}

// The LM update is a chain of STAGES, each instantiated exactly once in the kernel (lm_decide -> [wave-wide minimiser] ->
// lm_trial_next_decide -> lm_apply = {lm_finish_iteration, lm_begin_iteration}); a stage hands the next one an action code.  (As
// mutually calling inline functions the iteration start was instantiated five times: 13 k instructions, and the register allocator
// spilled inside the sweep loops.)
enum { ACT_NONE = 0, ACT_BEGIN = 1, ACT_FINISH_CUR = 2, ACT_FINISH_FIRST = 3, ACT_TRIAL_NEXT = 4, ACT_POLY = 5 };

// candidate (xe, cand_cost, ge, Ae) against the current iterate: tolerance tests, accept / reject.  -> true: start the next iteration
template <int NP>
__device__ __forceinline__ bool lm_finish_iteration(LMState<NP>& st, double cand_cost, const double* ge, const double* Ae) {
    constexpr int NT = Tri<NP>::N;
    const double kMaxRadius = 1e16, kMinRelDec = 1e-3, kFuncTol = 1e-6, kParamTol = 1e-8;
    double xo[NP], xn[NP], gl[NP], Al[NT], lb[NP], ub[NP], sc[4];
#pragma unroll
    for (int a = 0; a < NP; ++a) { xo[a] = st.x[a]; xn[a] = st.xe[a]; gl[a] = ge[a]; lb[a] = st.lb[a]; ub[a] = st.ub[a]; }
#pragma unroll
    for (int i = 0; i < NT; ++i) Al[i] = Ae[i];
    sc[0] = st.cost; sc[1] = st.model_change; sc[2] = st.radius; sc[3] = st.decrease;
    pin_regs<NP>(xo); pin_regs<NP>(xn); pin_regs<NP>(gl); pin_regs<NT>(Al); pin_regs<NP>(lb); pin_regs<NP>(ub); pin_regs<4>(sc);
    double step_norm = 0.0, x_norm = 0.0;
#pragma unroll
    for (int a = 0; a < NP; ++a) { step_norm += (xo[a] - xn[a]) * (xo[a] - xn[a]); x_norm += xo[a] * xo[a]; }
    step_norm = lm_sqrt(step_norm); x_norm = lm_sqrt(x_norm);
    if (step_norm <= kParamTol * (x_norm + kParamTol)) { st.done = 1; return false; }
    if (fabs(sc[0] - cand_cost) <= kFuncTol * sc[0]) { st.done = 1; return false; }
    const double rel = lm_div(sc[0] - cand_cost, sc[1]);
    if (rel > kMinRelDec) {
#pragma unroll
        for (int a = 0; a < NP; ++a) { st.x[a] = xn[a]; st.g[a] = gl[a]; }
#pragma unroll
        for (int i = 0; i < NT; ++i) st.A[i] = Al[i];
        st.cost = cand_cost;
        st.gmax = grad_max_norm<NP>(xn, gl, lb, ub);
        const double w = 2.0 * rel - 1.0;
        st.radius = fmin(kMaxRadius, lm_div(sc[2], fmax(1.0 / 3.0, 1.0 - w * w * w)));
        st.decrease = 2.0; st.reuse_diag = 0;
    } else {
        st.radius = sc[2] / sc[3]; st.decrease = sc[3] * 2.0; st.reuse_diag = 1;
    }
    return true;
}

// Second half of a failed line-search trial: the next step size st.tn is known.  -> ACT_FINISH_FIRST when the search gives up
// (the candidate is then the first trial point, whose sums were kept), ACT_NONE when the next sweep evaluates the new trial point.
template <int NP>
__device__ __forceinline__ int lm_trial_next_decide(LMState<NP>& st) {
    const double tn = st.tn;
    if (tn * st.dmax < 1e-9) return ACT_FINISH_FIRST;
    st.t = tn;
    plus_proj<NP>(st.x, st.delta, tn, st.lb, st.ub, st.xe);
    return ACT_NONE;
}

// Last stage: finish the iteration with the chosen candidate (the point just swept, or the first trial point) and start the next one.
template <int NP>
__device__ __forceinline__ void lm_apply(LMState<NP>& st, int action, double fe, const double* ge, const double* Ae) {
    bool begin = action == ACT_BEGIN;
    if (action == ACT_FINISH_CUR || action == ACT_FINISH_FIRST) {
        DI2P_LMSTAMP(tf0);
        const bool first = action == ACT_FINISH_FIRST;
        if (first) plus_proj<NP>(st.x, st.delta, 1.0, st.lb, st.ub, st.xe);     // delta stays unscaled: back to the first trial point
        begin = lm_finish_iteration<NP>(st, first ? st.f1 : fe, first ? st.g1 : ge, first ? st.A1 : Ae);
        DI2P_LMCLK(0, tf0);
    }
    if (begin) lm_begin_iteration<NP>(st);
}

// Wave 0, all lanes: minimise the pending interpolant (MinimizePolynomial over u in [1e-3 t, 0.6 t] / t).
template <int NP>
__device__ __forceinline__ void lm_poly_wave(LMState<NP>& st) {
    double p[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) p[j] = st.poly[j];
    const double t = st.t;
    const double u = poly_min_on_wave(p, (1e-3 * t) / t, (0.6 * t) / t);
    if ((threadIdx.x & 63) == 0) st.tn = u * t;
}

// First stage, called by thread 0 after every sweep with the combined sums of the point just evaluated (st.xe).  -> action code
template <int NP>
__device__ __forceinline__ int lm_decide(LMState<NP>& st, bool ok, double fe, const double* ge_in, const double* Ae_in) {
    double ge[NP], Ae[Tri<NP>::N];       // the combined sums, fetched in one batch (copied field by field they were read -> wait -> write pairs)
#pragma unroll
    for (int a = 0; a < NP; ++a) ge[a] = ge_in[a];
#pragma unroll
    for (int i = 0; i < Tri<NP>::N; ++i) Ae[i] = Ae_in[i];
    pin_regs<NP>(ge); pin_regs<Tri<NP>::N>(Ae);
    ++st.nsweep;
    if (st.phase == PH_INIT) {
        st.cost = fe;
        // evaluation failure at the start: the sums that exist leave out the record that failed (a label-0 record on a frustum plane is flagged
        // and skipped), so a finite fe is NOT the cost of this pose -- report NaN, as the reference's final evaluation does; never the argmin
        if (!ok) { st.cost = __builtin_nan(""); st.done = 1; return ACT_NONE; }
#pragma unroll
        for (int a = 0; a < NP; ++a) { st.g[a] = ge[a]; st.S[a] = 1.0 / (1.0 + sqrt(Ae[a * (a + 1) / 2 + a])); }
#pragma unroll
        for (int i = 0; i < Tri<NP>::N; ++i) st.A[i] = Ae[i];
        st.gmax = grad_max_norm<NP>(st.x, st.g, st.lb, st.ub);
        return ACT_BEGIN;
    }
    // PH_TRIAL: projected Armijo search along delta (Ceres ArmijoLineSearch, CUBIC interpolation: every trial needs its
    // gradient).  Every sweep also carries the normal equations (10 more fma per Jacobian row, ~3 % of a sweep), so whichever
    // trial satisfies Armijo is used at once; the sums of the first trial (t = 1) are kept: it is the candidate when the
    // search fails.
    if (st.ls_it == 0) {
        st.f1 = ok ? fe : DBL_MAX; st.ok1 = ok;
#pragma unroll
        for (int a = 0; a < NP; ++a) st.g1[a] = ge[a];
#pragma unroll
        for (int i = 0; i < Tri<NP>::N; ++i) st.A1[i] = Ae[i];
    } else {
        ++st.n_ls_extra;
    }
    if (ok && fe <= st.cost + 1e-4 * st.gd * st.t) {
        if (st.ls_it > 0) ++st.n_ls_late_accept;
        return ACT_FINISH_CUR;       // every sweep carries its normal equations: an accepted trial needs no second sweep
    }
    if (++st.ls_it >= 20) return ACT_FINISH_FIRST;      // the search gives up
    LsSample cur{st.t, fe, 0.0, ok, false}, prev{st.prev_t, st.prev_f, st.prev_g, st.prev_vok != 0, st.prev_gok != 0};
    if (ok) {
        double gdir = 0.0;
#pragma unroll
        for (int a = 0; a < NP; ++a) gdir += st.delta[a] * ge[a];
        cur.gradient = gdir;
        cur.grad_ok = isfinite(gdir);
    }
    st.prev_t = cur.x; st.prev_f = cur.value; st.prev_g = cur.gradient; st.prev_vok = cur.value_ok; st.prev_gok = cur.grad_ok;
    double p[6];
    DI2P_LMSTAMP(tfit0);
    const bool fitted = interpolating_fit(st.cost, st.gd, cur, prev, p);
    DI2P_LMCLK(6, tfit0);
    if (fitted) {
        // the minimiser of the interpolant over [1e-3, 0.6] x t is found by the whole wavefront (lm_poly_wave), then lm_trial_next_decide
#pragma unroll
        for (int j = 0; j < 6; ++j) st.poly[j] = p[j];
        st.poly_req = 1;
        return ACT_POLY;
    }
    st.tn = fmin(fmax(st.t * 0.5, 1e-3 * st.t), 0.6 * st.t);
    return ACT_TRIAL_NEXT;
}

}  // namespace
