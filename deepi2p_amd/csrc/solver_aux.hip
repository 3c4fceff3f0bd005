// The once-per-frame kernels around the batched pose solve (solver.hip) and their entry points: initial guess and front filter, argmin over
// the restarts, loss-corrected residuals, and the pose confidence (information matrix, bounded covariance, restart consensus).  None is hot;
// they share the solver's geometry (solver_model.h) and evaluate residuals plainly: per point, IEEE division, no clusters, no cache.
#include "common.h"
#include "pose_diff.h"
#include "solver_model.h"

namespace {

// one wavefront per frame: argmin over R (ties -> lowest r), assemble P
__global__ __launch_bounds__(64) void select_best_kernel(const double* __restrict__ params, const double* __restrict__ cost,
                                                         const int* __restrict__ has_inside, int np, int R, int* __restrict__ best,
                                                         double* __restrict__ P, double* __restrict__ best_cost) {
    const int f = blockIdx.x, lane = threadIdx.x;
    double bc = __builtin_inf();
    int bi = 0x7fffffff;
    for (int r = lane; r < R; r += 64) {
        const double c = cost[(long long)f * R + r];
        if (c < bc || (c == bc && r < bi)) { bc = c; bi = r; }   // NaN never wins
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double oc = __shfl_xor(bc, o);
        const int oi = __shfl_xor(bi, o);
        if (oc < bc || (oc == bc && oi < bi)) { bc = oc; bi = oi; }
    }
    if (lane != 0) return;
    double* Pf = P + (long long)f * 16;
    for (int i = 0; i < 16; ++i) Pf[i] = (i % 5 == 0) ? 1.0 : 0.0;
    if (has_inside && has_inside[f] == 0) {  // registration_lsq.py:329-332
        best[f] = -1;
        best_cost[f] = 1e4;
        return;
    }
    if (bi == 0x7fffffff) bi = 0;
    params_to_pose(params + ((long long)f * R + bi) * np, np, Pf);
    best[f] = bi;
    best_cost[f] = cost[(long long)f * R + bi];
}

// registration_lsq.py:196-220.  One 1024-thread workgroup per frame, fixed-order tree reductions.
__global__ __launch_bounds__(1024) void initial_guess_kernel(const double* __restrict__ points, const int* __restrict__ labels,
                                                             double* __restrict__ yaw0, int* __restrict__ labels_out,
                                                             int* __restrict__ has_inside, int N) {
    __shared__ double s_a[1024], s_b[1024], s_c[1024];
    const int f = blockIdx.x, tid = threadIdx.x;
    const double* px = points + (long long)f * 3 * N;
    const double* pz = px + 2 * (long long)N;
    const int* lab = labels + (long long)f * N;
    double sx = 0, sz = 0, cnt = 0;
    for (int n = tid; n < N; n += 1024)
        if (lab[n] == 1) { sx += px[n]; sz += pz[n]; cnt += 1.0; }
    s_a[tid] = sx; s_b[tid] = sz; s_c[tid] = cnt;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if (tid < o) { s_a[tid] += s_a[tid + o]; s_b[tid] += s_b[tid + o]; s_c[tid] += s_c[tid + o]; }
        __syncthreads();
    }
    const double count = s_c[0];
    const double mx = s_a[0] / count, mz = s_b[0] / count;
    __syncthreads();
    if (!(count > 0.0)) {
        if (tid == 0) { yaw0[f] = 0.0; has_inside[f] = 0; }
        for (int n = tid; n < N; n += 1024) labels_out[(long long)f * N + n] = lab[n];
        return;
    }
    const double kPi = 3.14159265358979323846;
    double a = fmod(atan2(mz, mx) - kPi / 2 + kPi, 2 * kPi);   // wrap_in_pi (:189-193)
    if (a < 0) a += 2 * kPi;
    a -= kPi;
    const double c = cos(a), s = sin(a);
    double zmin = __builtin_inf();
    for (int n = tid; n < N; n += 1024)
        if (lab[n] == 1) zmin = fmin(zmin, -s * px[n] + c * pz[n]);
    s_a[tid] = zmin;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if (tid < o) s_a[tid] = fmin(s_a[tid], s_a[tid + o]);
        __syncthreads();
    }
    const double thr = s_a[0] - 10.0;
    for (int n = tid; n < N; n += 1024) {
        const double zr = -s * px[n] + c * pz[n];
        labels_out[(long long)f * N + n] = zr > thr ? lab[n] : -1;
    }
    if (tid == 0) { yaw0[f] = a; has_inside[f] = 1; }
}

// Problem::Evaluate (registration.cpp:150-155): loss-corrected residuals in point order, compacted.
template <int NP>
__global__ __launch_bounds__(256) void residuals_kernel(const double* __restrict__ points, const int* __restrict__ labels,
                                                        const double* __restrict__ Kmat, const double* __restrict__ params, double H,
                                                        double W, int N, double* __restrict__ residuals, int* __restrict__ counts,
                                                        double* __restrict__ cost_out) {
    __shared__ int s_scan[256];
    __shared__ double s_cost[256];
    __shared__ int s_base;
    const int f = blockIdx.x, tid = threadIdx.x;
    const double* px = points + (long long)f * 3 * N;
    const int* lab = labels + (long long)f * N;
    const double* Kf = Kmat + (long long)f * 9;
    const Cam k{Kf[0], Kf[4], Kf[2], Kf[5], H - 1.0, W - 1.0};
    const double* x = params + (long long)f * NP;
    double xr[NP];
    for (int i = 0; i < NP; ++i) xr[i] = x[i];
    Rot<NP> rot;
    make_rot<NP>(xr, rot);
    double* out = residuals + (long long)f * 3 * N;
    if (tid == 0) s_base = 0;
    double cost = 0.0;
    __syncthreads();
    for (int n0 = 0; n0 < N; n0 += 256) {
        const int n = n0 + tid;
        int nr = 0;
        double rv[3] = {0, 0, 0};
        if (n < N && (lab[n] == 0 || lab[n] == 1)) {
            const Proj p = project_point<NP>(rot, xr, k, px[n], px[N + n], px[2 * (long long)N + n]);
            nr = lab[n] == 1 ? 3 : 1;
            residual_rows<false>(lab[n], p.pix_x, p.pix_y, p.p2, k, rv);
            const double s = rv[0] * rv[0] + rv[1] * rv[1] + rv[2] * rv[2];
            cost += 0.5 * log1p(s);
            const double sq = sqrt(1.0 / (1.0 + s));
            for (int i = 0; i < 3; ++i) rv[i] *= sq;
        }
        s_scan[tid] = nr;
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {
            const int v = tid >= o ? s_scan[tid - o] : 0;
            __syncthreads();
            s_scan[tid] += v;
            __syncthreads();
        }
        const int excl = s_scan[tid] - nr + s_base;
        for (int i = 0; i < nr; ++i) out[excl + i] = rv[i];
        __syncthreads();
        if (tid == 255) s_base += s_scan[255];
        __syncthreads();
    }
    s_cost[tid] = cost;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) s_cost[tid] += s_cost[tid + o];
        __syncthreads();
    }
    if (tid == 0) { counts[f] = s_base; cost_out[f] = s_cost[0]; }
}

// ----------------------------------------------------------------------------------------------
// Pose confidence: the normal matrix A = sum_blocks rho'(s) J^T J, the gradient g = sum rho'(s) J^T r and the cost 1/2 sum log1p(s) at GIVEN
// parameters, by the plain per-point evaluation of residuals_kernel (no clusters, no cache, no fast reciprocal) with the analytic Jacobian
// rows of eval_active.  Grid (F, C): workgroup (f, c) owns the points [c * INFO_CHUNK, (c + 1) * INFO_CHUNK) of frame f, thread t the points
// c * INFO_CHUNK + t + 256 j in ascending j; the wave butterflies and the in-order sum of the four wave partials give one partial per
// workgroup, and info_finish_kernel adds the C partials of a frame in index order.  No atomics: a frame's sums are a function of its own
// points, labels, K and parameters alone.
constexpr int INFO_CHUNK = 1024;                 // points per workgroup: C = ceil(N / INFO_CHUNK) depends on N only
constexpr int INFO_STRIDE = 32;                  // fp64 words per partial: NP (NP + 1) / 2 of A | NP of g | cost | label-1 count | label-0 count
template <int NP> struct InfoWords { static constexpr int A = 0, G = Tri<NP>::N, COST = G + NP, ACT1 = COST + 1, ACT0 = COST + 2, N = COST + 3; };
static_assert(InfoWords<6>::N <= INFO_STRIDE && InfoWords<4>::N <= INFO_STRIDE, "a partial has INFO_STRIDE words");

template <int NP>
__global__ __launch_bounds__(256) void info_partial_kernel(const float* __restrict__ points, const int* __restrict__ labels,
                                                           const double* __restrict__ Kmat, const double* __restrict__ params, double H,
                                                           double W, int N, int C, double* __restrict__ partial) {
    using IW = InfoWords<NP>;
    __shared__ double s_part[4][INFO_STRIDE];
    constexpr int TOFF = NP == 4 ? 1 : 3;
    const int f = blockIdx.x, c = blockIdx.y, tid = threadIdx.x;
    const float* px = points + (long long)f * 3 * N;
    const int* lab = labels + (long long)f * N;
    const double* Kf = Kmat + (long long)f * 9;
    const Cam k{Kf[0], Kf[4], Kf[2], Kf[5], H - 1.0, W - 1.0};
    double xr[NP];
    for (int i = 0; i < NP; ++i) xr[i] = params[(long long)f * NP + i];
    Rot<NP> rot;
    make_rot<NP>(xr, rot);
    double acc[IW::N];
#pragma unroll
    for (int i = 0; i < IW::N; ++i) acc[i] = 0.0;
    const int n_end = min(N, (c + 1) * INFO_CHUNK);
    for (int n = c * INFO_CHUNK + tid; n < n_end; n += 256) {
        const int l = lab[n];
        if (l != 0 && l != 1) continue;
        const double X = (double)px[n], Y = (double)px[N + n], Z = (double)px[2 * (long long)N + n];
        const Proj p = project_point<NP>(rot, xr, k, X, Y, Z);
        double rv[3] = {0, 0, 0}, sx[3] = {0, 0, 0}, sy[3] = {0, 0, 0}, sz[3] = {0, 0, 0};      // residual rows as value and slopes
        residual_rows<true>(l, p.pix_x, p.pix_y, p.p2, k, rv, sx, sy, sz);
        const double s = rv[0] * rv[0] + rv[1] * rv[1] + rv[2] * rv[2];       // rows 1 and 2 of a label-0 block are 0
        acc[IW::COST] += 0.5 * log1p(s);
        if (s != 0.0) { acc[IW::ACT1] += l == 1 ? 1.0 : 0.0; acc[IW::ACT0] += l == 1 ? 0.0 : 1.0; }
        const double rho1 = 1.0 / (1.0 + s);
        // dp_i / dparam: rotation columns from dR (NP == 6) or d/dtheta of Ry(theta) X (NP == 4), then the identity of t
        double dp0[NP], dp1[NP], dp2[NP];
        if (NP == 4) {
            const bool first_order = !(xr[0] * xr[0] > DBL_EPSILON);
            dp0[0] = first_order ? Z : p.qz; dp1[0] = 0.0; dp2[0] = first_order ? -X : -p.qx;
        } else {
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                dp0[i] = rot.dR[i][0] * X + rot.dR[i][1] * Y + rot.dR[i][2] * Z;
                dp1[i] = rot.dR[i][3] * X + rot.dR[i][4] * Y + rot.dR[i][5] * Z;
                dp2[i] = rot.dR[i][6] * X + rot.dR[i][7] * Y + rot.dR[i][8] * Z;
            }
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) { dp0[TOFF + i] = i == 0 ? 1.0 : 0.0; dp1[TOFF + i] = i == 1 ? 1.0 : 0.0; dp2[TOFF + i] = i == 2 ? 1.0 : 0.0; }
        const double iz = 1.0 / p.p2;
        const double ax = k.fx * iz, bx = -k.fx * p.p0 * iz * iz;   // dpix_x = ax*dp0 + bx*dp2
        const double ay = k.fy * iz, by = -k.fy * p.p1 * iz * iz;   // dpix_y = ay*dp1 + by*dp2
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            if (sx[i] == 0.0 && sy[i] == 0.0 && sz[i] == 0.0) continue;       // a constant row (NaN slopes do not compare equal: they are added)
            double J[NP];
#pragma unroll
            for (int a = 0; a < NP; ++a) J[a] = sx[i] * (ax * dp0[a] + bx * dp2[a]) + sy[i] * (ay * dp1[a] + by * dp2[a]) + sz[i] * dp2[a];
            const double wr = rho1 * rv[i];
#pragma unroll
            for (int a = 0; a < NP; ++a) {
                acc[IW::G + a] += wr * J[a];
                const double wa = rho1 * J[a];
#pragma unroll
                for (int b = 0; b <= a; ++b) acc[IW::A + a * (a + 1) / 2 + b] += wa * J[b];
            }
        }
    }
#pragma unroll
    for (int i = 0; i < IW::N; ++i) acc[i] = wave_sum(acc[i]);
    if ((tid & 63) == 0) {
#pragma unroll
        for (int i = 0; i < IW::N; ++i) s_part[tid >> 6][i] = acc[i];
    }
    __syncthreads();
    if (tid < IW::N) partial[((long long)f * C + c) * INFO_STRIDE + tid] = ((s_part[0][tid] + s_part[1][tid]) + s_part[2][tid]) + s_part[3][tid];
}

template <int NP>
__global__ __launch_bounds__(64) void info_finish_kernel(const double* __restrict__ partial, int C, double* __restrict__ info,
                                                         double* __restrict__ grad, double* __restrict__ cost, int* __restrict__ active) {
    using IW = InfoWords<NP>;
    __shared__ double s_sum[INFO_STRIDE];
    const int f = blockIdx.x, tid = threadIdx.x;
    if (tid < IW::N) {
        double v = 0.0;
        for (int c = 0; c < C; ++c) v += partial[((long long)f * C + c) * INFO_STRIDE + tid];
        s_sum[tid] = v;
    }
    __syncthreads();
    if (tid < NP * NP) info[(long long)f * NP * NP + tid] = s_sum[IW::A + tri<NP>(tid / NP, tid % NP)];
    if (tid < NP) grad[(long long)f * NP + tid] = s_sum[IW::G + tid];
    if (tid == 0) cost[f] = s_sum[IW::COST];
    if (tid < 2) active[2 * f + tid] = (int)s_sum[tid == 0 ? IW::ACT1 : IW::ACT0];
}

// params[f, best[f]] -> out[f] (a frame without a selected restart, best < 0, takes restart 0: its covariance reports status 2 anyway)
__global__ __launch_bounds__(64) void gather_best_kernel(const double* __restrict__ params, const int* __restrict__ best, int F, int R, int np,
                                                         double* __restrict__ out) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= F * np) return;
    const int f = i / np;
    int b = best[f];
    if (b < 0 || b >= R) b = 0;
    out[i] = params[((long long)f * R + b) * np + (i - f * np)];
}

// Bounded inverse of the information matrix, one thread per frame.  A translation parameter exactly on its bound is fixed: its row and
// column are replaced by the identity's before the Cholesky factorisation (the factor of the free block is then the factor of the free
// sub-matrix, operation for operation: the replaced entries contribute exact zeros) and its covariance entries are written as 0.
template <int NP>
__global__ __launch_bounds__(64) void pose_covariance_kernel(const double* __restrict__ info, const double* __restrict__ params,
                                                             const int* __restrict__ has_inside, Bounds bnd, int F, double* __restrict__ cov,
                                                             int* __restrict__ free_mask, int* __restrict__ status, double* __restrict__ sigma_t,
                                                             double* __restrict__ sigma_r) {
    constexpr int TOFF = NP == 4 ? 1 : 3;
    const int f = blockIdx.x * 64 + threadIdx.x;
    if (f >= F) return;
    double A[NP][NP], x[NP];
    bool finite = true;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        x[i] = params[(long long)f * NP + i];
        finite = finite && isfinite(x[i]);
#pragma unroll
        for (int j = 0; j < NP; ++j) { A[i][j] = info[((long long)f * NP + i) * NP + j]; finite = finite && isfinite(A[i][j]); }
    }
    int mask = 0;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const int ti = i >= TOFF ? i - TOFF : 0;
        const bool fixed = i >= TOFF && (x[i] == bnd.lb[ti] || x[i] == bnd.ub[ti]);
        if (!fixed) mask |= 1 << i;
    }
    free_mask[f] = mask;
    int st = (!finite || (has_inside && has_inside[f] == 0)) ? 2 : (mask == 0 ? 1 : 0);
    double amax = 0.0;
#pragma unroll
    for (int i = 0; i < NP; ++i) if ((mask >> i) & 1) amax = fmax(amax, A[i][i]);
    const double tiny = NP * DBL_EPSILON * amax;
    // L: Cholesky factor of the free block (identity on the fixed parameters)
    double L[NP][NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const bool fi = (mask >> i) & 1;
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            const bool fj = (mask >> j) & 1;
            double s = (fi && fj) ? A[i][j] : (i == j ? 1.0 : 0.0);
#pragma unroll
            for (int q = 0; q < j; ++q) s -= L[i][q] * L[j][q];
            if (i == j) {
                if (fi && !(s > tiny) && st == 0) st = 1;
                L[i][i] = sqrt(s);
            } else {
                L[i][j] = s / L[j][j];
            }
        }
    }
    // M = L^-1 (lower triangular, column by column), cov = M^T M
    double M[NP][NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) {
#pragma unroll
        for (int i = j; i < NP; ++i) {
            double s = i == j ? 1.0 : 0.0;
#pragma unroll
            for (int q = j; q < i; ++q) s -= L[i][q] * M[q][j];
            M[i][j] = s / L[i][i];
        }
    }
    const double nan = __builtin_nan("");
    double tr_r = 0.0, tr_t = 0.0;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            double s = 0.0;
#pragma unroll
            for (int q = i; q < NP; ++q) s += M[q][i] * M[q][j];
            if (!((mask >> i) & 1) || !((mask >> j) & 1)) s = 0.0;
            if (st != 0) s = nan;
            cov[((long long)f * NP + i) * NP + j] = s;
            cov[((long long)f * NP + j) * NP + i] = s;
            if (i == j) { if (i < TOFF) tr_r += s; else tr_t += s; }
        }
    }
    status[f] = st;
    sigma_t[f] = sqrt(tr_t);
    sigma_r[f] = sqrt(tr_r) * (180.0 / 3.14159265358979323846);
}

// What the other restarts say: one wave per frame, lanes stride over R.  A restart AGREES when its cost is finite and get_P_diff of
// P_r^-1 P_best is below both tolerances (pose_diff.h, the rule of di2p_pose_errors); the gap is the cheapest disagreeing restart's cost
// minus the best's.
__global__ __launch_bounds__(64) void restart_consensus_kernel(const double* __restrict__ params, const double* __restrict__ cost,
                                                               const int* __restrict__ best, const int* __restrict__ has_inside, int np, int R,
                                                               double t_tol, double r_tol_deg, int* __restrict__ finite_out,
                                                               int* __restrict__ agree_out, double* __restrict__ gap) {
    const int f = blockIdx.x, lane = threadIdx.x;
    const int b = best[f];
    if ((has_inside && has_inside[f] == 0) || b < 0 || b >= R) {        // wave-uniform
        if (lane == 0) { finite_out[f] = 0; agree_out[f] = 0; gap[f] = __builtin_nan(""); }
        return;
    }
    double G[16], A[16];
    params_to_pose(params + ((long long)f * R + b) * np, np, G);
    int n_finite = 0, n_agree = 0;
    double other = __builtin_inf();
    for (int r = lane; r < R; r += 64) {
        const double c = cost[(long long)f * R + r];
        if (!isfinite(c)) continue;
        n_finite += 1;
        params_to_pose(params + ((long long)f * R + r) * np, np, A);
        double t, ang;
        di2p_pose_diff(A, G, t, ang);
        if (t < t_tol && ang < r_tol_deg) n_agree += 1;
        else other = fmin(other, c);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        n_finite += __shfl_xor(n_finite, o);
        n_agree += __shfl_xor(n_agree, o);
        other = fmin(other, __shfl_xor(other, o));
    }
    if (lane == 0) { finite_out[f] = n_finite; agree_out[f] = n_agree; gap[f] = other - cost[(long long)f * R + b]; }
}

}  // namespace

extern "C" int di2p_select_best(const double* params, const double* cost, const int32_t* has_inside, int is_2d, int F, int R,
                                int32_t* best, double* P, double* best_cost, void* stream) {
    DI2P_CHECK_ARG(params && cost && best && P && best_cost && F >= 0 && R >= 1, "bad args");
    if (F == 0) return 0;
    hipLaunchKernelGGL(select_best_kernel, dim3(F), dim3(64), 0, (hipStream_t)stream, params, cost, has_inside, is_2d ? 4 : 6, R, best, P, best_cost);
    DI2P_RETURN_LAUNCH();
}

extern "C" int di2p_initial_guess(const double* points, const int32_t* labels, double* yaw0, int32_t* labels_out,
                                  int32_t* has_inside, int F, int N, void* stream) {
    DI2P_CHECK_ARG(points && labels && yaw0 && labels_out && has_inside && F >= 0 && N >= 0, "bad args");
    if (F == 0) return 0;
    hipLaunchKernelGGL(initial_guess_kernel, dim3(F), dim3(1024), 0, (hipStream_t)stream, points, labels, yaw0, labels_out, has_inside, N);
    DI2P_RETURN_LAUNCH();
}

extern "C" int di2p_solver_residuals(const double* points, const int32_t* labels, const double* K, const double* params, double H,
                                     double W, int is_2d, int F, int N, double* residuals, int32_t* counts, double* cost,
                                     void* stream) {
    DI2P_CHECK_ARG(points && labels && K && params && residuals && counts && cost && F >= 0 && N >= 0, "bad args");
    if (F == 0) return 0;
    if (is_2d)
        hipLaunchKernelGGL(residuals_kernel<4>, dim3(F), dim3(256), 0, (hipStream_t)stream, points, labels, K, params, H, W, N, residuals, counts, cost);
    else
        hipLaunchKernelGGL(residuals_kernel<6>, dim3(F), dim3(256), 0, (hipStream_t)stream, points, labels, K, params, H, W, N, residuals, counts, cost);
    DI2P_RETURN_LAUNCH();
}

static int info_chunks(int N) { return N > 0 ? (N + INFO_CHUNK - 1) / INFO_CHUNK : 1; }      // (an empty cloud still launches: a grid of 0 is an error)

extern "C" long long di2p_pose_information_workspace_bytes(int F, int N) {
    if (F < 0 || N < 0) return 0;
    return (long long)F * info_chunks(N) * INFO_STRIDE * (long long)sizeof(double);
}

extern "C" int di2p_pose_information(const float* points, const int32_t* labels, const double* K, const double* params, double H, double W,
                                     int is_2d, int F, int N, double* info, double* grad, double* cost, int32_t* active, void* workspace,
                                     void* stream) {
    DI2P_CHECK_ARG(F >= 0 && N >= 0, "bad size");
    if (F == 0) return 0;
    DI2P_CHECK_ARG(points && labels && K && params && info && grad && cost && active && workspace, "null pointer");
    const int C = info_chunks(N);
    DI2P_CHECK_ARG(C <= 65535, "N too large");
    double* partial = (double*)workspace;
    if (is_2d) {
        hipLaunchKernelGGL(info_partial_kernel<4>, dim3(F, C), dim3(256), 0, (hipStream_t)stream, points, labels, K, params, H, W, N, C, partial);
        hipLaunchKernelGGL(info_finish_kernel<4>, dim3(F), dim3(64), 0, (hipStream_t)stream, (const double*)partial, C, info, grad, cost, active);
    } else {
        hipLaunchKernelGGL(info_partial_kernel<6>, dim3(F, C), dim3(256), 0, (hipStream_t)stream, points, labels, K, params, H, W, N, C, partial);
        hipLaunchKernelGGL(info_finish_kernel<6>, dim3(F), dim3(64), 0, (hipStream_t)stream, (const double*)partial, C, info, grad, cost, active);
    }
    DI2P_RETURN_LAUNCH();
}

extern "C" int di2p_gather_best_params(const double* params, const int32_t* best, int is_2d, int F, int R, double* out, void* stream) {
    DI2P_CHECK_ARG(F >= 0 && R >= 1, "bad size (F >= 0, R >= 1)");
    if (F == 0) return 0;
    DI2P_CHECK_ARG(params && best && out, "null pointer");
    const int np = is_2d ? 4 : 6;
    hipLaunchKernelGGL(gather_best_kernel, dim3(di2p_cdiv((long long)F * np, 64)), dim3(64), 0, (hipStream_t)stream, params, best, F, R, np, out);
    DI2P_RETURN_LAUNCH();
}

extern "C" int di2p_pose_covariance(const double* info, const double* params, const int32_t* has_inside, const double* lb_host,
                                    const double* ub_host, int is_2d, int F, double* cov, int32_t* free_mask, int32_t* status, double* sigma_t,
                                    double* sigma_r, void* stream) {
    DI2P_CHECK_ARG(F >= 0, "bad size");
    if (F == 0) return 0;
    DI2P_CHECK_ARG(info && params && lb_host && ub_host && cov && free_mask && status && sigma_t && sigma_r, "null pointer");
    const Bounds b = make_bounds(lb_host, ub_host);
    if (is_2d)
        hipLaunchKernelGGL(pose_covariance_kernel<4>, dim3(di2p_cdiv(F, 64)), dim3(64), 0, (hipStream_t)stream, info, params, has_inside, b, F, cov,
                           free_mask, status, sigma_t, sigma_r);
    else
        hipLaunchKernelGGL(pose_covariance_kernel<6>, dim3(di2p_cdiv(F, 64)), dim3(64), 0, (hipStream_t)stream, info, params, has_inside, b, F, cov,
                           free_mask, status, sigma_t, sigma_r);
    DI2P_RETURN_LAUNCH();
}

extern "C" int di2p_restart_consensus(const double* params, const double* cost, const int32_t* best, const int32_t* has_inside, int is_2d,
                                      int F, int R, double t_tol, double r_tol_deg, int32_t* finite, int32_t* agree, double* gap, void* stream) {
    DI2P_CHECK_ARG(F >= 0 && R >= 1, "bad size (F >= 0, R >= 1)");
    if (F == 0) return 0;
    DI2P_CHECK_ARG(params && cost && best && finite && agree && gap, "null pointer");
    hipLaunchKernelGGL(restart_consensus_kernel, dim3(F), dim3(64), 0, (hipStream_t)stream, params, cost, best, has_inside, is_2d ? 4 : 6, R, t_tol,
                       r_tol_deg, finite, agree, gap);
    DI2P_RETURN_LAUNCH();
}
