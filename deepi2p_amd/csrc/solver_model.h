// The geometry that every kernel of the pose solver shares (included by solver.hip, solver_lm.h and solver_aux.hip): camera, rotation of an
// iterate, translation bounds, packed-triangle indices, parameters -> 4x4 pose.
#pragma once
#include <hip/hip_runtime.h>
#include <float.h>

namespace {

struct Cam { double fx, fy, cx, cy, H1, W1; };

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

template <int NP> struct Tri { static constexpr int N = NP * (NP + 1) / 2; };
template <int NP> __device__ __forceinline__ constexpr int tri(int a, int b) { return a >= b ? a * (a + 1) / 2 + b : b * (b + 1) / 2 + a; }

// Rotation of the current iterate and its parameter derivatives, computed once per sweep.
template <int NP>
struct Rot {
    double R[9];        // row-major
    double dR[3][9];    // NP == 6 only: dR/dw_i
};

__device__ __forceinline__ void skew_add(double* M, double s, double ux, double uy, double uz) {  // M += s*[u]x
    M[1] -= s * uz; M[2] += s * uy; M[3] += s * uz; M[5] -= s * ux; M[6] -= s * uy; M[7] += s * ux;
}

template <int NP>
__device__ __forceinline__ void make_rot(const double* x, Rot<NP>& r) {
    if (NP == 4) {
        // AngleAxisRotatePoint with axis (0,theta,0): Ry(theta); first-order branch for theta^2 <= eps
        const double th = x[0];
        double c, s;
        if (th * th > DBL_EPSILON) { sincos(th, &s, &c); } else { c = 1.0; s = th; }      // one argument reduction for both
        r.R[0] = c; r.R[1] = 0; r.R[2] = s; r.R[3] = 0; r.R[4] = 1; r.R[5] = 0; r.R[6] = -s; r.R[7] = 0; r.R[8] = c;
    } else {
        const double wx = x[0], wy = x[1], wz = x[2];
        const double t2 = wx * wx + wy * wy + wz * wz;
        for (int i = 0; i < 9; ++i) { r.R[i] = 0; r.dR[0][i] = r.dR[1][i] = r.dR[2][i] = 0; }
        if (t2 > DBL_EPSILON) {
            const double th = sqrt(t2), ux = wx / th, uy = wy / th, uz = wz / th;
            double c, s;
            sincos(th, &s, &c);
            const double oc = 1.0 - c;
            const double u[3] = {ux, uy, uz};
            r.R[0] = r.R[4] = r.R[8] = c;
            skew_add(r.R, s, ux, uy, uz);
            for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) r.R[a * 3 + b] += oc * u[a] * u[b];
            for (int i = 0; i < 3; ++i) {
                double du[3];
                for (int j = 0; j < 3; ++j) du[j] = ((i == j ? 1.0 : 0.0) - u[i] * u[j]) / th;
                double* D = r.dR[i];
                D[0] = D[4] = D[8] = -s * u[i];
                skew_add(D, c * u[i], ux, uy, uz);
                skew_add(D, s, du[0], du[1], du[2]);
                for (int a = 0; a < 3; ++a)
                    for (int b = 0; b < 3; ++b) D[a * 3 + b] += s * u[i] * u[a] * u[b] + oc * (du[a] * u[b] + u[a] * du[b]);
            }
        } else {  // pt + w x pt
            r.R[0] = r.R[4] = r.R[8] = 1.0;
            skew_add(r.R, 1.0, wx, wy, wz);
            skew_add(r.dR[0], 1.0, 1, 0, 0);
            skew_add(r.dR[1], 1.0, 0, 1, 0);
            skew_add(r.dR[2], 1.0, 0, 0, 1);
        }
    }
}

// The plain per-point evaluation (residuals_kernel, info_partial_kernel): IEEE division, the reference's expression order.  The hot path's
// project / eval_active (solver.hip) keep their own statement: fast reciprocal, another association, pinned bit for bit by the tests.
struct Proj { double qx, qz, p0, p1, p2, pix_x, pix_y; };
template <int NP>
__device__ __forceinline__ Proj project_point(const Rot<NP>& rot, const double* x, const Cam& k, double X, double Y, double Z) {
    constexpr int TOFF = NP == 4 ? 1 : 3;
    Proj p;
    p.qx = rot.R[0] * X + rot.R[1] * Y + rot.R[2] * Z;
    const double qy = rot.R[3] * X + rot.R[4] * Y + rot.R[5] * Z;
    p.qz = rot.R[6] * X + rot.R[7] * Y + rot.R[8] * Z;
    p.p0 = p.qx + x[TOFF]; p.p1 = qy + x[TOFF + 1]; p.p2 = p.qz + x[TOFF + 2];
    p.pix_x = p.p0 * k.fx / p.p2 + k.cx; p.pix_y = p.p1 * k.fy / p.p2 + k.cy;
    return p;
}

// Residual rows of one point (registration_2d.hpp:35-69): label 1: three hinge rows; label 0: one row times the three indicators, which are
// constant where they are defined: 1 inside the frustum, 0 outside, NaN on a plane (as the functor's).  SLOPES: also every row's d/dpix_x,
// d/dpix_y and direct d/dp2; fmax(v, 0) keeps v and its slope at v == 0 (Ceres' Jet max).  Entries not written here stay as the caller set them: 0.
template <bool SLOPES>
__device__ __forceinline__ void residual_rows(int label, double pix_x, double pix_y, double p2, const Cam& k, double* rv, double* sx = nullptr,
                                              double* sy = nullptr, double* sz = nullptr) {
    if (label == 1) {
        const double a0 = -pix_x, b0 = pix_x - k.W1, a1 = -pix_y, b1 = pix_y - k.H1, a2 = -p2;
        rv[0] = fmax(a0, 0.0) + fmax(b0, 0.0);
        rv[1] = fmax(a1, 0.0) + fmax(b1, 0.0);
        rv[2] = fmax(a2, 0.0) * 100.0;
        if (SLOPES) {
            sx[0] = (a0 < 0.0 ? 0.0 : -1.0) + (b0 < 0.0 ? 0.0 : 1.0);
            sy[1] = (a1 < 0.0 ? 0.0 : -1.0) + (b1 < 0.0 ? 0.0 : 1.0);
            sz[2] = a2 < 0.0 ? 0.0 : -100.0;
        }
    } else {
        const double ex = pix_x - k.W1 * 0.5, ey = pix_y - k.H1 * 0.5;
        const double dx = k.W1 * 0.5 - fabs(ex), dy = k.H1 * 0.5 - fabs(ey);
        const double ind = (fmax(p2, 0.0) / p2) * (fmax(dx, 0.0) / dx) * (fmax(dy, 0.0) / dy);
        rv[0] = (dx + dy) * ind;
        if (SLOPES) { sx[0] = (ex < 0.0 ? 1.0 : -1.0) * ind; sy[0] = (ey < 0.0 ? 1.0 : -1.0) * ind; }
    }
}

// v_rcp_f64 + two Newton steps: <= 1 ulp for finite non-zero inputs; 0 / inf / NaN give inf / 0 / NaN-like values that the
// callers' finiteness tests catch.  ~5 instructions instead of the ~15 of the IEEE division sequence.
__device__ __forceinline__ double fast_rcp(double v) {
    double r = __builtin_amdgcn_rcp(v);
    r = fma(fma(-v, r, 1.0), r, r);
    r = fma(fma(-v, r, 1.0), r, r);
    return r;
}

struct Bounds { double lb[3], ub[3]; };
inline Bounds make_bounds(const double* lb, const double* ub) {      // host: the translation box of an entry point's two 3-vectors
    Bounds b;
    for (int i = 0; i < 3; ++i) { b.lb[i] = lb[i]; b.ub[i] = ub[i]; }
    return b;
}

__device__ __forceinline__ void angle_axis_to_R(const double* w, double* R) {
    const double t2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
    if (t2 > DBL_EPSILON) {
        const double t = sqrt(t2), wx = w[0] / t, wy = w[1] / t, wz = w[2] / t, c = cos(t), s = sin(t);
        R[0] = c + wx * wx * (1 - c);       R[1] = wx * wy * (1 - c) - wz * s;  R[2] = wy * s + wx * wz * (1 - c);
        R[3] = wz * s + wx * wy * (1 - c);  R[4] = c + wy * wy * (1 - c);       R[5] = -wx * s + wy * wz * (1 - c);
        R[6] = -wy * s + wx * wz * (1 - c); R[7] = wx * s + wy * wz * (1 - c);  R[8] = c + wz * wz * (1 - c);
    } else {
        R[0] = 1; R[1] = -w[2]; R[2] = w[1]; R[3] = w[2]; R[4] = 1; R[5] = -w[0]; R[6] = -w[1]; R[7] = w[0]; R[8] = 1;
    }
}

__device__ __forceinline__ void params_to_pose(const double* x, int np, double* P) {      // row-major 4x4 (select_best_kernel, restart_consensus_kernel)
    double w[3] = {0, 0, 0};
    int toff;
    if (np == 4) { w[1] = x[0]; toff = 1; } else { w[0] = x[0]; w[1] = x[1]; w[2] = x[2]; toff = 3; }
    double Rm[9];
    angle_axis_to_R(w, Rm);
    for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) P[r * 4 + c] = Rm[r * 3 + c]; P[r * 4 + 3] = x[toff + r]; }
    P[12] = P[13] = P[14] = 0.0; P[15] = 1.0;
}

}  // namespace
