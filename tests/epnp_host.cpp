// csrc/epnp.h on the CPU: a one-thread point-set policy and a C wrapper around epnp::solve, built by tests/pnp_cases.py
// (plain C++, -ffp-contract=off) and loaded with ctypes.  TEST INFRASTRUCTURE ONLY; no GPU is involved.
#define DI2P_EPNP_HOST
#include "epnp.h"

namespace {

struct HostPoints {             // n correspondences, one thread: X[n][3], uv[n][2]
    const double* X;
    const double* uv;
    int n;
    int count() const { return n; }
    template <class F> void for_each(F f) const { for (int i = 0; i < n; ++i) f(X[3 * i], X[3 * i + 1], X[3 * i + 2], uv[2 * i], uv[2 * i + 1], i == 0); }
    double reduce(double v) const { return v; }
};

}  // namespace

// `sets` point sets of n points each: X[sets][n][3], uv[sets][n][2], cam = {fu, fv, uc, vc}
// -> R[sets][9] (row-major), t[sets][3], err[sets] (mean reprojection error), ok[sets]; an unaccepted set leaves R, t, err untouched
extern "C" void epnp_host_solve(const double* X, const double* uv, int n, int sets, const double* cam, double* R, double* t, double* err,
                                int* ok) {
    const epnp::Cam4 k{cam[0], cam[1], cam[2], cam[3]};
    for (int s = 0; s < sets; ++s) {
        HostPoints ps{X + (long long)s * n * 3, uv + (long long)s * n * 2, n};
        epnp::Pose pose;
        epnp::solve(ps, k, pose);
        ok[s] = pose.ok ? 1 : 0;
        if (!pose.ok) continue;
        for (int a = 0; a < 9; ++a) R[s * 9 + a] = pose.R[a];
        for (int a = 0; a < 3; ++a) t[s * 3 + a] = pose.t[a];
        err[s] = pose.err;
    }
}
