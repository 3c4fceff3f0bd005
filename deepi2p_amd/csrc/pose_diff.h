// get_P_diff (evaluation/registration_lsq.py:87-95) on the device, shared by pose_errors_kernel (eval.hip) and restart_consensus_kernel
// (solver_aux.hip): translation norm and summed absolute extrinsic 'xzy' Euler angles, in degrees, of A^-1 G.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

// A, G: row-major 4x4 with the bottom row 0 0 0 1 (only G's is read).  t = |D[0:3,3]|, r = sum |euler 'xzy'| of D = A^-1 G in degrees.
__device__ __forceinline__ void di2p_pose_diff(const double* A, const double* G, double& t, double& r) {
    // affine inverse of A from the 3x3 cofactors: Ri = adj(R) / det, ti = -Ri t
    const double c00 = A[5] * A[10] - A[6] * A[9], c01 = A[6] * A[8] - A[4] * A[10], c02 = A[4] * A[9] - A[5] * A[8];
    const double det = A[0] * c00 + A[1] * c01 + A[2] * c02;
    const double inv = 1.0 / det;
    double Ri[9];
    Ri[0] = c00 * inv; Ri[1] = (A[2] * A[9] - A[1] * A[10]) * inv; Ri[2] = (A[1] * A[6] - A[2] * A[5]) * inv;
    Ri[3] = c01 * inv; Ri[4] = (A[0] * A[10] - A[2] * A[8]) * inv; Ri[5] = (A[2] * A[4] - A[0] * A[6]) * inv;
    Ri[6] = c02 * inv; Ri[7] = (A[1] * A[8] - A[0] * A[9]) * inv;  Ri[8] = (A[0] * A[5] - A[1] * A[4]) * inv;
    double ti[3];
    for (int r = 0; r < 3; ++r) ti[r] = -(Ri[3 * r] * A[3] + Ri[3 * r + 1] * A[7] + Ri[3 * r + 2] * A[11]);
    double D[12];                                                              // rows 0..2 of A^-1 G
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c)
            D[4 * r + c] = Ri[3 * r] * G[c] + Ri[3 * r + 1] * G[4 + c] + Ri[3 * r + 2] * G[8 + c] + ti[r] * G[12 + c];
    t = sqrt(D[3] * D[3] + D[7] * D[7] + D[11] * D[11]);
    // extrinsic 'xzy': R = Ry(c) Rz(b) Rx(a)  ->  R10 = sin b, R11 = cos b cos a, R12 = -cos b sin a, R00 = cos c cos b, R20 = -sin c cos b.
    // Within about 1e-3 deg of gimbal lock (|b| -> 90 deg) a and c are ill-conditioned (only their combination is determined); the
    // clamp keeps the result finite there and nothing more is promised.
    const double deg = 180.0 / 3.14159265358979323846;
    const double b = asin(fmin(1.0, fmax(-1.0, D[4])));
    const double a = atan2(-D[6], D[5]);
    const double c = atan2(-D[8], D[0]);
    r = fabs(a * deg) + fabs(b * deg) + fabs(c * deg);
}
