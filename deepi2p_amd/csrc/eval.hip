// Evaluation mode: what the reference does with a pose after it has one.
//
//  * pose errors -- evaluation/registration_lsq.py:87-95 (get_P_diff): RTE = |t| of P_pred^-1 P_gt, RRE = sum |euler 'xzy'| in degrees,
//    with the frame swap of :237-248 (enu2cam) for z-up clouds.  One thread per frame, fp64.
//  * summary statistics -- evaluation/registration_result_analysis.py:22-47,59,63: frames with cost > 1e-6, mean / sigma of both errors, the
//    success rate (t < 2 m and r < 5 deg), the two histograms of the plots; plus the per-batch label accuracies of
//    evaluation/visualize_and_save_data.py.  One workgroup folds a batch into a small device accumulator, frame by frame in index order.
//  * enu2cam on the points: (x, y, z) -> (x, -z, y), a permutation and one sign.
//
// Plain HIP C++: vector stores only, no allocation, no synchronisation -- every entry point can be captured into a hipGraph.
#include "common.h"
#include "pose_diff.h"

#include <math.h>

namespace {

constexpr int EVAL_BINS = 60;                 // per histogram: RTE over [0, 15) m, RRE over [0, 30) deg (the reference's plot ranges)
constexpr double RTE_BINS_PER_UNIT = 4.0;     // 60 / 15: bin edges k / 4 are exact in fp64, so floor(v * 4) is np.histogram's bin
constexpr double RRE_BINS_PER_UNIT = 2.0;     // 60 / 30
constexpr double RTE_RANGE = 15.0, RRE_RANGE = 30.0;
// The accumulator: 136 eight-byte words.
//   i64 [0] frames seen (mask != 0)   [1] frames valid (flags bit 0)   [2] successes among the valid   [3] frames with a coarse accuracy
//       [4] frames with a fine accuracy (NaN = no ground-truth point inside the image = not counted)   [5] RTE overflow   [6] RRE overflow   [7] 0
//   f64 [8] sum rte  [9] sum rte^2  [10] sum rre  [11] sum rre^2  (valid frames)   [12] sum coarse accuracy  [13] sum fine accuracy   [14] [15] 0
//   i64 [16..75] RTE histogram   [76..135] RRE histogram   (valid frames; a value at or above the range, or NaN, goes to the overflow count)
constexpr int ACC_COUNTS = 8, ACC_SUMS = 6, ACC_SUM0 = 8, ACC_HIST0 = 16;
constexpr int ACC_WORDS = ACC_HIST0 + 2 * EVAL_BINS;
constexpr int CNT_SEEN = 0, CNT_VALID = 1, CNT_SUCCESS = 2, CNT_COARSE = 3, CNT_FINE = 4, CNT_RTE_OVER = 5, CNT_RRE_OVER = 6;

// Both matrices times the inverse of the reference's P_convert (rows 1 0 0 0 / 0 0 -1 0 / 0 1 0 0 / 0 0 0 1) on the right:
// column 1 <- -column 2, column 2 <- column 1.  Exact.
__device__ inline void to_cam_columns(double* M) {
    for (int r = 0; r < 4; ++r) {
        const double c1 = M[4 * r + 1], c2 = M[4 * r + 2];
        M[4 * r + 1] = -c2;
        M[4 * r + 2] = c1;
    }
}

__global__ __launch_bounds__(64) void pose_errors_kernel(const double* __restrict__ P_pred, const double* __restrict__ P_gt, int gt_rows,
                                                         const double* __restrict__ cost, int enu, int F, double t_thresh, double r_thresh,
                                                         double* __restrict__ rte, double* __restrict__ rre, int* __restrict__ flags) {
    const int f = blockIdx.x * 64 + threadIdx.x;
    if (f >= F) return;
    double A[16], G[16];
    for (int i = 0; i < 12; ++i) A[i] = P_pred[16 * (long long)f + i];
    A[12] = A[13] = A[14] = 0.0; A[15] = 1.0;                                  // the bottom row of P_pred is taken as 0 0 0 1
    for (int i = 0; i < 4 * gt_rows; ++i) G[i] = P_gt[4 * (long long)gt_rows * f + i];
    if (gt_rows == 3) { G[12] = G[13] = G[14] = 0.0; G[15] = 1.0; }            // registration_lsq.py:298-299
    if (enu) { to_cam_columns(A); to_cam_columns(G); }
    double t, r;
    di2p_pose_diff(A, G, t, r);                                                // P_pred^-1 P_gt (pose_diff.h, shared with the restart consensus)
    rte[f] = t;
    rre[f] = r;
    const int valid = cost ? (cost[f] > 1e-6) : 1;                             // registration_result_analysis.py:22
    const int success = (t < t_thresh) && (r < r_thresh);                      // :37
    flags[f] = valid | (success << 1);
}

__device__ inline void count_bin(double v, double per_unit, double range, unsigned int* hist, unsigned int* over) {
    if (v >= 0.0 && v < range) {
        int k = (int)(v * per_unit);
        atomicAdd(&hist[k < EVAL_BINS ? k : EVAL_BINS - 1], 1u);
    } else if (v == range) {
        atomicAdd(&hist[EVAL_BINS - 1], 1u);                                    // np.histogram's last bin is closed
    } else {
        atomicAdd(over, 1u);
    }
}

// One workgroup of one wave.  The integer counts go through LDS atomics (integer sums do not depend on the order); the six fp64 sums are
// each carried by one lane that adds the frames in index order, so the accumulator is a function of the sequence of calls alone.
__global__ __launch_bounds__(64) void eval_accumulate_kernel(const double* __restrict__ rte, const double* __restrict__ rre,
                                                             const int* __restrict__ flags, const int* __restrict__ frame_mask,
                                                             const float* __restrict__ accuracy, int F, unsigned long long* acc) {
    __shared__ double s_add[ACC_SUMS][64];
    __shared__ unsigned int s_cnt[ACC_COUNTS + 2 * EVAL_BINS];
    const int tid = threadIdx.x;
    for (int i = tid; i < ACC_COUNTS + 2 * EVAL_BINS; i += 64) s_cnt[i] = 0u;
    double* accd = reinterpret_cast<double*>(acc);
    double sum = tid < ACC_SUMS ? accd[ACC_SUM0 + tid] : 0.0;
    __syncthreads();
    for (int base = 0; base < F; base += 64) {
        const int f = base + tid;
        double add[ACC_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (f < F && (!frame_mask || frame_mask[f] != 0)) {
            atomicAdd(&s_cnt[CNT_SEEN], 1u);
            const int fl = flags[f];
            if (fl & 1) {
                const double t = rte[f], r = rre[f];
                atomicAdd(&s_cnt[CNT_VALID], 1u);
                if (fl & 2) atomicAdd(&s_cnt[CNT_SUCCESS], 1u);
                add[0] = t; add[1] = __dmul_rn(t, t); add[2] = r; add[3] = __dmul_rn(r, r);
                count_bin(t, RTE_BINS_PER_UNIT, RTE_RANGE, &s_cnt[ACC_COUNTS], &s_cnt[CNT_RTE_OVER]);
                count_bin(r, RRE_BINS_PER_UNIT, RRE_RANGE, &s_cnt[ACC_COUNTS + EVAL_BINS], &s_cnt[CNT_RRE_OVER]);
            }
            if (accuracy) {
                const float ac = accuracy[2 * (long long)f], af = accuracy[2 * (long long)f + 1];
                if (ac == ac) { add[4] = (double)ac; atomicAdd(&s_cnt[CNT_COARSE], 1u); }
                if (af == af) { add[5] = (double)af; atomicAdd(&s_cnt[CNT_FINE], 1u); }
            }
        }
        for (int q = 0; q < ACC_SUMS; ++q) s_add[q][tid] = add[q];
        __syncthreads();
        if (tid < ACC_SUMS) {
            const int n = F - base < 64 ? F - base : 64;
            for (int j = 0; j < n; ++j) sum = __dadd_rn(sum, s_add[tid][j]);      // a skipped frame adds 0.0: exact
        }
        __syncthreads();
    }
    if (tid < ACC_SUMS) accd[ACC_SUM0 + tid] = sum;
    for (int i = tid; i < ACC_COUNTS + 2 * EVAL_BINS; i += 64) {
        const int w = i < ACC_COUNTS ? i : i - ACC_COUNTS + ACC_HIST0;
        acc[w] += (unsigned long long)s_cnt[i];
    }
}

__global__ __launch_bounds__(64) void eval_acc_reset_kernel(unsigned long long* acc) {
    for (int i = threadIdx.x; i < ACC_WORDS; i += 64) acc[i] = 0ull;
}

__global__ void enu2cam_points_kernel(const float* pc_in, float* pc_out, int N) {          // no __restrict__: in place is allowed
    const int b = blockIdx.y;
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const long long o = (long long)b * 3 * N + n;
    const float x = pc_in[o], y = pc_in[o + N], z = pc_in[o + 2ll * N];
    pc_out[o] = x;
    pc_out[o + N] = -z;
    pc_out[o + 2ll * N] = y;
}

}  // namespace

extern "C" long long di2p_eval_acc_bytes(void) { return 8ll * ACC_WORDS; }

extern "C" int di2p_pose_errors(const double* P_pred, const double* P_gt, int gt_rows, const double* cost, int enu, int F, double t_thresh,
                                double r_thresh, double* rte, double* rre, int32_t* flags, void* stream) {
    DI2P_CHECK_ARG(F >= 0 && (gt_rows == 3 || gt_rows == 4), "bad args (F >= 0, gt_rows 3 or 4)");
    if (F == 0) return 0;
    DI2P_CHECK_ARG(P_pred && P_gt && rte && rre && flags, "null pointer");
    hipLaunchKernelGGL(pose_errors_kernel, dim3(di2p_cdiv(F, 64)), dim3(64), 0, (hipStream_t)stream, P_pred, P_gt, gt_rows, cost, enu != 0, F,
                       t_thresh, r_thresh, rte, rre, flags);
    DI2P_RETURN_LAUNCH();
}

extern "C" int di2p_eval_accumulate(const double* rte, const double* rre, const int32_t* flags, const int32_t* frame_mask,
                                    const float* accuracy, int F, void* acc, void* stream) {
    DI2P_CHECK_ARG(F >= 0, "bad size");
    DI2P_CHECK_ARG(acc, "null accumulator");
    if (F == 0) return 0;
    DI2P_CHECK_ARG(rte && rre && flags, "null pointer");
    hipLaunchKernelGGL(eval_accumulate_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, rte, rre, flags, frame_mask, accuracy, F,
                       (unsigned long long*)acc);
    DI2P_RETURN_LAUNCH();
}

extern "C" int di2p_eval_acc_reset(void* acc, void* stream) {
    DI2P_CHECK_ARG(acc, "null accumulator");
    hipLaunchKernelGGL(eval_acc_reset_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (unsigned long long*)acc);
    DI2P_RETURN_LAUNCH();
}

extern "C" int di2p_enu2cam_points(const float* pc_in, float* pc_out, int B, int N, void* stream) {
    DI2P_CHECK_ARG(B >= 0 && N >= 0, "bad size");
    if (B == 0 || N == 0) return 0;
    DI2P_CHECK_ARG(pc_in && pc_out, "null pointer");
    hipLaunchKernelGGL(enu2cam_points_kernel, dim3(di2p_cdiv(N, 256), B), dim3(256), 0, (hipStream_t)stream, pc_in, pc_out, N);
    DI2P_RETURN_LAUNCH();
}
