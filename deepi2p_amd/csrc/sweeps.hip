// nuScenes sweep accumulation on the device (gfx950): the raw stage of the nuScenes loader, from up to seven LiDAR sweeps per sample and the
// data set's pose / calibration records to one cloud in the key sweep's LiDAR frame, and P_cam_pc.
//
// Replaces  data/nuscenes_pc_img_pose_loader.py:58-78     get_sample_data_ego_pose_P / get_calibration_P / get_P_from_Rt: (quaternion wxyz,
//                                                          translation) -> 4x4 whose entries are float32 values               pose_kernel
//           :227-229, :249-252                             T_j = inv(P_vehicle_lidar) . (inv(P_oi) . P_oj) . P_vehicle_lidar
//           :292-293, :324-325, :351-354                   P_cam_pc = inv(camera_calib) . (inv(camera_pose) . (lidar_pose . lidar_calib))  transforms_kernel
//           :194-210, :242-267                             the ego-box filter of every sweep, the transform of the six neighbours, the
//                                                          concatenation key | next picks | prev picks                         di2p_sweep_accumulate
//
// A batch is ragged on two levels: frame -> sweeps (frame_offsets, key sweep first), sweep -> rows (sweep_offsets).  A sweep has about 35 k
// rows, so the unit of work is not the sweep but one of its PARTS equal parts (a multiple of TILE rows each): a frame's rows are spread over
// 32 x (its sweeps) workgroups.  Stages of the accumulation, the count / prefix / write split of submap.hip; what the two files share of it
// is in ragged2.h: the offset acceptance (check_offsets2), the chunked 64-bit wave prefix (wave_prefix), offsets_kernel, the status codes
// and the workspace helpers.
//   check_kernel    one wave per frame: offset checks (ragged2.h), sweep -> frame map
//   count_kernel    one workgroup per part: rows outside the ego box (ballot + popcount)
//   prefix_kernel   one wave per frame: exclusive prefix of the counts over the frame's parts (ragged2.h's wave_prefix), the kept rows per
//                   sweep, the frame's total
//   offsets_kernel  (ragged2.h) one wave: exclusive prefix over the frames, status
//   write_kernel    one workgroup per part: one 16-byte load and one 16-byte store per row, ordered compaction with the ballot prefix
// Every value that decides a bit is fp64 with explicit roundings (__dmul_rn / __dadd_rn) and FMA contraction off for this file (build.py), so
// tests/sweeps_oracle.py restates it in numpy value for value.  The box test is float32, as numpy compares a float32 column with a Python
// constant.
#include "common.h"
#include "ragged2.h"

namespace {

constexpr int MAX_SWEEPS = 1 << 24;          // PARTS * S_cap stays an int
constexpr int PARTS = 32;                    // workgroups a sweep is cut into
constexpr int TILE = 256;                    // rows a workgroup takes per iteration: one per thread

struct Layout {
    size_t sweep_frame;                      // per sweep (S_cap): its frame or -1
    size_t part_cnt, part_off;               // per part (PARTS * S_cap): surviving rows, first output row inside the frame
    size_t frame_total, frame_stat;          // per frame (B)
    size_t total;
};

Layout layout(int B, int S_cap) {
    Layout L;
    Take take;
    L.sweep_frame = take(4 * (size_t)S_cap);
    L.part_cnt = take(4 * (size_t)S_cap * PARTS); L.part_off = take(4 * (size_t)S_cap * PARTS);
    L.frame_total = take(4 * (size_t)B); L.frame_stat = take(4 * (size_t)B);
    L.total = take.o;
    return L;
}

// ---------------------------------------------------------------------------------------------------------------- poses
// One thread per record (w, x, y, z, tx, ty, tz): q / |q|, the closed form of the rotation matrix in fp64, every entry and the translation
// rounded to float32 and stored as fp64 (get_P_from_Rt puts float32 arrays into np.identity(4)).
__global__ __launch_bounds__(256) void pose_kernel(const double* __restrict__ rec, int n, double* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double* q = rec + 7 * (long long)i;
    double w = q[0], x = q[1], y = q[2], z = q[3];
    const double nrm = __dsqrt_rn(__dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(w, w), __dmul_rn(x, x)), __dmul_rn(y, y)), __dmul_rn(z, z)));
    w = __ddiv_rn(w, nrm); x = __ddiv_rn(x, nrm); y = __ddiv_rn(y, nrm); z = __ddiv_rn(z, nrm);
    const double xx = __dmul_rn(x, x), yy = __dmul_rn(y, y), zz = __dmul_rn(z, z);
    const double xy = __dmul_rn(x, y), xz = __dmul_rn(x, z), yz = __dmul_rn(y, z);
    const double wx = __dmul_rn(w, x), wy = __dmul_rn(w, y), wz = __dmul_rn(w, z);
    double R[9];
    R[0] = __dsub_rn(1.0, __dmul_rn(2.0, __dadd_rn(yy, zz))); R[1] = __dmul_rn(2.0, __dsub_rn(xy, wz)); R[2] = __dmul_rn(2.0, __dadd_rn(xz, wy));
    R[3] = __dmul_rn(2.0, __dadd_rn(xy, wz)); R[4] = __dsub_rn(1.0, __dmul_rn(2.0, __dadd_rn(xx, zz))); R[5] = __dmul_rn(2.0, __dsub_rn(yz, wx));
    R[6] = __dmul_rn(2.0, __dsub_rn(xz, wy)); R[7] = __dmul_rn(2.0, __dadd_rn(yz, wx)); R[8] = __dsub_rn(1.0, __dmul_rn(2.0, __dadd_rn(xx, yy)));
    double* P = out + 16 * (long long)i;
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) P[4 * r + c] = (double)(float)R[3 * r + c];
        P[4 * r + 3] = (double)(float)q[4 + r];
    }
    P[12] = 0.0; P[13] = 0.0; P[14] = 0.0; P[15] = 1.0;
}

// C = A . B, row-major 4x4: every entry a dot product in ascending k, products and sums rounded separately
__device__ __forceinline__ void mul44(const double* A, const double* B, double* C) {
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double a = __dmul_rn(A[4 * i], B[j]);
            for (int k = 1; k < 4; ++k) a = __dadd_rn(a, __dmul_rn(A[4 * i + k], B[4 * k + j]));
            C[4 * i + j] = a;
        }
}

// Ai = inverse of the affine A = [M t; 0 0 0 1] (its last row is not read): M^-1 = adj(M) / det(M) -- the poses have float32 rotation
// entries, so M is orthogonal only to about 2^-24 and its transpose is NOT its inverse to fp64 accuracy -- then -(M^-1 . t).
__device__ __forceinline__ void inv_affine(const double* A, double* Ai) {
    double c[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
            c[3 * i + j] = __dsub_rn(__dmul_rn(A[4 * i1 + j1], A[4 * i2 + j2]), __dmul_rn(A[4 * i1 + j2], A[4 * i2 + j1]));          // cofactor (i, j)
        }
    const double det = __dadd_rn(__dadd_rn(__dmul_rn(A[0], c[0]), __dmul_rn(A[1], c[1])), __dmul_rn(A[2], c[2]));
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) Ai[4 * i + j] = __ddiv_rn(c[3 * j + i], det);
        Ai[4 * i + 3] = -__dadd_rn(__dadd_rn(__dmul_rn(Ai[4 * i], A[3]), __dmul_rn(Ai[4 * i + 1], A[7])), __dmul_rn(Ai[4 * i + 2], A[11]));
    }
    Ai[12] = 0.0; Ai[13] = 0.0; Ai[14] = 0.0; Ai[15] = 1.0;
}

__device__ __forceinline__ void load44(const double* __restrict__ src, double* M) {
    for (int k = 0; k < 16; ++k) M[k] = src[k];
}

// One wave per frame whose sweep range [frame_off[b], frame_off[b+1]) lies inside [0, S_cap]; a lane per sweep.  The key sweep (the
// frame's first) gets the exact identity.  A frame without a sweep gets a zero P_cam_pc; one with a bad range is left alone.
__global__ __launch_bounds__(64) void transforms_kernel(const double* __restrict__ P_ego, const int* __restrict__ frame_off, const double* __restrict__ P_vl,
                                                        const double* __restrict__ P_ec, const double* __restrict__ P_vc, int S_cap,
                                                        double* __restrict__ T, double* __restrict__ P_cam_pc) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int s0 = frame_off[b], s1 = frame_off[b + 1];
    if (s0 < 0 || s1 < s0 || s1 > S_cap) return;
    double A[16], Bm[16], C[16], vl[16];
    if (s1 == s0) {
        if (lane < 16) P_cam_pc[16 * (long long)b + lane] = 0.0;
        return;
    }
    load44(P_vl + 16 * (long long)b, vl);
    if (lane == 0) {          // inv(camera_calib) . (inv(camera_pose) . (lidar_pose . lidar_calib))
        load44(P_ego + 16 * (long long)s0, A);
        mul44(A, vl, C);
        load44(P_ec + 16 * (long long)b, A);
        inv_affine(A, Bm);
        mul44(Bm, C, A);
        load44(P_vc + 16 * (long long)b, C);
        inv_affine(C, Bm);
        mul44(Bm, A, C);
        for (int k = 0; k < 16; ++k) P_cam_pc[16 * (long long)b + k] = C[k];
    }
    for (int s = s0 + lane; s < s1; s += 64) {
        double* dst = T + 16 * (long long)s;
        if (s == s0) {
            for (int k = 0; k < 16; ++k) dst[k] = (k % 5 == 0) ? 1.0 : 0.0;
            continue;
        }
        load44(P_ego + 16 * (long long)s0, A);
        inv_affine(A, Bm);                              // P_io
        load44(P_ego + 16 * (long long)s, A);
        mul44(Bm, A, C);                                // P_ij = P_io . P_oj
        inv_affine(vl, Bm);                             // P_lidar_vehicle
        mul44(Bm, C, A);
        mul44(A, vl, C);                                // (P_lidar_vehicle . P_ij) . P_vehicle_lidar
        for (int k = 0; k < 16; ++k) dst[k] = C[k];
    }
}

// ---------------------------------------------------------------------------------------------------------------- accumulation
__global__ __launch_bounds__(256) void init_kernel(int S_cap, int* __restrict__ kept, int* __restrict__ sweep_frame, int* __restrict__ part_cnt) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < (long long)S_cap * PARTS) part_cnt[i] = 0;
    if (i < S_cap) { kept[i] = 0; sweep_frame[i] = -1; }
}

// Frame b is accepted iff frame_offsets[0 .. b+1] is a non-decreasing sequence in [0, S_cap] that starts at 0 (accepted frames therefore
// never share a sweep) and every sweep of it has 0 <= sweep_offsets[s] <= sweep_offsets[s+1] <= P_cap.
__global__ __launch_bounds__(64) void check_kernel(const int* __restrict__ sweep_off, const int* __restrict__ frame_off, int S_cap, int P_cap,
                                                   int* __restrict__ sweep_frame, int* __restrict__ frame_stat) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const Units u = check_offsets2(sweep_off, frame_off, b, lane, S_cap, P_cap);
    if (!u.bad)
        for (int s = u.s0 + lane; s < u.s1; s += 64) sweep_frame[s] = b;
    if (lane == 0) frame_stat[b] = u.bad ? ST_OFFSETS : ST_OK;
}

// rows of one part of a sweep of n rows: a multiple of TILE, PARTS of them cover the sweep
__device__ __forceinline__ long long part_rows(int n) {
    const long long per = ((long long)n + PARTS - 1) / PARTS;
    return (per + TILE - 1) / TILE * TILE;
}

// the reference's mask, in float32: inside iff -bx < x < bx and -by < y < by (a NaN is outside, as in numpy)
__device__ __forceinline__ bool inside_box(float x, float y, float bx, float by) { return x < bx && x > -bx && y < by && y > -by; }

__global__ __launch_bounds__(TILE) void count_kernel(const float* __restrict__ rows, const int* __restrict__ sweep_off, int cols, float bx, float by,
                                                     const int* __restrict__ sweep_frame, int* __restrict__ part_cnt) {
    __shared__ int wc[TILE / 64];
    const int s = blockIdx.x / PARTS, p = blockIdx.x % PARTS;
    if (sweep_frame[s] < 0) return;
    const int r0 = sweep_off[s], r1 = sweep_off[s + 1];
    const long long len = part_rows(r1 - r0), a = (long long)r0 + p * len, e = min((long long)r1, a + len);
    if (a >= e) return;          // part_cnt stays 0
    int n = 0;
    for (long long r = a; r < e; r += TILE) {
        const long long row = r + threadIdx.x;
        bool keep = false;
        if (row < e) {
            const float2 xy = cols == 4 ? *(const float2*)(rows + 4 * row) : make_float2(rows[5 * row], rows[5 * row + 1]);
            keep = !inside_box(xy.x, xy.y, bx, by);
        }
        n += __popcll(__ballot(keep));
    }
    if ((threadIdx.x & 63) == 0) wc[wave_id()] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int w = 0; w < TILE / 64; ++w) t += wc[w];
        part_cnt[blockIdx.x] = t;
    }
}

// One wave per frame: part_off = surviving rows of the frame's parts before this one, kept[s] = those of sweep s, frame_total (a 64-bit
// running sum, clamped).
__global__ __launch_bounds__(64) void prefix_kernel(const int* __restrict__ frame_off, const int* __restrict__ frame_stat, const int* __restrict__ part_cnt,
                                                    int* __restrict__ part_off, int* __restrict__ kept, int* __restrict__ frame_total) {
    const int b = blockIdx.x, lane = threadIdx.x;
    if (frame_stat[b] != ST_OK) { if (lane == 0) frame_total[b] = 0; return; }
    const int s0 = frame_off[b], s1 = frame_off[b + 1];
    const int total = wave_prefix(part_cnt, (long long)s0 * PARTS, (long long)s1 * PARTS, lane, part_off);
    for (int s = s0 + lane; s < s1; s += 64) {
        long long t = 0;
        for (int p = 0; p < PARTS; ++p) t += part_cnt[(long long)s * PARTS + p];          // the parts of a sweep are disjoint: at most 2^31 - 1
        kept[s] = (int)t;
    }
    if (lane == 0) frame_total[b] = total;
}

// One workgroup per part of a sweep of a frame with status 0.  Thread t of iteration i holds row a + 256 i + t: the loads and, after the
// compaction (rank = rows kept by the waves before + the ballot prefix inside the wave), the stores of a wave are contiguous 16-byte pieces.
// The wave counts go through a double-buffered LDS array: one barrier per iteration.
__global__ __launch_bounds__(TILE) void write_kernel(const float* __restrict__ rows, const int* __restrict__ sweep_off, const int* __restrict__ frame_off,
                                                     const double* __restrict__ T, int cols, float bx, float by, const int* __restrict__ sweep_frame,
                                                     const int* __restrict__ part_off, const int* __restrict__ frame_stat,
                                                     const int* __restrict__ out_off, float* __restrict__ out) {
    __shared__ int wc[2][TILE / 64];
    const int s = blockIdx.x / PARTS, p = blockIdx.x % PARTS;
    const int b = sweep_frame[s];
    if (b < 0 || frame_stat[b] != ST_OK) return;
    const int r0 = sweep_off[s], r1 = sweep_off[s + 1];
    const long long len = part_rows(r1 - r0), a = (long long)r0 + p * len, e = min((long long)r1, a + len);
    if (a >= e) return;
    const bool key = s == frame_off[b];          // the key sweep is copied bit for bit
    double M[12];
    for (int k = 0; k < 12; ++k) M[k] = T[16 * (long long)s + k];
    const int w = wave_id(), lane = threadIdx.x & 63;
    long long dst = (long long)out_off[b] + part_off[blockIdx.x];
    int it = 0;
    for (long long r = a; r < e; r += TILE, it ^= 1) {
        const long long row = r + threadIdx.x;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        bool keep = false;
        if (row < e) {
            if (cols == 4) v = *(const float4*)(rows + 4 * row);
            else v = make_float4(rows[5 * row], rows[5 * row + 1], rows[5 * row + 2], rows[5 * row + 3]);
            keep = !inside_box(v.x, v.y, bx, by);
        }
        const unsigned long long mask = __ballot(keep);
        if (lane == 0) wc[it][w] = __popcll(mask);
        __syncthreads();
        int before = 0, all = 0;
        for (int k = 0; k < TILE / 64; ++k) {
            const int c = wc[it][k];
            before += k < w ? c : 0;
            all += c;
        }
        if (keep) {
            const int rank = before + __popcll(mask & ((1ull << lane) - 1ull));
            float4 o = v;
            if (!key) {
                const double x = (double)v.x, y = (double)v.y, z = (double)v.z;
                o.x = (float)__dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(M[0], x), __dmul_rn(M[1], y)), __dmul_rn(M[2], z)), M[3]);
                o.y = (float)__dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(M[4], x), __dmul_rn(M[5], y)), __dmul_rn(M[6], z)), M[7]);
                o.z = (float)__dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(M[8], x), __dmul_rn(M[9], y)), __dmul_rn(M[10], z)), M[11]);
            }
            *(float4*)(out + 4 * (dst + rank)) = o;
        }
        dst += all;
    }
}

}  // namespace

extern "C" long long di2p_sweep_workspace_bytes(int B, int S_cap) {
    if (B < 0 || S_cap < 0 || S_cap > MAX_SWEEPS) return 0;
    return (long long)layout(B, S_cap).total;
}

extern "C" int di2p_pose_matrices(const double* records, int n, double* out, void* stream) {
    DI2P_CHECK_ARG(n >= 0, "bad size (n >= 0)");
    DI2P_CHECK_ARG(n == 0 || (records && out), "null pointer");
    DI2P_CHECK_ARG(((uintptr_t)records & 7) == 0 && ((uintptr_t)out & 7) == 0, "records / out must be 8-byte aligned");
    if (n == 0) return 0;
    hipLaunchKernelGGL(pose_kernel, dim3(di2p_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, records, n, out);
    DI2P_RETURN_LAUNCH();
}

extern "C" int di2p_sweep_transforms(const double* P_ego, const int32_t* frame_offsets, const double* P_vehicle_lidar, const double* P_ego_cam,
                                     const double* P_vehicle_cam, int B, int S_cap, double* T, double* P_cam_pc, void* stream) {
    DI2P_CHECK_ARG(B >= 0 && S_cap >= 0, "bad sizes (B, S_cap >= 0)");
    DI2P_CHECK_ARG(B == 0 || (frame_offsets && P_vehicle_lidar && P_ego_cam && P_vehicle_cam && P_cam_pc), "null pointer");
    DI2P_CHECK_ARG(B == 0 || S_cap == 0 || (P_ego && T), "null pointer (P_ego, T)");
    DI2P_CHECK_ARG((((uintptr_t)P_ego | (uintptr_t)P_vehicle_lidar | (uintptr_t)P_ego_cam | (uintptr_t)P_vehicle_cam | (uintptr_t)T | (uintptr_t)P_cam_pc) & 7) == 0,
                   "the matrices must be 8-byte aligned");
    if (B == 0) return 0;
    hipLaunchKernelGGL(transforms_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, P_ego, frame_offsets, P_vehicle_lidar, P_ego_cam, P_vehicle_cam,
                       S_cap, T, P_cam_pc);
    DI2P_RETURN_LAUNCH();
}

extern "C" int di2p_sweep_accumulate(const float* rows, const int32_t* sweep_offsets, const int32_t* frame_offsets, const double* T, int B, int S_cap,
                                     int P_cap, int cols, int cap, int max_frame_points, float box_x, float box_y, int32_t* kept,
                                     int32_t* out_offsets, float* out_points, int32_t* status, void* workspace, void* stream) {
    DI2P_CHECK_ARG(B >= 0 && S_cap >= 0 && P_cap >= 0 && cap >= 0, "bad sizes (B, S_cap, P_cap, cap >= 0)");
    DI2P_CHECK_ARG(S_cap <= MAX_SWEEPS, "more than 2^24 sweeps");
    DI2P_CHECK_ARG(cols == 4 || cols == 5, "cols must be 4 (x, y, z, intensity) or 5 (the .pcd.bin rows: + ring)");
    DI2P_CHECK_ARG(max_frame_points >= 0 && max_frame_points <= MAX_FRAME_POINTS, "max_frame_points above 2^20 rows per frame");
    DI2P_CHECK_ARG(box_x == box_x && box_y == box_y, "the box half-extents must be numbers");
    DI2P_CHECK_ARG(B == 0 || (sweep_offsets && frame_offsets && out_offsets && out_points && workspace), "null pointer");
    DI2P_CHECK_ARG(B == 0 || S_cap == 0 || (T && kept), "null pointer (T, kept)");
    DI2P_CHECK_ARG(B == 0 || P_cap == 0 || rows, "null pointer (rows)");
    DI2P_CHECK_ARG(((uintptr_t)workspace & 255) == 0 && ((uintptr_t)out_points & 15) == 0 && ((uintptr_t)rows & (cols == 4 ? 15 : 3)) == 0 &&
                       ((uintptr_t)T & 7) == 0,
                   "workspace must be 256-byte, out_points (and rows with cols = 4) 16-byte, T 8-byte aligned");
    if (B == 0) return 0;
    const Layout L = layout(B, S_cap);
    hipStream_t st = (hipStream_t)stream;
    void* ws = workspace;
    int *sweep_frame = at<int>(ws, L.sweep_frame), *part_cnt = at<int>(ws, L.part_cnt), *part_off = at<int>(ws, L.part_off);
    int *frame_total = at<int>(ws, L.frame_total), *frame_stat = at<int>(ws, L.frame_stat);
    const int parts = S_cap * PARTS;
    if (S_cap > 0) hipLaunchKernelGGL(init_kernel, dim3(di2p_cdiv(parts, 256)), dim3(256), 0, st, S_cap, kept, sweep_frame, part_cnt);
    hipLaunchKernelGGL(check_kernel, dim3(B), dim3(64), 0, st, sweep_offsets, frame_offsets, S_cap, P_cap, sweep_frame, frame_stat);
    if (S_cap > 0)
        hipLaunchKernelGGL(count_kernel, dim3(parts), dim3(TILE), 0, st, rows, sweep_offsets, cols, box_x, box_y, sweep_frame, part_cnt);
    hipLaunchKernelGGL(prefix_kernel, dim3(B), dim3(64), 0, st, frame_offsets, frame_stat, part_cnt, part_off, kept, frame_total);
    hipLaunchKernelGGL(offsets_kernel, dim3(1), dim3(64), 0, st, B, cap, max_frame_points, frame_total, frame_stat, out_offsets, status);
    if (S_cap > 0)
        hipLaunchKernelGGL(write_kernel, dim3(parts), dim3(TILE), 0, st, rows, sweep_offsets, frame_offsets, T, cols, box_x, box_y, sweep_frame, part_off,
                           frame_stat, out_offsets, out_points);
    DI2P_RETURN_LAUNCH();
}
