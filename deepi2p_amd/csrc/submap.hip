// Oxford sub-map building on the device (gfx950): the reference's raw stage of the Oxford data set, from 2-D LMS push-broom profiles
// and one vehicle pose per profile to the stored sub-map record.
//
// Replaces  data/oxford/build_dataset.py:79-148   my_build_pointcloud: per profile the keep rule (missing file, the "car did not move"
//                                                  skip against the last KEPT profile), the ground filter x < threshold, the transform
//                                                  pose . G_posesource_laser of (x, y, 0, 1), the reflectance carried along
//           data/oxford/build_dataset.py:310,319-321  the camera-frame transform of the voxel means and the float32 record
// The voxel pass between the two (:151-166, downsample) is di2p_voxel_down_sample (scan_prep.hip), unchanged.
//
// A batch is ragged on two levels: sub-map -> profiles (submap_offsets), profile -> rows (scan_offsets).  What that shares with the
// frames and sweeps of sweeps.hip is in ragged2.h: the offset acceptance (check_offsets2), the chunked 64-bit wave prefix (wave_prefix),
// offsets_kernel, the status codes and the workspace helpers.  Stages:
//   A  keep_kernel      one wave per sub-map: offset checks (ragged2.h), then the sequential keep chain (poses staged through LDS 64 at a time)
//   B  count_kernel     one wave per profile: surviving rows (ballot + popcount)
//      prefix_kernel    one wave per sub-map: exclusive prefix of the counts over its profiles, the sub-map's total (ragged2.h's wave_prefix)
//      offsets_kernel   (ragged2.h) one wave: exclusive prefix over the sub-maps, status
//   C  write_kernel     one wave per profile: M = pose . G once, rows read as coalesced 8-byte loads through LDS, ordered compaction with the
//                       ballot prefix, one 16-byte store per surviving row
//   E  to_camera_kernel one thread per voxel mean: G_cam in fp64, the record row
// All arithmetic that decides a bit is fp64 with explicit roundings (__dmul_rn / __dadd_rn) and FMA contraction off for this file (build.py),
// so tests/submap_oracle.py restates it in numpy value for value.
#include "common.h"
#include "ragged2.h"

namespace {

constexpr int WAVES = 4;          // waves of a workgroup in the per-profile kernels

struct Layout {
    size_t prof_sub, cnt, prof_off;          // per profile (S_cap): its sub-map or -1, surviving rows, first output row inside the sub-map
    size_t sub_total, sub_stat;              // per sub-map (B): surviving rows, status of stages A / B
    size_t total;
};

Layout layout(int B, int S_cap) {
    Layout L;
    Take take;
    L.prof_sub = take(4 * (size_t)S_cap); L.cnt = take(4 * (size_t)S_cap); L.prof_off = take(4 * (size_t)S_cap);
    L.sub_total = take(4 * (size_t)B); L.sub_stat = take(4 * (size_t)B);
    L.total = take.o;
    return L;
}

// Barrier between the LDS accesses of the lanes of ONE wave (the waves of a workgroup work on different profiles and never meet): a wave's
// LDS instructions execute in order; the fences keep the compiler from moving accesses across the point.
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(256) void init_kernel(int S_cap, int* __restrict__ kept, int* __restrict__ prof_sub, int* __restrict__ cnt) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s < S_cap) { kept[s] = -1; prof_sub[s] = -1; cnt[s] = 0; }
}

// Stage A.  Sub-map b is accepted iff submap_offsets[0 .. b+1] is a non-decreasing sequence in [0, S_cap] that starts at 0 (accepted
// sub-maps therefore never share a profile) and every profile of it has 0 <= scan_offsets[s] <= scan_offsets[s+1] <= P_cap.
// The chain: a missing profile (present[s] == 0) is passed over; a present one is skipped iff a previous KEPT profile exists and
// |R_prev^T (t - t_prev)|^2 < skip_threshold^2 (the translation of inv(prev) . pose for a rigid prev; squares compared, no square root).
__global__ __launch_bounds__(64) void keep_kernel(const int* __restrict__ scan_off, const int* __restrict__ sub_off, const double* __restrict__ poses,
                                                  const unsigned char* __restrict__ present, int B, int S_cap, int P_cap, double skip_threshold,
                                                  int* __restrict__ kept, int* __restrict__ skip_count, int* __restrict__ prof_sub,
                                                  int* __restrict__ sub_stat) {
    __shared__ double sp[64][13];          // R | t of 64 profiles, row-major 3 x 4; 13: odd stride in doubles
    __shared__ int spres[64];
    const int b = blockIdx.x, lane = threadIdx.x;
    const Units u = check_offsets2(scan_off, sub_off, b, lane, S_cap, P_cap);
    const int s0 = u.s0, s1 = u.s1;
    if (u.bad) {
        if (lane == 0) { sub_stat[b] = ST_OFFSETS; skip_count[b] = 0; }
        return;
    }
    const bool use_skip = skip_threshold >= 0.0;
    const double thr2 = __dmul_rn(skip_threshold, skip_threshold);
    bool have_prev = false;
    double pr[12];
    for (int k = 0; k < 12; ++k) pr[k] = 0.0;
    int skipped = 0;
    for (int c0 = s0; c0 < s1; c0 += 64) {
        const int n = min(64, s1 - c0);
        __syncthreads();
        if (lane < n) {
            const double* p = poses + 16 * (long long)(c0 + lane);
            for (int k = 0; k < 12; ++k) sp[lane][k] = p[k];
            spres[lane] = present ? (int)present[c0 + lane] : 1;
        }
        __syncthreads();
        int mine = -1;
        for (int j = 0; j < n; ++j) {          // every lane runs the same chain on LDS broadcasts; lane j keeps profile j's verdict
            if (!spres[j]) continue;
            int verdict = 1;
            if (have_prev && use_skip) {
                const double dx = __dsub_rn(sp[j][3], pr[3]), dy = __dsub_rn(sp[j][7], pr[7]), dz = __dsub_rn(sp[j][11], pr[11]);
                double n2 = 0.0;
                for (int i = 0; i < 3; ++i) {
                    const double e = __dadd_rn(__dadd_rn(__dmul_rn(pr[i], dx), __dmul_rn(pr[4 + i], dy)), __dmul_rn(pr[8 + i], dz));
                    n2 = __dadd_rn(n2, __dmul_rn(e, e));
                }
                if (n2 < thr2) verdict = 0;
            }
            if (verdict) {
                have_prev = true;
                for (int k = 0; k < 12; ++k) pr[k] = sp[j][k];
            } else {
                ++skipped;
            }
            if (j == lane) mine = verdict;
        }
        if (lane < n) { kept[c0 + lane] = mine; prof_sub[c0 + lane] = b; }
    }
    if (lane == 0) { sub_stat[b] = ST_OK; skip_count[b] = skipped; }
}

__device__ __forceinline__ bool row_survives(double x, int remove_ground, double ground_threshold) {
    return !remove_ground || x < ground_threshold;
}

// Stage B: one wave per profile of an accepted sub-map; cnt[s] = rows of a kept profile that pass the ground filter.
__global__ __launch_bounds__(WAVES * 64) void count_kernel(const double* __restrict__ xyr, const int* __restrict__ scan_off, int S_cap,
                                                           const int* __restrict__ kept, const int* __restrict__ prof_sub, int remove_ground,
                                                           double ground_threshold, int* __restrict__ cnt) {
    const int s = blockIdx.x * WAVES + wave_id(), lane = threadIdx.x & 63;
    if (s >= S_cap || prof_sub[s] < 0 || kept[s] != 1) return;
    const int r0 = scan_off[s], r1 = scan_off[s + 1];
    int n = r1 - r0;
    if (remove_ground) {
        n = 0;
        for (int r = r0; r < r1; r += 64) {
            const bool in = r + lane < r1;
            const double x = in ? xyr[3 * (long long)(r + lane)] : 0.0;
            n += __popcll(__ballot(in && row_survives(x, 1, ground_threshold)));
        }
    }
    if (lane == 0) cnt[s] = n;
}

// One wave per sub-map: prof_off[s] = surviving rows of the sub-map's profiles before s; sub_total[b] (wave_prefix: 64-bit lanes, clamped).
__global__ __launch_bounds__(64) void prefix_kernel(const int* __restrict__ sub_off, const int* __restrict__ sub_stat, const int* __restrict__ cnt,
                                                    int* __restrict__ prof_off, int* __restrict__ sub_total) {
    const int b = blockIdx.x, lane = threadIdx.x;
    if (sub_stat[b] != ST_OK) { if (lane == 0) sub_total[b] = 0; return; }
    const int total = wave_prefix(cnt, sub_off[b], sub_off[b + 1], lane, prof_off);
    if (lane == 0) sub_total[b] = total;
}

// Stage C: one wave per kept profile of a sub-map with status 0.
__global__ __launch_bounds__(WAVES * 64) void write_kernel(const double* __restrict__ xyr, const int* __restrict__ scan_off, const double* __restrict__ poses,
                                                           const double* __restrict__ G, int S_cap, const int* __restrict__ kept,
                                                           const int* __restrict__ prof_sub, const int* __restrict__ prof_off,
                                                           const int* __restrict__ sub_stat, const int* __restrict__ out_off, int remove_ground,
                                                           double ground_threshold, float* __restrict__ out) {
    __shared__ double rows[WAVES][192];
    const int w = wave_id(), s = blockIdx.x * WAVES + w, lane = threadIdx.x & 63;
    if (s >= S_cap) return;
    const int b = prof_sub[s];
    if (b < 0 || kept[s] != 1 || sub_stat[b] != ST_OK) return;
    // M = pose . G, the columns a row (x, y, 0, 1) meets: every entry a dot product in ascending k
    const double* P = poses + 16 * (long long)s;
    double M0[3], M1[3], M3[3];
    for (int i = 0; i < 3; ++i) {
        double a0 = 0.0, a1 = 0.0, a3 = 0.0;
        for (int k = 0; k < 4; ++k) {
            const double pik = P[4 * i + k];
            const double t0 = __dmul_rn(pik, G[4 * k + 0]), t1 = __dmul_rn(pik, G[4 * k + 1]), t3 = __dmul_rn(pik, G[4 * k + 3]);
            a0 = k ? __dadd_rn(a0, t0) : t0; a1 = k ? __dadd_rn(a1, t1) : t1; a3 = k ? __dadd_rn(a3, t3) : t3;
        }
        M0[i] = a0; M1[i] = a1; M3[i] = a3;
    }
    const int r0 = scan_off[s], r1 = scan_off[s + 1];
    long long dst = (long long)out_off[b] + prof_off[s];
    double* buf = rows[w];
    for (int r = r0; r < r1; r += 64) {
        const int n = min(64, r1 - r);
        const double* src = xyr + 3 * (long long)r;
        for (int k = 0; k < 3; ++k)          // 3 n consecutive doubles: lane-contiguous 8-byte loads
            if (64 * k + lane < 3 * n) buf[64 * k + lane] = src[64 * k + lane];
        wave_sync();
        const bool in = lane < n;
        const double x = in ? buf[3 * lane] : 0.0, y = in ? buf[3 * lane + 1] : 0.0, refl = in ? buf[3 * lane + 2] : 0.0;
        const bool keep = in && row_survives(x, remove_ground, ground_threshold);
        const unsigned long long mask = __ballot(keep);
        if (keep) {
            const int rank = __popcll(mask & ((1ull << lane) - 1ull));
            float4 o;
            o.x = (float)__dadd_rn(__dadd_rn(__dmul_rn(M0[0], x), __dmul_rn(M1[0], y)), M3[0]);
            o.y = (float)__dadd_rn(__dadd_rn(__dmul_rn(M0[1], x), __dmul_rn(M1[1], y)), M3[1]);
            o.z = (float)__dadd_rn(__dadd_rn(__dmul_rn(M0[2], x), __dmul_rn(M1[2], y)), M3[2]);
            o.w = (float)refl;
            *(float4*)(out + 4 * (dst + rank)) = o;
        }
        dst += __popcll(mask);
        wave_sync();
    }
}

// Stage E: q = G_cam[b] . (mean, 1) in fp64 (ascending k), the record row (q, intensity) rounded once.
__global__ __launch_bounds__(256) void to_camera_kernel(const double* __restrict__ cen, const float* __restrict__ inten, const int* __restrict__ off,
                                                        const double* __restrict__ G_cam, int B, int cap, float* __restrict__ out) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    const int total = min(max(off[B], 0), cap);
    if (v >= total) return;
    const int b = frame_of(off, B, v);
    const double* G = G_cam + 16 * (long long)b;
    const double x = cen[3 * v], y = cen[3 * v + 1], z = cen[3 * v + 2];
    float4 o;
    float* q = &o.x;
    for (int i = 0; i < 3; ++i)
        q[i] = (float)__dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(G[4 * i], x), __dmul_rn(G[4 * i + 1], y)), __dmul_rn(G[4 * i + 2], z)), G[4 * i + 3]);
    o.w = inten[v];
    *(float4*)(out + 4 * v) = o;
}

}  // namespace

extern "C" long long di2p_submap_workspace_bytes(int B, int S_cap) {
    if (B < 0 || S_cap < 0) return 0;
    return (long long)layout(B, S_cap).total;
}

extern "C" int di2p_submap_build(const double* scan_xyr, const int32_t* scan_offsets, const int32_t* submap_offsets, const double* poses,
                                 const uint8_t* present, const double* G_posesource_laser, int B, int S_cap, int P_cap, int cap,
                                 int max_frame_points, double skip_threshold, double ground_threshold, int remove_ground, int32_t* kept,
                                 int32_t* skip_count, int32_t* out_offsets, float* out_points, int32_t* status, void* workspace, void* stream) {
    DI2P_CHECK_ARG(B >= 0 && S_cap >= 0 && P_cap >= 0 && cap >= 0, "bad sizes (B, S_cap, P_cap, cap >= 0)");
    DI2P_CHECK_ARG(max_frame_points >= 0 && max_frame_points <= MAX_FRAME_POINTS, "max_frame_points above 2^20 rows per sub-map");
    DI2P_CHECK_ARG(skip_threshold == skip_threshold && skip_threshold < 1e150, "skip_threshold must be a number below 1e150 (negative: no skip rule)");
    DI2P_CHECK_ARG(!remove_ground || ground_threshold == ground_threshold, "ground_threshold must be a number");
    DI2P_CHECK_ARG(B == 0 || (scan_offsets && submap_offsets && G_posesource_laser && kept && skip_count && out_offsets && out_points && workspace),
                   "null pointer");
    DI2P_CHECK_ARG(B == 0 || S_cap == 0 || poses, "null pointer (poses)");
    DI2P_CHECK_ARG(B == 0 || P_cap == 0 || scan_xyr, "null pointer (scan_xyr)");
    DI2P_CHECK_ARG(((uintptr_t)workspace & 255) == 0 && ((uintptr_t)out_points & 15) == 0 && ((uintptr_t)scan_xyr & 7) == 0 &&
                       ((uintptr_t)poses & 7) == 0 && ((uintptr_t)G_posesource_laser & 7) == 0,
                   "workspace must be 256-byte, out_points 16-byte, scan_xyr / poses / G_posesource_laser 8-byte aligned");
    if (B == 0) return 0;
    const Layout L = layout(B, S_cap);
    hipStream_t st = (hipStream_t)stream;
    void* ws = workspace;
    int *prof_sub = at<int>(ws, L.prof_sub), *cnt = at<int>(ws, L.cnt), *prof_off = at<int>(ws, L.prof_off);
    int *sub_total = at<int>(ws, L.sub_total), *sub_stat = at<int>(ws, L.sub_stat);
    if (S_cap > 0) hipLaunchKernelGGL(init_kernel, dim3(di2p_cdiv(S_cap, 256)), dim3(256), 0, st, S_cap, kept, prof_sub, cnt);
    hipLaunchKernelGGL(keep_kernel, dim3(B), dim3(64), 0, st, scan_offsets, submap_offsets, poses, present, B, S_cap, P_cap, skip_threshold, kept,
                       skip_count, prof_sub, sub_stat);
    if (S_cap > 0)
        hipLaunchKernelGGL(count_kernel, dim3(di2p_cdiv(S_cap, WAVES)), dim3(WAVES * 64), 0, st, scan_xyr, scan_offsets, S_cap, kept, prof_sub,
                           remove_ground, ground_threshold, cnt);
    hipLaunchKernelGGL(prefix_kernel, dim3(B), dim3(64), 0, st, submap_offsets, sub_stat, cnt, prof_off, sub_total);
    hipLaunchKernelGGL(offsets_kernel, dim3(1), dim3(64), 0, st, B, cap, max_frame_points, sub_total, sub_stat, out_offsets, status);
    if (S_cap > 0)
        hipLaunchKernelGGL(write_kernel, dim3(di2p_cdiv(S_cap, WAVES)), dim3(WAVES * 64), 0, st, scan_xyr, scan_offsets, poses, G_posesource_laser,
                           S_cap, kept, prof_sub, prof_off, sub_stat, out_offsets, remove_ground, ground_threshold, out_points);
    DI2P_RETURN_LAUNCH();
}

extern "C" int di2p_submap_to_camera(const double* centroids, const float* intensity, const int32_t* voxel_offsets, const double* G_cam, int B,
                                     int cap, float* out_points, void* stream) {
    DI2P_CHECK_ARG(B >= 0 && cap >= 0, "bad sizes (B >= 0, cap >= 0)");
    DI2P_CHECK_ARG(B == 0 || cap == 0 || (centroids && intensity && voxel_offsets && G_cam && out_points), "null pointer");
    DI2P_CHECK_ARG(((uintptr_t)centroids & 7) == 0 && ((uintptr_t)G_cam & 7) == 0 && ((uintptr_t)out_points & 15) == 0,
                   "centroids / G_cam must be 8-byte, out_points 16-byte aligned");
    if (B == 0 || cap == 0) return 0;
    hipLaunchKernelGGL(to_camera_kernel, dim3(di2p_cdiv(cap, 256)), dim3(256), 0, (hipStream_t)stream, centroids, intensity, voxel_offsets, G_cam, B,
                       cap, out_points);
    DI2P_RETURN_LAUNCH();
}
