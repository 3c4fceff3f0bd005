// Raw LiDAR scan preparation on the device (gfx950): the CPU stage between a Velodyne .bin scan and the network input.
//
// Replaces  data/kitti/kitti_pc_bin_to_npy_with_downsample_sn.py:50-74   Open3D voxel_down_sample (0.1), estimate_normals
//                                                                        (hybrid radius 0.6 / max_nn 30), orient_normals_to_align_with_direction
//                                                                        ([0,0,1]), cKDTree 1-NN intensity lookup
//           data/kitti_pc_img_pose_loader.py:26-44,296-306             the loader's second voxel pass (0.3 m, averaged intensity and normals)
//           data/kitti_pc_img_pose_loader.py:158-171,380               ragged random down-sample + the rigid transform into the camera frame
//                                                                        (the choice itself lives in rng.hip, di2p_random_choice_ragged)
//
// One workspace carries the state of a batch from di2p_voxel_down_sample to di2p_estimate_normals and di2p_nearest_raw: the per-frame
// bounds, the raw points sorted by (frame, voxel key), and the fp64 centroids (Open3D works on its double points; so do the later stages).
// All key and mean arithmetic is fp64 with FMA contraction off for this file (build.py), so it equals numpy value for value.
// Sorting: rocPRIM's stable device radix sort, temporary storage from the workspace.  Stability makes the summation order (ascending
// input index inside a voxel) and therefore the bits reproducible.
#include "common.h"
#include "normals_nn.h"
#include "philox.h"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

namespace {

constexpr int MAX_FRAME_POINTS = 1 << 20;
constexpr unsigned long long PAD_KEY = (1ull << 63) - 1;
constexpr int NN_CAP = 1024;          // LDS candidate buffer of one query (entries); compacted to the best max_nn when full
constexpr int CELL_WAVES = 4;          // normals_cells_kernel: waves of a workgroup, each on a query of its own
constexpr int CELL_CAND = 960;         // ... candidate capacity of a cell in LDS (entries: fp64 position + frame-local index, 28 B)
constexpr int ST_OK = 0, ST_TOO_MANY = 1, ST_SPAN = 2, ST_OFFSETS = 3;

// largest b in [0, B) with off[b] <= i (off non-decreasing)
__device__ __forceinline__ int frame_of(const int* __restrict__ off, int B, long long i) {
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((long long)off[mid] <= i) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// ---------------------------------------------------------------- workspace layout
struct Layout {
    size_t minb, imax, fstat, pass, nvox;                  // per frame: f64[B*3], f32[B], i32[B], i32[B]; i32[1]
    size_t pfr, key, iota, k1, i1, f1, f2, i2, k2;         // per raw point (cap)
    size_t head, scan, vstart, vfr, cen;                   // per voxel (cap + 1)
    size_t ck, ci2, ck2, cpos;                             // cell sort of the centroids
    size_t tmp, tmp_bytes;
    size_t chead, cscan, cstart, ncell;                    // cell runs of the sorted centroids (cap + 1 each; i32[1]): behind everything else
    size_t total;
};

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

size_t sort_tmp_bound(int cap) { return (size_t)24 * cap + ((size_t)1 << 20); }

Layout layout(int B, int cap) {
    Layout L;
    size_t o = 0;
    const size_t n = (size_t)cap, n1 = (size_t)cap + 1;
    auto take = [&](size_t bytes) { const size_t r = o; o = align256(o + bytes); return r; };
    L.minb = take(8 * 3 * (size_t)B); L.imax = take(4 * (size_t)B); L.fstat = take(4 * (size_t)B); L.pass = take(4 * (size_t)B); L.nvox = take(4);
    L.pfr = take(4 * n); L.key = take(8 * n); L.iota = take(4 * n); L.k1 = take(8 * n); L.i1 = take(4 * n);
    L.f1 = take(4 * n); L.f2 = take(4 * n); L.i2 = take(4 * n); L.k2 = take(8 * n);
    L.head = take(4 * n1); L.scan = take(4 * n1); L.vstart = take(4 * n1); L.vfr = take(4 * n1); L.cen = take(8 * 3 * n);
    L.ck = take(8 * n); L.ci2 = take(4 * n); L.ck2 = take(8 * n); L.cpos = take(8 * 3 * n);
    L.tmp_bytes = sort_tmp_bound(cap);
    L.tmp = take(L.tmp_bytes);
    L.chead = take(4 * n1); L.cscan = take(4 * n1); L.cstart = take(4 * n1); L.ncell = take(4);
    L.total = o;
    return L;
}

template <class T> T* at(void* ws, size_t off) { return (T*)((char*)ws + off); }

// ---------------------------------------------------------------- stage 1: voxel grid
// One workgroup per frame: bounds, maximum intensity, status.  min_bound = min - voxel/2 (Open3D VoxelDownSample).
__global__ __launch_bounds__(256) void frame_bounds_kernel(const float* __restrict__ pts, const int* __restrict__ off, int B, int cap,
                                                           int max_frame_points, double voxel, double max_extent, int min_points,
                                                           double* __restrict__ minb, float* __restrict__ imax, int* __restrict__ fstat,
                                                           int* __restrict__ pass, int* __restrict__ status) {
    __shared__ float s[7][256];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int s0 = off[b], s1 = off[b + 1];
    const bool offsets_ok = s0 >= 0 && s1 >= s0 && s1 <= cap && off[0] == 0;
    const int n = offsets_ok ? s1 - s0 : 0;
    const bool scan_ok = offsets_ok && n <= max_frame_points;
    float mn[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()}, mx[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
    float im = -__builtin_inff();
    if (scan_ok) {
        for (int i = s0 + tid; i < s1; i += 256) {
            const float4 p = *(const float4*)(pts + 4 * (long long)i);
            mn[0] = fminf(mn[0], p.x); mn[1] = fminf(mn[1], p.y); mn[2] = fminf(mn[2], p.z);
            mx[0] = fmaxf(mx[0], p.x); mx[1] = fmaxf(mx[1], p.y); mx[2] = fmaxf(mx[2], p.z);
            im = fmaxf(im, p.w);
        }
    }
    for (int c = 0; c < 3; ++c) { s[c][tid] = mn[c]; s[3 + c][tid] = mx[c]; }
    s[6][tid] = im;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
            for (int c = 0; c < 3; ++c) { s[c][tid] = fminf(s[c][tid], s[c][tid + o]); s[3 + c][tid] = fmaxf(s[3 + c][tid], s[3 + c][tid + o]); }
            s[6][tid] = fmaxf(s[6][tid], s[6][tid + o]);
        }
        __syncthreads();
    }
    if (tid == 0) {
        int st = !offsets_ok ? ST_OFFSETS : (n > max_frame_points ? ST_TOO_MANY : ST_OK);
        for (int c = 0; c < 3; ++c) {
            const double lo = n > 0 && st == ST_OK ? __dsub_rn((double)s[c][0], __dmul_rn(voxel, 0.5)) : 0.0;
            minb[3 * b + c] = lo;
            if (n > 0 && st == ST_OK) {
                const double ext = (double)s[3 + c][0] - (double)s[c][0];
                const double top = floor(((double)s[3 + c][0] - lo) / voxel);
                if (!(ext <= max_extent) || !(top <= (double)AXIS_MAX)) st = ST_SPAN;
            }
        }
        imax[b] = n > 0 ? s[6][0] : 0.0f;
        fstat[b] = st;
        pass[b] = n <= min_points;
        if (status) status[b] = st;
    }
}

// Voxel key of every raw point (original order) and its frame; positions past the batch sort last (frame B).
__global__ __launch_bounds__(256) void point_keys_kernel(const float* __restrict__ pts, const int* __restrict__ off, int B, int cap, double voxel,
                                                         const double* __restrict__ minb, const int* __restrict__ fstat,
                                                         unsigned* __restrict__ pfr, unsigned long long* __restrict__ key, int* __restrict__ iota) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= cap) return;
    iota[i] = (int)i;
    const int total = min(max(off[B], 0), cap);
    if (i >= total) { pfr[i] = (unsigned)B; key[i] = PAD_KEY; return; }
    const int b = frame_of(off, B, i);
    pfr[i] = (unsigned)b;
    if (fstat[b] != ST_OK) { key[i] = 0; return; }
    const float4 p = *(const float4*)(pts + 4 * i);
    const long long ix = clamp_axis(floor(((double)p.x - minb[3 * b + 0]) / voxel));
    const long long iy = clamp_axis(floor(((double)p.y - minb[3 * b + 1]) / voxel));
    const long long iz = clamp_axis(floor(((double)p.z - minb[3 * b + 2]) / voxel));
    key[i] = compose_key(ix, iy, iz);
}

__global__ __launch_bounds__(256) void gather_frames_kernel(const unsigned* __restrict__ elem_frame, const int* __restrict__ idx,
                                                            unsigned* __restrict__ out, int n) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j < n) out[j] = elem_frame[idx[j]];
}

__global__ __launch_bounds__(256) void gather_keys_kernel(const unsigned long long* __restrict__ key, const int* __restrict__ idx,
                                                          unsigned long long* __restrict__ out, int n) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j < n) out[j] = key[idx[j]];
}

// head[j] = 1 where sorted position j starts an output point (a new voxel; every point of a pass-through frame)
__global__ __launch_bounds__(256) void heads_kernel(const int* __restrict__ off, int B, int cap, const unsigned* __restrict__ sfr,
                                                    const unsigned long long* __restrict__ skey, const int* __restrict__ fstat,
                                                    const int* __restrict__ pass, int* __restrict__ head) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j > cap) return;
    const int total = min(max(off[B], 0), cap);
    int h = 0;
    if (j < total) {
        const unsigned b = sfr[j];
        if (b < (unsigned)B && fstat[b] == ST_OK)
            h = pass[b] ? 1 : (j == 0 || j == off[b] || skey[j] != skey[j - 1]);
    }
    head[j] = h;
}

__global__ __launch_bounds__(256) void voxel_index_kernel(const int* __restrict__ off, int B, int cap, const unsigned* __restrict__ sfr,
                                                          const int* __restrict__ head, const int* __restrict__ scan, int* __restrict__ vstart,
                                                          unsigned* __restrict__ vfr, int* __restrict__ out_off, int* __restrict__ nvox) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int total = min(max(off[B], 0), cap);
    if (j < total && head[j]) { vstart[scan[j]] = j; vfr[scan[j]] = sfr[j]; }
    if (j == total) { vstart[scan[j]] = total; *nvox = scan[j]; }
    if (j <= B) out_off[j] = scan[min(max(off[j], 0), total)];
}

// One thread per output point: the fp64 mean of the voxel's members in ascending input index (Open3D AccumulatedPoint: sum, then
// / double(n)); intensity as the loader's fake colour i / max averaged, then * max; normals averaged and not renormalised.
__global__ __launch_bounds__(256) void voxel_mean_kernel(const float* __restrict__ pts, const float* __restrict__ nrm_in, const int* __restrict__ off,
                                                         const int* __restrict__ out_off, const int* __restrict__ nvox_p, int cap,
                                                         const int* __restrict__ vstart, const unsigned* __restrict__ vfr,
                                                         const int* __restrict__ sidx, const unsigned long long* __restrict__ skey,
                                                         const unsigned long long* __restrict__ key, const float* __restrict__ imax,
                                                         const int* __restrict__ pass, double* __restrict__ cen, float* __restrict__ out_pts,
                                                         float* __restrict__ out_int, float* __restrict__ out_nrm, long long* __restrict__ out_key) {
    const int nvox = *nvox_p;
    for (int v = blockIdx.x * 256 + threadIdx.x; v < nvox && v < cap; v += gridDim.x * 256) {
        const int b = (int)vfr[v];
        double sx = 0.0, sy = 0.0, sz = 0.0, sc = 0.0, nx = 0.0, ny = 0.0, nz = 0.0;
        int cnt;
        unsigned long long k;
        const double mxi = (double)imax[b];
        if (pass[b]) {
            const long long gi = (long long)off[b] + (v - out_off[b]);
            const float4 p = *(const float4*)(pts + 4 * gi);
            cen[3 * (long long)v + 0] = (double)p.x; cen[3 * (long long)v + 1] = (double)p.y; cen[3 * (long long)v + 2] = (double)p.z;
            out_pts[3 * (long long)v + 0] = p.x; out_pts[3 * (long long)v + 1] = p.y; out_pts[3 * (long long)v + 2] = p.z;
            if (out_int) out_int[v] = p.w;
            if (out_nrm)
                for (int c = 0; c < 3; ++c) out_nrm[3 * (long long)v + c] = nrm_in[3 * gi + c];
            if (out_key) out_key[v] = (long long)key[gi];
            continue;
        }
        // the members end where the next voxel starts, and at the frame's end: the points of a REJECTED frame that follows sit between this
        // frame's last voxel and the next head (they start no voxel) and must not be averaged into it
        const int s = vstart[v], e = min(vstart[v + 1], off[b + 1]);
        cnt = e - s;
        k = skey[s];
        for (int j = s; j < e; ++j) {
            const long long gi = sidx[j];
            const float4 p = *(const float4*)(pts + 4 * gi);
            sx = __dadd_rn(sx, (double)p.x); sy = __dadd_rn(sy, (double)p.y); sz = __dadd_rn(sz, (double)p.z);
            if (out_int) sc = __dadd_rn(sc, (double)p.w / mxi);
            if (out_nrm) {
                nx = __dadd_rn(nx, (double)nrm_in[3 * gi + 0]); ny = __dadd_rn(ny, (double)nrm_in[3 * gi + 1]);
                nz = __dadd_rn(nz, (double)nrm_in[3 * gi + 2]);
            }
        }
        const double dn = (double)cnt;
        const double mx = sx / dn, my = sy / dn, mz = sz / dn;
        cen[3 * (long long)v + 0] = mx; cen[3 * (long long)v + 1] = my; cen[3 * (long long)v + 2] = mz;
        out_pts[3 * (long long)v + 0] = (float)mx; out_pts[3 * (long long)v + 1] = (float)my; out_pts[3 * (long long)v + 2] = (float)mz;
        if (out_int) out_int[v] = (float)__dmul_rn(sc / dn, mxi);
        if (out_nrm) {
            out_nrm[3 * (long long)v + 0] = (float)(nx / dn); out_nrm[3 * (long long)v + 1] = (float)(ny / dn);
            out_nrm[3 * (long long)v + 2] = (float)(nz / dn);
        }
        if (out_key) out_key[v] = (long long)k;
    }
}

// ---------------------------------------------------------------- stage 2: normals
// Grid key of every centroid: cell = radius * (1 + 2^-20) (slightly larger than r: a rounding at a cell border can never hide a
// neighbour from the 27-cell scan).  Frame from the voxel offsets; positions past the batch sort last.
__global__ __launch_bounds__(256) void cell_keys_kernel(const double* __restrict__ cen, const int* __restrict__ out_off, int B, int cap,
                                                        const int* __restrict__ nvox_p, const double* __restrict__ minb, double cell,
                                                        unsigned* __restrict__ cfr, unsigned long long* __restrict__ ck, int* __restrict__ iota) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= cap) return;
    iota[v] = v;
    if (v >= *nvox_p) { cfr[v] = (unsigned)B; ck[v] = PAD_KEY; return; }
    const int b = frame_of(out_off, B, v);
    cfr[v] = (unsigned)b;
    ck[v] = compose_key(clamp_axis(floor((cen[3 * (long long)v + 0] - minb[3 * b + 0]) / cell)),
                        clamp_axis(floor((cen[3 * (long long)v + 1] - minb[3 * b + 1]) / cell)),
                        clamp_axis(floor((cen[3 * (long long)v + 2] - minb[3 * b + 2]) / cell)));
}

__global__ __launch_bounds__(256) void cell_positions_kernel(const double* __restrict__ cen, const int* __restrict__ ci2, const int* __restrict__ nvox_p,
                                                             double* __restrict__ cpos) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= *nvox_p) return;
    const long long v = ci2[j];
    for (int c = 0; c < 3; ++c) cpos[3 * (long long)j + c] = cen[3 * v + c];
}

// normal_from_list's positions (normals_nn.h): list entry i is centroid fs + i of the frame, already fp64
struct CentroidPos {
    const double* __restrict__ cen;
    int fs;
    __device__ __forceinline__ void operator()(int i, double& x, double& y, double& z) const {
        const long long g = (long long)fs + i;
        x = cen[3 * g + 0]; y = cen[3 * g + 1]; z = cen[3 * g + 2];
    }
};

// One wave (workgroup of 64) per query centroid, persistent over the batch.  The 27 neighbour cells (9 key ranges of 3 z-adjacent cells)
// are located by binary search in the frame's cell-sorted keys (18 lanes in parallel), their members streamed 64 at a time; candidates with d2 < r2 that beat the
// current max_nn-th best (d2, index) are appended to an LDS list, which is sorted and cut back to max_nn whenever it fills.  The list
// never spills and the selection is exact: the result is the max_nn smallest (d2, index) pairs inside the ball.
__global__ __launch_bounds__(64) void normals_kernel(const double* __restrict__ cen, const double* __restrict__ cpos, const int* __restrict__ ci2,
                                                     const unsigned long long* __restrict__ ck2, const int* __restrict__ out_off, int B,
                                                     const int* __restrict__ nvox_p, const double* __restrict__ minb, double cell, double r2,
                                                     int max_nn, float* __restrict__ normals, int* __restrict__ nn_count, int* __restrict__ nn_idx) {
    __shared__ unsigned long long sd[NN_CAP];
    __shared__ int si[NN_CAP];
    const int lane = threadIdx.x;
    const int nvox = *nvox_p;
    for (int jq = blockIdx.x; jq < nvox; jq += gridDim.x) {
        const int v = ci2[jq];              // queries in cell order: neighbouring workgroups read the same cells
        const int b = frame_of(out_off, B, v);
        const int fs = out_off[b], fe = out_off[b + 1];
        const double qx = cen[3 * (long long)v + 0], qy = cen[3 * (long long)v + 1], qz = cen[3 * (long long)v + 2];
        // the three z-neighbour cells of an (x, y) column are one key range: 9 ranges, lanes 0-8 find their starts, 9-17 their ends
        int pos = fs;
        if (lane < 18) {
            const int r = lane % 9;
            const long long cx = (long long)floor((qx - minb[3 * b + 0]) / cell) + r % 3 - 1;
            const long long cy = (long long)floor((qy - minb[3 * b + 1]) / cell) + r / 3 - 1;
            const long long cz = (long long)floor((qz - minb[3 * b + 2]) / cell);
            if (cx >= 0 && cy >= 0 && cx <= AXIS_MAX && cy <= AXIS_MAX) {
                const bool upper = lane >= 9;
                const unsigned long long k = upper ? compose_key(cx, cy, cz + 1 < AXIS_MAX ? cz + 1 : AXIS_MAX) : compose_key(cx, cy, cz > 0 ? cz - 1 : 0);
                int lo = fs, hi = fe;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (upper ? ck2[mid] <= k : ck2[mid] < k) lo = mid + 1; else hi = mid;
                }
                pos = lo;
            }
        }
        int cnt = 0;
        unsigned long long thr_d = ~0ull;
        int thr_i = 0x7fffffff;
        for (int c = 0; c < 9; ++c) {
            const int s = __shfl(pos, c, 64), e = __shfl(pos, c + 9, 64);
            for (int base = s; base < e; base += 64) {
                const int j = base + lane;
                bool acc = false;
                unsigned long long db = 0;
                int li = 0;
                if (j < e) {
                    const double d2 = d2_of(cpos[3 * (long long)j + 0], cpos[3 * (long long)j + 1], cpos[3 * (long long)j + 2], qx, qy, qz);
                    db = (unsigned long long)__double_as_longlong(d2);
                    li = ci2[j] - fs;
                    acc = d2 < r2 && nn_less(db, li, thr_d, thr_i);
                }
                const unsigned long long m = __ballot(acc);
                if (acc) {
                    const int pos = cnt + __popcll(m & ((1ull << lane) - 1));
                    sd[pos] = db; si[pos] = li;
                }
                cnt += __popcll(m);
                __syncthreads();
                if (cnt > NN_CAP - 64) {
                    nn_sort<false>(sd, si, cnt, lane);
                    if (cnt >= max_nn) { thr_d = sd[max_nn - 1]; thr_i = si[max_nn - 1]; cnt = max_nn; }
                    __syncthreads();
                }
            }
        }
        nn_sort<false>(sd, si, cnt, lane);
        normal_from_list(CentroidPos{cen, fs}, si, cnt, max_nn, v, lane, 2, 1, normals, nn_count, nn_idx);          // Open3D's direction [0,0,1]
        __syncthreads();
    }
}

// ---- cell-cooperative normals
// head[j] = 1 where sorted position j starts a cell: a run of equal (frame, cell key) among the centroids
__global__ __launch_bounds__(256) void cell_heads_kernel(const unsigned* __restrict__ sfr, const unsigned long long* __restrict__ ck2,
                                                         const int* __restrict__ nvox_p, int cap, int* __restrict__ head) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j > cap) return;
    const int nvox = min(max(*nvox_p, 0), cap);
    head[j] = j < nvox && (j == 0 || sfr[j] != sfr[j - 1] || ck2[j] != ck2[j - 1]);
}

// cstart[c] = first sorted position of cell c, cstart[ncell] = nvox
__global__ __launch_bounds__(256) void cell_starts_kernel(const int* __restrict__ head, const int* __restrict__ scan, const int* __restrict__ nvox_p,
                                                          int cap, int* __restrict__ cstart, int* __restrict__ ncell) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j > cap) return;
    const int nvox = min(max(*nvox_p, 0), cap);
    if (j < nvox && head[j]) cstart[scan[j]] = j;
    if (j == nvox) { cstart[scan[j]] = nvox; *ncell = scan[j]; }
}

// One workgroup (CELL_WAVES waves) per occupied grid cell, persistent over the batch.  Once per cell: the 9 key ranges of the 27 neighbour
// cells by binary search (18 threads), their members staged into LDS (fp64 position + frame-local index).  Then every wave takes
// queries of the cell in turn and selects from the staged set exactly as normals_kernel does from global memory: the same acceptance
// rule, an LDS list per wave cut back to the best max_nn when it fills, the same final sort and the same tail (normal_from_list), so
// the outputs are the per-query kernel's bit for bit (the selection is exact, hence independent of the candidate order and the list size).
// A cell whose candidate set exceeds CELL_CAND is not staged: its queries stream the ranges from global memory.
__global__ __launch_bounds__(CELL_WAVES * 64) void normals_cells_kernel(const double* __restrict__ cen, const double* __restrict__ cpos,
                                                                        const int* __restrict__ ci2, const unsigned long long* __restrict__ ck2,
                                                                        const unsigned* __restrict__ sfr, const int* __restrict__ cstart,
                                                                        const int* __restrict__ ncell_p, const int* __restrict__ out_off, int B,
                                                                        double r2, int max_nn, float* __restrict__ normals,
                                                                        int* __restrict__ nn_count, int* __restrict__ nn_idx) {
    __shared__ double cx[CELL_CAND], cy[CELL_CAND], cz[CELL_CAND];
    __shared__ int cli[CELL_CAND];
    __shared__ unsigned long long sd_all[CELL_WAVES * CELL_NN_CAP];
    __shared__ int si_all[CELL_WAVES * CELL_NN_CAP];
    __shared__ int rs[9], re[9], pre[10];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    unsigned long long* sd = sd_all + w * CELL_NN_CAP;
    int* si = si_all + w * CELL_NN_CAP;
    const int ncell = *ncell_p;
    for (int c = blockIdx.x; c < ncell; c += gridDim.x) {
        const int s0 = cstart[c], s1 = cstart[c + 1];
        const int b = min((int)sfr[s0], B - 1);
        const int fs = out_off[b], fe = out_off[b + 1];
        if (tid < 18) {
            const unsigned long long key = ck2[s0];
            const int r = tid % 9;
            const bool upper = tid >= 9;
            const long long kx = (long long)(key >> (2 * AXIS_BITS)) + r % 3 - 1;
            const long long ky = (long long)((key >> AXIS_BITS) & AXIS_MAX) + r / 3 - 1;
            const long long kz = (long long)(key & AXIS_MAX);
            int pos = fs;
            if (kx >= 0 && ky >= 0 && kx <= AXIS_MAX && ky <= AXIS_MAX) {
                const unsigned long long k = upper ? compose_key(kx, ky, kz + 1 < AXIS_MAX ? kz + 1 : AXIS_MAX) : compose_key(kx, ky, kz > 0 ? kz - 1 : 0);
                int lo = fs, hi = fe;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (upper ? ck2[mid] <= k : ck2[mid] < k) lo = mid + 1; else hi = mid;
                }
                pos = lo;
            }
            (upper ? re : rs)[r] = pos;
        }
        __syncthreads();
        if (tid == 0) {
            int a = 0;
            for (int r = 0; r < 9; ++r) { pre[r] = a; a += re[r] - rs[r]; }
            pre[9] = a;
        }
        __syncthreads();
        const int total = pre[9];
        const bool staged = total <= CELL_CAND;
        if (staged) {
            for (int t = tid; t < total; t += CELL_WAVES * 64) {
                int r = 0;
                while (r < 8 && t >= pre[r + 1]) ++r;
                const long long j = rs[r] + (t - pre[r]);
                cx[t] = cpos[3 * j + 0]; cy[t] = cpos[3 * j + 1]; cz[t] = cpos[3 * j + 2];
                cli[t] = ci2[j] - fs;
            }
        }
        __syncthreads();
        for (int q = s0 + w; q < s1; q += CELL_WAVES) {
            const int v = ci2[q];
            const double qx = cpos[3 * (long long)q + 0], qy = cpos[3 * (long long)q + 1], qz = cpos[3 * (long long)q + 2];   // = cen[3 v + .]
            int cnt = 0;
            unsigned long long thr_d = ~0ull;
            int thr_i = 0x7fffffff;
            if (staged) {
                for (int base = 0; base < total; base += 64) {
                    const int t = base + lane;
                    const bool in = t < total;
                    const double d2 = in ? d2_of(cx[t], cy[t], cz[t], qx, qy, qz) : 0.0;
                    nn_offer(in, d2, in ? cli[t] : 0, r2, max_nn, sd, si, cnt, thr_d, thr_i, lane);
                }
            } else {
                for (int r = 0; r < 9; ++r) {
                    const int e = re[r];
                    for (int base = rs[r]; base < e; base += 64) {
                        const int j = base + lane;
                        const bool in = j < e;
                        const double d2 = in ? d2_of(cpos[3 * (long long)j + 0], cpos[3 * (long long)j + 1], cpos[3 * (long long)j + 2], qx, qy, qz) : 0.0;
                        nn_offer(in, d2, in ? ci2[j] - fs : 0, r2, max_nn, sd, si, cnt, thr_d, thr_i, lane);
                    }
                }
            }
            nn_sort<true>(sd, si, cnt, lane);
            normal_from_list(CentroidPos{cen, fs}, si, cnt, max_nn, v, lane, 2, 1, normals, nn_count, nn_idx);          // Open3D's direction [0,0,1]
            nn_sync<true>();
        }
        __syncthreads();          // the next cell's staging overwrites what the other waves may still read
    }
}

// ---------------------------------------------------------------- stage 3: 1-NN in the raw scan
__device__ __forceinline__ void scan_voxel(const float* __restrict__ pts, const int* __restrict__ sidx, const unsigned long long* __restrict__ skey,
                                           int fs, int fe, unsigned long long k, double qx, double qy, double qz, double& best, int& bi) {
    int lo = fs, hi = fe;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (skey[mid] < k) lo = mid + 1; else hi = mid; }
    for (int j = lo; j < fe && skey[j] == k; ++j) {
        const int gi = sidx[j];
        const float4 p = *(const float4*)(pts + 4 * (long long)gi);
        const double d2 = d2_of((double)p.x, (double)p.y, (double)p.z, qx, qy, qz);
        if (d2 < best || (d2 == best && gi < bi)) { best = d2; bi = gi; }
    }
}

// One thread per centroid: own voxel first, then every voxel the ball of the best distance so far touches (bounds widened by 1e-9
// relative + 1e-9 absolute against rounding), ties -> the lower raw index.  Exact.
__global__ __launch_bounds__(256) void nearest_raw_kernel(const float* __restrict__ pts, const int* __restrict__ off, const int* __restrict__ out_off,
                                                          int B, const int* __restrict__ nvox_p, const double* __restrict__ cen,
                                                          const double* __restrict__ minb, double voxel, const int* __restrict__ sidx,
                                                          const unsigned long long* __restrict__ skey, int* __restrict__ nn_idx,
                                                          float* __restrict__ nn_int, double* __restrict__ nn_d2) {
    const int nvox = *nvox_p;
    for (int v = blockIdx.x * 256 + threadIdx.x; v < nvox; v += gridDim.x * 256) {
        const int b = frame_of(out_off, B, v);
        const int fs = off[b], fe = off[b + 1];
        const double q[3] = {cen[3 * (long long)v + 0], cen[3 * (long long)v + 1], cen[3 * (long long)v + 2]};
        long long own[3];
        for (int c = 0; c < 3; ++c) own[c] = clamp_axis(floor((q[c] - minb[3 * b + c]) / voxel));
        double best = __builtin_inf();
        int bi = 0x7fffffff;
        const unsigned long long kown = compose_key(own[0], own[1], own[2]);
        scan_voxel(pts, sidx, skey, fs, fe, kown, q[0], q[1], q[2], best, bi);
        long long lo[3], hi[3];
        const double rad = best < __builtin_inf() ? sqrt(best) * (1.0 + 1e-9) + 1e-9 : 0.0;
        for (int c = 0; c < 3; ++c) {
            if (best < __builtin_inf()) {
                lo[c] = clamp_axis(floor((q[c] - rad - minb[3 * b + c]) / voxel));
                hi[c] = clamp_axis(floor((q[c] + rad - minb[3 * b + c]) / voxel));
            } else {             // (not reached for a centroid of this frame: its own voxel holds its members)
                lo[c] = own[c] > 2 ? own[c] - 2 : 0;
                hi[c] = own[c] + 2 < AXIS_MAX ? own[c] + 2 : AXIS_MAX;
            }
        }
        for (long long x = lo[0]; x <= hi[0]; ++x)
            for (long long y = lo[1]; y <= hi[1]; ++y)
                for (long long z = lo[2]; z <= hi[2]; ++z) {
                    const unsigned long long k = compose_key(x, y, z);
                    if (k != kown) scan_voxel(pts, sidx, skey, fs, fe, k, q[0], q[1], q[2], best, bi);
                }
        const bool found = bi != 0x7fffffff;
        if (nn_idx) nn_idx[v] = found ? bi - fs : -1;
        if (nn_int) nn_int[v] = found ? pts[4 * (long long)bi + 3] : 0.0f;
        if (nn_d2) nn_d2[v] = best;
    }
}

// ---------------------------------------------------------------- stage 4: ragged gather (+ jitter) (+ rigid transform)
// Jitter (sigma > 0): clip(sigma * N(0,1), +-clip) rounded to float32, a pure function of (seed, stream_id, frame, output index, component):
// Philox counter (n, frame, stream_id * 8 + component, 5), component 0..2 the point, 3 the intensity (di2p_gather_ragged_aug_intensity only),
// 4..6 the normal; Box-Muller on two 53-bit uniforms.
struct Jitter { unsigned long long seed; const unsigned long long* seed_dev; int stream_id; double sigma, clip; int intensity; };

__device__ __forceinline__ float jitter_noise(unsigned long long seed, const Jitter& j, int b, int n, int comp) {
    const U4 r = philox4x32_10(U4{(unsigned)n, (unsigned)b, (unsigned)(j.stream_id * 8 + comp), 5u}, (unsigned)seed, (unsigned)(seed >> 32));
    const double z = sqrt(-2.0 * log(u53(r.x, r.y))) * cos(6.283185307179586476925 * u53(r.z, r.w));
    const double v = j.sigma * z;
    return (float)(v < -j.clip ? -j.clip : v > j.clip ? j.clip : v);
}

__global__ __launch_bounds__(256) void gather_ragged_kernel(const float* __restrict__ pts, const float* __restrict__ inten, const float* __restrict__ nrm,
                                                            const int* __restrict__ off, const int* __restrict__ idx, const double* __restrict__ T,
                                                            int n_out, float* __restrict__ pc, float* __restrict__ out_int, float* __restrict__ sn,
                                                            Jitter jit) {
    const int b = blockIdx.y, n = blockIdx.x * 256 + threadIdx.x;
    if (n >= n_out) return;
    const int i = idx[(long long)b * n_out + n];
    const bool ok = i >= 0 && i < off[b + 1] - off[b];
    const long long g = (long long)off[b] + (ok ? i : 0);
    double p[3] = {0.0, 0.0, 0.0}, s[3] = {0.0, 0.0, 0.0};
    float it = 0.0f;
    if (ok) {
        for (int c = 0; c < 3; ++c) p[c] = (double)pts[3 * g + c];
        if (nrm) for (int c = 0; c < 3; ++c) s[c] = (double)nrm[3 * g + c];
        if (inten) it = inten[g];
        if (jit.sigma > 0.0) {      // augmentation.jitter_point_cloud: float32 noise + float32 value, before the transform, normals not re-normalised
            const unsigned long long seed = jit.seed_dev ? *jit.seed_dev : jit.seed;
            for (int c = 0; c < 3; ++c) {
                p[c] = (double)__fadd_rn(jitter_noise(seed, jit, b, n, c), (float)p[c]);
                if (nrm) s[c] = (double)__fadd_rn(jitter_noise(seed, jit, b, n, 4 + c), (float)s[c]);
            }
            if (jit.intensity && inten) it = __fadd_rn(jitter_noise(seed, jit, b, n, DI2P_JITTER_SLOT_INTENSITY), it);
        }
    }
    const long long o3 = (long long)b * 3 * n_out + n;
    if (T && ok) {
        const double* M = T + 16 * (long long)b;
        for (int r = 0; r < 3; ++r) {
            pc[o3 + (long long)r * n_out] = (float)(((M[4 * r] * p[0] + M[4 * r + 1] * p[1]) + M[4 * r + 2] * p[2]) + M[4 * r + 3]);
            if (sn) sn[o3 + (long long)r * n_out] = (float)((M[4 * r] * s[0] + M[4 * r + 1] * s[1]) + M[4 * r + 2] * s[2]);
        }
    } else {
        for (int r = 0; r < 3; ++r) {
            pc[o3 + (long long)r * n_out] = (float)p[r];
            if (sn) sn[o3 + (long long)r * n_out] = (float)s[r];
        }
    }
    if (out_int) out_int[(long long)b * n_out + n] = it;
}

// ---------------------------------------------------------------- stage 0 (Oxford loader): range filter + shuffle + compaction
// data/oxford_pc_img_pose_loader.py:269-279.  Point i of frame b is kept iff fl32(fl32(x x) + fl32(z z)) < fl32(r r) (r <= 0: every point);
// the kept points of a frame come out in ascending order of key(seed, b, i) = the upper 63 bits of the first two words of Philox counter
// (i, b, 0, 6), ties to the lower i (the sort is stable).  Dropped points, the rows past the batch and every point of a rejected frame go
// to the sentinel frame B and are never written.
__global__ __launch_bounds__(256) void shuffle_keys_kernel(const float* __restrict__ pts, const int* __restrict__ off, int B, int cap,
                                                           int max_frame_points, float r2, unsigned long long seed,
                                                           const unsigned long long* __restrict__ seed_dev, unsigned* __restrict__ pfr,
                                                           unsigned long long* __restrict__ key, int* __restrict__ iota, int* __restrict__ status) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool head_ok = off[0] == 0;
    if (i < B && status) {
        const int s0 = off[i], s1 = off[i + 1];
        const bool ok = head_ok && s0 >= 0 && s1 >= s0 && s1 <= cap;
        status[i] = !ok ? ST_OFFSETS : (s1 - s0 > max_frame_points ? ST_TOO_MANY : ST_OK);
    }
    if (i >= cap) return;
    iota[i] = (int)i;
    pfr[i] = (unsigned)B;
    key[i] = PAD_KEY;
    const int total = min(max(off[B], 0), cap);
    if (i >= total) return;
    const int b = frame_of(off, B, i);
    const int s0 = off[b], s1 = off[b + 1];
    if (!(head_ok && s0 >= 0 && s1 >= s0 && s1 <= cap && s1 - s0 <= max_frame_points && i >= s0 && i < s1)) return;
    const float4 p = *(const float4*)(pts + 4 * i);
    if (r2 > 0.0f && !(__fadd_rn(__fmul_rn(p.x, p.x), __fmul_rn(p.z, p.z)) < r2)) return;
    if (seed_dev) seed = *seed_dev;
    const U4 r = philox4x32_10(U4{(unsigned)(i - s0), (unsigned)b, 0u, 6u}, (unsigned)seed, (unsigned)(seed >> 32));
    pfr[i] = (unsigned)b;
    key[i] = (((unsigned long long)r.x << 32) | (unsigned long long)r.y) >> 1;
}

// out_off[j] = the first sorted position whose frame is >= j (j = 0 .. B); sorted position p of a kept point is its output row
__global__ __launch_bounds__(256) void shuffle_compact_kernel(const float* __restrict__ pts, const unsigned* __restrict__ sfr,
                                                              const int* __restrict__ sidx, int B, int cap, float* __restrict__ out,
                                                              int* __restrict__ out_off) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j <= B) {
        int lo = 0, hi = cap;
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (sfr[mid] < (unsigned)j) lo = mid + 1; else hi = mid; }
        out_off[j] = lo;
    }
    if (j < cap && sfr[j] < (unsigned)B) *(float4*)(out + 4 * j) = *(const float4*)(pts + 4 * (long long)sidx[j]);
}

int frame_bits(int B) { int bits = 1; while ((1ll << bits) <= B) ++bits; return bits; }

// Stable sort of `cap` elements by (frame, 63-bit key): a stable radix sort on the key, then a stable one on the frame of each element
// (LSD order).  idx_out = original positions, key_out = their keys, fr_out = their frames.
// Above 2^20 elements rocPRIM's radix sort switches from its merge-sort path to onesweep (decoupled look-back: a memset of the look-back
// states and of an atomic workgroup counter before every digit place).  Memset nodes of a captured graph are not reliably ordered before
// the kernel node behind them when the graph is replayed here: replayed with 1.92 M elements that path ended in an
// illegal memory access (eager launches of the same sort are fine, and so are replays of the merge-sort path, which clears nothing), so
// while the stream is capturing the sorts stay on the merge-sort path at every size.  Both paths are stable sorts: the same output, bit for bit.
using SortMergeOnly = rocprim::radix_sort_config<rocprim::default_config, rocprim::default_config, rocprim::default_config, (size_t)1 << 40>;

template <class Cfg>
hipError_t sort_by_frame_key_cfg(void* ws, const Layout& L, int B, int cap, const unsigned long long* key_in, const unsigned* elem_frame,
                                 int* idx_out, unsigned long long* key_out, unsigned* fr_out, hipStream_t st) {
    void* tmp = at<void>(ws, L.tmp);
    size_t need1 = 0, need2 = 0;
    hipError_t e;
    e = rocprim::radix_sort_pairs<Cfg>(nullptr, need1, key_in, at<unsigned long long>(ws, L.k1), at<int>(ws, L.iota), at<int>(ws, L.i1), cap, 0, 63, st);
    if (e != hipSuccess) return e;
    e = rocprim::radix_sort_pairs<Cfg>(nullptr, need2, at<unsigned>(ws, L.f1), fr_out, at<int>(ws, L.i1), idx_out, cap, 0, frame_bits(B), st);
    if (e != hipSuccess) return e;
    if (need1 > L.tmp_bytes || need2 > L.tmp_bytes) return hipErrorInvalidValue;
    size_t sz = L.tmp_bytes;
    e = rocprim::radix_sort_pairs<Cfg>(tmp, sz, key_in, at<unsigned long long>(ws, L.k1), at<int>(ws, L.iota), at<int>(ws, L.i1), cap, 0, 63, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(gather_frames_kernel, dim3(di2p_cdiv(cap, 256)), dim3(256), 0, st, elem_frame, at<int>(ws, L.i1), at<unsigned>(ws, L.f1), cap);
    sz = L.tmp_bytes;
    e = rocprim::radix_sort_pairs<Cfg>(tmp, sz, at<unsigned>(ws, L.f1), fr_out, at<int>(ws, L.i1), idx_out, cap, 0, frame_bits(B), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(gather_keys_kernel, dim3(di2p_cdiv(cap, 256)), dim3(256), 0, st, key_in, idx_out, key_out, cap);
    return hipGetLastError();
}

hipError_t sort_by_frame_key(void* ws, const Layout& L, int B, int cap, const unsigned long long* key_in, const unsigned* elem_frame,
                             int* idx_out, unsigned long long* key_out, unsigned* fr_out, hipStream_t st) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    const hipError_t e = hipStreamIsCapturing(st, &cs);
    if (e != hipSuccess) return e;
    if (cs != hipStreamCaptureStatusNone) return sort_by_frame_key_cfg<SortMergeOnly>(ws, L, B, cap, key_in, elem_frame, idx_out, key_out, fr_out, st);
    return sort_by_frame_key_cfg<rocprim::default_config>(ws, L, B, cap, key_in, elem_frame, idx_out, key_out, fr_out, st);
}

int persistent_grid(int per_cu) { return di2p_cu_count() * per_cu; }

}  // namespace

extern "C" long long di2p_scan_prep_workspace_bytes(int B, int cap) {
    if (B < 0 || cap < 0) return 0;
    return (long long)layout(B, cap).total;
}

// Byte offset, inside the workspace of (B, cap), of the fp64 means f64[cap,3] di2p_voxel_down_sample leaves there (output point order):
// later stages that go on in fp64 (submap.hip's camera transform) read them instead of the rounded out_points.
extern "C" long long di2p_scan_prep_centroids_offset(int B, int cap) {
    if (B < 0 || cap < 0) return -1;
    return (long long)layout(B, cap).cen;
}

extern "C" int di2p_voxel_down_sample(const float* points, const int32_t* offsets, int B, int cap, int max_frame_points, double voxel,
                                      double max_extent, int min_points, const float* normals_in, int32_t* out_offsets, float* out_points,
                                      float* out_intensity, float* out_normals, int64_t* out_keys, int32_t* status, void* workspace,
                                      void* stream) {
    DI2P_CHECK_ARG(B >= 0 && cap >= 0, "bad sizes (B >= 0, cap >= 0)");
    DI2P_CHECK_ARG(voxel > 0.0 && voxel < 1e30, "voxel size must be positive and finite");
    DI2P_CHECK_ARG(max_frame_points >= 0 && max_frame_points <= MAX_FRAME_POINTS, "max_frame_points above 2^20 points per frame");
    DI2P_CHECK_ARG(max_extent >= 0.0 && max_extent / voxel < (double)AXIS_MAX - 2.0, "voxel index span above 2^21 per axis (max_extent / voxel)");
    DI2P_CHECK_ARG(!out_normals || normals_in, "out_normals needs normals_in");
    DI2P_CHECK_ARG(B == 0 || (points && offsets && out_offsets && out_points && workspace), "null pointer");
    DI2P_CHECK_ARG(((uintptr_t)workspace & 255) == 0, "workspace must be 256-byte aligned");
    if (B == 0) return 0;
    const Layout L = layout(B, cap);
    hipStream_t st = (hipStream_t)stream;
    void* ws = workspace;
    hipLaunchKernelGGL(frame_bounds_kernel, dim3(B), dim3(256), 0, st, points, offsets, B, cap, max_frame_points, voxel, max_extent, min_points,
                       at<double>(ws, L.minb), at<float>(ws, L.imax), at<int>(ws, L.fstat), at<int>(ws, L.pass), status);
    if (cap > 0) {
        hipLaunchKernelGGL(point_keys_kernel, dim3(di2p_cdiv(cap, 256)), dim3(256), 0, st, points, offsets, B, cap, voxel, at<double>(ws, L.minb),
                           at<int>(ws, L.fstat), at<unsigned>(ws, L.pfr), at<unsigned long long>(ws, L.key), at<int>(ws, L.iota));
        const hipError_t e = sort_by_frame_key(ws, L, B, cap, at<unsigned long long>(ws, L.key), at<unsigned>(ws, L.pfr), at<int>(ws, L.i2),
                                               at<unsigned long long>(ws, L.k2), at<unsigned>(ws, L.f2), st);
        if (e != hipSuccess) { di2p_set_error("di2p_voxel_down_sample: sort failed: %s", hipGetErrorString(e)); return (int)e; }
    }
    hipLaunchKernelGGL(heads_kernel, dim3(di2p_cdiv(cap + 1, 256)), dim3(256), 0, st, offsets, B, cap, at<unsigned>(ws, L.f2),
                       at<unsigned long long>(ws, L.k2), at<int>(ws, L.fstat), at<int>(ws, L.pass), at<int>(ws, L.head));
    size_t need = 0;
    hipError_t e = rocprim::exclusive_scan(nullptr, need, at<int>(ws, L.head), at<int>(ws, L.scan), 0, (size_t)cap + 1, rocprim::plus<int>(), st);
    if (e == hipSuccess && need > L.tmp_bytes) e = hipErrorInvalidValue;
    if (e == hipSuccess) {
        need = L.tmp_bytes;
        e = rocprim::exclusive_scan(at<void>(ws, L.tmp), need, at<int>(ws, L.head), at<int>(ws, L.scan), 0, (size_t)cap + 1, rocprim::plus<int>(), st);
    }
    if (e != hipSuccess) { di2p_set_error("di2p_voxel_down_sample: scan failed: %s", hipGetErrorString(e)); return (int)e; }
    hipLaunchKernelGGL(voxel_index_kernel, dim3(di2p_cdiv(cap + 1 > B + 1 ? cap + 1 : B + 1, 256)), dim3(256), 0, st, offsets, B, cap,
                       at<unsigned>(ws, L.f2), at<int>(ws, L.head), at<int>(ws, L.scan), at<int>(ws, L.vstart), at<unsigned>(ws, L.vfr),
                       out_offsets, at<int>(ws, L.nvox));
    if (cap > 0)
        hipLaunchKernelGGL(voxel_mean_kernel, dim3(min(di2p_cdiv(cap, 256), persistent_grid(8))), dim3(256), 0, st, points, normals_in, offsets,
                           out_offsets, at<int>(ws, L.nvox), cap, at<int>(ws, L.vstart), at<unsigned>(ws, L.vfr), at<int>(ws, L.i2),
                           at<unsigned long long>(ws, L.k2), at<unsigned long long>(ws, L.key), at<float>(ws, L.imax), at<int>(ws, L.pass),
                           at<double>(ws, L.cen), out_points, out_intensity, out_normals, (long long*)out_keys);
    DI2P_RETURN_LAUNCH();
}

namespace {

// Shared front of the two normals entry points: argument checks, cell keys, the (frame, key) sort, positions in sorted order.
// -> 0 to go on, 1 when there is nothing to do, else the error code
int normals_front(const char* fn, const int32_t* voxel_offsets, int B, int cap, double radius, int max_nn, double max_extent, float* normals,
                  void* workspace, hipStream_t st, Layout& L, double& cell) {
#define FRONT_CHECK(cond, msg) do { if (!(cond)) { di2p_set_error("%s: %s", fn, msg); return -1; } } while (0)
    FRONT_CHECK(B >= 0 && cap >= 0, "bad sizes (B >= 0, cap >= 0)");
    FRONT_CHECK(radius > 0.0 && radius < 1e30, "radius must be positive and finite");
    FRONT_CHECK(max_nn >= 1 && max_nn <= NN_MAX, "max_nn must be in [1, 64]");
    FRONT_CHECK(max_extent >= 0.0 && max_extent / radius < (double)AXIS_MAX - 4.0, "grid cell index span above 2^21 per axis (max_extent / radius)");
    FRONT_CHECK(B == 0 || (voxel_offsets && normals && workspace), "null pointer");
    FRONT_CHECK(((uintptr_t)workspace & 255) == 0, "workspace must be 256-byte aligned");
#undef FRONT_CHECK
    if (B == 0 || cap == 0) return 1;
    L = layout(B, cap);
    void* ws = workspace;
    cell = radius * (1.0 + 1.0 / 1048576.0);
    // cell keys into L.ck, frames into L.pfr (the raw frames are no longer needed: the raw sort result lives in i2 / k2 / f2)
    hipLaunchKernelGGL(cell_keys_kernel, dim3(di2p_cdiv(cap, 256)), dim3(256), 0, st, at<double>(ws, L.cen), voxel_offsets, B, cap, at<int>(ws, L.nvox),
                       at<double>(ws, L.minb), cell, at<unsigned>(ws, L.pfr), at<unsigned long long>(ws, L.ck), at<int>(ws, L.iota));
    // the frame-sorted output goes to f1's twin: reuse L.head (i32, cap + 1) for the sorted frames; it is not read after stage 1
    const hipError_t e = sort_by_frame_key(ws, L, B, cap, at<unsigned long long>(ws, L.ck), at<unsigned>(ws, L.pfr), at<int>(ws, L.ci2),
                                           at<unsigned long long>(ws, L.ck2), at<unsigned>(ws, L.head), st);
    if (e != hipSuccess) { di2p_set_error("%s: sort failed: %s", fn, hipGetErrorString(e)); return (int)e; }
    hipLaunchKernelGGL(cell_positions_kernel, dim3(di2p_cdiv(cap, 256)), dim3(256), 0, st, at<double>(ws, L.cen), at<int>(ws, L.ci2),
                       at<int>(ws, L.nvox), at<double>(ws, L.cpos));
    return 0;
}

}  // namespace

extern "C" int di2p_estimate_normals(const int32_t* voxel_offsets, int B, int cap, double radius, int max_nn, double max_extent, float* normals,
                                     int32_t* nn_count, int32_t* nn_idx, void* workspace, void* stream) {
    Layout L;
    double cell;
    hipStream_t st = (hipStream_t)stream;
    const int rc = normals_front("di2p_estimate_normals", voxel_offsets, B, cap, radius, max_nn, max_extent, normals, workspace, st, L, cell);
    if (rc) return rc == 1 ? 0 : rc;
    void* ws = workspace;
    hipLaunchKernelGGL(normals_kernel, dim3(min(cap, persistent_grid(32))), dim3(64), 0, st, at<double>(ws, L.cen), at<double>(ws, L.cpos),
                       at<int>(ws, L.ci2), at<unsigned long long>(ws, L.ck2), voxel_offsets, B, at<int>(ws, L.nvox), at<double>(ws, L.minb), cell,
                       radius * radius, max_nn, normals, nn_count, nn_idx);
    DI2P_RETURN_LAUNCH();
}

extern "C" int di2p_normals_cells_candidates(void) { return CELL_CAND; }

extern "C" int di2p_estimate_normals_cells(const int32_t* voxel_offsets, int B, int cap, double radius, int max_nn, double max_extent,
                                           float* normals, int32_t* nn_count, int32_t* nn_idx, void* workspace, void* stream) {
    Layout L;
    double cell;
    hipStream_t st = (hipStream_t)stream;
    const int rc = normals_front("di2p_estimate_normals_cells", voxel_offsets, B, cap, radius, max_nn, max_extent, normals, workspace, st, L, cell);
    if (rc) return rc == 1 ? 0 : rc;
    void* ws = workspace;
    // the cells: runs of equal (frame, key) in the sorted order -> their start positions (flags, exclusive scan, scatter)
    hipLaunchKernelGGL(cell_heads_kernel, dim3(di2p_cdiv(cap + 1, 256)), dim3(256), 0, st, at<unsigned>(ws, L.head), at<unsigned long long>(ws, L.ck2),
                       at<int>(ws, L.nvox), cap, at<int>(ws, L.chead));
    size_t need = 0;
    hipError_t e = rocprim::exclusive_scan(nullptr, need, at<int>(ws, L.chead), at<int>(ws, L.cscan), 0, (size_t)cap + 1, rocprim::plus<int>(), st);
    if (e == hipSuccess && need > L.tmp_bytes) e = hipErrorInvalidValue;
    if (e == hipSuccess) {
        need = L.tmp_bytes;
        e = rocprim::exclusive_scan(at<void>(ws, L.tmp), need, at<int>(ws, L.chead), at<int>(ws, L.cscan), 0, (size_t)cap + 1, rocprim::plus<int>(), st);
    }
    if (e != hipSuccess) { di2p_set_error("di2p_estimate_normals_cells: scan failed: %s", hipGetErrorString(e)); return (int)e; }
    hipLaunchKernelGGL(cell_starts_kernel, dim3(di2p_cdiv(cap + 1, 256)), dim3(256), 0, st, at<int>(ws, L.chead), at<int>(ws, L.cscan),
                       at<int>(ws, L.nvox), cap, at<int>(ws, L.cstart), at<int>(ws, L.ncell));
    hipLaunchKernelGGL(normals_cells_kernel, dim3(min(cap, persistent_grid(4))), dim3(CELL_WAVES * 64), 0, st, at<double>(ws, L.cen),
                       at<double>(ws, L.cpos), at<int>(ws, L.ci2), at<unsigned long long>(ws, L.ck2), at<unsigned>(ws, L.head), at<int>(ws, L.cstart),
                       at<int>(ws, L.ncell), voxel_offsets, B, radius * radius, max_nn, normals, nn_count, nn_idx);
    DI2P_RETURN_LAUNCH();
}

extern "C" int di2p_nearest_raw(const float* points, const int32_t* offsets, const int32_t* voxel_offsets, int B, int cap, double voxel,
                                int32_t* nn_idx, float* nn_intensity, double* nn_dist2, void* workspace, void* stream) {
    DI2P_CHECK_ARG(B >= 0 && cap >= 0, "bad sizes (B >= 0, cap >= 0)");
    DI2P_CHECK_ARG(voxel > 0.0 && voxel < 1e30, "voxel size must be positive and finite");
    DI2P_CHECK_ARG(B == 0 || (points && offsets && voxel_offsets && workspace), "null pointer");
    DI2P_CHECK_ARG(((uintptr_t)workspace & 255) == 0, "workspace must be 256-byte aligned");
    if (B == 0 || cap == 0) return 0;
    const Layout L = layout(B, cap);
    void* ws = workspace;
    hipLaunchKernelGGL(nearest_raw_kernel, dim3(min(di2p_cdiv(cap, 256), persistent_grid(8))), dim3(256), 0, (hipStream_t)stream, points, offsets,
                       voxel_offsets, B, at<int>(ws, L.nvox), at<double>(ws, L.cen), at<double>(ws, L.minb), voxel, at<int>(ws, L.i2),
                       at<unsigned long long>(ws, L.k2), nn_idx, nn_intensity, nn_dist2);
    DI2P_RETURN_LAUNCH();
}

extern "C" int di2p_gather_ragged(const float* points, const float* intensity, const float* normals, const int32_t* offsets, const int32_t* idx,
                                  const double* transform, int B, int n_out, float* pc, float* intensity_out, float* sn, void* stream) {
    DI2P_CHECK_ARG(B >= 0 && n_out >= 0, "bad sizes");
    DI2P_CHECK_ARG(B == 0 || n_out == 0 || (points && offsets && idx && pc), "null pointer");
    DI2P_CHECK_ARG(!intensity_out || intensity, "intensity_out needs intensity");
    DI2P_CHECK_ARG(!sn || normals, "sn needs normals");
    if (B == 0 || n_out == 0) return 0;
    hipLaunchKernelGGL(gather_ragged_kernel, dim3(di2p_cdiv(n_out, 256), B), dim3(256), 0, (hipStream_t)stream, points, intensity, normals, offsets,
                       idx, transform, n_out, pc, intensity_out, sn, Jitter{0ull, nullptr, 0, 0.0, 0.0, 0});
    DI2P_RETURN_LAUNCH();
}

extern "C" int di2p_gather_ragged_aug(const float* points, const float* intensity, const float* normals, const int32_t* offsets, const int32_t* idx,
                                      const double* transform, int B, int n_out, unsigned long long seed, const unsigned long long* seed_dev,
                                      int stream_id, double sigma, double clip, float* pc, float* intensity_out, float* sn, void* stream) {
    DI2P_CHECK_ARG(B >= 0 && n_out >= 0, "bad sizes");
    DI2P_CHECK_ARG(B == 0 || n_out == 0 || (points && offsets && idx && pc), "null pointer");
    DI2P_CHECK_ARG(!intensity_out || intensity, "intensity_out needs intensity");
    DI2P_CHECK_ARG(!sn || normals, "sn needs normals");
    DI2P_CHECK_ARG(sigma >= 0.0 && sigma < 1e30 && clip > 0.0 && stream_id >= 0 && stream_id < (1 << 28), "jitter needs 0 <= sigma, clip > 0");
    DI2P_CHECK_ARG(((uintptr_t)seed_dev & 7) == 0, "seed_dev must be 8-byte aligned");
    if (B == 0 || n_out == 0) return 0;
    hipLaunchKernelGGL(gather_ragged_kernel, dim3(di2p_cdiv(n_out, 256), B), dim3(256), 0, (hipStream_t)stream, points, intensity, normals, offsets,
                       idx, transform, n_out, pc, intensity_out, sn, Jitter{seed, seed_dev, stream_id, sigma, clip, 0});
    DI2P_RETURN_LAUNCH();
}

extern "C" int di2p_gather_ragged_aug_intensity(const float* points, const float* intensity, const int32_t* offsets, const int32_t* idx,
                                                const double* transform, int B, int n_out, unsigned long long seed,
                                                const unsigned long long* seed_dev, int stream_id, double sigma, double clip, float* pc,
                                                float* intensity_out, void* stream) {
    DI2P_CHECK_ARG(B >= 0 && n_out >= 0, "bad sizes");
    DI2P_CHECK_ARG(B == 0 || n_out == 0 || (points && intensity && offsets && idx && pc && intensity_out), "null pointer");
    DI2P_CHECK_ARG(sigma >= 0.0 && sigma < 1e30 && clip > 0.0 && stream_id >= 0 && stream_id < (1 << 28), "jitter needs 0 <= sigma, clip > 0");
    DI2P_CHECK_ARG(((uintptr_t)seed_dev & 7) == 0, "seed_dev must be 8-byte aligned");
    if (B == 0 || n_out == 0) return 0;
    hipLaunchKernelGGL(gather_ragged_kernel, dim3(di2p_cdiv(n_out, 256), B), dim3(256), 0, (hipStream_t)stream, points, intensity,
                       (const float*)nullptr, offsets, idx, transform, n_out, pc, intensity_out, (float*)nullptr,
                       Jitter{seed, seed_dev, stream_id, sigma, clip, 1});
    DI2P_RETURN_LAUNCH();
}

extern "C" int di2p_range_shuffle(const float* points, const int32_t* offsets, int B, int cap, int max_frame_points, double max_range,
                                  unsigned long long seed, const unsigned long long* seed_dev, float* out_points, int32_t* out_offsets,
                                  int32_t* status, void* workspace, void* stream) {
    DI2P_CHECK_ARG(B >= 0 && cap >= 0, "bad sizes (B >= 0, cap >= 0)");
    DI2P_CHECK_ARG(max_frame_points >= 0 && max_frame_points <= MAX_FRAME_POINTS, "max_frame_points above 2^20 points per frame");
    DI2P_CHECK_ARG(max_range == max_range && max_range < 1e18, "max_range must be finite (<= 0: no range filter)");
    DI2P_CHECK_ARG(B == 0 || (points && offsets && out_points && out_offsets && workspace), "null pointer");
    DI2P_CHECK_ARG(((uintptr_t)workspace & 255) == 0 && ((uintptr_t)seed_dev & 7) == 0 && ((uintptr_t)points & 15) == 0 &&
                       ((uintptr_t)out_points & 15) == 0, "workspace must be 256-byte, points 16-byte, seed_dev 8-byte aligned");
    if (B == 0) return 0;
    const Layout L = layout(B, cap);
    hipStream_t st = (hipStream_t)stream;
    void* ws = workspace;
    const float r = (float)max_range;
    const float r2 = max_range > 0.0 ? r * r : 0.0f;
    const int n = cap > B + 1 ? cap : B + 1;
    hipLaunchKernelGGL(shuffle_keys_kernel, dim3(di2p_cdiv(n, 256)), dim3(256), 0, st, points, offsets, B, cap, max_frame_points, r2, seed, seed_dev,
                       at<unsigned>(ws, L.pfr), at<unsigned long long>(ws, L.key), at<int>(ws, L.iota), status);
    if (cap > 0) {
        const hipError_t e = sort_by_frame_key(ws, L, B, cap, at<unsigned long long>(ws, L.key), at<unsigned>(ws, L.pfr), at<int>(ws, L.i2),
                                               at<unsigned long long>(ws, L.k2), at<unsigned>(ws, L.f2), st);
        if (e != hipSuccess) { di2p_set_error("di2p_range_shuffle: sort failed: %s", hipGetErrorString(e)); return (int)e; }
    }
    hipLaunchKernelGGL(shuffle_compact_kernel, dim3(di2p_cdiv(n, 256)), dim3(256), 0, st, points, at<unsigned>(ws, L.f2), at<int>(ws, L.i2), B, cap,
                       out_points, out_offsets);
    DI2P_RETURN_LAUNCH();
}
