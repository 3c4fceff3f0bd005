// Surface normals of a resident map (gfx950): di2p_estimate_normals' definition on ONE cloud of up to 2^27 float32 rows, the row itself
// as the point.  Eager, once per map, as di2p_map_index_build.
//
//   bounds_partial_kernel / bounds_final_kernel   the map's own bounds, status 1 (a non-finite coordinate), status 2 (an edge above
//                                                 radius (2^21 - 4)); partial results per workgroup, no atomics
//   keys_kernel                                   cell = radius (1 + 2^-20) over the bounds, 21 bits per axis -> a 63-bit key per row
//   rocPRIM radix_sort_pairs                      stable sort of (key, row)
//   positions_kernel                              the rows' coordinates and row numbers in sorted order, 16 bytes each
//   map_normals_kernel                            one wave per query, MAP_WAVES queries per workgroup, persistent, queries in cell order
//
// The neighbours of row q are the at most max_nn rows j with d2 < r2 (q included), taken in ascending (d2, j), d2 fp64 on (double) of the
// float32 coordinates; duplicated rows are distinct neighbours.  The selection (nn_offer), the sort and the tail (normal_from_list) are
// scan_prep.hip's, from normals_nn.h: on the same points the two files give the same bits.  FMA contraction is off for this file (build.py).
//
// One wave per query, not one workgroup per cell (scan_prep.hip's normals_cells_kernel): a map's density is not bounded as a voxel-filtered
// frame's is, so a cell's 27-cell candidate set has no size the LDS could be dimensioned for; the per-query form streams the nine key ranges
// from the sorted 16-byte positions (coalesced, one load per candidate) whatever their length, and the waves of a workgroup take
// consecutive queries of the cell order, so they read the same ranges through the cache.
#include "common.h"
#include "normals_nn.h"
#include "ragged2.h"

#include <rocprim/device/device_radix_sort.hpp>

namespace {

constexpr int MAX_ROWS = 1 << 27;
constexpr int MAP_WAVES = 4;               // waves of a map_normals_kernel workgroup, each on a query of its own
constexpr int BOUNDS_BLOCKS = 1024;        // workgroups of bounds_partial_kernel at most
constexpr int ST_NONFINITE = 1, ST_EXTENT = 2;

struct NormalsLayout {
    size_t part, bad, minb, stat, key, iota, key2, idx2, spos, tmp, tmp_bytes, total;
};

NormalsLayout normals_layout(int M) {
    NormalsLayout L;
    Take take;
    const size_t n = (size_t)max(M, 1);
    L.part = take(4 * 6 * (size_t)BOUNDS_BLOCKS); L.bad = take(4 * (size_t)BOUNDS_BLOCKS); L.minb = take(8 * 3); L.stat = take(4);
    L.key = take(8 * n); L.iota = take(4 * n); L.key2 = take(8 * n); L.idx2 = take(4 * n); L.spos = take(16 * n);
    L.tmp_bytes = (size_t)24 * n + ((size_t)1 << 20);          // scan_prep.hip's bound for rocPRIM's radix sort; checked against its own answer
    L.tmp = take(L.tmp_bytes);
    L.total = take.o;
    return L;
}

int bounds_blocks(int M) { return min(di2p_cdiv(M, 256), BOUNDS_BLOCKS); }

// per workgroup: min and max of the three coordinates over its rows (grid-stride), and whether one of them is not finite
__global__ __launch_bounds__(256) void bounds_partial_kernel(const float* __restrict__ pts, int M, float* __restrict__ part, int* __restrict__ bad) {
    __shared__ float s[6][256];
    __shared__ int sb[256];
    const int tid = threadIdx.x;
    float mn[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()}, mx[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
    int nf = 0;
    for (long long i = (long long)blockIdx.x * 256 + tid; i < M; i += (long long)gridDim.x * 256) {
        const float4 p = *(const float4*)(pts + 4 * i);
        nf |= !(p.x - p.x == 0.0f) || !(p.y - p.y == 0.0f) || !(p.z - p.z == 0.0f);
        mn[0] = fminf(mn[0], p.x); mn[1] = fminf(mn[1], p.y); mn[2] = fminf(mn[2], p.z);
        mx[0] = fmaxf(mx[0], p.x); mx[1] = fmaxf(mx[1], p.y); mx[2] = fmaxf(mx[2], p.z);
    }
    for (int c = 0; c < 3; ++c) { s[c][tid] = mn[c]; s[3 + c][tid] = mx[c]; }
    sb[tid] = nf;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
            for (int c = 0; c < 3; ++c) { s[c][tid] = fminf(s[c][tid], s[c][tid + o]); s[3 + c][tid] = fmaxf(s[3 + c][tid], s[3 + c][tid + o]); }
            sb[tid] |= sb[tid + o];
        }
        __syncthreads();
    }
    if (tid < 6) part[6 * blockIdx.x + tid] = s[tid][0];
    if (tid == 0) bad[blockIdx.x] = sb[0];
}

// one workgroup: the bounds of the map from the partial ones, the status
__global__ __launch_bounds__(256) void bounds_final_kernel(const float* __restrict__ part, const int* __restrict__ bad, int nb, double radius,
                                                           double* __restrict__ minb, int* __restrict__ stat, int* __restrict__ status) {
    __shared__ float s[6][256];
    __shared__ int sb[256];
    const int tid = threadIdx.x;
    float mn[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()}, mx[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
    int nf = 0;
    for (int i = tid; i < nb; i += 256) {
        for (int c = 0; c < 3; ++c) { mn[c] = fminf(mn[c], part[6 * i + c]); mx[c] = fmaxf(mx[c], part[6 * i + 3 + c]); }
        nf |= bad[i];
    }
    for (int c = 0; c < 3; ++c) { s[c][tid] = mn[c]; s[3 + c][tid] = mx[c]; }
    sb[tid] = nf;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
            for (int c = 0; c < 3; ++c) { s[c][tid] = fminf(s[c][tid], s[c][tid + o]); s[3 + c][tid] = fmaxf(s[3 + c][tid], s[3 + c][tid + o]); }
            sb[tid] |= sb[tid + o];
        }
        __syncthreads();
    }
    if (tid == 0) {
        int st = sb[0] ? ST_NONFINITE : ST_OK;
        for (int c = 0; c < 3; ++c) {
            minb[c] = st == ST_OK ? (double)s[c][0] : 0.0;
            if (st == ST_OK && !((double)s[3 + c][0] - (double)s[c][0] <= radius * (double)(AXIS_MAX - 3))) st = ST_EXTENT;
        }
        *stat = st;
        *status = st;
    }
}

// key of every row and its row number; a map with a status gets the key 0 everywhere (the sort still leaves a permutation behind)
__global__ __launch_bounds__(256) void keys_kernel(const float* __restrict__ pts, int M, const double* __restrict__ minb, const int* __restrict__ stat,
                                                   double cell, unsigned long long* __restrict__ key, int* __restrict__ iota) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    iota[i] = i;
    if (*stat != ST_OK) { key[i] = 0; return; }
    const float4 p = *(const float4*)(pts + 4 * (long long)i);
    key[i] = compose_key(clamp_axis(floor(((double)p.x - minb[0]) / cell)), clamp_axis(floor(((double)p.y - minb[1]) / cell)),
                         clamp_axis(floor(((double)p.z - minb[2]) / cell)));
}

// sorted position j -> (x, y, z bits, row): what a candidate costs the search is this one 16-byte load
__global__ __launch_bounds__(256) void positions_kernel(const float* __restrict__ pts, const int* __restrict__ idx2, int M, int4* __restrict__ spos) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= M) return;
    const int row = min(max(idx2[j], 0), M - 1);
    const float4 p = *(const float4*)(pts + 4 * (long long)row);
    spos[j] = make_int4(__float_as_int(p.x), __float_as_int(p.y), __float_as_int(p.z), row);
}

// normal_from_list's positions (normals_nn.h): list entry i is map row i
struct RowPos {
    const float* __restrict__ pts;
    __device__ __forceinline__ void operator()(int i, double& x, double& y, double& z) const {
        const float4 p = *(const float4*)(pts + 4 * (long long)i);
        x = (double)p.x; y = (double)p.y; z = (double)p.z;
    }
};

// One wave per query, in cell order.  The 27 neighbour cells are 9 key ranges of 3 z-adjacent cells each, located by binary search in the
// sorted keys (lanes 0-8 the starts, 9-17 the ends) and streamed 64 candidates at a time through nn_offer.
__global__ __launch_bounds__(MAP_WAVES * 64) void map_normals_kernel(const float* __restrict__ pts, int M, const int4* __restrict__ spos,
                                                                     const unsigned long long* __restrict__ key2, const int* __restrict__ stat,
                                                                     double r2, int max_nn, int up_axis, int orient, float* __restrict__ normals,
                                                                     int* __restrict__ nn_count, int* __restrict__ nn_idx) {
    __shared__ unsigned long long sd_all[MAP_WAVES * CELL_NN_CAP];
    __shared__ int si_all[MAP_WAVES * CELL_NN_CAP];
    if (*stat != ST_OK) return;
    const int lane = threadIdx.x & 63, w = wave_id();
    unsigned long long* sd = sd_all + w * CELL_NN_CAP;
    int* si = si_all + w * CELL_NN_CAP;
    for (long long jq = (long long)blockIdx.x * MAP_WAVES + w; jq < M; jq += (long long)gridDim.x * MAP_WAVES) {
        const int4 q = spos[jq];
        const double qx = (double)__int_as_float(q.x), qy = (double)__int_as_float(q.y), qz = (double)__int_as_float(q.z);
        const unsigned long long key = key2[jq];
        int pos = 0;
        if (lane < 18) {
            const int r = lane % 9;
            const bool upper = lane >= 9;
            const long long kx = (long long)(key >> (2 * AXIS_BITS)) + r % 3 - 1;
            const long long ky = (long long)((key >> AXIS_BITS) & AXIS_MAX) + r / 3 - 1;
            const long long kz = (long long)(key & AXIS_MAX);
            if (kx >= 0 && ky >= 0 && kx <= AXIS_MAX && ky <= AXIS_MAX) {
                const unsigned long long k = upper ? compose_key(kx, ky, kz + 1 < AXIS_MAX ? kz + 1 : AXIS_MAX) : compose_key(kx, ky, kz > 0 ? kz - 1 : 0);
                int lo = 0, hi = M;
                while (lo < hi) {
                    const int mid = lo + ((hi - lo) >> 1);
                    if (upper ? key2[mid] <= k : key2[mid] < k) lo = mid + 1; else hi = mid;
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
                const bool in = j < e;
                int4 p = make_int4(0, 0, 0, 0);
                if (in) p = spos[j];
                const double d2 = in ? d2_of((double)__int_as_float(p.x), (double)__int_as_float(p.y), (double)__int_as_float(p.z), qx, qy, qz) : 0.0;
                nn_offer(in, d2, p.w, r2, max_nn, sd, si, cnt, thr_d, thr_i, lane);
            }
        }
        nn_sort<true>(sd, si, cnt, lane);
        normal_from_list(RowPos{pts}, si, cnt, max_nn, (long long)q.w, lane, up_axis, orient, normals, nn_count, nn_idx);
        nn_sync<true>();
    }
}

}  // namespace

extern "C" long long di2p_map_normals_workspace_bytes(int M) {
    if (M < 1 || M > MAX_ROWS) return 0;
    return (long long)normals_layout(M).total;
}

extern "C" int di2p_map_normals(const float* points, int M, int up_axis, int orient, double radius, int max_nn, float* normals, int32_t* nn_count,
                                int32_t* nn_idx, int32_t* status, void* workspace, void* stream) {
    DI2P_CHECK_ARG(M >= 1 && M <= MAX_ROWS, "bad size (1 <= M <= 2^27)");
    DI2P_CHECK_ARG(up_axis >= 0 && up_axis <= 2 && (orient == 1 || orient == -1), "up_axis must be 0, 1 or 2 and orient +1 or -1");
    DI2P_CHECK_ARG(radius > 0.0 && radius - radius == 0.0, "radius must be positive and finite");
    DI2P_CHECK_ARG(max_nn >= 1 && max_nn <= NN_MAX, "max_nn must be in [1, 64]");
    DI2P_CHECK_ARG(points && normals && status && workspace, "null pointer");
    DI2P_CHECK_ARG(((uintptr_t)workspace & 255) == 0 && ((uintptr_t)points & 15) == 0, "workspace must be 256-byte, points 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    hipError_t e = hipStreamIsCapturing(st, &cs);
    if (e != hipSuccess) { di2p_set_error("%s: hipStreamIsCapturing failed: %s", __func__, hipGetErrorString(e)); return (int)e; }
    DI2P_CHECK_ARG(cs == hipStreamCaptureStatusNone, "the stream is capturing: a map's normals are computed eagerly, once per map");
    const NormalsLayout L = normals_layout(M);
    void* ws = workspace;
    const double cell = radius * (1.0 + 1.0 / 1048576.0);
    const int nb = bounds_blocks(M);
    unsigned long long *key = at<unsigned long long>(ws, L.key), *key2 = at<unsigned long long>(ws, L.key2);
    int *iota = at<int>(ws, L.iota), *idx2 = at<int>(ws, L.idx2), *stat = at<int>(ws, L.stat);
    hipLaunchKernelGGL(bounds_partial_kernel, dim3(nb), dim3(256), 0, st, points, M, at<float>(ws, L.part), at<int>(ws, L.bad));
    hipLaunchKernelGGL(bounds_final_kernel, dim3(1), dim3(256), 0, st, at<float>(ws, L.part), at<int>(ws, L.bad), nb, radius, at<double>(ws, L.minb),
                       stat, status);
    hipLaunchKernelGGL(keys_kernel, dim3(di2p_cdiv(M, 256)), dim3(256), 0, st, points, M, at<double>(ws, L.minb), stat, cell, key, iota);
    size_t need = 0;
    e = rocprim::radix_sort_pairs(nullptr, need, key, key2, iota, idx2, (size_t)M, 0, 3 * AXIS_BITS, st);
    if (e == hipSuccess && need > L.tmp_bytes) e = hipErrorInvalidValue;
    if (e == hipSuccess) {
        need = L.tmp_bytes;
        e = rocprim::radix_sort_pairs(at<void>(ws, L.tmp), need, key, key2, iota, idx2, (size_t)M, 0, 3 * AXIS_BITS, st);
    }
    if (e != hipSuccess) { di2p_set_error("%s: sort failed: %s", __func__, hipGetErrorString(e)); return (int)e; }
    hipLaunchKernelGGL(positions_kernel, dim3(di2p_cdiv(M, 256)), dim3(256), 0, st, points, idx2, M, at<int4>(ws, L.spos));
    hipLaunchKernelGGL(map_normals_kernel, dim3(min(di2p_cdiv(M, MAP_WAVES), di2p_cu_count() * 8)), dim3(MAP_WAVES * 64), 0, st, points, M,
                       at<int4>(ws, L.spos), key2, stat, radius * radius, max_nn, up_axis, orient, normals, nn_count, nn_idx);
    DI2P_RETURN_LAUNCH();
}
