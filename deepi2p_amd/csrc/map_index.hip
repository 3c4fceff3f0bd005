// Map localisation on the device (gfx950): a uniform cell index over a resident LiDAR map, the crop of one disc per frame around a pose
// prior read from device memory, and the camera pose in the map from the prior and the solved pose.
//
//   di2p_map_index_build   once per map, eager: cell of every row -> stable radix sort (rocPRIM) -> cell_start, order, sorted
//   di2p_map_crop          per batch, graph-safe: frame -> window cells -> rows, the count / prefix / write split of submap.hip and sweeps.hip on
//                          ragged2.h (wave_prefix, offsets_kernel, the status codes, the workspace helpers)
//   di2p_map_crop_normals  per batch, graph-safe, behind the crop: the map's normals (map_normals.hip, or the user's own) of the kept rows,
//                          rotated into the prior frame; a second launch, so di2p_map_crop and its outputs are what they were
//   di2p_map_pose          T_map_cam = T_map_prior . P_scan^-1
//
// The map is f32[M,4] rows (x, y, z, intensity) in a map frame whose coordinates are small enough for float32 (relative to a map origin the
// caller keeps).  up_axis names the vertical axis; the ground axes (a, b) are the other two in ascending order.  Cell of a row:
// ix = floor(((double)p[a] - origin[0]) / cell), iy likewise on b, id = iy * nx + ix.  `sorted` holds the rows cell after cell in ascending id,
// inside a cell in ascending map row (a stable sort), so the cells of one window row (iy fixed, ix0 .. ix1) are ONE contiguous span of it.
// Stages of the crop:
//   window_kernel   one thread per frame: the prior and the radius checked, the clamped window ix0 .. ix1, iy0 .. iy1
//   count_kernel    one wave per (frame, window cell): rows with dx dx + dy dy < r r (ballot + popcount)
//   prefix_kernel   one wave per frame: exclusive prefix of the counts over the frame's window cells, iy-major (ragged2.h's wave_prefix)
//   offsets_kernel  (ragged2.h) one wave: exclusive prefix over the frames, status
//   write_kernel    one wave per (frame, window cell): one 16-byte load and one 16-byte store per row, ordered compaction with the ballot prefix
// Every count and offset the crop reads is written by a kernel of the same call: no memset node, no atomics.  Every value that decides a bit
// is fp64, each operation rounded once: FMA contraction is off for this file (build.py), so tests/map_index_oracle.py restates it in numpy
// value for value.
#include "common.h"
#include "ragged2.h"

#include <rocprim/device/device_radix_sort.hpp>

namespace {

constexpr int MAX_ROWS = 1 << 27;            // rows of a map
constexpr int MAX_CELLS = 1 << 24;           // cells of a grid
constexpr int MAX_CHUNKS = 1 << 28;          // (frame, window cell) pairs of one crop: B * max_cells
constexpr int ST_PRIOR = 5;                  // a non-finite prior, or a radius that is not finite and positive
constexpr int WAVES = 4;                     // waves of a count / write workgroup: one (frame, window cell) each

struct Grid {
    double o0, o1, cell;
    int nx, ny, a, b;                        // a, b: the ground axes
};

Grid make_grid(int up_axis, double o0, double o1, double cell, int nx, int ny) {
    return {o0, o1, cell, nx, ny, up_axis == 0 ? 1 : 0, up_axis == 2 ? 1 : 2};
}

bool grid_ok(int up_axis, double o0, double o1, double cell, int nx, int ny) {
    return up_axis >= 0 && up_axis <= 2 && o0 - o0 == 0.0 && o1 - o1 == 0.0 && cell > 0.0 && cell - cell == 0.0 && nx >= 1 && ny >= 1 &&
           (long long)nx * ny <= MAX_CELLS;
}

// The kernels that read rows are instantiated per up axis, so a row's ground coordinates are named at compile time.  (With the axis as a
// run-time argument hipcc narrowed the 16-byte row load of count_kernel to two dword loads behind a chain of address selects and took the
// first ground coordinate for both: the count of a frame then differed from the rows written.)
template <int K> __device__ __forceinline__ float axis(const float4& v) { return K == 0 ? v.x : K == 1 ? v.y : v.z; }
template <int UP> struct Ground { static constexpr int A = UP == 0 ? 1 : 0, B = UP == 2 ? 1 : 2; };
__device__ __forceinline__ bool finite(double x) { return x - x == 0.0; }

// ---------------------------------------------------------------------------------------------------------------- build
struct BuildLayout {
    size_t key, key_sorted, iota, tmp, tmp_bytes, total;
};

BuildLayout build_layout(int M) {
    BuildLayout L;
    Take take;
    const size_t n = (size_t)max(M, 1);
    L.key = take(4 * n); L.key_sorted = take(4 * n); L.iota = take(4 * n);
    L.tmp_bytes = (size_t)24 * n + ((size_t)1 << 20);          // scan_prep.hip's bound for rocPRIM's radix sort; checked against its own answer
    L.tmp = take(L.tmp_bytes);
    L.total = take.o;
    return L;
}

int key_bits(int ncell) { int bits = 1; while ((1ll << bits) <= ncell) ++bits; return bits; }          // the keys are 0 .. ncell

__global__ __launch_bounds__(64) void build_init_kernel(int* __restrict__ status) {
    if (threadIdx.x == 0) status[0] = 0;
}

// key = the row's cell, or ncell for a row with a non-finite coordinate or outside the grid (status 1; every such thread stores the same value)
template <int UP>
__global__ __launch_bounds__(256) void key_kernel(const float* __restrict__ pts, int M, Grid g, unsigned* __restrict__ key, int* __restrict__ iota,
                                                  int* __restrict__ status) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    const float4 v = *(const float4*)(pts + 4 * (long long)i);
    const double fx = floor(((double)axis<Ground<UP>::A>(v) - g.o0) / g.cell), fy = floor(((double)axis<Ground<UP>::B>(v) - g.o1) / g.cell);
    const bool ok = finite((double)v.x) && finite((double)v.y) && finite((double)v.z) && fx >= 0.0 && fx <= (double)(g.nx - 1) && fy >= 0.0 &&
                    fy <= (double)(g.ny - 1);
    key[i] = ok ? (unsigned)((int)fy * g.nx + (int)fx) : (unsigned)(g.nx * g.ny);
    iota[i] = i;
    if (!ok) status[0] = 1;
}

// cell_start[c] = the first stored row whose key is >= c, c in [0, ncell]
__global__ __launch_bounds__(256) void cell_start_kernel(const unsigned* __restrict__ key_sorted, int M, int ncell, int* __restrict__ cell_start) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c > ncell) return;
    int lo = 0, hi = M;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (key_sorted[mid] < (unsigned)c) lo = mid + 1; else hi = mid;
    }
    cell_start[c] = lo;
}

__global__ __launch_bounds__(256) void gather_rows_kernel(const float* __restrict__ pts, const int* __restrict__ order, int M, float* __restrict__ sorted) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    const int r = min(max(order[i], 0), M - 1);
    *(float4*)(sorted + 4 * (long long)i) = *(const float4*)(pts + 4 * (long long)r);
}

// ---------------------------------------------------------------------------------------------------------------- crop
struct CropLayout {
    size_t win, cnt, off, frame_total, frame_stat, total;
};

CropLayout crop_layout(int B, int max_cells) {
    CropLayout L;
    Take take;
    const size_t chunks = (size_t)max(B, 1) * (size_t)max(max_cells, 1);
    L.win = take(16 * (size_t)max(B, 1));
    L.cnt = take(4 * chunks); L.off = take(4 * chunks);
    L.frame_total = take(4 * (size_t)max(B, 1)); L.frame_stat = take(4 * (size_t)max(B, 1));
    L.total = take.o;
    return L;
}

// the cells floor((c -/+ r - origin) / cell) of one axis, clamped to [0, n - 1]; i0 > i1 for a range that misses the grid
__device__ __forceinline__ void axis_window(double c, double r, double origin, double cell, int n, int& i0, int& i1) {
    const double f0 = floor(((c - r) - origin) / cell), f1 = floor(((c + r) - origin) / cell);
    if (!(f0 <= (double)(n - 1)) || !(f1 >= 0.0)) { i0 = 1; i1 = 0; return; }
    i0 = f0 < 0.0 ? 0 : (int)f0;
    i1 = f1 > (double)(n - 1) ? n - 1 : (int)f1;
}

// win[b] = (ix0, iy0, cells per window row, window cells); no cells for a frame with a status, or whose disc misses the grid
__global__ __launch_bounds__(64) void window_kernel(const double* __restrict__ T, const double* __restrict__ radius, int B, Grid g, int max_cells,
                                                    int4* __restrict__ win, int* __restrict__ frame_stat) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const double* P = T + 16 * (long long)b;
    bool ok = true;
    for (int k = 0; k < 16; ++k) ok &= finite(P[k]);
    const double r = radius[b];
    ok &= finite(r) && r > 0.0;
    int st = ok ? ST_OK : ST_PRIOR;
    int4 w = make_int4(0, 0, 0, 0);
    if (ok) {
        int ix0, ix1, iy0, iy1;
        axis_window(P[4 * g.a + 3], r, g.o0, g.cell, g.nx, ix0, ix1);
        axis_window(P[4 * g.b + 3], r, g.o1, g.cell, g.ny, iy0, iy1);
        if (ix0 <= ix1 && iy0 <= iy1) {
            const long long n = (long long)(ix1 - ix0 + 1) * (iy1 - iy0 + 1);
            if (n > max_cells) st = ST_TOO_MANY;
            else w = make_int4(ix0, iy0, ix1 - ix0 + 1, (int)n);
        }
    }
    win[b] = w;
    frame_stat[b] = st;
}

// what a wave of the count / write kernels works on: window cell j of frame b, its rows [r0, r1) of `sorted`, the disc
struct Chunk {
    int b, r0, r1;
    double c0, c1, rr;
    bool any;
};

__device__ __forceinline__ Chunk chunk_of(long long chunk, int B, int max_cells, const int4* __restrict__ win, const int* __restrict__ cell_start,
                                          const double* __restrict__ T, const double* __restrict__ radius, const Grid& g, int M) {
    Chunk c;
    c.b = (int)(chunk / max_cells);
    c.any = false;
    if (c.b >= B) return c;
    const int j = (int)(chunk % max_cells);
    const int4 w = win[c.b];
    if (j >= w.w) return c;
    const int cellid = (w.y + j / w.z) * g.nx + w.x + j % w.z;          // iy-major
    c.r0 = min(max(cell_start[cellid], 0), M);
    c.r1 = min(max(cell_start[cellid + 1], c.r0), M);
    const double r = radius[c.b];
    c.c0 = T[16 * (long long)c.b + 4 * g.a + 3];
    c.c1 = T[16 * (long long)c.b + 4 * g.b + 3];
    c.rr = r * r;
    c.any = true;
    return c;
}

template <int UP>
__device__ __forceinline__ bool inside_disc(const float4& v, const Chunk& c) {
    const double dx = (double)axis<Ground<UP>::A>(v) - c.c0, dy = (double)axis<Ground<UP>::B>(v) - c.c1;
    return dx * dx + dy * dy < c.rr;
}

template <int UP>
__global__ __launch_bounds__(64 * WAVES) void count_kernel(const float* __restrict__ sorted, const int* __restrict__ cell_start, int M,
                                                           const double* __restrict__ T, const double* __restrict__ radius, int B, Grid g,
                                                           int max_cells, const int4* __restrict__ win, int* __restrict__ cnt) {
    const long long chunk = (long long)blockIdx.x * WAVES + wave_id();
    const int lane = threadIdx.x & 63;
    const Chunk c = chunk_of(chunk, B, max_cells, win, cell_start, T, radius, g, M);
    if (!c.any) return;          // never read: the prefix stops at the frame's window cells
    int n = 0;
    for (int r = c.r0; r < c.r1; r += 64) {
        const int row = r + lane;
        bool keep = false;
        if (row < c.r1) {
            const float4 v = *(const float4*)(sorted + 4 * (long long)row);
            keep = inside_disc<UP>(v, c);
        }
        n += __popcll(__ballot(keep));
    }
    if (lane == 0) cnt[chunk] = n;
}

__global__ __launch_bounds__(64) void prefix_kernel(int max_cells, const int4* __restrict__ win, const int* __restrict__ frame_stat,
                                                    const int* __restrict__ cnt, int* __restrict__ off, int* __restrict__ frame_total) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const long long j0 = (long long)b * max_cells;
    const int total = frame_stat[b] == ST_OK ? wave_prefix(cnt, j0, j0 + win[b].w, lane, off) : 0;
    if (lane == 0) frame_total[b] = total;
}

// A kept row in the prior frame: q = R^T (p - t), every d_k = (double)p[k] - T[k][3], the three products summed left to right, rounded once to
// float32; the intensity bit for bit.
template <int UP>
__global__ __launch_bounds__(64 * WAVES) void write_kernel(const float* __restrict__ sorted, const int* __restrict__ cell_start,
                                                           const int* __restrict__ order, int M, const double* __restrict__ T,
                                                           const double* __restrict__ radius, int B, Grid g, int max_cells,
                                                           const int4* __restrict__ win, const int* __restrict__ off,
                                                           const int* __restrict__ frame_stat, const int* __restrict__ out_off, int cap,
                                                           float* __restrict__ out, int* __restrict__ out_index) {
    const long long chunk = (long long)blockIdx.x * WAVES + wave_id();
    const int lane = threadIdx.x & 63;
    const Chunk c = chunk_of(chunk, B, max_cells, win, cell_start, T, radius, g, M);
    if (!c.any || frame_stat[c.b] != ST_OK) return;
    double P[12];
    for (int k = 0; k < 12; ++k) P[k] = T[16 * (long long)c.b + k];
    long long dst = (long long)out_off[c.b] + off[chunk];
    const long long end = out_off[c.b + 1];          // <= cap; what count_kernel counted ends here
    for (int r = c.r0; r < c.r1; r += 64) {
        const int row = r + lane;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        bool keep = false;
        if (row < c.r1) {
            v = *(const float4*)(sorted + 4 * (long long)row);
            keep = inside_disc<UP>(v, c);
        }
        const unsigned long long mask = __ballot(keep);
        const long long at_row = dst + __popcll(mask & ((1ull << lane) - 1ull));
        if (keep && at_row < end && at_row < cap) {
            const double d0 = (double)v.x - P[3], d1 = (double)v.y - P[7], d2 = (double)v.z - P[11];
            float4 o;
            o.x = (float)((P[0] * d0 + P[4] * d1) + P[8] * d2);
            o.y = (float)((P[1] * d0 + P[5] * d1) + P[9] * d2);
            o.z = (float)((P[2] * d0 + P[6] * d1) + P[10] * d2);
            o.w = v.w;
            *(float4*)(out + 4 * at_row) = o;
            if (out_index) out_index[at_row] = order[row];
        }
        dst += __popcll(mask);
    }
}

// The normals of the kept rows in the prior frame: R^T n, write_kernel's row formula without the translation.  One thread per kept row; the
// frame of a row by binary search in the offsets the crop left, so the launch reads everything that varies from device memory.
__global__ __launch_bounds__(256) void crop_normals_kernel(const float* __restrict__ normals, const int* __restrict__ index,
                                                           const int* __restrict__ offsets, const double* __restrict__ T, int B, int cap,
                                                           float* __restrict__ out) {
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k >= min(offsets[B], cap)) return;
    const int b = frame_of(offsets, B, k);
    const double* P = T + 16 * (long long)b;
    const long long row = max(index[k], 0);
    const double n0 = (double)normals[3 * row + 0], n1 = (double)normals[3 * row + 1], n2 = (double)normals[3 * row + 2];
    out[3 * k + 0] = (float)((P[0] * n0 + P[4] * n1) + P[8] * n2);
    out[3 * k + 1] = (float)((P[1] * n0 + P[5] * n1) + P[9] * n2);
    out[3 * k + 2] = (float)((P[2] * n0 + P[6] * n1) + P[10] * n2);
}

// ---------------------------------------------------------------------------------------------------------------- pose
// out = A . inv(Pm) with the rigid inverse [R^T | -R^T t] of Pm (its last row is not read); the product as di2p_compose_poses writes it
__global__ __launch_bounds__(64) void map_pose_kernel(const double* A, const double* Pm, double* out, int n) {          // no __restrict__: out may be A or Pm
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= n) return;
    const double* a = A + 16 * (long long)b;
    const double* p = Pm + 16 * (long long)b;
    double m[16], r[16];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) m[4 * i + j] = p[4 * j + i];
        m[4 * i + 3] = -((p[i] * p[3] + p[4 + i] * p[7]) + p[8 + i] * p[11]);
    }
    m[12] = 0.0; m[13] = 0.0; m[14] = 0.0; m[15] = 1.0;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double acc = a[4 * i] * m[j];
            for (int k = 1; k < 4; ++k) acc = acc + a[4 * i + k] * m[4 * k + j];
            r[4 * i + j] = acc;
        }
    for (int i = 0; i < 16; ++i) out[16 * (long long)b + i] = r[i];
}

// the five launches of di2p_map_crop for one up axis
template <int UP>
void launch_crop(const float* sorted, const int* cell_start, const int* order, int M, const Grid& g, const double* T, const double* radius, int B,
                 int cap, int max_frame_points, int max_cells, float* rows, int* offsets, int* index, int* status, void* ws, hipStream_t st) {
    const CropLayout L = crop_layout(B, max_cells);
    int4* win = at<int4>(ws, L.win);
    int *cnt = at<int>(ws, L.cnt), *off = at<int>(ws, L.off), *frame_total = at<int>(ws, L.frame_total), *frame_stat = at<int>(ws, L.frame_stat);
    const int blocks = di2p_cdiv((long long)B * max_cells, WAVES);
    hipLaunchKernelGGL(window_kernel, dim3(di2p_cdiv(B, 64)), dim3(64), 0, st, T, radius, B, g, max_cells, win, frame_stat);
    hipLaunchKernelGGL(count_kernel<UP>, dim3(blocks), dim3(64 * WAVES), 0, st, sorted, cell_start, M, T, radius, B, g, max_cells, win, cnt);
    hipLaunchKernelGGL(prefix_kernel, dim3(B), dim3(64), 0, st, max_cells, win, frame_stat, cnt, off, frame_total);
    hipLaunchKernelGGL(offsets_kernel, dim3(1), dim3(64), 0, st, B, cap, max_frame_points, frame_total, frame_stat, offsets, status);
    hipLaunchKernelGGL(write_kernel<UP>, dim3(blocks), dim3(64 * WAVES), 0, st, sorted, cell_start, order, M, T, radius, B, g, max_cells, win, off,
                       frame_stat, offsets, cap, rows, index);
}

}  // namespace

extern "C" long long di2p_map_index_workspace_bytes(int M, int ncell) {
    if (M < 0 || M > MAX_ROWS || ncell < 1 || ncell > MAX_CELLS) return 0;
    return (long long)build_layout(M).total;
}

extern "C" long long di2p_map_crop_workspace_bytes(int B, int max_cells) {
    if (B < 0 || max_cells < 1 || (long long)B * max_cells > MAX_CHUNKS) return 0;
    return (long long)crop_layout(B, max_cells).total;
}

extern "C" int di2p_map_index_build(const float* points, int M, int up_axis, double origin0, double origin1, double cell, int nx, int ny,
                                    int32_t* cell_start, int32_t* order, float* sorted, int32_t* status, void* workspace, void* stream) {
    DI2P_CHECK_ARG(M >= 0 && M <= MAX_ROWS, "bad size (0 <= M <= 2^27)");
    DI2P_CHECK_ARG(grid_ok(up_axis, origin0, origin1, cell, nx, ny), "bad grid (up_axis in {0, 1, 2}, a finite origin, cell > 0, nx ny <= 2^24)");
    DI2P_CHECK_ARG(cell_start && status && workspace && (M == 0 || (points && order && sorted)), "null pointer");
    DI2P_CHECK_ARG(((uintptr_t)workspace & 255) == 0 && ((uintptr_t)points & 15) == 0 && ((uintptr_t)sorted & 15) == 0,
                   "workspace must be 256-byte, points and sorted 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    hipError_t e = hipStreamIsCapturing(st, &cs);
    if (e != hipSuccess) { di2p_set_error("%s: hipStreamIsCapturing failed: %s", __func__, hipGetErrorString(e)); return (int)e; }
    DI2P_CHECK_ARG(cs == hipStreamCaptureStatusNone, "the stream is capturing: the index is built eagerly, once per map");
    const Grid g = make_grid(up_axis, origin0, origin1, cell, nx, ny);
    const int ncell = nx * ny;
    const BuildLayout L = build_layout(M);
    unsigned *key = at<unsigned>(workspace, L.key), *key_sorted = at<unsigned>(workspace, L.key_sorted);
    int* iota = at<int>(workspace, L.iota);
    hipLaunchKernelGGL(build_init_kernel, dim3(1), dim3(64), 0, st, status);
    if (M > 0) {
        const dim3 grid(di2p_cdiv(M, 256));
        if (up_axis == 0) hipLaunchKernelGGL(key_kernel<0>, grid, dim3(256), 0, st, points, M, g, key, iota, status);
        else if (up_axis == 1) hipLaunchKernelGGL(key_kernel<1>, grid, dim3(256), 0, st, points, M, g, key, iota, status);
        else hipLaunchKernelGGL(key_kernel<2>, grid, dim3(256), 0, st, points, M, g, key, iota, status);
        size_t need = 0;
        e = rocprim::radix_sort_pairs(nullptr, need, key, key_sorted, iota, order, (size_t)M, 0, key_bits(ncell), st);
        if (e == hipSuccess && need > L.tmp_bytes) e = hipErrorInvalidValue;
        if (e == hipSuccess) {
            need = L.tmp_bytes;
            e = rocprim::radix_sort_pairs(at<void>(workspace, L.tmp), need, key, key_sorted, iota, order, (size_t)M, 0, key_bits(ncell), st);
        }
        if (e != hipSuccess) { di2p_set_error("%s: sort failed: %s", __func__, hipGetErrorString(e)); return (int)e; }
        hipLaunchKernelGGL(gather_rows_kernel, dim3(di2p_cdiv(M, 256)), dim3(256), 0, st, points, order, M, sorted);
    }
    hipLaunchKernelGGL(cell_start_kernel, dim3(di2p_cdiv(ncell + 1, 256)), dim3(256), 0, st, key_sorted, M, ncell, cell_start);
    DI2P_RETURN_LAUNCH();
}

extern "C" int di2p_map_crop(const float* sorted, const int32_t* cell_start, const int32_t* order, int M, int up_axis, double origin0,
                             double origin1, double cell, int nx, int ny, const double* T_map_prior, const double* radius, int B, int cap,
                             int max_frame_points, int max_cells, float* rows, int32_t* offsets, int32_t* index, int32_t* status,
                             void* workspace, void* stream) {
    DI2P_CHECK_ARG(M >= 0 && M <= MAX_ROWS && B >= 0 && cap >= 0, "bad sizes (0 <= M <= 2^27, B, cap >= 0)");
    DI2P_CHECK_ARG(grid_ok(up_axis, origin0, origin1, cell, nx, ny), "bad grid (up_axis in {0, 1, 2}, a finite origin, cell > 0, nx ny <= 2^24)");
    DI2P_CHECK_ARG(max_frame_points >= 0 && max_frame_points <= MAX_FRAME_POINTS, "max_frame_points above 2^20 rows per frame");
    DI2P_CHECK_ARG(max_cells >= 1 && (long long)B * max_cells <= MAX_CHUNKS, "bad max_cells (>= 1, B max_cells <= 2^28)");
    DI2P_CHECK_ARG(B == 0 || (cell_start && T_map_prior && radius && rows && offsets && workspace), "null pointer");
    DI2P_CHECK_ARG(B == 0 || M == 0 || (sorted && (!index || order)), "null pointer (sorted, order)");
    DI2P_CHECK_ARG(((uintptr_t)workspace & 255) == 0 && ((uintptr_t)rows & 15) == 0 && ((uintptr_t)sorted & 15) == 0 &&
                       (((uintptr_t)T_map_prior | (uintptr_t)radius) & 7) == 0,
                   "workspace must be 256-byte, rows and sorted 16-byte, T_map_prior and radius 8-byte aligned");
    if (B == 0) return 0;
    const Grid g = make_grid(up_axis, origin0, origin1, cell, nx, ny);
    hipStream_t st = (hipStream_t)stream;
    if (up_axis == 0) launch_crop<0>(sorted, cell_start, order, M, g, T_map_prior, radius, B, cap, max_frame_points, max_cells, rows, offsets, index, status, workspace, st);
    else if (up_axis == 1) launch_crop<1>(sorted, cell_start, order, M, g, T_map_prior, radius, B, cap, max_frame_points, max_cells, rows, offsets, index, status, workspace, st);
    else launch_crop<2>(sorted, cell_start, order, M, g, T_map_prior, radius, B, cap, max_frame_points, max_cells, rows, offsets, index, status, workspace, st);
    DI2P_RETURN_LAUNCH();
}

extern "C" int di2p_map_crop_normals(const float* normals, const int32_t* index, const int32_t* offsets, const double* T_map_prior, int B, int cap,
                                     float* out, void* stream) {
    DI2P_CHECK_ARG(B >= 0 && cap >= 0, "bad sizes (B, cap >= 0)");
    DI2P_CHECK_ARG(B == 0 || cap == 0 || (normals && index && offsets && T_map_prior && out), "null pointer");
    DI2P_CHECK_ARG(((uintptr_t)T_map_prior & 7) == 0, "T_map_prior must be 8-byte aligned");
    if (B == 0 || cap == 0) return 0;
    hipLaunchKernelGGL(crop_normals_kernel, dim3(di2p_cdiv(cap, 256)), dim3(256), 0, (hipStream_t)stream, normals, index, offsets, T_map_prior, B, cap,
                       out);
    DI2P_RETURN_LAUNCH();
}

extern "C" int di2p_map_pose(const double* T_map_prior, const double* P_scan, int n, double* T_map_cam, void* stream) {
    DI2P_CHECK_ARG(n >= 0, "bad size");
    DI2P_CHECK_ARG(n == 0 || (T_map_prior && P_scan && T_map_cam), "null pointer");
    DI2P_CHECK_ARG((((uintptr_t)T_map_prior | (uintptr_t)P_scan | (uintptr_t)T_map_cam) & 7) == 0, "the matrices must be 8-byte aligned");
    if (n == 0) return 0;
    hipLaunchKernelGGL(map_pose_kernel, dim3(di2p_cdiv(n, 64)), dim3(64), 0, (hipStream_t)stream, T_map_prior, P_scan, T_map_cam, n);
    DI2P_RETURN_LAUNCH();
}
