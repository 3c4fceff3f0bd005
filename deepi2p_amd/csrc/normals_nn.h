// Radius-bounded k-nearest selection and the PCA normal of the selected set: what the normals kernels of scan_prep.hip (per frame, on the
// voxel pass's fp64 centroids) and map_normals.hip (one map-sized cloud of float32 rows) have in common.  Included by those two files;
// everything is in the anonymous namespace.  Both files are built with FMA contraction off (build.py): every product and sum below rounds once.
//   compose_key / clamp_axis   21 bits per axis into a 63-bit cell key
//   d2_of                      ((dx dx + dy dy) + dz dz) in fp64
//   nn_less / nn_sort          the (d2 bits, index) order and the bitonic sort of one wave's LDS candidate list
//   nn_offer                   one candidate per lane into a wave's list, cut back to the best max_nn whenever it fills: exact selection
//   normal_from_list           sorted list -> neighbour outputs, butterfly sums, cyclic Jacobi, the orientation rule, the stored normal
#pragma once
#include "common.h"

namespace {

constexpr int AXIS_BITS = 21;
constexpr int AXIS_MAX = (1 << AXIS_BITS) - 1;
constexpr int NN_MAX = 64;
constexpr int CELL_NN_CAP = 256;       // LDS candidate list of one wave that selects with nn_offer (entries)

__device__ __forceinline__ unsigned long long compose_key(long long ix, long long iy, long long iz) {
    return ((unsigned long long)ix << (2 * AXIS_BITS)) | ((unsigned long long)iy << AXIS_BITS) | (unsigned long long)iz;
}

__device__ __forceinline__ long long clamp_axis(double f) {
    return f < 0.0 ? 0 : (f > (double)AXIS_MAX ? AXIS_MAX : (long long)f);
}

__device__ __forceinline__ double d2_of(double ax, double ay, double az, double bx, double by, double bz) {
    const double dx = ax - bx, dy = ay - by, dz = az - bz;
    return __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
}

__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = __dadd_rn(x, __shfl_xor(x, o, 64));
    return x;
}

// (d2 bits, index) lexicographic order; d2 >= 0 so the bit pattern orders like the value
__device__ __forceinline__ bool nn_less(unsigned long long da, int ia, unsigned long long db, int ib) {
    return da < db || (da == db && ia < ib);
}

// Barrier between the LDS accesses of the lanes that share a candidate list: the workgroup's when it is one wave (normals_kernel), else
// a wave-level one (normals_cells_kernel, map_normals_kernel: the waves of a workgroup work on different queries and never meet inside
// one).  A wave's LDS instructions execute in order; the fences keep the compiler from moving or merging accesses across the point.
template <bool kWave> __device__ __forceinline__ void nn_sync() {
    if (kWave) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    } else {
        __syncthreads();
    }
}

// bitonic sort of n2 (power of two >= cnt) entries of the LDS list, padding [cnt, n2) with +inf first; one wave
template <bool kWave> __device__ void nn_sort(unsigned long long* sd, int* si, int cnt, int lane) {
    int n2 = 64;
    while (n2 < cnt) n2 <<= 1;
    for (int i = cnt + lane; i < n2; i += 64) { sd[i] = ~0ull; si[i] = 0x7fffffff; }
    nn_sync<kWave>();
    for (int k = 2; k <= n2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = lane; t < n2 / 2; t += 64) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const int l = i + j;
                const bool up = (i & k) == 0;
                const unsigned long long a = sd[i], c = sd[l];
                const int ia = si[i], ic = si[l];
                if (nn_less(c, ic, a, ia) == up) { sd[i] = c; sd[l] = a; si[i] = ic; si[l] = ia; }
            }
            nn_sync<kWave>();
        }
    }
}

// One candidate of one wave's query: accepted when it lies inside the ball and beats the current max_nn-th best (d2, index); the wave's own
// LDS list (CELL_NN_CAP entries) is sorted and cut back to max_nn whenever it fills, so it never spills and the selection is exact.
__device__ __forceinline__ void nn_offer(bool in, double d2, int li, double r2, int max_nn, unsigned long long* sd, int* si, int& cnt,
                                         unsigned long long& thr_d, int& thr_i, int lane) {
    const unsigned long long db = (unsigned long long)__double_as_longlong(d2);
    const bool acc = in && d2 < r2 && nn_less(db, li, thr_d, thr_i);
    const unsigned long long m = __ballot(acc);
    if (acc) {
        const int pos = cnt + __popcll(m & ((1ull << lane) - 1));
        sd[pos] = db; si[pos] = li;
    }
    cnt += __popcll(m);
    if (cnt > CELL_NN_CAP - 64) {       // (> max_nn: always cut back)
        nn_sort<true>(sd, si, cnt, lane);
        if (cnt >= max_nn) { thr_d = sd[max_nn - 1]; thr_i = si[max_nn - 1]; cnt = max_nn; }
        nn_sync<true>();
    }
}

// eigenvector of the smallest eigenvalue of a symmetric 3x3 matrix (cyclic Jacobi, fp64, registers only)
__device__ void smallest_eigvec(double a00, double a01, double a02, double a11, double a12, double a22, double& nx, double& ny, double& nz) {
    double A[3][3] = {{a00, a01, a02}, {a01, a11, a12}, {a02, a12, a22}};
    double V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    for (int sweep = 0; sweep < 24; ++sweep) {
        if (A[0][1] == 0.0 && A[0][2] == 0.0 && A[1][2] == 0.0) break;
#pragma unroll
        for (int pq = 0; pq < 3; ++pq) {
            const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
            if (A[p][q] != 0.0) {
                const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
                for (int r = 0; r < 3; ++r) {          // A <- A J
                    const double arp = A[r][p], arq = A[r][q];
                    A[r][p] = c * arp - s * arq;
                    A[r][q] = s * arp + c * arq;
                }
#pragma unroll
                for (int r = 0; r < 3; ++r) {          // A <- J^T A
                    const double apr = A[p][r], aqr = A[q][r];
                    A[p][r] = c * apr - s * aqr;
                    A[q][r] = s * apr + c * aqr;
                }
                A[p][q] = 0.0; A[q][p] = 0.0;
#pragma unroll
                for (int r = 0; r < 3; ++r) {          // V <- V J
                    const double vrp = V[r][p], vrq = V[r][q];
                    V[r][p] = c * vrp - s * vrq;
                    V[r][q] = s * vrp + c * vrq;
                }
            }
        }
    }
    int m = 0;
    if (A[1][1] < A[m][m]) m = 1;
    if (A[2][2] < (m == 0 ? A[0][0] : A[1][1])) m = 2;
    nx = m == 0 ? V[0][0] : m == 1 ? V[0][1] : V[0][2];
    ny = m == 0 ? V[1][0] : m == 1 ? V[1][1] : V[1][2];
    nz = m == 0 ? V[2][0] : m == 1 ? V[2][1] : V[2][2];
}

// From the sorted candidate list of query v to its stored normal (one wave; rank t in lane t): the neighbour outputs, the mean and the
// six covariance sums by the wave_sum butterfly, the eigenvector, the orientation rule.  Shared by all normals kernels.  pos(i, x, y, z)
// gives the fp64 position of list entry i.  Orientation (Open3D's orient_normals_to_align_with_direction with direction orient . e_up):
// a zero normal becomes the direction, orient . n[up_axis] < 0 flips.
template <class Pos>
__device__ __forceinline__ void normal_from_list(const Pos& pos, const int* si, int cnt, int max_nn, long long v, int lane, int up_axis, int orient,
                                                 float* __restrict__ normals, int* __restrict__ nn_count, int* __restrict__ nn_idx) {
    const int k = cnt < max_nn ? cnt : max_nn;
    if (nn_idx)
        for (int t = lane; t < max_nn; t += 64) nn_idx[v * max_nn + t] = t < k ? si[t] : -1;
    if (nn_count && lane == 0) nn_count[v] = k;
    double px = 0.0, py = 0.0, pz = 0.0;
    if (lane < k) pos(si[lane], px, py, pz);
    const double dk = (double)k;
    const double mx = wave_sum(px) / dk, my = wave_sum(py) / dk, mz = wave_sum(pz) / dk;
    const double ex = lane < k ? px - mx : 0.0, ey = lane < k ? py - my : 0.0, ez = lane < k ? pz - mz : 0.0;
    const double cxx = wave_sum(ex * ex), cxy = wave_sum(ex * ey), cxz = wave_sum(ex * ez);
    const double cyy = wave_sum(ey * ey), cyz = wave_sum(ey * ez), czz = wave_sum(ez * ez);
    double nx = 0.0, ny = 0.0, nz = 0.0;
    if (k >= 3 && (cxx != 0.0 || cxy != 0.0 || cxz != 0.0 || cyy != 0.0 || cyz != 0.0 || czz != 0.0))
        smallest_eigvec(cxx, cxy, cxz, cyy, cyz, czz, nx, ny, nz);
    const double dir = orient < 0 ? -1.0 : 1.0;
    if (nx == 0.0 && ny == 0.0 && nz == 0.0) {
        if (up_axis == 0) nx = dir; else if (up_axis == 1) ny = dir; else nz = dir;
    } else if (dir * (up_axis == 0 ? nx : up_axis == 1 ? ny : nz) < 0.0) {
        nx = -nx; ny = -ny; nz = -nz;
    }
    if (lane == 0) {
        normals[3 * v + 0] = (float)nx; normals[3 * v + 1] = (float)ny; normals[3 * v + 2] = (float)nz;
    }
}

}  // namespace
