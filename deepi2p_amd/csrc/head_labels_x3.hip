// The labels-only tail of the FINE per-point head (per_point_pn of models/networks_united.py:57-74 for fine models, 736 -> 256 -> 256 -> 2+L,
// applied at :188-197, followed by the two argmaxes of models/multimodal_classifier.py:100-117) on the bf16 matrix instructions with EXACT
// three-way fp32 operand splits ("bf16x3", see head_x3.hip / conv_x3.hip).  Layer 0 stays a gathered pointwise GEMM; from its output y0 one launch
// computes, for every point,
//   layer 1   y1 = relu?(scale1 * W1 y0 + shift1)                K = M = 256
//   layer 2   s  = scale2? * W2 y1 + shift2                       P = 2 + L outputs, any P >= 3
//   labels    coarse = argmax(s[0:2]), fine = argmax(s[2:P])      int32 [B, N]
// and writes the scores f32[B,P,N] only when asked to.  The score tensor (2.7 GB per step at 16 x 30000 points and L = 1400) never exists.
//
// A workgroup of eight waves owns 64 points of one frame at a time (persistent: one workgroup per compute unit walks its tiles):
//   * y0 of the tile is split ONCE while it is staged into LDS, as three bf16 planes in B-fragment order ([plane][K-step][column tile][lane] x
//     16 B: a wave's fragment read is one contiguous KB, ds_read_b128, conflict-free) -- 96 KB;
//   * layer 1: wave w computes output rows 32 w .. 32 w + 31 for both 32-point column tiles (12 MFMAs per K-step); after a barrier its epilogue
//     writes y1, split the same way, over y0's LDS (y0 is dead by then) -- so LDS holds 96 KB of planes + 8 KB for the final reduction;
//   * the next tile's y0 is requested into registers right there and flies under layer 2;
//   * layer 2: the waves walk the output row tiles (32 channels each; with at most four row tiles, row tile x column tile pairs so that more
//     waves have work); the accumulators go through the epilogue, the optional score store and a running per-lane (value, channel) maximum;
//   * lanes n and n + 32 hold the two halves of a column: they meet through ds_bpermute, the eight waves through LDS.
// The weights are split once per checkpoint into fragment order ([row tile][K-step][plane][lane] x 16 B, rows padded to a multiple of 32 with
// zeros: di2p_head_labels_x3_pack) and stream from L2 / L1 a K-step ahead (the split W2 of P = 1402 is 2.1 MB).
//
// Argmax semantics are those of argmax_channels_kernel (point_ops.hip): the first maximum wins, a NaN ranks above everything and the first NaN
// wins.  The (value, channel) pairs are combined with a total order -- NaN above numbers, then larger value, then lower channel -- which is
// associative and commutative, so the order in which lanes, row tiles and waves meet does not matter and the result equals a channel-by-channel
// scan with a strict comparison.
#include <stdint.h>

#include "bf16x3.h"
#include "common.h"

namespace {

using bf16x3::u32x4_t;
using bf16x3::f32x16;

constexpr int HL_K = 256;                  // hidden width (input and output of layer 1, input of layer 2)
constexpr int HL_KS = HL_K / 16;           // K-steps of one layer
constexpr int HL_NW = 8;                   // waves per workgroup
constexpr int HL_PTS = 64;                 // points per tile = two 32-point column tiles
constexpr int HL_PLANE_U4 = HL_KS * 2 * 64;                           // u32x4 per plane (16 K-steps x 2 column tiles x 64 lanes)
constexpr size_t HL_LDS = (size_t)3 * HL_PLANE_U4 * 16 + (size_t)HL_NW * HL_PTS * 4 * 4;   // planes + reduction slots = 104 KB

struct HlArgs {
    const float* y0; long long bs; int rs;              // f32[B, 256, N] (batch / row strides in floats)
    const u32x4_t* W1p; const float* sc1; const float* sh1; int relu1;
    const u32x4_t* W2p; const float* sc2; const float* sh2; int P, ptiles;
    float* scores; int* coarse; int* fine;
    int N, nblk, total;                                  // nblk = 64-point tiles per frame; total = B * nblk
};

// (v, i) ranks above (w, j): NaN above every number (the lower channel among NaNs), else the larger value, else the lower channel.
// An empty slot is (-inf, INT_MAX): every real candidate ranks above it.
__device__ __forceinline__ bool hl_better(float v, int i, float w, int j) {
    const bool vn = v != v, wn = w != w;
    if (vn || wn) return vn && (!wn || i < j);
    return v > w || (v == w && i < j);
}
__device__ __forceinline__ void hl_take(float& bv, int& bi, float v, int i) {
    if (hl_better(v, i, bv, bi)) { bv = v; bi = i; }
}

// One K-step of the six products (small terms first, like head_x3.hip): acc += A (3 planes) x B (3 planes)
__device__ __forceinline__ f32x16 hl_kstep(const u32x4_t (&a)[3], const u32x4_t (&b)[3], f32x16 acc) {
    acc = bf16x3::mma(a[2], b[0], acc);
    acc = bf16x3::mma(a[1], b[1], acc);
    acc = bf16x3::mma(a[1], b[0], acc);
    acc = bf16x3::mma(a[0], b[2], acc);
    acc = bf16x3::mma(a[0], b[1], acc);
    acc = bf16x3::mma(a[0], b[0], acc);
    return acc;
}

// acc[jj] (jj < CT) = W[row tile t] x planes[column tile j0 + jj], all 16 K-steps; the weight fragments of K-step s + 1 are requested before the
// products of K-step s
template <int CT>
__device__ __forceinline__ void hl_tile(const u32x4_t* __restrict__ Wp, int t, const u32x4_t* planes, int j0, int lane, f32x16 (&acc)[CT]) {
#pragma unroll
    for (int jj = 0; jj < CT; ++jj)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[jj][r] = 0.0f;
    const u32x4_t* W = Wp + (long long)t * HL_KS * 3 * 64 + lane;
    auto a_load = [&](u32x4_t (&a)[3], int s) __attribute__((always_inline)) {
#pragma unroll
        for (int p = 0; p < 3; ++p) a[p] = W[(s * 3 + p) * 64];
    };
    auto products = [&](const u32x4_t (&a)[3], int s) __attribute__((always_inline)) {
#pragma unroll
        for (int jj = 0; jj < CT; ++jj) {
            u32x4_t b[3];
#pragma unroll
            for (int p = 0; p < 3; ++p) b[p] = planes[(p * HL_KS + s) * 2 * 64 + (j0 + jj) * 64 + lane];
            acc[jj] = hl_kstep(a, b, acc[jj]);
        }
    };
    // two K-steps per trip, not unrolled further: unrolled, hipcc requests every fragment of the layer up front -- and spills them
    u32x4_t a0[3], a1[3];
    a_load(a0, 0);
#pragma unroll 1
    for (int s = 0; s < HL_KS; s += 2) {
        a_load(a1, s + 1);
        products(a0, s);
        if (s + 2 < HL_KS) a_load(a0, s + 2);
        products(a1, s + 1);
    }
}

// CT2: column tiles per layer-2 work unit (2: a unit is a row tile for all 64 points; 1: a row tile for 32 points -- twice the units, for
// heads with at most four row tiles, where eight waves would otherwise mostly wait)
template <int CT2>
__global__ __launch_bounds__(HL_NW * 64, 1) void point_head_labels_x3_kernel(const HlArgs a) {
    extern __shared__ __attribute__((aligned(16))) u32x4_t hl_lds[];
    u32x4_t* planes = hl_lds;                                              // [3][16][2][64]: y0, then y1
    float4* red = reinterpret_cast<float4*>(hl_lds + 3 * HL_PLANE_U4);     // [8 waves][64 points]: coarse (v, i), fine (v, i)
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nl = lane & 31, h = lane >> 5;

    // this thread's four fragments of a tile's y0: fragment f = tid + 512 i -> lane f & 63 (= lane), column tile (f >> 6) & 1, K-step f >> 7
    float xr[4][8];
    auto y0_request = [&](int tile) __attribute__((always_inline)) {
        const int fb = tile / a.nblk;
        const int n = (tile - fb * a.nblk) * HL_PTS + 32 * ((tid >> 6) & 1) + nl;
        const int nc = min(n, a.N - 1);
        const float* src = a.y0 + (long long)fb * a.bs + nc;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int k0 = 16 * ((tid >> 7) + 4 * i) + 8 * h;
#pragma unroll
            for (int e = 0; e < 8; ++e) xr[i][e] = src[(long long)(k0 + e) * a.rs];
        }
        if (n >= a.N) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int e = 0; e < 8; ++e) xr[i][e] = 0.0f;
        }
    };
    auto y0_store = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float p0[8], p1[8], p2[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) bf16x3::split(xr[i][e], p0[e], p1[e], p2[e]);
            const int f = tid + 512 * i;
            planes[0 * HL_PLANE_U4 + f] = u32x4_t{bf16x3::pack_hi(p0[0], p0[1]), bf16x3::pack_hi(p0[2], p0[3]), bf16x3::pack_hi(p0[4], p0[5]), bf16x3::pack_hi(p0[6], p0[7])};
            planes[1 * HL_PLANE_U4 + f] = u32x4_t{bf16x3::pack_hi(p1[0], p1[1]), bf16x3::pack_hi(p1[2], p1[3]), bf16x3::pack_hi(p1[4], p1[5]), bf16x3::pack_hi(p1[6], p1[7])};
            planes[2 * HL_PLANE_U4 + f] = u32x4_t{bf16x3::pack_hi(p2[0], p2[1]), bf16x3::pack_hi(p2[2], p2[3]), bf16x3::pack_hi(p2[4], p2[5]), bf16x3::pack_hi(p2[6], p2[7])};
        }
    };

    int tile = blockIdx.x;
    if (tile >= a.total) return;                       // whole workgroup
    y0_request(tile);
    for (; tile < a.total; tile += gridDim.x) {
        const int fb = tile / a.nblk;
        const int n0 = (tile - fb * a.nblk) * HL_PTS;
        y0_store();
        __syncthreads();
        // ---- layer 1: row tile `wave`, both column tiles
        f32x16 acc1[2];
        hl_tile<2>(a.W1p, wave, planes, 0, lane, acc1);
        __syncthreads();                               // every wave is done with y0: y1 goes over it
        // ---- epilogue 1: rows 32 w + 8 g + 4 h + q of column 32 j + n -> K-step 2 w + (g >> 1), fragment lane n + 32 (g & 1), elements 4 h + q
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                float p[3][4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int row = 32 * wave + 8 * g + 4 * h + q;
                    float v = acc1[j][4 * g + q] * a.sc1[row] + a.sh1[row];
                    if (a.relu1) v = fmaxf(v, 0.0f);
                    bf16x3::split(v, p[0][q], p[1][q], p[2][q]);
                }
                const int s = 2 * wave + (g >> 1);
#pragma unroll
                for (int pl = 0; pl < 3; ++pl) {
                    uint2* dst = reinterpret_cast<uint2*>(planes + (pl * HL_KS + s) * 2 * 64 + j * 64 + nl + 32 * (g & 1)) + h;
                    *dst = make_uint2(bf16x3::pack_hi(p[pl][0], p[pl][1]), bf16x3::pack_hi(p[pl][2], p[pl][3]));
                }
            }
        // the next tile's y0 flies under layer 2
        if (tile + (int)gridDim.x < a.total) y0_request(tile + gridDim.x);
        __syncthreads();
        // ---- layer 2 + labels: running (value, channel) maxima of this lane's column(s)
        float cv[2] = {-__builtin_inff(), -__builtin_inff()}, fv[2] = {-__builtin_inff(), -__builtin_inff()};
        int ci[2] = {0x7fffffff, 0x7fffffff}, fi[2] = {0x7fffffff, 0x7fffffff};
        constexpr int UPT = 2 / CT2;                   // work units per row tile
        const int units = a.ptiles * UPT;
        for (int u = wave; u < units; u += HL_NW) {
            const int t = u / UPT, j0 = (u - t * UPT) * CT2;
            f32x16 acc2[CT2];
            hl_tile<CT2>(a.W2p, t, planes, j0, lane, acc2);
#pragma unroll
            for (int jj = 0; jj < 2; ++jj) {
                if (CT2 == 1 && jj != j0) continue;
                const f32x16& acc = acc2[CT2 == 2 ? jj : 0];
                const int n = n0 + 32 * jj + nl;
                const bool live = n < a.N;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int c = 32 * t + (r & 3) + 8 * (r >> 2) + 4 * h;
                    if (c < a.P) {
                        float o = acc[r];
                        if (a.sc2) o *= a.sc2[c];
                        if (a.sh2) o += a.sh2[c];
                        if (a.scores && live) a.scores[((long long)fb * a.P + c) * a.N + n] = o;
                        if (c < 2) hl_take(cv[jj], ci[jj], o, c);
                        else hl_take(fv[jj], fi[jj], o, c - 2);
                    }
                }
            }
        }
        // lanes n and n + 32 hold the two halves of column n; then the eight waves meet in LDS
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            const float ocv = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute((lane ^ 32) * 4, __builtin_bit_cast(int, cv[jj])));
            const int oci = __builtin_amdgcn_ds_bpermute((lane ^ 32) * 4, ci[jj]);
            const float ofv = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute((lane ^ 32) * 4, __builtin_bit_cast(int, fv[jj])));
            const int ofi = __builtin_amdgcn_ds_bpermute((lane ^ 32) * 4, fi[jj]);
            hl_take(cv[jj], ci[jj], ocv, oci);
            hl_take(fv[jj], fi[jj], ofv, ofi);
            if (h == 0)
                red[wave * HL_PTS + 32 * jj + nl] = make_float4(cv[jj], __builtin_bit_cast(float, ci[jj]), fv[jj], __builtin_bit_cast(float, fi[jj]));
        }
        __syncthreads();
        if (tid < HL_PTS) {
            float4 m = red[tid];
            for (int w = 1; w < HL_NW; ++w) {
                const float4 o = red[w * HL_PTS + tid];
                if (hl_better(o.x, __builtin_bit_cast(int, o.y), m.x, __builtin_bit_cast(int, m.y))) { m.x = o.x; m.y = o.y; }
                if (hl_better(o.z, __builtin_bit_cast(int, o.w), m.z, __builtin_bit_cast(int, m.w))) { m.z = o.z; m.w = o.w; }
            }
            const int n = n0 + tid;
            if (n < a.N) {
                a.coarse[(long long)fb * a.N + n] = __builtin_bit_cast(int, m.y);
                a.fine[(long long)fb * a.N + n] = __builtin_bit_cast(int, m.w);
            }
        }
        // (the reduction slots are next written after two more barriers; the planes are overwritten only after the barrier above)
    }
}

}  // namespace

extern "C" long long di2p_head_labels_x3_packed_bytes(int K, int P) {
    return K >= 16 && K % 16 == 0 && P >= 1 ? (long long)((P + 31) / 32) * (K / 16) * 3 * 1024 : 0;
}

// Wt f32[K][P] (the [K, M] layout of every pointwise layer; K % 16 == 0) -> the fragment-ordered split operand of di2p_point_head_labels_x3
// (di2p_head_labels_x3_packed_bytes(K, P) bytes, 16-byte aligned).
extern "C" int di2p_head_labels_x3_pack(const float* Wt, int K, int P, void* Wp, void* stream) {
    DI2P_CHECK_ARG(Wt && Wp, "null pointer");
    DI2P_CHECK_ARG(K >= 16 && K % 16 == 0 && P >= 1, "needs K % 16 == 0 and P >= 1");
    DI2P_CHECK_ARG(((uintptr_t)Wp & 15) == 0, "packed weights must be 16-byte aligned");
    // fragment order [ceil(P / 32) row tiles][K / 16][3 planes][64 lanes] x 8 bf16, rows P .. 32 ceil(P / 32) - 1 zero
    di2p_pack_a32(Wt, K, P, (P + 31) / 32, K / 16, 1, Wp, stream);
    DI2P_RETURN_LAUNCH();
}

// Layers 1-2 of the fine per-point head and the two argmaxes in one launch (see the top of this file and di2p_head_labels_x3_t).
extern "C" int di2p_point_head_labels_x3(const di2p_head_labels_x3_t* hd, int B, int N, void* stream) {
    DI2P_CHECK_ARG(hd, "null pointer");
    DI2P_CHECK_ARG(B >= 0 && N >= 1, "bad size");
    DI2P_CHECK_ARG(hd->K == HL_K, "this build runs a hidden width of 256 (the fine per_point_pn)");
    DI2P_CHECK_ARG(hd->P >= 3, "needs P >= 3 (two coarse channels and at least one fine channel)");
    DI2P_CHECK_ARG(hd->y0 && hd->W1p && hd->W2p && hd->scale1 && hd->shift1 && hd->coarse && hd->fine, "null operand");
    DI2P_CHECK_ARG(((uintptr_t)hd->W1p & 15) == 0 && ((uintptr_t)hd->W2p & 15) == 0, "packed weights must be 16-byte aligned");
    DI2P_CHECK_ARG(hd->row_stride >= N && hd->batch_stride >= (long long)HL_K * hd->row_stride, "y0 must be [B, 256, N] with row stride >= N");
    if (B == 0) return 0;
    HlArgs a{};
    a.y0 = hd->y0; a.bs = hd->batch_stride; a.rs = hd->row_stride;
    a.W1p = (const u32x4_t*)hd->W1p; a.sc1 = hd->scale1; a.sh1 = hd->shift1; a.relu1 = hd->relu1;
    a.W2p = (const u32x4_t*)hd->W2p; a.sc2 = hd->scale2; a.sh2 = hd->shift2; a.P = hd->P; a.ptiles = (hd->P + 31) / 32;
    a.scores = hd->scores; a.coarse = hd->coarse; a.fine = hd->fine;
    a.N = N; a.nblk = di2p_cdiv(N, HL_PTS);
    DI2P_CHECK_ARG((long long)B * a.nblk < (1ll << 31), "too many points");
    a.total = B * a.nblk;
    const int grid = a.total < di2p_cu_count() ? a.total : di2p_cu_count();      // one 104 KB workgroup per compute unit, persistent
    hipStream_t st = (hipStream_t)stream;
    if (a.ptiles <= 4) {
        if (di2p_allow_dynamic_lds((const void*)point_head_labels_x3_kernel<1>, HL_LDS, __func__)) return -1;
        hipLaunchKernelGGL(point_head_labels_x3_kernel<1>, dim3(grid), dim3(HL_NW * 64), HL_LDS, st, a);
    } else {
        if (di2p_allow_dynamic_lds((const void*)point_head_labels_x3_kernel<2>, HL_LDS, __func__)) return -1;
        hipLaunchKernelGGL(point_head_labels_x3_kernel<2>, dim3(grid), dim3(HL_NW * 64), HL_LDS, st, a);
    }
    DI2P_RETURN_LAUNCH();
}
