// Result overlays: the images the reference writes for every evaluated frame (util/vis_tools.py:96-339), for a whole batch on the device.
//
//  * canvas u8 [B, H + 2 H_delta, W + 2 W_delta, 3]: white, the frame's image in the middle, (fine variant) white grid lines over the image;
//  * every point that survives the reference's skip tests stamps cv2.circle(radius 1, filled) = five pixels in its colour, in index order,
//    later points over earlier ones.
//
// "Later over earlier" is "the largest index wins", so the paint order needs no serial loop: one thread per point issues an atomicMax of
// ((n + 1) << 3) | colour code into a u32 key plane for each of its five pixels (integer max: the result does not depend on arrival order), and
// one pass over the canvas pixels writes the colour of the winning key or, for key 0, the base pixel, which it works out from the pixel's
// coordinates (margin, image, grid line) without a base pass of its own.  Three launches per overlay: clear keys, stamp, compose.
//
// Compiled with -ffp-contract=off: the registration variant's fp64 projection is compared with numpy.
// Plain HIP C++: vector stores only, no allocation, no synchronisation -- every entry point can be captured into a hipGraph.
#include "common.h"

#include <math.h>

namespace {

constexpr int MAX_POINTS = 1 << 28;           // (n + 1) << 3 must fit 32 bits
constexpr int MAX_SIDE = 1 << 24;             // canvas sides stay exact in fp32 (the skip test compares rounded floats with them)
// colour codes of a key's low three bits; 0 is "no stamp"
constexpr int C_RED = 1, C_BLUE = 2, C_GREEN = 3, C_YELLOW = 4;

struct Geometry {
    int H, W, H_delta, W_delta, HL, WL;       // HL, WL: the canvas (image + both margins)
};

__device__ inline uint32_t colour_rgb(uint32_t code) {      // r | g << 8 | b << 16
    return code == C_RED ? 0x0000ffu : code == C_BLUE ? 0xff0000u : code == C_GREEN ? 0x00ff00u : 0x00ffffu;
}

// The five pixels of cv2.circle(img, (cx, cy), 1, colour, -1), clipped to the canvas.  The caller has 0 <= cx < WL - 1, 0 <= cy < HL - 1.
__device__ inline void stamp(uint32_t* __restrict__ keys, const Geometry g, int cx, int cy, uint32_t key) {
    uint32_t* row = keys + (long long)cy * g.WL;
    atomicMax(row + cx, key);
    if (cx >= 1) atomicMax(row + cx - 1, key);
    if (cx + 1 < g.WL) atomicMax(row + cx + 1, key);
    if (cy >= 1) atomicMax(row - g.WL + cx, key);
    if (cy + 1 < g.HL) atomicMax(row + g.WL + cx, key);
}

// int(round(p)) + delta inside [0, side - 1) ?  r is rint(p): an integer-valued float or double, compared before any conversion to int
// (1e30 never reaches one); the bounds are small integers and exact in either type.
template <typename T>
__device__ inline bool centre(T r, int delta, int side, int* c) {
    if (!(r >= (T)(-delta) && r < (T)(side - 1 - delta))) return false;      // NaN fails both
    *c = (int)r + delta;
    return true;
}

__global__ __launch_bounds__(256) void stamp_classification_kernel(const float* __restrict__ pxpy, const int* __restrict__ coarse_pred,
                                                                   const int* __restrict__ coarse_gt, const int* __restrict__ fine_pred,
                                                                   const int* __restrict__ fine_gt, int N, Geometry g,
                                                                   uint32_t* __restrict__ keys) {
    const int b = blockIdx.y;
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const long long o = (long long)b * N + n;
    const bool pred = coarse_pred[o] == 1, gt = coarse_gt[o] == 1;
    uint32_t code;
    if (pred && gt) code = (fine_pred && fine_pred[o] != fine_gt[o]) ? C_YELLOW : C_GREEN;
    else if (gt) code = C_RED;                 // false negative
    else if (pred) code = C_BLUE;              // false positive
    else return;                               // nothing drawn, nothing covered
    const float px = pxpy[2 * (long long)b * N + n], py = pxpy[(2 * (long long)b + 1) * N + n];
    if (isinf(px) || isinf(py) || isnan(px) || isnan(py)) return;
    int cx, cy;
    if (!centre(rintf(px), g.W_delta, g.WL, &cx) || !centre(rintf(py), g.H_delta, g.HL, &cy)) return;
    stamp(keys + (long long)b * g.HL * g.WL, g, cx, cy, ((uint32_t)(n + 1) << 3) | code);
}

__global__ __launch_bounds__(256) void stamp_registration_kernel(const float* __restrict__ pc, const double* __restrict__ P,
                                                                 const double* __restrict__ K, const int* __restrict__ labels, int N, Geometry g,
                                                                 uint32_t* __restrict__ keys) {
    const int b = blockIdx.y;
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const long long o = (long long)b * 3 * N + n;
    const double x = (double)pc[o], y = (double)pc[o + N], z = (double)pc[o + 2ll * N];
    const double* Pb = P + 16 * (long long)b;
    const double* Kb = K + 9 * (long long)b;
    double q[3], k[3];
    for (int r = 0; r < 3; ++r) q[r] = Pb[4 * r] * x + Pb[4 * r + 1] * y + Pb[4 * r + 2] * z + Pb[4 * r + 3];      // rows 0..2 of P [p; 1]
    for (int r = 0; r < 3; ++r) k[r] = Kb[3 * r] * q[0] + Kb[3 * r + 1] * q[1] + Kb[3 * r + 2] * q[2];
    const double px = k[0] / k[2], py = k[1] / k[2];
    if (isinf(px) || isinf(py) || isnan(px) || isnan(py)) return;
    int cx, cy;
    if (!centre(rint(px), g.W_delta, g.WL, &cx) || !centre(rint(py), g.H_delta, g.HL, &cy) || k[2] < 0.0) return;
    const uint32_t code = labels[(long long)b * N + n] == 1 ? C_RED : C_BLUE;
    stamp(keys + (long long)b * g.HL * g.WL, g, cx, cy, ((uint32_t)(n + 1) << 3) | code);
}

// img.round().to(uint8) with the out-of-range values clamped (NaN -> 0)
__device__ inline uint32_t to_u8(float v) { return (uint32_t)fminf(fmaxf(rintf(v), 0.0f), 255.0f); }

// The canvas before any point: r | g << 8 | b << 16 of pixel (X, Y) of frame b.
template <bool U8>
__device__ inline uint32_t base_pixel(const void* __restrict__ img, const Geometry g, int grid_s, int n_rows, int n_cols, int b, int Y, int X) {
    const int iy = Y - g.H_delta, ix = X - g.W_delta;
    if (iy < 0 || iy >= g.H || ix < 0 || ix >= g.W) return 0xffffffu;          // margin
    if (grid_s > 0) {                                                          // cv2.line, white, one pixel wide, over the image only
        const int h = iy / grid_s, w = ix / grid_s;
        if ((iy == h * grid_s && h >= 1 && h <= n_rows) || (ix == w * grid_s && w >= 1 && w <= n_cols)) return 0xffffffu;
    }
    if (U8) {
        const unsigned char* p = (const unsigned char*)img + (((long long)b * g.H + iy) * g.W + ix) * 3;
        return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
    }
    const long long plane = (long long)g.H * g.W;
    const float* p = (const float*)img + 3 * plane * b + (long long)iy * g.W + ix;
    return to_u8(p[0]) | (to_u8(p[plane]) << 8) | (to_u8(p[2 * plane]) << 16);
}

__device__ inline uint32_t pixel(uint32_t key, uint32_t base) { return key ? colour_rgb(key & 7u) : base; }

// One canvas pixel per thread, three byte stores: canvases whose width is no multiple of four, or unaligned buffers.
template <bool U8>
__global__ __launch_bounds__(256) void compose_kernel(const uint32_t* __restrict__ keys, const void* __restrict__ img, Geometry g, int grid_s,
                                                      int n_rows, int n_cols, long long pixels, unsigned char* __restrict__ canvas) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= pixels) return;
    const int X = (int)(i % g.WL);
    const long long row = i / g.WL;
    const int Y = (int)(row % g.HL), b = (int)(row / g.HL);
    const uint32_t key = keys[i];
    const uint32_t v = pixel(key, key ? 0u : base_pixel<U8>(img, g, grid_s, n_rows, n_cols, b, Y, X));
    canvas[3 * i] = (unsigned char)v;
    canvas[3 * i + 1] = (unsigned char)(v >> 8);
    canvas[3 * i + 2] = (unsigned char)(v >> 16);
}

// Four pixels of one row per thread (WL % 4 == 0): one 16-byte key load, twelve canvas bytes as three dword stores.  Where the four pixels
// lie inside the image, away from its grid columns, and the image rows allow it (img_vec: W % 4 == 0, W_delta % 4 == 0, aligned base), the base
// comes in as three dwords (u8) or three float4 (f32) instead of twelve scalar loads.
template <bool U8>
__global__ __launch_bounds__(256) void compose4_kernel(const uint32_t* __restrict__ keys, const void* __restrict__ img, Geometry g, int grid_s,
                                                       int n_rows, int n_cols, int img_vec, long long groups, uint32_t* __restrict__ canvas) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= groups) return;
    const int per_row = g.WL >> 2;
    const int X = (int)(i % per_row) << 2;
    const long long row = i / per_row;
    const int Y = (int)(row % g.HL), b = (int)(row / g.HL);
    const uint4 k4 = *reinterpret_cast<const uint4*>(keys + 4 * i);
    const uint32_t key[4] = {k4.x, k4.y, k4.z, k4.w};
    uint32_t v[4];
    const int iy = Y - g.H_delta, ix = X - g.W_delta;
    bool fast = img_vec && iy >= 0 && iy < g.H && ix >= 0 && ix + 3 < g.W && !(key[0] && key[1] && key[2] && key[3]);
    if (fast && grid_s > 0) {
        const int h = iy / grid_s;
        const int w0 = ix / grid_s, w3 = (ix + 3) / grid_s;                    // a grid column among the four: ix itself or a multiple in (ix, ix + 3]
        fast = !(iy == h * grid_s && h >= 1 && h <= n_rows) && !((ix == w0 * grid_s || w3 != w0) && w3 >= 1 && w0 <= n_cols);
    }
    if (fast) {
        if (U8) {
            const uint32_t* p = reinterpret_cast<const uint32_t*>((const unsigned char*)img + (((long long)b * g.H + iy) * g.W + ix) * 3);
            const uint32_t d0 = p[0], d1 = p[1], d2 = p[2];
            v[0] = d0 & 0xffffffu;
            v[1] = (d0 >> 24) | ((d1 & 0xffffu) << 8);
            v[2] = (d1 >> 16) | ((d2 & 0xffu) << 16);
            v[3] = d2 >> 8;
        } else {
            const long long plane = (long long)g.H * g.W;
            const float* p = (const float*)img + 3 * plane * b + (long long)iy * g.W + ix;
            const float4 r = *reinterpret_cast<const float4*>(p), gg = *reinterpret_cast<const float4*>(p + plane),
                         bb = *reinterpret_cast<const float4*>(p + 2 * plane);
            v[0] = to_u8(r.x) | (to_u8(gg.x) << 8) | (to_u8(bb.x) << 16);
            v[1] = to_u8(r.y) | (to_u8(gg.y) << 8) | (to_u8(bb.y) << 16);
            v[2] = to_u8(r.z) | (to_u8(gg.z) << 8) | (to_u8(bb.z) << 16);
            v[3] = to_u8(r.w) | (to_u8(gg.w) << 8) | (to_u8(bb.w) << 16);
        }
        for (int j = 0; j < 4; ++j) v[j] = pixel(key[j], v[j]);
    } else {
        for (int j = 0; j < 4; ++j) v[j] = pixel(key[j], key[j] ? 0u : base_pixel<U8>(img, g, grid_s, n_rows, n_cols, b, Y, X + j));
    }
    uint32_t* out = canvas + 3 * i;
    out[0] = v[0] | (v[1] << 24);
    out[1] = (v[1] >> 8) | (v[2] << 16);
    out[2] = (v[2] >> 16) | (v[3] << 8);
}

__global__ __launch_bounds__(256) void clear_keys_kernel(uint4* __restrict__ keys, long long n16) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n16) keys[i] = make_uint4(0u, 0u, 0u, 0u);
}

long long key_bytes(long long B, long long HL, long long WL) { return (4 * B * HL * WL + 255) / 256 * 256; }

int check_geometry(const char* who, int B, int N, int H, int W, int H_delta, int W_delta, Geometry* g) {
    if (!(B >= 0 && N >= 0 && N <= MAX_POINTS && H >= 1 && W >= 1 && H_delta >= 0 && W_delta >= 0 && H < MAX_SIDE && W < MAX_SIDE &&
          H_delta < MAX_SIDE / 4 && W_delta < MAX_SIDE / 4)) {
        di2p_set_error("%s: bad sizes (B >= 0, 0 <= N <= 2^28, H, W >= 1, deltas >= 0, sides below 2^24)", who);
        return -1;
    }
    g->H = H; g->W = W; g->H_delta = H_delta; g->W_delta = W_delta;
    g->HL = H + 2 * H_delta; g->WL = W + 2 * W_delta;
    if (g->HL >= MAX_SIDE || g->WL >= MAX_SIDE || (long long)B * g->HL * g->WL >= (1ll << 38)) {
        di2p_set_error("%s: canvas too large", who);
        return -1;
    }
    return 0;
}

void clear_keys(void* workspace, const Geometry& g, int B, hipStream_t s) {
    const long long n16 = key_bytes(B, g.HL, g.WL) / 16;
    hipLaunchKernelGGL(clear_keys_kernel, dim3(di2p_cdiv(n16, 256)), dim3(256), 0, s, (uint4*)workspace, n16);
}

void compose(const void* workspace, const void* img, int img_is_u8, const Geometry& g, int B, int grid_s, int n_rows, int n_cols, void* canvas,
             hipStream_t s) {
    const uint32_t* keys = (const uint32_t*)workspace;
    const long long pixels = (long long)B * g.HL * g.WL;
    if (g.WL % 4 == 0 && (uintptr_t)canvas % 4 == 0 && (uintptr_t)workspace % 16 == 0) {
        const int img_vec = g.W % 4 == 0 && g.W_delta % 4 == 0 && (uintptr_t)img % 16 == 0;
        const long long groups = pixels / 4;
        if (img_is_u8)
            hipLaunchKernelGGL(compose4_kernel<true>, dim3(di2p_cdiv(groups, 256)), dim3(256), 0, s, keys, img, g, grid_s, n_rows, n_cols, img_vec,
                               groups, (uint32_t*)canvas);
        else
            hipLaunchKernelGGL(compose4_kernel<false>, dim3(di2p_cdiv(groups, 256)), dim3(256), 0, s, keys, img, g, grid_s, n_rows, n_cols, img_vec,
                               groups, (uint32_t*)canvas);
        return;
    }
    if (img_is_u8)
        hipLaunchKernelGGL(compose_kernel<true>, dim3(di2p_cdiv(pixels, 256)), dim3(256), 0, s, keys, img, g, grid_s, n_rows, n_cols, pixels,
                           (unsigned char*)canvas);
    else
        hipLaunchKernelGGL(compose_kernel<false>, dim3(di2p_cdiv(pixels, 256)), dim3(256), 0, s, keys, img, g, grid_s, n_rows, n_cols, pixels,
                           (unsigned char*)canvas);
}

}  // namespace

extern "C" long long di2p_vis_workspace_bytes(int B, int H, int W, int H_delta, int W_delta) {
    Geometry g;
    if (check_geometry(__func__, B, 0, H, W, H_delta, W_delta, &g) != 0) return -1;
    return key_bytes(B, g.HL, g.WL);
}

extern "C" int di2p_vis_classification(const float* pxpy, const int32_t* coarse_pred, const int32_t* coarse_gt, const int32_t* fine_pred,
                                       const int32_t* fine_gt, const void* img, int img_is_u8, int B, int N, int H, int W, int H_delta,
                                       int W_delta, int grid_s, int n_rows, int n_cols, uint8_t* canvas, void* workspace, void* stream) {
    Geometry g;
    if (check_geometry(__func__, B, N, H, W, H_delta, W_delta, &g) != 0) return -1;
    DI2P_CHECK_ARG((fine_pred == nullptr) == (fine_gt == nullptr), "fine_pred and fine_gt come together");
    DI2P_CHECK_ARG(fine_pred ? grid_s >= 1 : grid_s == 0, "grid_s >= 1 with the fine labels, 0 without (the coarse variant)");
    DI2P_CHECK_ARG(n_rows >= 0 && n_cols >= 0, "negative grid line count");
    if (B == 0) return 0;
    DI2P_CHECK_ARG(img && canvas && workspace, "null pointer");
    DI2P_CHECK_ARG(N == 0 || (pxpy && coarse_pred && coarse_gt), "null pointer");
    DI2P_CHECK_ARG((uintptr_t)workspace % 16 == 0, "workspace must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    clear_keys(workspace, g, B, s);
    if (N > 0)
        hipLaunchKernelGGL(stamp_classification_kernel, dim3(di2p_cdiv(N, 256), B), dim3(256), 0, s, pxpy, coarse_pred, coarse_gt, fine_pred,
                           fine_gt, N, g, (uint32_t*)workspace);
    compose(workspace, img, img_is_u8, g, B, grid_s, n_rows, n_cols, canvas, s);
    DI2P_RETURN_LAUNCH();
}

extern "C" int di2p_vis_registration(const float* pc, const double* P, const double* K, const int32_t* labels, const void* img, int img_is_u8,
                                     int B, int N, int H, int W, int H_delta, int W_delta, uint8_t* canvas, void* workspace, void* stream) {
    Geometry g;
    if (check_geometry(__func__, B, N, H, W, H_delta, W_delta, &g) != 0) return -1;
    if (B == 0) return 0;
    DI2P_CHECK_ARG(img && canvas && workspace && P && K, "null pointer");
    DI2P_CHECK_ARG(N == 0 || (pc && labels), "null pointer");
    DI2P_CHECK_ARG((uintptr_t)workspace % 16 == 0, "workspace must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    clear_keys(workspace, g, B, s);
    if (N > 0)
        hipLaunchKernelGGL(stamp_registration_kernel, dim3(di2p_cdiv(N, 256), B), dim3(256), 0, s, pc, P, K, labels, N, g, (uint32_t*)workspace);
    compose(workspace, img, img_is_u8, g, B, 0, 0, 0, canvas, s);
    DI2P_RETURN_LAUNCH();
}
