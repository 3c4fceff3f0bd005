// Synthetic worlds on the device (gfx950): one analytic scene per frame -- a ground plane, axis-aligned boxes and vertical cylinders, at most
// 32 primitives -- ray-cast through ONE trace function for the camera (a uint8 HWC raw frame) and for an HDL-64-like LiDAR (ragged [n,4]
// rows): the two inputs RawFramePlan.run takes, showing the same scene.  deepi2p_amd/world.py's docstring fixes the scene table and the
// shading formula; tests/world_oracle.py restates every operation in numpy fp64.
//
// trace is the arithmetic of synthetic._ray_box / _ray_pole / the ground line of make_velodyne_scan, operation for operation: the slab test
// with 1 / d (a zero component gives +-inf; a 0 * inf product is a NaN that np.nanmax / np.nanmin skip), the smaller root of the cylinder,
// (z0 - o.z) / min(d.z, -1e-12) for the ground.  The nearest hit wins, ties go to the lowest index (np.argmin), a miss is (inf, -1).  Only
// + - * / sqrt floor, comparisons and integer code on the camera path; the scan's directions come from host tables of cosines and sines,
// its noise from the library's Philox (stream tag 7) and fp64 Box-Muller.  FMA contraction is off for this file (build.py).
//
// A workgroup works on one frame: the frame's table (4 KB) is staged in LDS once and every lane walks the same primitive at the same time
// (the branch on the primitive's type is wave-uniform, the hit tests are selects; the one lane-dependent branch is the cylinder's early
// return for disc < 0, which whole waves take: it skips a square root and a division, measured 12 % of the camera kernel).
//   trace_kernel    one ray per thread
//   camera_kernel   four adjacent pixels per thread, the workgroup's 3072 bytes through LDS to dword stores (single bytes only at the
//                   two ends of a workgroup's range: a frame may start off a dword when 3 H0 W0 is no multiple of 4)
//   scan: rays_kernel (trace + keep rule + noise -> a full row per ray, the wave's keep mask, the workgroup's count), prefix_kernel (one
//   wave per frame, ragged2.h's wave_prefix), scan_offsets_kernel, write_kernel (stable compaction in ray order)
//   push-broom profiles (a 2-D laser with one pose per profile, one scene per sub-map; stream tag 8): the section further down
#include "common.h"
#include "philox.h"
#include "ragged2.h"

namespace {

constexpr int MAX_PRIMS = 32, SLOTS = 16;          // f64[B, P, 16]: type, six geometry slots, albedo r g b, reflectance, cell, four unused
constexpr int T_GROUND = 0, T_BOX = 1, T_CYL = 2;
constexpr int BLOCK = 256, PIX = 4;                // camera: pixels per thread
constexpr unsigned TAG_WORLD = 7u;
#define DI2P_INF __builtin_inf()
#define DI2P_NAN __builtin_nan("")

struct Ray { double ox, oy, oz, dx, dy, dz, ix, iy, iz; };
struct Hit { double t; int prim; };

__device__ __forceinline__ Ray make_ray(double ox, double oy, double oz, double dx, double dy, double dz) {
    return Ray{ox, oy, oz, dx, dy, dz, __ddiv_rn(1.0, dx), __ddiv_rn(1.0, dy), __ddiv_rn(1.0, dz)};
}

// np.minimum / np.maximum: a NaN operand gives NaN
__device__ __forceinline__ double np_min(double a, double b) { return (a < b || a != a) ? a : b; }
__device__ __forceinline__ double np_max(double a, double b) { return (a > b || a != a) ? a : b; }
// one step of np.nanmax / np.nanmin over an axis: NaN entries are skipped, all NaN stays NaN
__device__ __forceinline__ double nan_max(double acc, double v) { return (v == v && (acc != acc || v > acc)) ? v : acc; }
__device__ __forceinline__ double nan_min(double acc, double v) { return (v == v && (acc != acc || v < acc)) ? v : acc; }

// entry parameter of one slab (the pair of planes lo, hi along one axis)
__device__ __forceinline__ void slab(double lo, double hi, double o, double inv, double& mn, double& mx) {
    const double t0 = __dmul_rn(__dsub_rn(lo, o), inv), t1 = __dmul_rn(__dsub_rn(hi, o), inv);
    mn = np_min(t0, t1);
    mx = np_max(t0, t1);
}

// the hit parameter of primitive g (16 doubles, LDS) or inf; type is the same in every lane
__device__ __forceinline__ double hit_prim(const double* g, const Ray& r) {
    const int type = __builtin_amdgcn_readfirstlane((int)g[0]);
    if (type == T_BOX) {
        double mnx, mxx, mny, mxy, mnz, mxz;
        slab(g[1], g[4], r.ox, r.ix, mnx, mxx);
        slab(g[2], g[5], r.oy, r.iy, mny, mxy);
        slab(g[3], g[6], r.oz, r.iz, mnz, mxz);
        const double tmin = nan_max(nan_max(nan_max(DI2P_NAN, mnx), mny), mnz);
        const double tmax = nan_min(nan_min(nan_min(DI2P_NAN, mxx), mxy), mxz);
        return (tmax >= tmin && tmin > 0.0) ? tmin : DI2P_INF;
    }
    if (type == T_CYL) {
        const double ox = __dsub_rn(r.ox, g[1]), oy = __dsub_rn(r.oy, g[2]);
        const double a = __dadd_rn(__dmul_rn(r.dx, r.dx), __dmul_rn(r.dy, r.dy));
        const double bq = __dmul_rn(2.0, __dadd_rn(__dmul_rn(ox, r.dx), __dmul_rn(oy, r.dy)));
        const double c = __dsub_rn(__dadd_rn(__dmul_rn(ox, ox), __dmul_rn(oy, oy)), __dmul_rn(g[3], g[3]));
        const double disc = __dsub_rn(__dmul_rn(bq, bq), __dmul_rn(__dmul_rn(4.0, a), c));
        if (!(disc >= 0.0)) return DI2P_INF;          // poles are thin: most waves skip the square root and the division altogether
        const double t =__ddiv_rn(__dsub_rn(-bq, __dsqrt_rn(disc)), __dmul_rn(2.0, a));
        const double z = __dadd_rn(r.oz, __dmul_rn(t, r.dz));
        return (disc >= 0.0 && t > 0.0 && z >= g[4] && z <= g[5]) ? t : DI2P_INF;
    }
    const double t = __ddiv_rn(__dsub_rn(g[1], r.oz), r.dz < -1e-12 ? r.dz : -1e-12);          // np.minimum(d.z, -1e-12); d.z is no NaN where it counts
    return (r.dz < 0.0 && t > 0.0) ? t : DI2P_INF;
}

__device__ __forceinline__ Hit trace(const double* tab, int count, const Ray& r) {
    Hit h{DI2P_INF, -1};
    for (int i = 0; i < count; ++i) {
        const double t = hit_prim(tab + SLOTS * i, r);
        const bool nearer = t < h.t;          // strict: the first of equal hits stays, inf never wins
        h.t = nearer ? t : h.t;
        h.prim = nearer ? i : h.prim;
    }
    return h;
}

// the frame's table into LDS (all threads of the workgroup; ends with a barrier) -> its primitive count, clamped to [0, P]
__device__ __forceinline__ int stage_table(const double* __restrict__ prims, const int* __restrict__ count, int b, int P, double* tab) {
    int n = count[b];
    n = n < 0 ? 0 : (n > P ? P : n);
    for (int k = threadIdx.x; k < n * SLOTS; k += blockDim.x) tab[k] = prims[(long long)b * P * SLOTS + k];
    __syncthreads();
    return n;
}

// ---------------------------------------------------------------------------------------------------------------- trace
__global__ __launch_bounds__(BLOCK) void trace_kernel(const double* __restrict__ prims, const int* __restrict__ count, const double* __restrict__ origin,
                                                      const double* __restrict__ dirs, int P, int R, double* __restrict__ t_out,
                                                      int* __restrict__ prim_out) {
    __shared__ double tab[MAX_PRIMS * SLOTS];
    const int b = blockIdx.y;
    const int n = stage_table(prims, count, b, P, tab);
    const int r = blockIdx.x * BLOCK + threadIdx.x;
    if (r >= R) return;
    const long long i = (long long)b * R + r;
    const Hit h = trace(tab, n, make_ray(origin[3 * b], origin[3 * b + 1], origin[3 * b + 2], dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]));
    t_out[i] = h.t;
    prim_out[i] = h.prim;
}

// ---------------------------------------------------------------------------------------------------------------- camera
__device__ __forceinline__ double clamp255(double c) { return c < 0.0 ? 0.0 : (c > 255.0 ? 255.0 : c); }
__device__ __forceinline__ unsigned to_u8(double c) { return (unsigned)(int)floor(__dadd_rn(clamp255(c), 0.5)); }
// floor(h / cell) as the low 32 bits of its integer value (clamped to +-2^52 first: the conversion is always defined)
__device__ __forceinline__ unsigned cell_index(double h, double cell) {
    double q = floor(__ddiv_rn(h, cell));
    q = q < -4503599627370496.0 ? -4503599627370496.0 : (q > 4503599627370496.0 ? 4503599627370496.0 : q);
    return (unsigned)(unsigned long long)(long long)q;
}

__constant__ double TEX[8] = {0.70, 0.78, 0.86, 0.92, 1.00, 0.96, 0.82, 0.74};
constexpr double SHADE_X = 0.80, SHADE_Y = 0.65, SHADE_Z = 1.00, LIGHT_X = 0.6, LIGHT_Y = 0.8;
__constant__ double SKY_TOP[3] = {90.0, 140.0, 230.0}, SKY_SPAN[3] = {110.0, 80.0, 15.0};          // top + span * (v + 0.5) / H0

// the colour of a hit (world.py's docstring): albedo * face shade * cell texture * distance fade; -> the three bytes, r in bits 0-7
__device__ __forceinline__ unsigned shade_hit(const double* tab, const Ray& r, const Hit& h, double max_range) {
    const double* g = tab + SLOTS * h.prim;
    const int type = (int)g[0];
    const double hx = __dadd_rn(r.ox, __dmul_rn(h.t, r.dx)), hy = __dadd_rn(r.oy, __dmul_rn(h.t, r.dy)), hz = __dadd_rn(r.oz, __dmul_rn(h.t, r.dz));
    const double cell = g[11];
    unsigned qx = cell_index(hx, cell), qy = cell_index(hy, cell), qz = cell_index(hz, cell);
    double shade = 1.0;
    if (type == T_BOX) {          // the face is the slab the entry parameter came from (the first of equal ones): its axis is left out of the cell
        double mnx, mny, mx;
        slab(g[1], g[4], r.ox, r.ix, mnx, mx);
        slab(g[2], g[5], r.oy, r.iy, mny, mx);
        const int face = mnx == h.t ? 0 : (mny == h.t ? 1 : 2);
        shade = face == 0 ? SHADE_X : (face == 1 ? SHADE_Y : SHADE_Z);
        qx = face == 0 ? 0u : qx; qy = face == 1 ? 0u : qy; qz = face == 2 ? 0u : qz;
    } else if (type == T_CYL) {
        const double nx = __ddiv_rn(__dsub_rn(hx, g[1]), g[3]), ny = __ddiv_rn(__dsub_rn(hy, g[2]), g[3]);
        const double nl = __dadd_rn(__dmul_rn(nx, LIGHT_X), __dmul_rn(ny, LIGHT_Y));
        shade = __dadd_rn(0.6, __dmul_rn(0.4, nl > 0.0 ? nl : 0.0));
        qx = 0u; qy = 0u;
    } else {
        qz = 0u;
    }
    unsigned k = (qx * 73856093u) ^ (qy * 19349663u) ^ (qz * 83492791u) ^ ((unsigned)h.prim * 2654435761u);
    k ^= k >> 13; k *= 0x5bd1e995u; k ^= k >> 15;
    const double tex = TEX[k & 7u];
    double far = __ddiv_rn(h.t, max_range);
    far = far > 1.0 ? 1.0 : far;
    const double fade = __dsub_rn(1.0, __dmul_rn(0.5, far));
    unsigned rgb = 0;
    for (int c = 0; c < 3; ++c) rgb |= to_u8(__dmul_rn(__dmul_rn(__dmul_rn(__dmul_rn(g[7 + c], shade), tex), fade), 255.0)) << (8 * c);
    return rgb;
}

__device__ __forceinline__ unsigned shade_sky(int v, int H0) {
    const double gy = __ddiv_rn(__dadd_rn((double)v, 0.5), (double)H0);
    unsigned rgb = 0;
    for (int c = 0; c < 3; ++c) rgb |= to_u8(__dadd_rn(SKY_TOP[c], __dmul_rn(SKY_SPAN[c], gy))) << (8 * c);
    return rgb;
}

// Workgroup x of frame y takes pixels [1024 x, 1024 x + 1024) of the frame, thread t four adjacent ones.  Their 12 bytes go to LDS; then
// the workgroup's byte range [lo, hi) of the image is written from LDS: single bytes up to the first dword boundary and from the last one,
// dwords between them.  image is 4-byte aligned, so no dword store leaves [lo, hi).
__global__ __launch_bounds__(BLOCK) void camera_kernel(const double* __restrict__ prims, const int* __restrict__ count, const double* __restrict__ K_raw,
                                                       const double* __restrict__ cam_to_world, int P, int H0, int W0, double max_range,
                                                       unsigned char* __restrict__ image, float* __restrict__ depth, int* __restrict__ prim_out) {
    __shared__ double tab[MAX_PRIMS * SLOTS];
    __shared__ unsigned char bytes[BLOCK * PIX * 3];
    const int b = blockIdx.y;
    const int n = stage_table(prims, count, b, P, tab);
    const double* K = K_raw + 9 * (long long)b;
    const double* M = cam_to_world + 16 * (long long)b;
    const double fx = K[0], cx = K[2], fy = K[4], cy = K[5];
    const long long HW = (long long)H0 * W0, p0 = (long long)blockIdx.x * (BLOCK * PIX);
    for (int j = 0; j < PIX; ++j) {
        const long long p = p0 + PIX * threadIdx.x + j;
        if (p >= HW) break;
        const int v = (int)(p / W0), u = (int)(p - (long long)v * W0);
        const double xc = __ddiv_rn(__dsub_rn((double)u, cx), fx), yc = __ddiv_rn(__dsub_rn((double)v, cy), fy);
        const Ray r = make_ray(M[3], M[7], M[11], __dadd_rn(__dadd_rn(__dmul_rn(M[0], xc), __dmul_rn(M[1], yc)), M[2]),
                               __dadd_rn(__dadd_rn(__dmul_rn(M[4], xc), __dmul_rn(M[5], yc)), M[6]),
                               __dadd_rn(__dadd_rn(__dmul_rn(M[8], xc), __dmul_rn(M[9], yc)), M[10]));
        const Hit h = trace(tab, n, r);
        const unsigned rgb = h.prim >= 0 ? shade_hit(tab, r, h, max_range) : shade_sky(v, H0);
        unsigned char* dst = bytes + 3 * (PIX * threadIdx.x + j);
        dst[0] = (unsigned char)(rgb & 255u); dst[1] = (unsigned char)((rgb >> 8) & 255u); dst[2] = (unsigned char)((rgb >> 16) & 255u);
        if (depth) depth[b * HW + p] = h.prim >= 0 ? (float)h.t : 0.f;
        if (prim_out) prim_out[b * HW + p] = h.prim;
    }
    __syncthreads();
    const long long pe = min(HW, p0 + BLOCK * PIX);
    const long long lo = 3 * (b * HW + p0), hi = 3 * (b * HW + pe);          // byte range of this workgroup in the image
    const long long a0 = min(hi, (lo + 3) & ~3ll), a1 = max(a0, hi & ~3ll);  // dword-aligned interior [a0, a1)
    for (long long q = a0 + 4 * (long long)threadIdx.x; q < a1; q += 4 * BLOCK) {
        const unsigned char* s = bytes + (q - lo);
        *(unsigned*)(image + q) = (unsigned)s[0] | ((unsigned)s[1] << 8) | ((unsigned)s[2] << 16) | ((unsigned)s[3] << 24);
    }
    if (threadIdx.x < 3) {
        const long long head = lo + threadIdx.x, tail = a1 + threadIdx.x;
        if (head < a0) image[head] = bytes[head - lo];
        if (tail < hi) image[tail] = bytes[tail - lo];
    }
}

// ---------------------------------------------------------------------------------------------------------------- scan
struct Layout { size_t rows, mask, part_cnt, part_off, total; };

Layout layout(int B, int R) {
    Layout L;
    Take take;
    const size_t parts = (size_t)B * di2p_cdiv(R, BLOCK);
    L.rows = take(16 * (size_t)B * R);
    L.mask = take(8 * parts * (BLOCK / 64));
    L.part_cnt = take(4 * parts); L.part_off = take(4 * parts);
    L.total = take.o;
    return L;
}

struct ScanOpt { double max_range, dropout, range_sigma, intensity_sigma; unsigned long long seed; const unsigned long long* seed_dev; int frame0; };

// the library's Box-Muller (cosine branch) from one Philox block
__device__ __forceinline__ double gauss(const U4& r) {
    return sqrt(-2.0 * log(u53(r.x, r.y))) * cos(6.283185307179586476925 * u53(r.z, r.w));
}

// Ray r = beam * azimuths + azimuth of frame y, one per thread; the draws are Philox counter (r, frame0 + b, k, 7): block 0 the dropout
// uniform, block 1 the range noise, block 2 the intensity noise.  Every ray's row is written (kept or not), with the wave's keep mask.
__global__ __launch_bounds__(BLOCK) void rays_kernel(const double* __restrict__ prims, const int* __restrict__ count, const double* __restrict__ elev,
                                                     const double* __restrict__ azim, const double* __restrict__ pose, int P, int beams, int azimuths,
                                                     ScanOpt o, float4* __restrict__ rows, unsigned long long* __restrict__ masks,
                                                     int* __restrict__ part_cnt) {
    __shared__ double tab[MAX_PRIMS * SLOTS];
    __shared__ int wc[BLOCK / 64];
    const int b = blockIdx.y, R = beams * azimuths;
    const int n = stage_table(prims, count, b, P, tab);
    const int r = blockIdx.x * BLOCK + threadIdx.x;
    bool keep = false;
    if (r < R) {
        const int beam = r / azimuths, az = r - beam * azimuths;
        const double cE = elev[2 * beam], sE = elev[2 * beam + 1];
        const double cA = azim[2 * ((long long)b * azimuths + az)], sA = azim[2 * ((long long)b * azimuths + az) + 1];
        const double sx = __dmul_rn(cE, cA), sy = __dmul_rn(cE, sA), sz = sE;
        const double* M = pose + 16 * (long long)b;
        const Ray ray = make_ray(M[3], M[7], M[11], __dadd_rn(__dadd_rn(__dmul_rn(M[0], sx), __dmul_rn(M[1], sy)), __dmul_rn(M[2], sz)),
                                 __dadd_rn(__dadd_rn(__dmul_rn(M[4], sx), __dmul_rn(M[5], sy)), __dmul_rn(M[6], sz)),
                                 __dadd_rn(__dadd_rn(__dmul_rn(M[8], sx), __dmul_rn(M[9], sy)), __dmul_rn(M[10], sz)));
        const Hit h = trace(tab, n, ray);
        const unsigned long long seed = o.seed_dev ? *o.seed_dev : o.seed;
        const unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32), f = (unsigned)(o.frame0 + b);
        const U4 d0 = philox4x32_10(U4{(unsigned)r, f, 0u, TAG_WORLD}, k0, k1);
        keep = h.t < o.max_range && u53(d0.x, d0.y) >= o.dropout;          // decided before the noise
        double t = h.t, inten = h.prim >= 0 ? tab[SLOTS * h.prim + 10] : 0.0;
        if (o.range_sigma > 0.0) t = __dadd_rn(t, __dmul_rn(o.range_sigma, gauss(philox4x32_10(U4{(unsigned)r, f, 1u, TAG_WORLD}, k0, k1))));
        if (o.intensity_sigma > 0.0) inten = __dadd_rn(inten, __dmul_rn(o.intensity_sigma, gauss(philox4x32_10(U4{(unsigned)r, f, 2u, TAG_WORLD}, k0, k1))));
        inten = inten < 0.0 ? 0.0 : (inten > 1.0 ? 1.0 : inten);
        if (keep) rows[(long long)b * R + r] = make_float4((float)__dmul_rn(sx, t), (float)__dmul_rn(sy, t), (float)__dmul_rn(sz, t), (float)inten);
    }
    const unsigned long long mask = __ballot(keep);
    const int w = wave_id();
    const long long part = (long long)b * gridDim.x + blockIdx.x;
    if ((threadIdx.x & 63) == 0) { masks[part * (BLOCK / 64) + w] = mask; wc[w] = __popcll(mask); }
    __syncthreads();
    if (threadIdx.x == 0) {
        int c = 0;
        for (int k = 0; k < BLOCK / 64; ++k) c += wc[k];
        part_cnt[part] = c;
    }
}

__global__ __launch_bounds__(64) void prefix_kernel(int parts, const int* __restrict__ part_cnt, int* __restrict__ part_off, int* __restrict__ out_count) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int total = wave_prefix(part_cnt, (long long)b * parts, (long long)(b + 1) * parts, lane, part_off);
    if (lane == 0) out_count[b] = total;
}

__global__ __launch_bounds__(64) void scan_offsets_kernel(int B, const int* __restrict__ out_count, int* __restrict__ out_off) {
    if (threadIdx.x != 0) return;
    int run = 0;          // at most B * R < 2^31 rows (checked on the host)
    out_off[0] = 0;
    for (int b = 0; b < B; ++b) { run += out_count[b]; out_off[b + 1] = run; }
}

__global__ __launch_bounds__(BLOCK) void write_kernel(int R, const float4* __restrict__ rows, const unsigned long long* __restrict__ masks,
                                                      const int* __restrict__ part_off, const int* __restrict__ out_off, float4* __restrict__ out) {
    const int b = blockIdx.y, r = blockIdx.x * BLOCK + threadIdx.x, w = wave_id(), lane = threadIdx.x & 63;
    const long long part = (long long)b * gridDim.x + blockIdx.x;
    int before = 0;
    for (int k = 0; k < w; ++k) before += __popcll(masks[part * (BLOCK / 64) + k]);
    const unsigned long long mask = masks[part * (BLOCK / 64) + w];
    if (r < R && ((mask >> lane) & 1ull)) {
        const int rank = before + __popcll(mask & ((1ull << lane) - 1ull));
        out[(long long)out_off[b] + part_off[part] + rank] = rows[(long long)b * R + r];
    }
}

// ---------------------------------------------------------------------------------------------------------------- push-broom profiles
// Ray g = s * beams + k: beam k of profile s, profiles of sub-map b = [sub_off[b], sub_off[b+1]), one scene per sub-map.  The rays of a
// batch are ONE line of S * beams rays cut into parts of BLOCK; a part that holds profiles of several sub-maps stages their tables one
// after the other.  Compaction is global and stable (profile after profile, beam order), so scan_offsets[s] is simply the number of kept
// rays before ray s * beams:
//   accept_kernel         one wave: the leading sub-maps whose offsets are acceptable (ragged2.h's rule, outer level), status
//   profile_rays_kernel   trace + keep rule + noise -> the row of every kept ray, the wave's keep mask, the part's count
//   group_prefix_kernel   one wave per GROUP parts: wave_prefix of the part counts inside the group, the group's total
//   top_prefix_kernel     one wave: wave_prefix over the groups
//   profile_offsets_kernel  one thread per profile: scan_offsets and out_count from the prefixes and the mask of the wave ray s * beams is in
//   profile_write_kernel  stable compaction of the parked rows
constexpr unsigned TAG_PROFILES = 8u;
constexpr int GROUP = 1024;          // parts of one group_prefix_kernel wave (16 chunks of wave_prefix)

struct PLayout { size_t rows, mask, part_cnt, part_off, group_cnt, group_off, head, total; };

PLayout playout(long long R) {
    PLayout L;
    Take take;
    const size_t parts = (size_t)di2p_cdiv(R, (long long)BLOCK), groups = (size_t)di2p_cdiv((long long)parts, (long long)GROUP);
    L.rows = take(24 * (size_t)R);
    L.mask = take(8 * parts * (BLOCK / 64));
    L.part_cnt = take(4 * parts); L.part_off = take(4 * parts);
    L.group_cnt = take(4 * groups); L.group_off = take(4 * groups);
    L.head = take(8);          // n_ok (accepted sub-maps), total (kept rays)
    L.total = take.o;
    return L;
}

// Sub-map b is accepted iff sub_off[0 .. b+1] is a non-decreasing sequence in [0, S_cap] that starts at 0: the accepted ones are the first
// n_ok, they share no profile and cover the profiles [0, sub_off[n_ok]).
__global__ __launch_bounds__(64) void accept_kernel(const int* __restrict__ sub_off, int B, int S_cap, int* __restrict__ status, int* __restrict__ head) {
    const int lane = threadIdx.x;
    int first_bad = B;
    for (int j = lane; j < B; j += 64) {
        const int o0 = sub_off[j], o1 = sub_off[j + 1];
        if ((o0 < 0 || o1 < o0 || o1 > S_cap || (j == 0 && o0 != 0)) && j < first_bad) first_bad = j;
    }
    for (int o = 32; o; o >>= 1) first_bad = min(first_bad, __shfl_xor(first_bad, o));
    for (int j = lane; j < B; j += 64) status[j] = j < first_bad ? ST_OK : ST_OFFSETS;
    if (lane == 0) head[0] = first_bad;
}

// The draws are Philox counter (k, frame0 + s, j, 8): block 0 the dropout uniform, block 1 the range noise, block 2 the reflectance noise.
__global__ __launch_bounds__(BLOCK) void profile_rays_kernel(const double* __restrict__ prims, const int* __restrict__ count, const int* __restrict__ sub_off,
                                                             const int* __restrict__ head, const double* __restrict__ laser_to_world,
                                                             const double* __restrict__ beam, int P, int beams, ScanOpt o, double* __restrict__ rows,
                                                             unsigned long long* __restrict__ masks, int* __restrict__ part_cnt) {
    __shared__ double tab[MAX_PRIMS * SLOTS];
    __shared__ int wc[BLOCK / 64];
    const int n_ok = head[0];
    const long long R = n_ok > 0 ? (long long)sub_off[n_ok] * beams : 0;          // rays of the accepted sub-maps, < 2^31 (checked on the host)
    const long long g0 = (long long)blockIdx.x * BLOCK, g = g0 + threadIdx.x;
    bool keep = false;
    if (g0 < R) {          // the same in every thread, and so is the loop: its barriers are met by all of them
        const int s = (int)(g / beams), k = (int)(g - (long long)s * beams);
        const int b_last = frame_of(sub_off, n_ok, (min(R, g0 + BLOCK) - 1) / beams);
        for (int b = frame_of(sub_off, n_ok, g0 / beams); b <= b_last; ++b) {
            const int p0 = sub_off[b], p1 = sub_off[b + 1];
            if (p0 == p1) continue;
            __syncthreads();          // the previous sub-map's table may still be read
            const int n = stage_table(prims, count, b, P, tab);
            if (g >= R || s < p0 || s >= p1) continue;
            const double c = beam[2 * k], sn = beam[2 * k + 1];
            const double* M = laser_to_world + 16 * (long long)s;
            const Ray ray = make_ray(M[3], M[7], M[11], __dadd_rn(__dadd_rn(__dmul_rn(M[0], c), __dmul_rn(M[1], sn)), __dmul_rn(M[2], 0.0)),
                                     __dadd_rn(__dadd_rn(__dmul_rn(M[4], c), __dmul_rn(M[5], sn)), __dmul_rn(M[6], 0.0)),
                                     __dadd_rn(__dadd_rn(__dmul_rn(M[8], c), __dmul_rn(M[9], sn)), __dmul_rn(M[10], 0.0)));
            const Hit h = trace(tab, n, ray);
            const unsigned long long seed = o.seed_dev ? *o.seed_dev : o.seed;
            const unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32), f = (unsigned)(o.frame0 + s);
            const U4 d0 = philox4x32_10(U4{(unsigned)k, f, 0u, TAG_PROFILES}, k0, k1);
            keep = h.t < o.max_range && u53(d0.x, d0.y) >= o.dropout;          // decided before the noise
            double t = h.t, refl = h.prim >= 0 ? tab[SLOTS * h.prim + 10] : 0.0;
            if (o.range_sigma > 0.0) t = __dadd_rn(t, __dmul_rn(o.range_sigma, gauss(philox4x32_10(U4{(unsigned)k, f, 1u, TAG_PROFILES}, k0, k1))));
            if (o.intensity_sigma > 0.0)
                refl = __dadd_rn(refl, __dmul_rn(o.intensity_sigma, gauss(philox4x32_10(U4{(unsigned)k, f, 2u, TAG_PROFILES}, k0, k1))));
            if (keep) {
                double* row = rows + 3 * g;
                row[0] = __dmul_rn(t, c); row[1] = __dmul_rn(t, sn); row[2] = clamp255(__dmul_rn(255.0, refl));
            }
        }
    }
    const unsigned long long mask = __ballot(keep);
    const int w = wave_id();
    if ((threadIdx.x & 63) == 0) { masks[(long long)blockIdx.x * (BLOCK / 64) + w] = mask; wc[w] = __popcll(mask); }
    __syncthreads();
    if (threadIdx.x == 0) {
        int c = 0;
        for (int j = 0; j < BLOCK / 64; ++j) c += wc[j];
        part_cnt[blockIdx.x] = c;
    }
}

__global__ __launch_bounds__(64) void group_prefix_kernel(int parts, const int* __restrict__ part_cnt, int* __restrict__ part_off, int* __restrict__ group_cnt) {
    const long long j0 = (long long)blockIdx.x * GROUP;
    const int total = wave_prefix(part_cnt, j0, min(j0 + GROUP, (long long)parts), threadIdx.x, part_off);
    if (threadIdx.x == 0) group_cnt[blockIdx.x] = total;
}

__global__ __launch_bounds__(64) void top_prefix_kernel(int groups, const int* __restrict__ group_cnt, int* __restrict__ group_off, int* __restrict__ head) {
    const int total = wave_prefix(group_cnt, 0, groups, threadIdx.x, group_off);
    if (threadIdx.x == 0) head[1] = total;
}

// kept rays before ray g (g <= parts * BLOCK)
__device__ __forceinline__ int kept_before(long long g, int parts, const unsigned long long* __restrict__ masks, const int* __restrict__ part_off,
                                           const int* __restrict__ group_off, int total) {
    const long long part = g / BLOCK;
    if (part >= parts) return total;
    const int w = (int)((g % BLOCK) >> 6), lane = (int)(g & 63);
    int n = group_off[part / GROUP] + part_off[part];
    for (int j = 0; j < w; ++j) n += __popcll(masks[part * (BLOCK / 64) + j]);
    return n + __popcll(masks[part * (BLOCK / 64) + w] & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(BLOCK) void profile_offsets_kernel(int S_cap, int beams, int parts, const unsigned long long* __restrict__ masks,
                                                                const int* __restrict__ part_off, const int* __restrict__ group_off,
                                                                const int* __restrict__ head, int* __restrict__ scan_off, int* __restrict__ out_count) {
    const int s = blockIdx.x * BLOCK + threadIdx.x;
    if (s > S_cap) return;
    const int total = head[1];
    const int here = kept_before((long long)s * beams, parts, masks, part_off, group_off, total);
    scan_off[s] = here;
    if (s < S_cap) out_count[s] = kept_before((long long)(s + 1) * beams, parts, masks, part_off, group_off, total) - here;
}

__global__ __launch_bounds__(BLOCK) void profile_write_kernel(long long R_cap, const double* __restrict__ rows, const unsigned long long* __restrict__ masks,
                                                              const int* __restrict__ part_off, const int* __restrict__ group_off, double* __restrict__ out) {
    const long long g = (long long)blockIdx.x * BLOCK + threadIdx.x;
    const int w = wave_id(), lane = threadIdx.x & 63;
    const unsigned long long mask = masks[(long long)blockIdx.x * (BLOCK / 64) + w];
    if (g >= R_cap || !((mask >> lane) & 1ull)) return;
    int dst = group_off[blockIdx.x / GROUP] + part_off[blockIdx.x] + __popcll(mask & ((1ull << lane) - 1ull));
    for (int j = 0; j < w; ++j) dst += __popcll(masks[(long long)blockIdx.x * (BLOCK / 64) + j]);
    const double* src = rows + 3 * g;
    double* q = out + 3 * (long long)dst;
    q[0] = src[0]; q[1] = src[1]; q[2] = src[2];
}

bool finite_nonneg(double x) { return x >= 0.0 && x < 1e300; }

}  // namespace

extern "C" long long di2p_world_workspace_bytes(int B, int R) {
    if (B < 0 || R < 0 || (long long)B * R >= (1ll << 31)) return 0;
    return (long long)layout(B, R).total;
}

extern "C" int di2p_world_trace(const double* prims, const int32_t* count, int B, int P, const double* origin, const double* dirs, int R, double* t,
                                int32_t* prim, void* stream) {
    DI2P_CHECK_ARG(B >= 0 && R >= 0, "bad sizes (B, R >= 0)");
    DI2P_CHECK_ARG(P >= 0 && P <= MAX_PRIMS, "more than 32 primitives per frame");
    DI2P_CHECK_ARG(B <= 65535 && (long long)B * R < (1ll << 31), "B above 65535 or B * R above 2^31 - 1");
    DI2P_CHECK_ARG(B == 0 || (count && origin && (P == 0 || prims)), "null pointer");
    DI2P_CHECK_ARG(B == 0 || R == 0 || (dirs && t && prim), "null pointer (dirs, t, prim)");
    DI2P_CHECK_ARG((((uintptr_t)prims | (uintptr_t)origin | (uintptr_t)dirs | (uintptr_t)t) & 7) == 0, "prims, origin, dirs and t must be 8-byte aligned");
    if (B == 0 || R == 0) return 0;
    hipLaunchKernelGGL(trace_kernel, dim3(di2p_cdiv(R, BLOCK), B), dim3(BLOCK), 0, (hipStream_t)stream, prims, count, origin, dirs, P, R, t, prim);
    DI2P_RETURN_LAUNCH();
}

extern "C" int di2p_world_render_camera(const double* prims, const int32_t* count, int B, int P, const double* K_raw, const double* cam_to_world,
                                        int H0, int W0, double max_range, uint8_t* image, float* depth, int32_t* prim, void* stream) {
    DI2P_CHECK_ARG(B >= 0 && H0 >= 0 && W0 >= 0, "bad sizes (B, H0, W0 >= 0)");
    DI2P_CHECK_ARG(P >= 0 && P <= MAX_PRIMS, "more than 32 primitives per frame");
    DI2P_CHECK_ARG(B <= 65535 && (long long)H0 * W0 < (1ll << 29), "B above 65535 or H0 * W0 above 2^29 - 1");
    DI2P_CHECK_ARG(max_range > 0.0 && max_range < 1e300, "max_range must be a positive number");
    const long long HW = (long long)H0 * W0;
    DI2P_CHECK_ARG(B == 0 || HW == 0 || (count && K_raw && cam_to_world && image && (P == 0 || prims)), "null pointer");
    DI2P_CHECK_ARG((((uintptr_t)prims | (uintptr_t)K_raw | (uintptr_t)cam_to_world) & 7) == 0 && (((uintptr_t)image | (uintptr_t)depth | (uintptr_t)prim) & 3) == 0,
                   "prims, K_raw and cam_to_world must be 8-byte, image, depth and prim 4-byte aligned");
    if (B == 0 || HW == 0) return 0;
    hipLaunchKernelGGL(camera_kernel, dim3(di2p_cdiv(HW, BLOCK * PIX), B), dim3(BLOCK), 0, (hipStream_t)stream, prims, count, K_raw, cam_to_world, P, H0,
                       W0, max_range, image, depth, prim);
    DI2P_RETURN_LAUNCH();
}

extern "C" int di2p_world_render_scan(const double* prims, const int32_t* count, int B, int P, const double* elevation, const double* azimuth,
                                      const double* pose, int beams, int azimuths, double max_range, double dropout, double range_sigma,
                                      double intensity_sigma, unsigned long long seed, const unsigned long long* seed_dev, int frame0,
                                      float* out_points, int32_t* out_offsets, int32_t* out_count, void* workspace, void* stream) {
    DI2P_CHECK_ARG(B >= 0 && beams >= 0 && azimuths >= 0, "bad sizes (B, beams, azimuths >= 0)");
    DI2P_CHECK_ARG(P >= 0 && P <= MAX_PRIMS, "more than 32 primitives per frame");
    DI2P_CHECK_ARG(B <= 65535 && (long long)B * beams * azimuths < (1ll << 31) && (long long)beams * azimuths < (1ll << 31),
                   "B above 65535 or a capacity B * beams * azimuths above 2^31 - 1");
    DI2P_CHECK_ARG(max_range > 0.0 && max_range < 1e300 && dropout >= 0.0 && dropout <= 1.0 && finite_nonneg(range_sigma) && finite_nonneg(intensity_sigma),
                   "max_range > 0, 0 <= dropout <= 1 and sigmas >= 0 are needed");
    DI2P_CHECK_ARG(frame0 >= 0, "frame0 must be >= 0");
    const int R = beams * azimuths;
    DI2P_CHECK_ARG(B == 0 || (count && pose && out_offsets && out_count && (P == 0 || prims)), "null pointer");
    DI2P_CHECK_ARG(B == 0 || R == 0 || (elevation && azimuth && out_points && workspace), "null pointer (elevation, azimuth, out_points, workspace)");
    DI2P_CHECK_ARG((((uintptr_t)prims | (uintptr_t)elevation | (uintptr_t)azimuth | (uintptr_t)pose | (uintptr_t)seed_dev) & 7) == 0 &&
                       ((uintptr_t)out_points & 15) == 0 && ((uintptr_t)workspace & 255) == 0,
                   "the tables, pose and seed_dev must be 8-byte, out_points 16-byte, workspace 256-byte aligned");
    if (B == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const int parts = di2p_cdiv(R, BLOCK);
    const Layout L = layout(B, R);
    float4* rows = at<float4>(workspace, L.rows);
    unsigned long long* masks = at<unsigned long long>(workspace, L.mask);
    int *part_cnt = at<int>(workspace, L.part_cnt), *part_off = at<int>(workspace, L.part_off);
    if (R > 0)
        hipLaunchKernelGGL(rays_kernel, dim3(parts, B), dim3(BLOCK), 0, st, prims, count, elevation, azimuth, pose, P, beams, azimuths,
                           ScanOpt{max_range, dropout, range_sigma, intensity_sigma, seed, seed_dev, frame0}, rows, masks, part_cnt);
    hipLaunchKernelGGL(prefix_kernel, dim3(B), dim3(64), 0, st, parts, part_cnt, part_off, out_count);
    hipLaunchKernelGGL(scan_offsets_kernel, dim3(1), dim3(64), 0, st, B, out_count, out_offsets);
    if (R > 0) hipLaunchKernelGGL(write_kernel, dim3(parts, B), dim3(BLOCK), 0, st, R, rows, masks, part_off, out_offsets, (float4*)out_points);
    DI2P_RETURN_LAUNCH();
}

extern "C" long long di2p_world_profiles_workspace_bytes(int S_cap, int beams) {
    if (S_cap < 0 || beams < 0 || (long long)S_cap * beams >= (1ll << 31)) return 0;
    return (long long)playout((long long)S_cap * beams).total;
}

extern "C" int di2p_world_render_profiles(const double* prims, const int32_t* count, int B, int P, const int32_t* submap_offsets,
                                          const double* laser_to_world, const double* beam, int S_cap, int beams, double max_range, double dropout,
                                          double range_sigma, double reflectance_sigma, unsigned long long seed, const unsigned long long* seed_dev,
                                          int frame0, double* scan_xyr, int32_t* scan_offsets, int32_t* out_count, int32_t* status, void* workspace,
                                          void* stream) {
    DI2P_CHECK_ARG(B >= 0 && S_cap >= 0 && beams >= 0, "bad sizes (B, S_cap, beams >= 0)");
    DI2P_CHECK_ARG(P >= 0 && P <= MAX_PRIMS, "more than 32 primitives per sub-map");
    DI2P_CHECK_ARG(B <= 65535 && (long long)S_cap * beams < (1ll << 31), "B above 65535 or a capacity S_cap * beams above 2^31 - 1");
    DI2P_CHECK_ARG(max_range > 0.0 && max_range < 1e300 && dropout >= 0.0 && dropout <= 1.0 && finite_nonneg(range_sigma) && finite_nonneg(reflectance_sigma),
                   "max_range > 0, 0 <= dropout <= 1 and sigmas >= 0 are needed");
    DI2P_CHECK_ARG(frame0 >= 0 && (long long)frame0 + S_cap < (1ll << 31), "frame0 must be >= 0 and frame0 + S_cap below 2^31");
    DI2P_CHECK_ARG(scan_offsets && workspace && (S_cap == 0 || out_count), "null pointer (scan_offsets, out_count, workspace)");
    DI2P_CHECK_ARG(B == 0 || (count && submap_offsets && status && (P == 0 || prims)), "null pointer");
    const long long R = (long long)S_cap * beams;
    DI2P_CHECK_ARG(B == 0 || R == 0 || (laser_to_world && beam && scan_xyr), "null pointer (laser_to_world, beam, scan_xyr)");
    DI2P_CHECK_ARG((((uintptr_t)prims | (uintptr_t)laser_to_world | (uintptr_t)beam | (uintptr_t)seed_dev | (uintptr_t)scan_xyr) & 7) == 0 &&
                       ((uintptr_t)workspace & 255) == 0,
                   "the tables, laser_to_world, seed_dev and scan_xyr must be 8-byte, workspace 256-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int parts = di2p_cdiv(R, BLOCK), groups = di2p_cdiv(parts, GROUP);
    const PLayout L = playout(R);
    double* rows = at<double>(workspace, L.rows);
    unsigned long long* masks = at<unsigned long long>(workspace, L.mask);
    int *part_cnt = at<int>(workspace, L.part_cnt), *part_off = at<int>(workspace, L.part_off);
    int *group_cnt = at<int>(workspace, L.group_cnt), *group_off = at<int>(workspace, L.group_off), *head = at<int>(workspace, L.head);
    hipLaunchKernelGGL(accept_kernel, dim3(1), dim3(64), 0, st, submap_offsets, B, S_cap, status, head);
    if (parts > 0) {
        hipLaunchKernelGGL(profile_rays_kernel, dim3(parts), dim3(BLOCK), 0, st, prims, count, submap_offsets, head, laser_to_world, beam, P, beams,
                           ScanOpt{max_range, dropout, range_sigma, reflectance_sigma, seed, seed_dev, frame0}, rows, masks, part_cnt);
        hipLaunchKernelGGL(group_prefix_kernel, dim3(groups), dim3(64), 0, st, parts, part_cnt, part_off, group_cnt);
    }
    hipLaunchKernelGGL(top_prefix_kernel, dim3(1), dim3(64), 0, st, groups, group_cnt, group_off, head);
    hipLaunchKernelGGL(profile_offsets_kernel, dim3(di2p_cdiv(S_cap + 1, BLOCK)), dim3(BLOCK), 0, st, S_cap, beams, parts, masks, part_off, group_off, head,
                       scan_offsets, out_count);
    if (parts > 0) hipLaunchKernelGGL(profile_write_kernel, dim3(parts), dim3(BLOCK), 0, st, R, rows, masks, part_off, group_off, scan_xyr);
    DI2P_RETURN_LAUNCH();
}
