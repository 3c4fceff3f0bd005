// Frame preparation of the pose solver (included by solver.hip only): once per solve call the records of every frame are sorted by
// (label: 1 first, Hilbert cell of the (x, z) ground plane, point index), packed into 64-point clusters and given bounding boxes.
//
// Every STEP is one device function below; two sets of kernels call them and therefore agree bit for bit:
//   * prep_bounds / prep_hist / prep_scatter / prep_rank / prep_records_kernel: the shipped path, several workgroups per frame;
//   * prepare_kernel: one 1024-thread workgroup per frame -- the fallback for flagged frames (a bucket above 4096 keys: a degenerate scene),
//     whose bitonic network it alone holds, and the whole path behind the knobs solver_prep_single / solver_prep_bitonic.
// tests/test_gpu_solver.py compares the prepared data (counts, records, boxes) of the three paths byte for byte.
#pragma once

namespace {

// Packed, front-filtered point records: ONE aligned vector load per point per sweep.
//   PT=float : float4 {x, y, z, label bits}            (16 B)
//   PT=double: {double x, y, z; long long label}       (32 B)
// Points whose label is not 0/1 (incl. the -1 the front filter writes) are dropped here once, in stable
// order, so the hot sweeps never see them (registration.cpp:87-125 skips them per residual block).
template <typename PT> struct Rec;
template <> struct __attribute__((aligned(16))) Rec<float> { float x, y, z; int lab; };
template <> struct __attribute__((aligned(16))) Rec<double> { double x, y, z; long long lab; };

// Consecutive groups of CL = 64 sorted records of one label form a CLUSTER with an axis-aligned bounding box.  The solver's sweeps test each
// box against the five planes of the camera frustum of the current iterate and classify the points of a cluster individually only when the
// box touches a plane (see sweep_clusters).
constexpr int CL = 64;
// axis-aligned bounds of a cluster (centre, half extents) in fp32, rounded OUTWARD: the fp32 box contains every point of the cluster
// rxz / r3: the largest ground-plane radius sqrt(x^2 + z^2) and the largest norm of a point of the cluster, rounded UP -- how far a point of
// the cluster can move per radian of iterate rotation (2-D solver: about the y axis; 3-D: any axis), see the classification cache.
struct __attribute__((aligned(16))) Box { float cx, cy, cz, hx, hy, hz, rxz, r3; };

// Index of cell (x, y) of a 1024 x 1024 grid along the Hilbert curve.  Unlike the Z-order (Morton) curve it has no jumps: 64 consecutive
// records always form one connected patch of the ground plane, so the cluster boxes are tighter (modelled on the config-2 scene,
// tools/model_cluster_keys.py: 145 instead of 168 of 321 clusters per frame touch a frustum plane).
__device__ __forceinline__ unsigned hilbert10(unsigned x, unsigned y) {
    unsigned d = 0;
#pragma unroll
    for (unsigned s = 512; s > 0; s >>= 1) {
        const unsigned rx = (x & s) ? 1u : 0u, ry = (y & s) ? 1u : 0u;
        d += s * s * ((3u * rx) ^ ry);
        if (ry == 0) {
            if (rx == 1) { x = s - 1 - x; y = s - 1 - y; }
            const unsigned t = x; x = y; y = t;
        }
    }
    return d;
}

// Wave-wide reduction of 1, 2 or 4 registers at once by DPP: four joins inside rows of 16 lanes, then row_bcast15 / row_bcast31 carry the row
// results into lane 63, which wave_lane63 reads back as a scalar.  One asm block per reduction: hipcc expands fminf(v, dpp(v)) into mov +
// mov_dpp + canonicalise + min.  A DPP read needs two wait states after a VALU write of the same register: with four registers the three other
// joins cover them, with fewer the FILL (an s_nop) does.
//   DI2P_DPP_LADDER(JOIN, OP, FILL): JOIN = DI2P_DPP_J1 / J2 / J4 (registers %0 .. %3), OP = the _dpp opcode, FILL = text after every join
#define DI2P_DPP_J1(OP, CTRL) OP " %0, %0, %0 " CTRL "\n\t"
#define DI2P_DPP_J2(OP, CTRL) DI2P_DPP_J1(OP, CTRL) OP " %1, %1, %1 " CTRL "\n\t"
#define DI2P_DPP_J4(OP, CTRL) DI2P_DPP_J2(OP, CTRL) OP " %2, %2, %2 " CTRL "\n\t" OP " %3, %3, %3 " CTRL "\n\t"
#define DI2P_DPP_LADDER(JOIN, OP, FILL)                              \
    "s_nop 1\n\t"                                                    \
    JOIN(OP, "quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf") FILL  \
    JOIN(OP, "quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf") FILL  \
    JOIN(OP, "row_half_mirror row_mask:0xf bank_mask:0xf") FILL      \
    JOIN(OP, "row_mirror row_mask:0xf bank_mask:0xf") FILL           \
    JOIN(OP, "row_bcast:15 row_mask:0xa bank_mask:0xf") FILL         \
    JOIN(OP, "row_bcast:31 row_mask:0xc bank_mask:0xf") FILL
__device__ __forceinline__ float wave_lane63(float v) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63)); }

// Wave-wide min / max of four floats (v_min / v_max drop NaNs like fmin / fmax).
__device__ __forceinline__ void wave_min4_f32(float& a, float& b, float& c, float& d) {
    asm volatile(DI2P_DPP_LADDER(DI2P_DPP_J4, "v_min_f32_dpp", "") : "+v"(a), "+v"(b), "+v"(c), "+v"(d));
    a = wave_lane63(a); b = wave_lane63(b); c = wave_lane63(c); d = wave_lane63(d);
}
__device__ __forceinline__ void wave_max4_f32(float& a, float& b, float& c, float& d) {
    asm volatile(DI2P_DPP_LADDER(DI2P_DPP_J4, "v_max_f32_dpp", "") : "+v"(a), "+v"(b), "+v"(c), "+v"(d));
    a = wave_lane63(a); b = wave_lane63(b); c = wave_lane63(c); d = wave_lane63(d);
}

// ---------------------------------------------------------------------------------------------- the steps
constexpr int PREP_NBK = 2048;        // buckets of the counting sort: the top 11 key bits (label + 32 x 32 grid of the Hilbert curve)
constexpr int PREP_G = 8;             // workgroups per frame of the slice kernels (PREP_NBK % PREP_G == 0)
constexpr int PREP_CPW = 4;           // clusters per wavefront of prep_records_kernel (their keys, then their gathers, in flight together; parked in lanes 0..3, finished lane-parallel)
struct PrepWs { float* partial; int* cntg; int* bases; int* flag; };      // [F][G][8] | [F][G][NBK] bucket counts per slice | [F][NBK + 1] | [F]

// Ground-plane bounding box of the points with label 0 / 1 and the two label counts.  Minima, maxima and integer sums are exact, so the result
// does not depend on how the points are split among threads, waves and workgroups.
struct PrepBounds { float mnx, mxx, mnz, mxz; int n1, n0; };
__device__ __forceinline__ void prep_bounds_join(PrepBounds& b, const PrepBounds& o) {
    b.mnx = fminf(b.mnx, o.mnx); b.mxx = fmaxf(b.mxx, o.mxx); b.mnz = fminf(b.mnz, o.mnz); b.mxz = fmaxf(b.mxz, o.mxz);
    b.n1 += o.n1; b.n0 += o.n0;
}
// ... of the points first, first + stride, ... < end, reduced over the wave (every lane returns the wave's result)
template <typename PT>
__device__ __forceinline__ PrepBounds prep_wave_bounds(const PT* px, const PT* pz, const int* lab, int first, int end, int stride) {
    PrepBounds b = {__builtin_inff(), -__builtin_inff(), __builtin_inff(), -__builtin_inff(), 0, 0};
    for (int n = first; n < end; n += stride) {
        const int l = lab[n];
        if (l == 0 || l == 1) {
            const float x = (float)px[n], z = (float)pz[n];
            b.mnx = fminf(b.mnx, x); b.mxx = fmaxf(b.mxx, x); b.mnz = fminf(b.mnz, z); b.mxz = fmaxf(b.mxz, z);
            b.n1 += l == 1; b.n0 += l == 0;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        PrepBounds t;
        t.mnx = __shfl_xor(b.mnx, o); t.mxx = __shfl_xor(b.mxx, o); t.mnz = __shfl_xor(b.mnz, o); t.mxz = __shfl_xor(b.mxz, o);
        t.n1 = __shfl_xor(b.n1, o); t.n0 = __shfl_xor(b.n0, o);
        prep_bounds_join(b, t);
    }
    return b;
}
// the slice kernels park their partial bounds in the workspace: 8 words per (frame, slice), the six of PrepBounds in front
__device__ __forceinline__ PrepBounds* prep_partial(const PrepWs& w, int f, int g) {
    return reinterpret_cast<PrepBounds*>(w.partial + ((long long)f * PREP_G + g) * 8);
}

// What the sort key needs of a frame: the origin and the scale of its 1024 x 1024 grid (0 for an empty, degenerate or unbounded extent), the counts
struct PrepFrame { float mnx, mnz, scale; int n1, n0; };
__device__ __forceinline__ PrepFrame prep_frame_of(const PrepBounds& b) {
    const float ext = fmaxf(b.mxx - b.mnx, b.mxz - b.mnz);
    PrepFrame r;
    r.mnx = b.mnx; r.mnz = b.mnz; r.scale = (ext > 0.0f && ext < __builtin_inff()) ? 1023.0f / ext : 0.0f; r.n1 = b.n1; r.n0 = b.n0;
    return r;
}
__device__ __forceinline__ PrepFrame prep_frame(const PrepWs& w, int f) {       // from the G partial results of the slice kernels
    PrepBounds b = {__builtin_inff(), -__builtin_inff(), __builtin_inff(), -__builtin_inff(), 0, 0};
    for (int g = 0; g < PREP_G; ++g) prep_bounds_join(b, *prep_partial(w, f, g));
    return prep_frame_of(b);
}
__device__ __forceinline__ void prep_slice(int N, int g, int& lo, int& hi) {
    const int S = ((N + PREP_G - 1) / PREP_G + 255) & ~255;
    lo = min(g * S, N); hi = min(lo + S, N);
}

// Sort key of point n: [label != 1][20-bit Hilbert index of the cell] << 32 | n (unique); points with other labels get ~0 (they sort to the end)
template <typename PT>
__device__ __forceinline__ unsigned long long prep_key(const PT* px, const PT* pz, const int* lab, int n, const PrepFrame& fr) {
    const int l = lab[n];
    const float qx = fminf(fmaxf(((float)px[n] - fr.mnx) * fr.scale, 0.0f), 1023.0f);
    const float qz = fminf(fmaxf(((float)pz[n] - fr.mnz) * fr.scale, 0.0f), 1023.0f);
    const unsigned m = hilbert10((unsigned)qx, (unsigned)qz);
    const unsigned long long k = ((unsigned long long)((l == 1 ? 0u : 1u << 20) | m) << 32) | (unsigned)n;
    return (l == 0 || l == 1) ? k : ~0ull;
}
__device__ __forceinline__ int prep_bucket(unsigned long long key) { return (int)(key >> 42); }

// Exclusive scan of the PREP_NBK bucket totals by 1024 threads: thread t brings the totals a0, a1 of buckets 2t and 2t + 1 and gets the offset
// of bucket 2t (bucket 2t + 1 starts a0 later; thread 1023 knows the grand total: + a0 + a1).  Wave scan + the 16 wave totals through `wtot`
// (16 ints of LDS); contains one barrier.
__device__ __forceinline__ int prep_scan_buckets(int a0, int a1, int* wtot) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int v = a0 + a1;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(v, o); if (lane >= o) v += u; }
    if (lane == 63) wtot[wave] = v;
    __syncthreads();
    int woff = 0;
    for (int w = 0; w < wave; ++w) woff += wtot[w];
    return woff + v - (a0 + a1);
}

// Final position of key k of the bucket-scattered list `keys`: its bucket's offset + its rank inside the bucket, by counting
// (#{j : key_j < key}; the keys are unique).  One THREAD per key: neighbouring threads sit in the same bucket and read the same addresses
// (broadcast).  `bases`: the PREP_NBK + 1 bucket offsets.
__device__ __forceinline__ int prep_sorted_pos(const unsigned long long* __restrict__ keys, const int* bases, unsigned long long k) {
    const int bk = prep_bucket(k), b0 = bases[bk], c = bases[bk + 1] - b0;
    int rank = 0;
    for (int j = 0; j < c; j += 8) {            // eight loads in flight (clamped; the duplicates do not count)
        unsigned long long q[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) q[u] = keys[b0 + min(j + u, c - 1)];
#pragma unroll
        for (int u = 0; u < 8; ++u) rank += (j + u < c && q[u] < k) ? 1 : 0;
    }
    return b0 + rank;
}

// Records in sorted order, every label block CLUSTER-ALIGNED: label-1 block [0, n1), padded to nc1 * CL, label-0 block [nc1 * CL, nc1 * CL + n0),
// padded to (nc1 + nc0) * CL -- cluster c is always the records [c * CL, c * CL + CL), all of them addressable (the padding repeats the block's
// last record; the sweeps mask those lanes out).  Position in the sorted key list of record i, and whether i is a record or padding:
__device__ __forceinline__ int prep_record_key(int i, int n1, int n0, int nc1) {
    return i < nc1 * CL ? min(i, n1 - 1) : n1 + min(i - nc1 * CL, n0 - 1);
}
__device__ __forceinline__ bool prep_record_valid(int i, int n1, int n0, int nc1) { return i < (i < nc1 * CL ? n1 : nc1 * CL + n0); }
template <typename PT>
__device__ __forceinline__ Rec<PT> prep_gather(const PT* px, const PT* py, const PT* pz, const int* lab, int n) {
    Rec<PT> r;
    r.x = px[n]; r.y = py[n]; r.z = pz[n]; r.lab = lab[n];
    return r;
}

// What a box needs of its cluster, wave-uniform, from one record per lane (`valid`: the lane holds a record, not padding): per-axis minima
// and maxima, the two radii rounded UP to fp32, and whether a coordinate is NaN.
struct ClusterRed { double lo[3], hi[3]; float rxz, r3; bool nan; };
__device__ __forceinline__ float prep_round_up(double v) { return (float)(v * (1.0 + 1e-6)) + 1e-30f; }      // grown by 1e-6 (>> 2^-24) before the rounding
template <typename PT>
__device__ __forceinline__ ClusterRed prep_cluster_reduce(const Rec<PT>& r, bool valid) {
    const double x = valid ? (double)r.x : 0.0, y = valid ? (double)r.y : 0.0, z = valid ? (double)r.z : 0.0;
    ClusterRed c;
#pragma unroll
    for (int a = 0; a < 3; ++a) { const double v = a == 0 ? x : a == 1 ? y : z; c.lo[a] = valid ? v : __builtin_inf(); c.hi[a] = valid ? v : -__builtin_inf(); }
    double rxz = valid ? x * x + z * z : 0.0, r3 = valid ? x * x + y * y + z * z : 0.0;
    if (sizeof(PT) == 4) {
        // fp32 records: the coordinates ARE floats, so the eight reductions run on fp32 values by DPP (no LDS round trips) and give the
        // very same box -- min / max of floats are exact, and sqrt / scaling / rounding to float are monotone, so the radii may be
        // rounded per lane before the maximum (round 3: 100 ds_bpermute with their latencies per cluster)
        float l0 = (float)c.lo[0], l1 = (float)c.lo[1], l2 = (float)c.lo[2], h0 = (float)c.hi[0], h1 = (float)c.hi[1], h2 = (float)c.hi[2];
        float pad0 = __builtin_inff(), pad1 = 0.0f;
        c.rxz = prep_round_up(sqrt(rxz)); c.r3 = prep_round_up(sqrt(r3));
        wave_min4_f32(l0, l1, l2, pad0);
        wave_max4_f32(h0, h1, h2, pad1);
        float pad2 = 0.0f, pad3 = 0.0f;
        wave_max4_f32(c.rxz, c.r3, pad2, pad3);
        c.lo[0] = l0; c.lo[1] = l1; c.lo[2] = l2; c.hi[0] = h0; c.hi[1] = h1; c.hi[2] = h2;
    } else {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1)
#pragma unroll
            for (int a = 0; a < 3; ++a) { c.lo[a] = fmin(c.lo[a], __shfl_xor(c.lo[a], o)); c.hi[a] = fmax(c.hi[a], __shfl_xor(c.hi[a], o)); }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { rxz = fmax(rxz, __shfl_xor(rxz, o)); r3 = fmax(r3, __shfl_xor(r3, o)); }
        c.rxz = prep_round_up(sqrt(rxz)); c.r3 = prep_round_up(sqrt(r3));
    }
    // a NaN coordinate must poison the box (fmin / fmax drop it): such clusters are always classified per point
    c.nan = __any(valid && !(x == x && y == y && z == z)) != 0;
    return c;
}
// The box of a reduced cluster: centre, half extents measured from the ROUNDED centre and rounded up (centre +- half extent contains lo and hi)
__device__ __forceinline__ Box prep_box(const ClusterRed& m) {
    Box bx;
    float* bc = &bx.cx;
    float* bh = &bx.hx;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double cd = 0.5 * (m.lo[a] + m.hi[a]);
        const float cf = (float)cd;
        const double hd = fmax(m.hi[a] - (double)cf, (double)cf - m.lo[a]);
        bc[a] = cf;
        bh[a] = prep_round_up(hd);
    }
    if (m.nan) bx.hx = __builtin_nanf("");
    bx.rxz = m.rxz;
    bx.r3 = m.r3;
    return bx;
}

// Frame header: the counts, and the frame's NORMALISED frustum-plane coefficients in fp32 (see Pre32) -- they depend on the camera only, so every
// sweep of every hypothesis reads them back with scalar loads instead of re-deriving them (six conversions, four divisions, eight products per
// wave and sweep)
__device__ __forceinline__ void prep_header(int f, int n1, int n0, int* __restrict__ counts, const double* __restrict__ Kmat, double H, double W,
                                            float* __restrict__ camf_all) {
    counts[4 * f] = n1; counts[4 * f + 1] = n0; counts[4 * f + 2] = (n1 + CL - 1) / CL; counts[4 * f + 3] = (n0 + CL - 1) / CL;
    const double* Kf = Kmat + (long long)f * 9;
    float* cf = camf_all + (long long)f * 8;
    const float fx = (float)Kf[0], cx = (float)Kf[2], wcx = (float)((W - 1.0) - Kf[2]), fy = (float)Kf[4], cy = (float)Kf[5], hcy = (float)((H - 1.0) - Kf[5]);
    const float iL = 1.0f / (fabsf(fx) + fabsf(cx)), iR = 1.0f / (fabsf(fx) + fabsf(wcx));
    const float iT = 1.0f / (fabsf(fy) + fabsf(cy)), iB = 1.0f / (fabsf(fy) + fabsf(hcy));
    cf[0] = fx * iL; cf[1] = cx * iL; cf[2] = fx * iR; cf[3] = wcx * iR;
    cf[4] = fy * iT; cf[5] = cy * iT; cf[6] = fy * iB; cf[7] = hcy * iB;
}

// ---------------------------------------------------------------------------------------------- the multi-workgroup path
// Five launches, G workgroups per frame each:
//   prep_bounds_kernel   partial ground-plane bounds + label counts per slice; clears the frame's flag
//   prep_hist_kernel     keys of the slice (stored), bucket counts of the slice (LDS atomics) -> [frame][slice][bucket]
//   prep_scatter_kernel  bucket offsets = exclusive scan of the summed counts (every workgroup, into LDS); a slice's keys go to
//                        offset[bucket] + (counts of the slices before it) + an LDS cursor: no global atomics
//   prep_rank_kernel     one thread per key: rank inside its bucket by counting -> sorted keys
//   prep_records_kernel  one wavefront per cluster: gathers its 64 records, writes them and reduces the box FROM ITS REGISTERS
// The keys are nearly uniform over their 21 significant bits, so the buckets hold ~10-25 keys.  A frame with a bucket above 4096 keys is flagged
// by the scatter step, skipped by the last two and prepared by prepare_kernel (launched behind them with `only_flagged`).
template <typename PT>
__global__ __launch_bounds__(256) void prep_bounds_kernel(const PT* __restrict__ points, const int* __restrict__ labels, int N, PrepWs w) {
    __shared__ PrepBounds s_b[4];
    const int f = blockIdx.x / PREP_G, g = blockIdx.x % PREP_G, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const PT* px = points + (long long)f * 3 * N;
    const PT* pz = px + 2 * (long long)N;
    const int* lab = labels + (long long)f * N;
    if (g == 0 && tid == 0) w.flag[f] = 0;
    int lo, hi;
    prep_slice(N, g, lo, hi);
    PrepBounds b = prep_wave_bounds(px, pz, lab, lo + tid, hi, 256);
    if (lane == 0) s_b[wave] = b;
    __syncthreads();
    if (tid == 0) {
        for (int v = 1; v < 4; ++v) prep_bounds_join(b, s_b[v]);
        *prep_partial(w, f, g) = b;
    }
}

template <typename PT>
__global__ __launch_bounds__(256) void prep_hist_kernel(const PT* __restrict__ points, const int* __restrict__ labels, int N, int P,
                                                        unsigned long long* __restrict__ keys_all, PrepWs w) {
    __shared__ int cnt[PREP_NBK];
    const int f = blockIdx.x / PREP_G, g = blockIdx.x % PREP_G, tid = threadIdx.x;
    const PT* px = points + (long long)f * 3 * N;
    const PT* pz = px + 2 * (long long)N;
    const int* lab = labels + (long long)f * N;
    unsigned long long* raw = keys_all + (long long)f * 2 * P + P;         // the second key buffer holds the unsorted keys until the ranking
    const PrepFrame fr = prep_frame(w, f);
    for (int i = tid; i < PREP_NBK; i += 256) cnt[i] = 0;
    __syncthreads();
    int lo, hi;
    prep_slice(N, g, lo, hi);
    for (int n = lo + tid; n < hi; n += 256) {
        const unsigned long long k = prep_key(px, pz, lab, n, fr);
        raw[n] = k;
        if (k != ~0ull) atomicAdd(&cnt[prep_bucket(k)], 1);
    }
    __syncthreads();
    for (int i = tid; i < PREP_NBK; i += 256) w.cntg[((long long)f * PREP_G + g) * PREP_NBK + i] = cnt[i];
}

__global__ __launch_bounds__(1024) void prep_scatter_kernel(int N, int P, unsigned long long* __restrict__ keys_all, PrepWs w) {
    __shared__ int cur[PREP_NBK];           // where the slice's next key of a bucket goes
    __shared__ int s_w[16];
    const int f = blockIdx.x / PREP_G, g = blockIdx.x % PREP_G, tid = threadIdx.x;
    unsigned long long* keys = keys_all + (long long)f * 2 * P;
    const unsigned long long* raw = keys + P;
    {
        const int* cg = w.cntg + (long long)f * PREP_G * PREP_NBK;
        int a0 = 0, a1 = 0, before0 = 0, before1 = 0;       // totals of the thread's two buckets; the keys of the slices before this one
#pragma unroll
        for (int q = 0; q < PREP_G; ++q) {
            const int c0 = cg[q * PREP_NBK + 2 * tid], c1 = cg[q * PREP_NBK + 2 * tid + 1];
            a0 += c0; a1 += c1;
            before0 += q < g ? c0 : 0; before1 += q < g ? c1 : 0;
        }
        const int excl = prep_scan_buckets(a0, a1, s_w);
        cur[2 * tid] = excl + before0; cur[2 * tid + 1] = excl + a0 + before1;
        if (g == 0) {
            int* bases = w.bases + (long long)f * (PREP_NBK + 1);
            bases[2 * tid] = excl; bases[2 * tid + 1] = excl + a0;
            if (tid == 1023) bases[PREP_NBK] = excl + a0 + a1;
        }
        if (a0 > 4096 || a1 > 4096) w.flag[f] = 1;            // a degenerate scene: the frame goes to prepare_kernel's bitonic network
    }
    __syncthreads();
    int lo, hi;
    prep_slice(N, g, lo, hi);
    for (int n = lo + tid; n < hi; n += 1024) {
        const unsigned long long k = raw[n];
        if (k != ~0ull) keys[atomicAdd(&cur[prep_bucket(k)], 1)] = k;
    }
}

__global__ __launch_bounds__(256) void prep_rank_kernel(int P, unsigned long long* __restrict__ keys_all, PrepWs w) {
    const int f = blockIdx.y;
    if (w.flag[f]) return;
    const int* bases = w.bases + (long long)f * (PREP_NBK + 1);
    const unsigned long long* keys = keys_all + (long long)f * 2 * P;
    unsigned long long* keys2 = keys_all + (long long)f * 2 * P + P;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= bases[PREP_NBK]) return;
    const unsigned long long k = keys[p];
    keys2[prep_sorted_pos(keys, bases, k)] = k;
}

// One wavefront per cluster holds the cluster's 64 records in its lanes -- written out and reduced from registers; PREP_CPW clusters per
// wavefront, their reduced values parked in lanes 0 .. PREP_CPW - 1, which then finish their own boxes.
template <typename PT>
__global__ __launch_bounds__(256) void prep_records_kernel(const PT* __restrict__ points, const int* __restrict__ labels, int N, int P, int NCMAX,
                                                           const unsigned long long* __restrict__ keys_all, Rec<PT>* __restrict__ packed,
                                                           Box* __restrict__ boxes_all, int* __restrict__ counts, const double* __restrict__ Kmat,
                                                           double H, double W, float* __restrict__ camf_all, PrepWs w) {
    const int f = blockIdx.y;
    if (w.flag[f]) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const PT* px = points + (long long)f * 3 * N;
    const PT* py = px + N;
    const PT* pz = px + 2 * (long long)N;
    const int* lab = labels + (long long)f * N;
    const unsigned long long* skeys = keys_all + (long long)f * 2 * P + P;
    Rec<PT>* out = packed + (long long)f * (N + 2 * CL);
    Box* boxes = boxes_all + (long long)f * NCMAX;
    const PrepFrame fr = prep_frame(w, f);
    const int n1 = fr.n1, n0 = fr.n0;
    const int nc1 = (n1 + CL - 1) / CL, nc0 = (n0 + CL - 1) / CL, nct = nc1 + nc0;
    if (blockIdx.x == 0 && tid == 0) prep_header(f, n1, n0, counts, Kmat, H, W, camf_all);
    const int c_first = (blockIdx.x * 4 + wave) * PREP_CPW;
    if (c_first >= nct) return;              // wave-uniform
    // the PREP_CPW clusters' keys, then their gathers, are requested together (a cluster alone is a chain of two dependent round trips)
    int nn_all[PREP_CPW];
#pragma unroll
    for (int tt = 0; tt < PREP_CPW; ++tt)
        nn_all[tt] = (int)(unsigned)(skeys[prep_record_key(min(c_first + tt, nct - 1) * CL + lane, n1, n0, nc1)] & 0xffffffffull);
    Rec<PT> r_all[PREP_CPW];
#pragma unroll
    for (int tt = 0; tt < PREP_CPW; ++tt) r_all[tt] = prep_gather(px, py, pz, lab, nn_all[tt]);
    ClusterRed mine = {};
#pragma unroll
    for (int tt = 0; tt < PREP_CPW; ++tt) {
        if (c_first + tt >= nct) break;          // wave-uniform
        const int i = (c_first + tt) * CL + lane;
        out[i] = r_all[tt];
        const ClusterRed red = prep_cluster_reduce(r_all[tt], prep_record_valid(i, n1, n0, nc1));
        if (lane == tt) mine = red;
    }
    const int c = c_first + lane;
    if (lane < PREP_CPW && c < nct) boxes[c] = prep_box(mine);
}

// ---------------------------------------------------------------------------------------------- the single-workgroup path
// One 1024-thread workgroup per frame runs the same five steps.  only_flagged != nullptr: the launch is the FALLBACK behind the kernels above
// and leaves every frame alone whose flag is not set.  force_bitonic: sort with the bitonic network whatever the buckets hold.
template <typename PT>
__global__ __launch_bounds__(1024) void prepare_kernel(const PT* __restrict__ points, const int* __restrict__ labels, int N, int P,
                                                       int NCMAX, unsigned long long* __restrict__ keys_all,
                                                       Rec<PT>* __restrict__ packed, Box* __restrict__ boxes_all,
                                                       int* __restrict__ counts, int force_bitonic, const double* __restrict__ Kmat, double H,
                                                       double W, float* __restrict__ camf_all, const int* __restrict__ only_flagged) {
    if (only_flagged && only_flagged[blockIdx.x] == 0) return;
    constexpr int CH = 8192;                       // LDS chunk (64 KB)
    __shared__ unsigned long long chunk[CH];
    __shared__ PrepBounds s_b[16];
    __shared__ int s_flag;                         // fall back to the bitonic network
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const PT* px = points + (long long)f * 3 * N;
    const PT* py = px + N;
    const PT* pz = px + 2 * (long long)N;
    const int* lab = labels + (long long)f * N;
    unsigned long long* keys = keys_all + (long long)f * 2 * P;      // two buffers of P keys: scattered / ranked (the bitonic network sorts the first in place)
    unsigned long long* keys2 = keys + P;
    Rec<PT>* out = packed + (long long)f * (N + 2 * CL);      // frame stride: N records + the padding of the two label blocks
    Box* boxes = boxes_all + (long long)f * NCMAX;

    // 1. ground-plane bounds of the valid points, label counts: every thread combines the 16 wave results in the same order
    PrepBounds b = prep_wave_bounds(px, pz, lab, tid, N, 1024);
    if (lane == 0) s_b[wave] = b;
    __syncthreads();
    b = s_b[0];
    for (int w = 1; w < 16; ++w) prep_bounds_join(b, s_b[w]);
    const PrepFrame fr = prep_frame_of(b);
    const int n1 = fr.n1, n0 = fr.n0;

    // 2. sort keys; past N: ~0.  The loads are unconditional from a clamped index, so that the 4-way unrolled passes below keep them all in flight
    auto key_of = [&](int n) -> unsigned long long {
        const unsigned long long k = prep_key(px, pz, lab, min(n, N - 1), fr);
        return n < N ? k : ~0ull;
    };
    auto each_key = [&](auto&& body) {                    // one pass over the frame's valid keys, four per thread and trip
        for (int n = tid; n < N; n += 4096) {
            unsigned long long k4[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) k4[u] = key_of(n + 1024 * u);
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (k4[u] != ~0ull) body(k4[u]);
        }
    };
    // 3a. counting sort on the bucket (LDS atomics), then every key is ranked inside its bucket, which puts it at its final position in the
    //     second key buffer.  A bucket above 4096 keys sends the frame to the bitonic network of 3b: the SAME total order either way.
    int* cntv = reinterpret_cast<int*>(chunk);            // [NBK] bucket counts, then fill cursors
    int* basev = cntv + PREP_NBK;                         // [NBK + 1] exclusive offsets
    int* wtot = basev + PREP_NBK + 1;                     // [16] wave totals of the scan
    bool sorted = false;
    if (!force_bitonic) {
        for (int i = tid; i < PREP_NBK; i += 1024) cntv[i] = 0;
        if (tid == 0) s_flag = 0;
        __syncthreads();
        each_key([&](unsigned long long k) { atomicAdd(&cntv[prep_bucket(k)], 1); });
        __syncthreads();
        {
            const int a0 = cntv[2 * tid], a1 = cntv[2 * tid + 1];
            const int excl = prep_scan_buckets(a0, a1, wtot);
            basev[2 * tid] = excl; basev[2 * tid + 1] = excl + a0;
            if (tid == 1023) basev[PREP_NBK] = excl + a0 + a1;
            if (a0 > 4096 || a1 > 4096) s_flag = 1;
        }
        __syncthreads();
        for (int i = tid; i < PREP_NBK; i += 1024) cntv[i] = 0;
        __syncthreads();
        each_key([&](unsigned long long k) { const int bk = prep_bucket(k); keys[basev[bk] + atomicAdd(&cntv[bk], 1)] = k; });
        __syncthreads();
        sorted = s_flag == 0;
        if (sorted) {
            const int nv = basev[PREP_NBK];
            for (int p = tid; p < nv; p += 1024) {
                const unsigned long long k = keys[p];
                keys2[prep_sorted_pos(keys, basev, k)] = k;
            }
        }
        __syncthreads();
    }
    if (!sorted) {      // workgroup-uniform
        // 3b. bitonic sort, ascending, of P keys (a power of two): data-independent network, 64 KB LDS chunks with the wide strides done in
        //     the (L2-resident) global buffer
        for (int n = tid; n < P; n += 1024) keys[n] = key_of(n);
        __syncthreads();
        const int CHe = P < CH ? P : CH;
        const int nchunks = P / CHe;
        auto chunk_stages = [&](int base, int k, int j_first) {     // stages j_first, j_first/2, ..., 1 of merge size k on the LDS chunk
            for (int j = j_first; j > 0; j >>= 1) {
                for (int t = tid; t < CHe / 2; t += 1024) {
                    const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                    const bool up = ((base + i) & k) == 0;
                    const unsigned long long a = chunk[i], b = chunk[i + j];
                    if ((a > b) == up) { chunk[i] = b; chunk[i + j] = a; }
                }
                __syncthreads();
            }
        };
        auto each_chunk = [&](auto&& body) {                        // every chunk through LDS: load, body(base), store
            for (int c = 0; c < nchunks; ++c) {
                const int base = c * CHe;
                for (int i = tid; i < CHe; i += 1024) chunk[i] = keys[base + i];
                __syncthreads();
                body(base);
                for (int i = tid; i < CHe; i += 1024) keys[base + i] = chunk[i];
                __syncthreads();
            }
        };
        each_chunk([&](int base) { for (int k = 2; k <= CHe; k <<= 1) chunk_stages(base, k, k >> 1); });
        for (int k = CHe << 1; k <= P; k <<= 1) {
            for (int j = k >> 1; j >= CHe; j >>= 1) {
                for (int t = tid; t < P / 2; t += 1024) {
                    const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                    const bool up = (i & k) == 0;
                    const unsigned long long a = keys[i], b = keys[i + j];
                    if ((a > b) == up) { keys[i] = b; keys[i + j] = a; }
                }
                __syncthreads();
            }
            each_chunk([&](int base) { chunk_stages(base, k, CHe >> 1); });
        }
    }
    // 4. records in sorted order
    const int nc1 = (n1 + CL - 1) / CL, nc0 = (n0 + CL - 1) / CL, nct = nc1 + nc0;
    const unsigned long long* skeys = sorted ? keys2 : keys;
    const int nrec = nct * CL;
    for (int i0 = tid; i0 < nrec; i0 += 4096) {          // four records per trip: key loads, then the 16 gathers, all in flight together
        int nn[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) nn[u] = (int)(unsigned)(skeys[prep_record_key(min(i0 + 1024 * u, nrec - 1), n1, n0, nc1)] & 0xffffffffull);
        Rec<PT> r4[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) r4[u] = prep_gather(px, py, pz, lab, nn[u]);
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (i0 + 1024 * u < nrec) out[i0 + 1024 * u] = r4[u];
    }
    __syncthreads();

    // 5. boxes: one wavefront REDUCES a cluster (its 64 records), the reduced values are parked in one lane, and after up to 64 clusters every
    //    lane finishes its own box (~60 fp64 instructions that would otherwise run once per cluster, serially)
    for (int t0 = 0; wave + 16 * t0 < nct; t0 += 64) {
        ClusterRed mine = {};
        for (int tt = 0; tt < 64 && wave + 16 * (t0 + tt) < nct; ++tt) {
            const int i = (wave + 16 * (t0 + tt)) * CL + lane;
            const bool valid = prep_record_valid(i, n1, n0, nc1);
            Rec<PT> r = {};
            if (valid) r = out[i];
            const ClusterRed red = prep_cluster_reduce(r, valid);
            if (lane == tt) mine = red;
        }
        const int c = wave + 16 * (t0 + lane);
        if (c < nct) boxes[c] = prep_box(mine);
    }
    if (tid == 0) prep_header(f, n1, n0, counts, Kmat, H, W, camf_all);
}

}  // namespace
