// Batches that are ragged on two levels (batch entry -> units -> rows): what the count / prefix / write split of submap.hip (sub-map ->
// profiles -> rows) and sweeps.hip (frame -> sweeps -> rows) has in common.  Included by those two files (and by world.hip, for wave_prefix
// and the workspace helpers); everything is in the anonymous namespace, so each of them gets its own offsets_kernel.  Integer code throughout.
//   check_offsets2   (device, wave-wide) the acceptance of one entry's offsets on both levels
//   wave_prefix      (device, wave-wide) chunked exclusive prefix over a range of int counts, 64-bit lanes, clamped at 2^31 - 1
//   frame_of         (device) the entry a row or unit of a non-decreasing offset table belongs to, by binary search
//   offsets_kernel   one wave: exclusive prefix over the entries' totals, the final status
// and the status codes, the workspace helpers and wave_id.
#pragma once
#include "common.h"

namespace {

constexpr int MAX_FRAME_POINTS = 1 << 20;
constexpr int ST_OK = 0, ST_TOO_MANY = 1, ST_OFFSETS = 3, ST_EMPTY = 4;

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// Cuts a workspace into 256-byte aligned pieces: take(bytes) is the offset of the next piece, o the size so far.
struct Take {
    size_t o = 0;
    size_t operator()(size_t bytes) { const size_t r = o; o = align256(o + bytes); return r; }
};

template <class T> T* at(void* ws, size_t off) { return (T*)((char*)ws + off); }

__device__ __forceinline__ int wave_id() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

// Entry b is accepted iff outer_off[0 .. b+1] is a non-decreasing sequence in [0, N_cap] that starts at 0 (accepted entries therefore never
// share a unit) and every unit of it has 0 <= inner_off[s] <= inner_off[s+1] <= P_cap.  Called by all 64 lanes of a wave; s0 = s1 = 0 for a
// rejected entry.
struct Units { int s0, s1; bool bad; };

__device__ __forceinline__ Units check_offsets2(const int* __restrict__ inner_off, const int* __restrict__ outer_off, int b, int lane, int N_cap,
                                                int P_cap) {
    bool bad = false;
    for (int j = lane; j <= b; j += 64) {
        const int o0 = outer_off[j], o1 = outer_off[j + 1];
        bad |= o0 < 0 || o1 < o0 || o1 > N_cap || (j == 0 && o0 != 0);
    }
    bad = __any(bad);
    const int s0 = bad ? 0 : outer_off[b], s1 = bad ? 0 : outer_off[b + 1];
    for (int s = s0 + lane; s < s1; s += 64) {
        const int r0 = inner_off[s], r1 = inner_off[s + 1];
        bad |= r0 < 0 || r1 < r0 || r1 > P_cap;
    }
    bad = __any(bad);
    return {s0, s1, bad};
}

// off[j] = cnt[j0] + ... + cnt[j - 1] for j in [j0, j1), 64 at a time; -> the sum of them all, in every lane.  Both clamped at 2^31 - 1.
// The lanes are 64 bits wide: offsets that arrive on the device are only checked unit by unit, so the units of one entry may overlap in
// rows, and 64 counts can then hold more than 2^31 - 1 rows together.  Called by all 64 lanes of a wave.
__device__ __forceinline__ int wave_prefix(const int* __restrict__ cnt, long long j0, long long j1, int lane, int* __restrict__ off) {
    long long run = 0;
    for (long long c0 = j0; c0 < j1; c0 += 64) {
        const long long j = c0 + lane;
        const long long c = j < j1 ? cnt[j] : 0;
        long long v = c;
        for (int o = 1; o < 64; o <<= 1) {
            const long long t = __shfl_up(v, o);
            if (lane >= o) v += t;
        }
        if (j < j1) off[j] = (int)min(run + (v - c), (long long)0x7fffffff);
        run = min(run + __shfl(v, 63), (long long)0x7fffffff);          // a chunk adds at most 64 * (2^31 - 1): no overflow of the 64-bit sum
    }
    return (int)run;
}

// largest b in [0, B) with off[b] <= i (off non-decreasing)
__device__ __forceinline__ int frame_of(const int* __restrict__ off, int B, long long i) {
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((long long)off[mid] <= i) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// One wave: out_offsets over the entries, the final status.  An entry above max_frame_points rows, or whose rows would pass cap, has none.
__global__ __launch_bounds__(64) void offsets_kernel(int B, int cap, int max_frame_points, const int* __restrict__ total, int* __restrict__ stat,
                                                     int* __restrict__ out_off, int* __restrict__ status) {
    if (threadIdx.x != 0) return;
    long long run = 0;
    out_off[0] = 0;
    for (int b = 0; b < B; ++b) {
        int st = stat[b];
        const int n = total[b];
        if (st == ST_OK) {
            if (n > max_frame_points || run + n > (long long)cap) st = ST_TOO_MANY;
            else if (n == 0) st = ST_EMPTY;
        }
        if (st == ST_OK) run += n;
        stat[b] = st;
        if (status) status[b] = st;
        out_off[b + 1] = (int)run;
    }
}

}  // namespace
