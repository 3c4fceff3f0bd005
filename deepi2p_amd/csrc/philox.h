// Philox4x32-10 (Salmon et al., SC'11; Random123 constants) and the 53-bit uniform every draw of the library is made from.  One
// definition, so that a stream keeps its bits wherever it is drawn.  The fourth counter word is the stream tag:
//   0, 1 restart list   2 random choice   3 dropout keep-mask   4 per-frame sample draws   5 point / intensity / normal jitter
//   6 point shuffle (range filter of the Oxford loader)   7 synthetic-world scan: dropout, range and intensity noise (world.hip)
//   8 synthetic-world push-broom profiles: dropout, range and reflectance noise (world.hip)
#pragma once
#include <hip/hip_runtime.h>

namespace {

struct U4 { unsigned x, y, z, w; };

__device__ __forceinline__ U4 philox4x32_10(U4 ctr, unsigned k0, unsigned k1) {
    constexpr unsigned M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = (unsigned long long)M0 * ctr.x, p1 = (unsigned long long)M1 * ctr.z;
        const U4 n{(unsigned)(p1 >> 32) ^ ctr.y ^ k0, (unsigned)p1, (unsigned)(p0 >> 32) ^ ctr.w ^ k1, (unsigned)p0};
        ctr = n;
        k0 += W0; k1 += W1;
    }
    return ctr;
}

// 53-bit uniform in (0, 1]: never 0, so log() is finite
__device__ __forceinline__ double u53(unsigned hi, unsigned lo) {
    const unsigned long long m = ((unsigned long long)(hi >> 5) << 26) | (unsigned long long)(lo >> 6);
    return ((double)m + 1.0) * (1.0 / 9007199254740992.0);
}

}  // namespace
