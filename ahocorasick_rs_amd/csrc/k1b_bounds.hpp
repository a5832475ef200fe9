// The boundary mask of K1b's level 1 (kernels.hip): which of a lane's 16 positions may start a match.
// Host and device: the kernel applies it to the first and the last tiles of a stream only, and
// tests/test_k1b_bounds_cpu.py compares it with its definition on the CPU.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ACX_HD __host__ __device__
#else
#define ACX_HD
#endif

namespace acx {

// Bit j (0 .. 15) is set iff lo <= p0 + j <= hi; hi < lo: no bit.  (p0 + 15 must not wrap.)
// Two clamped differences and two shifts: the positions below lo are shifted out at the bottom, the
// positions above hi at the top.
ACX_HD inline uint32_t keep_mask16(uint64_t p0, uint64_t lo, uint64_t hi) {
    if (hi < p0) return 0u;
    const uint64_t below = lo > p0 ? lo - p0 : 0u;  // positions in front of lo
    const uint64_t upto = hi - p0;                  // the last position that may stay
    const uint32_t b = below < 16u ? (uint32_t)below : 16u;
    const uint32_t u = upto < 15u ? (uint32_t)upto : 15u;
    return ((0xFFFFu << b) & 0xFFFFu) & (0xFFFFu >> (15u - u));
}

} // namespace acx

#undef ACX_HD
