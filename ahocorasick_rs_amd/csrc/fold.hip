// fold.hip -- the ASCII case fold of a device haystack (fold.hpp).  A copy with a few VALU operations per word: aligned
// 16-byte loads and stores (global_load_dwordx4 / global_store_dwordx4) over the body, a grid-stride loop sized to the
// CU count, byte-wise head and tail for the unaligned ends.  Vector stores only.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "fold.hpp"

namespace acx {

constexpr uint32_t FOLD_THREADS = 256, FOLD_UNROLL = 4, FOLD_BLOCKS_PER_CU = 8;

// head: bytes [0, head) (src + head is 16-byte aligned); body: n16 pieces of 16 bytes; tail: bytes [head + 16 n16, len)
__global__ __launch_bounds__(FOLD_THREADS) void k_fold(const uint8_t *src, uint8_t *dst, uint64_t len, uint32_t head,
                                                        uint64_t n16) {
    const uint4 *s4 = (const uint4 *)(src + head);
    uint4 *d4 = (uint4 *)(dst + head);
    const uint64_t stride = (uint64_t)gridDim.x * FOLD_THREADS;
    uint64_t i = (uint64_t)blockIdx.x * FOLD_THREADS + threadIdx.x;
    // FOLD_UNROLL pieces in flight per thread ahead of their stores
    for (; i + (FOLD_UNROLL - 1) * stride < n16; i += FOLD_UNROLL * stride) {
        uint4 v[FOLD_UNROLL];
#pragma unroll
        for (uint32_t k = 0; k < FOLD_UNROLL; k++) v[k] = s4[i + k * stride];
#pragma unroll
        for (uint32_t k = 0; k < FOLD_UNROLL; k++)
            d4[i + k * stride] = make_uint4(fold_word(v[k].x), fold_word(v[k].y), fold_word(v[k].z), fold_word(v[k].w));
    }
    for (; i < n16; i += stride) {
        const uint4 v = s4[i];
        d4[i] = make_uint4(fold_word(v.x), fold_word(v.y), fold_word(v.z), fold_word(v.w));
    }
    if (blockIdx.x == 0) { // head (threads 0 .. 15) and tail (threads 16 .. 31): fewer than 16 bytes each
        const uint64_t t = head + 16 * n16 + threadIdx.x - 16;
        if (threadIdx.x < head) dst[threadIdx.x] = fold_byte(src[threadIdx.x]);
        else if (threadIdx.x >= 16 && threadIdx.x < 32 && t < len) dst[t] = fold_byte(src[t]);
    }
}

hipError_t fold_device(const uint8_t *src, uint8_t *dst, uint64_t len, int n_cus, hipStream_t st) {
    if (!len) return hipSuccess;
    if (((uintptr_t)src & 15) != ((uintptr_t)dst & 15)) return hipErrorInvalidValue;
    const uint64_t head = std::min<uint64_t>((16 - ((uintptr_t)src & 15)) & 15, len);
    const uint64_t n16 = (len - head) / 16;
    const uint64_t want = (n16 + FOLD_THREADS * FOLD_UNROLL - 1) / (FOLD_THREADS * FOLD_UNROLL);
    const uint64_t cap = (uint64_t)std::max(n_cus, 1) * FOLD_BLOCKS_PER_CU;
    const uint32_t blocks = (uint32_t)std::max<uint64_t>(1, std::min(want, cap));
    hipLaunchKernelGGL(k_fold, dim3(blocks), dim3(FOLD_THREADS), 0, st, src, dst, len, (uint32_t)head, n16);
    return hipGetLastError();
}

} // namespace acx
