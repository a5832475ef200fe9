// rows.hip -- the row-cut kernels behind acx_split_rows_device / acx_split_rows_into_device (rows.hpp says what each step
// computes).  The find pipeline (kernels.hip) and the other stages are not touched: the scan of the tile counts is
// replace_scan's.
//
// RELIED ON: both kernels cut the input into the same tiles (at 16-byte lines of the address) and mark the same bytes, so
// the ranks of k_rows_write add up to the counts k_rows_count left -- as long as the bytes are the same in both passes.  A
// caller who writes the input between the two gets wrong offsets, but no store behind offsets[rows]: every index is compared
// with the total the result was sized by.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "rows.hpp"

namespace acx {

constexpr uint32_t RW_LINES = ROWS_TILE / 16 / ROWS_THREADS; // 16-byte lines of one thread
constexpr uint32_t RW_WAVES = ROWS_THREADS / 64;
static_assert(RW_LINES * 16 * ROWS_THREADS == ROWS_TILE, "a tile is a whole number of lines per thread");
static_assert(ROWS_THREADS % 64 == 0, "whole waves");

// 0x80 in every byte of w that equals the delimiter (d4: the delimiter in all four bytes), 0 in every other byte -- EXACT:
// the sum never carries out of a byte (0x7F + 0x7F), so a byte next to a match says nothing about the match (the short form
// (x - 0x01010101) & ~x & 0x80808080 borrows across bytes and reports d ^ 1 behind a d).
__device__ inline uint32_t eq_bytes(uint32_t w, uint32_t d4) {
    const uint32_t x = w ^ d4;
    return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
}

__device__ inline uint4 marks_of(uint4 v, uint32_t d4) {
    return make_uint4(eq_bytes(v.x, d4), eq_bytes(v.y, d4), eq_bytes(v.z, d4), eq_bytes(v.w, d4));
}

// The marks of the 16-byte line at address a where the input [hb, he) may cover a part of it only (its first line, its last
// one, the lines of the last tile behind it): the bytes inside the input one by one, no mark for any other.
__device__ inline uint4 edge_marks(const uint8_t *hay, uintptr_t hb, uintptr_t he, uintptr_t a, uint32_t d4) {
    if (a >= hb && a + 16 <= he) return marks_of(*(const uint4 *)(hay + (a - hb)), d4);
    uint32_t m[4] = {0, 0, 0, 0};
#pragma unroll
    for (uint32_t j = 0; j < 16; j++) {
        const uintptr_t x = a + j;
        if (x >= hb && x < he && hay[x - hb] == (uint8_t)d4) m[j >> 2] |= 0x80u << (8 * (j & 3));
    }
    return make_uint4(m[0], m[1], m[2], m[3]);
}

// the marks of this thread's RW_LINES lines of tile `tile`; an interior tile's loads stand together, nothing between them
__device__ inline void tile_marks(const uint8_t *hay, uint64_t len, uint32_t d4, uint64_t tile, uint4 (&m)[RW_LINES], uintptr_t *first) {
    const uintptr_t hb = (uintptr_t)hay, he = hb + len;
    const uintptr_t T0 = (hb & ~(uintptr_t)15) + tile * ROWS_TILE + 16u * threadIdx.x;
    *first = T0;
    if (T0 - 16u * threadIdx.x >= hb && T0 - 16u * threadIdx.x + ROWS_TILE <= he) { // (the same in every thread)
        uint4 v[RW_LINES];
#pragma unroll
        for (uint32_t k = 0; k < RW_LINES; k++) v[k] = *(const uint4 *)(hay + (T0 - hb) + 16u * ROWS_THREADS * k);
#pragma unroll
        for (uint32_t k = 0; k < RW_LINES; k++) m[k] = marks_of(v[k], d4);
    } else {
#pragma unroll
        for (uint32_t k = 0; k < RW_LINES; k++) m[k] = edge_marks(hay, hb, he, T0 + 16u * ROWS_THREADS * k, d4);
    }
}

__device__ inline uint32_t marks_count(uint4 m) { return __popc(m.x) + __popc(m.y) + __popc(m.z) + __popc(m.w); }

__global__ __launch_bounds__(ROWS_THREADS) void k_rows_count(const uint8_t *__restrict__ hay, uint64_t len, uint32_t d4,
                                                             uint64_t *__restrict__ counts, uint64_t *__restrict__ last) {
    __shared__ uint32_t s_w[RW_WAVES];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint4 m[RW_LINES];
    uintptr_t first;
    tile_marks(hay, len, d4, blockIdx.x, m, &first);
    uint32_t c = 0;
#pragma unroll
    for (uint32_t k = 0; k < RW_LINES; k++) c += marks_count(m[k]);
#pragma unroll
    for (uint32_t d = 32; d; d >>= 1) c += __shfl_down(c, d);
    if (lane == 0) s_w[wave] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t sum = 0;
#pragma unroll
        for (uint32_t w = 0; w < RW_WAVES; w++) sum += s_w[w];
        counts[blockIdx.x] = sum;
        if (blockIdx.x == gridDim.x - 1) *last = hay[len - 1] == (uint8_t)d4 ? 1 : 0;
    }
}

// Lane i takes line i + k * ROWS_THREADS: within one k the lanes' lines rise with the lane, so rank order is position order
// per k only -- a scan per k, and the totals of the k before carried.
__global__ __launch_bounds__(ROWS_THREADS) void k_rows_write(const uint8_t *__restrict__ hay, uint64_t len, uint32_t d4,
                                                             const int64_t *__restrict__ base, uint64_t total, uint32_t unterminated,
                                                             int64_t *__restrict__ offsets) {
    __shared__ uint32_t s_w[RW_LINES][RW_WAVES];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint4 m[RW_LINES];
    uintptr_t first;
    tile_marks(hay, len, d4, blockIdx.x, m, &first);
    uint32_t excl[RW_LINES];
#pragma unroll
    for (uint32_t k = 0; k < RW_LINES; k++) {
        const uint32_t c = marks_count(m[k]);
        uint32_t inc = c;
#pragma unroll
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(inc, d);
            if (lane >= d) inc += up;
        }
        if (lane == 63) s_w[k][wave] = inc;
        excl[k] = inc - c;
    }
    __syncthreads();
    const uint64_t b = (uint64_t)base[blockIdx.x];
    uint32_t run = 0; // the marks of the k before
#pragma unroll
    for (uint32_t k = 0; k < RW_LINES; k++) {
        uint32_t before = run;
#pragma unroll
        for (uint32_t w = 0; w < RW_WAVES; w++) {
            const uint32_t t = s_w[k][w];
            before += w < wave ? t : 0;
            run += t;
        }
        uint64_t at = b + before + excl[k];                                                 // the rank of the line's first mark
        const uint64_t p1 = (uint64_t)(first + 16u * ROWS_THREADS * k - (uintptr_t)hay) + 1; // position + 1 of the line's byte 0
        const uint32_t word[4] = {m[k].x, m[k].y, m[k].z, m[k].w};
#pragma unroll
        for (uint32_t i = 0; i < 4; i++) {
            for (uint32_t t = word[i]; t; t &= t - 1, at++)
                if (at < total) offsets[1 + at] = (int64_t)(p1 + 4 * i + ((uint32_t)__builtin_ctz(t) >> 3));
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        offsets[0] = 0;
        if (unterminated) offsets[total + 1] = (int64_t)len;
    }
}

uint64_t rows_tiles(const void *hay, uint64_t len) {
    return len ? (((uintptr_t)hay & 15) + len + ROWS_TILE - 1) / ROWS_TILE : 0;
}

hipError_t rows_count(const uint8_t *hay, uint64_t len, uint8_t delimiter, uint64_t *counts, uint64_t *last, hipStream_t st) {
    const uint64_t ntiles = rows_tiles(hay, len);
    if (!ntiles) return hipSuccess;
    if (ntiles >= (1ull << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_rows_count, dim3((uint32_t)ntiles), dim3(ROWS_THREADS), 0, st, hay, len, (uint32_t)delimiter * 0x01010101u,
                       counts, last);
    return hipGetLastError();
}

hipError_t rows_write(const uint8_t *hay, uint64_t len, uint8_t delimiter, const int64_t *base, uint64_t total, bool unterminated,
                      int64_t *offsets, hipStream_t st) {
    const uint64_t ntiles = rows_tiles(hay, len);
    if (!ntiles) return hipSuccess;
    if (ntiles >= (1ull << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_rows_write, dim3((uint32_t)ntiles), dim3(ROWS_THREADS), 0, st, hay, len, (uint32_t)delimiter * 0x01010101u,
                       base, total, unterminated ? 1u : 0u, offsets);
    return hipGetLastError();
}

} // namespace acx
