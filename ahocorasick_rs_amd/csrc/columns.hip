// columns.hip -- the split kernel behind acx_find_columns_device / acx_split_device (columns.hpp says what it computes).
// The find pipeline (kernels.hip) is not touched: the kernel reads the records its write kernel left in HBM.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "columns.hpp"

namespace acx {

// ---------------------------------------------------------------------------
// n records of 24 bytes -> three columns of 8-byte words.
//
// The records are read as what they are in memory: a stream of 3 n 64-bit words.  A workgroup stages a tile of COL_TILE
// records (COL_TILE_WORDS words, 24 KiB) in LDS and writes the three columns from there:
//
//   in    the tile's words as 16-byte pieces, lane l next to lane l + 1: every load instruction of a wave reads 1 KiB of
//         whole lines.  A tile begins at an even word of the stream (COL_TILE_WORDS is even), so the pieces begin at the
//         tile's first word when the records lie at 0 mod 16 and at its second when they lie at 8 mod 16 (`odd`); the one
//         word in front of the pieces, and the one behind them when their number of words is odd, are 8-byte loads of one
//         lane each.  All of a thread's loads are issued before its first LDS write (COL_IN pieces in registers).
//   LDS   word i of the tile at word i: a record's three words lie 6 dwords behind the previous record's.  The 8-byte LDS
//         read of lane l for record l is at dword 6 l: within the 32 lanes that are served together, 6 l mod 64 takes 32
//         different even values (3 is odd: 6 l = 6 l' mod 64 only if l = l' mod 32), each lane its own pair of banks -- the
//         stride needs no padding.  (A 4-byte read would see 32 banks and 6 l mod 32 repeats after 16 lanes: read 8 bytes.)
//   out   thread i of the workgroup writes record i's word of a column, then record i + COL_THREADS's: neighbouring lanes
//         write neighbouring words, a wave 512 bytes of whole lines per store instruction, at any 8-byte alignment of the
//         column.
//
// 24 KiB per workgroup: six workgroups of four waves share a CU's 160 KiB, six waves per SIMD; COL_MAX_GRID = 256 CUs x 6
// is every workgroup resident at once, and the grid-stride loop goes on from there.  Every index into the records and the
// columns is 64-bit; the indexes within a tile are 32-bit.
//
// The form this one was measured against -- a thread per record, three 8-byte loads 24 bytes apart, three 8-byte stores --
// is tools/ubench_split.hip's k_col_split_direct (DESIGN.md section 14 has the pair).
// ---------------------------------------------------------------------------
constexpr uint32_t COL_TILE_WORDS = 3 * COL_TILE;
constexpr uint32_t COL_IN = COL_TILE_WORDS / 2 / COL_THREADS; // 16-byte pieces per thread and tile
constexpr uint32_t COL_OUT = COL_TILE / COL_THREADS;          // records per thread and tile
static_assert(COL_TILE_WORDS % 2 == 0 && COL_TILE_WORDS / 2 % COL_THREADS == 0 && COL_TILE % COL_THREADS == 0,
              "a tile is whole 16-byte pieces and whole rounds of the workgroup");

__global__ __launch_bounds__(COL_THREADS) void k_col_split(const uint64_t *__restrict__ w, uint64_t n,
                                                           uint64_t *__restrict__ pattern, uint64_t *__restrict__ start,
                                                           uint64_t *__restrict__ end) {
    __shared__ __attribute__((aligned(16))) uint64_t s_w[COL_TILE_WORDS];
    const uint64_t words = 3 * n, n_tiles = (n + COL_TILE - 1) / COL_TILE;
    const uint32_t odd = (uint32_t)(reinterpret_cast<uintptr_t>(w) >> 3) & 1u;
    for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const uint64_t lo = t * COL_TILE_WORDS;
        const uint32_t cnt = (uint32_t)std::min<uint64_t>(COL_TILE_WORDS, words - lo); // (a multiple of 3, at least 3)
        const uint32_t pieces = (cnt - odd) / 2;
        const uint64_t *src = w + lo + odd; // 16-byte aligned
        ulonglong2 v[COL_IN];
#pragma unroll
        for (uint32_t k = 0; k < COL_IN; k++) {
            const uint32_t j = threadIdx.x + k * COL_THREADS;
            if (j < pieces) v[k] = *reinterpret_cast<const ulonglong2 *>(src + 2 * (uint64_t)j);
        }
        if (threadIdx.x == 0 && odd) s_w[0] = w[lo];
        if (threadIdx.x == 64 && ((cnt - odd) & 1u)) s_w[cnt - 1] = w[lo + cnt - 1];
#pragma unroll
        for (uint32_t k = 0; k < COL_IN; k++) {
            const uint32_t j = threadIdx.x + k * COL_THREADS;
            if (j < pieces) { s_w[odd + 2 * j] = v[k].x; s_w[odd + 2 * j + 1] = v[k].y; }
        }
        __syncthreads();
        const uint32_t recs = cnt / 3;
        const uint64_t base = t * COL_TILE;
#pragma unroll
        for (uint32_t k = 0; k < COL_OUT; k++) {
            const uint32_t r = threadIdx.x + k * COL_THREADS;
            if (r < recs) {
                pattern[base + r] = s_w[3 * r];
                start[base + r] = s_w[3 * r + 1];
                end[base + r] = s_w[3 * r + 2];
            }
        }
        __syncthreads(); // (the next tile's words go where these were read)
    }
}

uint32_t col_split_grid(uint64_t n) {
    const uint64_t tiles = (n + COL_TILE - 1) / COL_TILE;
    return (uint32_t)std::min<uint64_t>(tiles, COL_MAX_GRID);
}

hipError_t col_split(const acx_match_t *m, uint64_t n, int64_t *pattern, int64_t *start, int64_t *end, hipStream_t st) {
    if (!n) return hipSuccess;
    if (n > UINT64_MAX / sizeof(acx_match_t)) return hipErrorInvalidValue; // (3 n words are counted in 64 bits)
    const uint32_t grid = col_split_grid(n);
    // (a workgroup's passes: the tile numbers are 64-bit, and no workgroup makes 2^32 of them)
    if (((n + COL_TILE - 1) / COL_TILE + grid - 1) / grid >= (1ull << 32)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_col_split, dim3(grid), dim3(COL_THREADS), 0, st, reinterpret_cast<const uint64_t *>(m), n,
                       reinterpret_cast<uint64_t *>(pattern), reinterpret_cast<uint64_t *>(start),
                       reinterpret_cast<uint64_t *>(end));
    return hipGetLastError();
}

} // namespace acx
