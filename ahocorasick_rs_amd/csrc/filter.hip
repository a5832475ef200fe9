// filter.hip -- the row-filter kernels behind acx_filter_device / acx_filter_rows_device (filter.hpp says what each step
// computes).  The find pipeline (kernels.hip) and the splice (replace.hip) are not touched: the scans are replace_scan's.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "filter.hpp"

namespace acx {

// ---------------------------------------------------------------------------
// 1. + 3. one thread per source row
// ---------------------------------------------------------------------------
__global__ void k_filter_flags(RowCut R, const uint64_t *__restrict__ counts, uint64_t min_matches, uint32_t keep_matched,
                               uint64_t *__restrict__ klen, uint64_t *__restrict__ kflag) {
    const uint64_t h = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= R.n) return;
    const uint64_t len = row_begin(R, h + 1) - row_begin(R, h);
    const bool kept = (counts[h] >= min_matches) == (keep_matched != 0);
    klen[h] = kept ? len : 0;
    kflag[h] = kept ? 1 : 0;
}

__global__ void k_filter_index(RowCut R, const int64_t *__restrict__ A, const int64_t *__restrict__ B,
                               int64_t *__restrict__ rows, int64_t *__restrict__ offsets, uint64_t *__restrict__ src) {
    const uint64_t h = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= R.n) return;
    const int64_t r = B[h];
    if (B[h + 1] != r) { // kept: its rank is r
        rows[r] = (int64_t)h;
        offsets[r] = A[h];
        src[r] = row_begin(R, h);
    }
    if (h == R.n - 1) offsets[B[R.n]] = A[R.n];
}

hipError_t filter_flags(const RowCut &R, const uint64_t *counts, uint64_t min_matches, bool keep_matched, uint64_t *klen,
                        uint64_t *kflag, hipStream_t st) {
    if (!R.n) return hipSuccess;
    hipLaunchKernelGGL(k_filter_flags, dim3((uint32_t)((R.n + 255) / 256)), dim3(256), 0, st, R, counts, min_matches,
                       keep_matched ? 1u : 0u, klen, kflag);
    return hipGetLastError();
}

hipError_t filter_index(const RowCut &R, const int64_t *A, const int64_t *B, int64_t *rows, int64_t *offsets, uint64_t *src,
                        hipStream_t st) {
    if (!R.n) return hipSuccess;
    hipLaunchKernelGGL(k_filter_index, dim3((uint32_t)((R.n + 255) / 256)), dim3(256), 0, st, R, A, B, rows, offsets, src);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// 4. the gather, output side.  Kept row r's bytes are output bytes offsets[r] .. offsets[r + 1]; output byte x of row r is
//    hay[x + (src[r] - offsets[r])].  A workgroup owns FILTER_TILE output bytes; its rows -- from the last one that begins
//    at or before the tile (it covers the tile's first byte: of several rows with one start, all but the last are empty)
//    up to the last one that begins inside it -- are staged in LDS, FILTER_WIN at a time (a tile of 1-byte rows holds
//    16 384 of them, and any number of empty ones: rounds, each thread keeps its chunks in registers between them).
//    A thread owns FG_CHUNKS 16-byte chunks, one aligned 16-byte store each.  Per round a thread first finds the row of
//    each of its chunks (the searches of the four chunks step together), then issues the loads of EVERY chunk that lies
//    inside one row -- two aligned 16-byte loads each -- and only then shifts them into place; a chunk that straddles a
//    row boundary (or a round's, or the input's first or last 16-byte line) is assembled byte by byte.
// ---------------------------------------------------------------------------
constexpr uint32_t FG_CHUNKS = FILTER_TILE / 16 / FILTER_THREADS;
static_assert(FG_CHUNKS * 16 * FILTER_THREADS == FILTER_TILE, "a tile is a whole number of chunks per thread");

// the kept rows that begin at or before, and before, every boundary of the output's tiles (stage_device.hpp)
__global__ void k_filter_tiles(const int64_t *__restrict__ offsets, uint64_t k, uint64_t total, uint64_t ntiles, uint64_t *U,
                               uint64_t *L) {
    out_tile_bounds<FILTER_TILE>(offsets, k, total, ntiles, U, L);
}

__global__ __launch_bounds__(FILTER_THREADS) void k_filter_gather(const uint8_t *__restrict__ hay, uint64_t len,
                                                                  const int64_t *__restrict__ offsets,
                                                                  const uint64_t *__restrict__ src,
                                                                  const uint64_t *__restrict__ U, const uint64_t *__restrict__ L,
                                                                  uint8_t *__restrict__ out, uint64_t total) {
    __shared__ uint64_t s_o[FILTER_WIN];
    __shared__ int64_t s_d[FILTER_WIN];
    __shared__ uint64_t s_hi;
    const uint64_t T0 = (uint64_t)blockIdx.x * FILTER_TILE, T1 = std::min<uint64_t>(T0 + FILTER_TILE, total);
    const uint64_t base = U[blockIdx.x] - 1, kend = L[blockIdx.x + 1];
    const uintptr_t hb = (uintptr_t)hay, he = hb + len;
    const uint4 *idle = (const uint4 *)(U + (((uintptr_t)U >> 3) & 1)); // (a 16-byte line of the >= 4 words at U)
    uint4 acc[FG_CHUNKS];
#pragma unroll
    for (uint32_t c = 0; c < FG_CHUNKS; c++) acc[c] = make_uint4(0, 0, 0, 0);
    for (uint64_t wb = base; wb < kend; wb += FILTER_WIN) {
        const uint64_t we = std::min<uint64_t>(wb + FILTER_WIN, kend);
        const uint32_t cnt = (uint32_t)(we - wb);
        if (wb != base) __syncthreads(); // (the last round's readers are done with the window)
        for (uint32_t t = threadIdx.x; t < cnt; t += FILTER_THREADS) {
            const uint64_t o = (uint64_t)offsets[wb + t];
            s_o[t] = o;
            s_d[t] = (int64_t)(src[wb + t] - o);
        }
        if (threadIdx.x == 0) s_hi = we == kend ? T1 : (uint64_t)offsets[we];
        __syncthreads();
        const uint64_t lo_w = wb == base ? T0 : s_o[0], hi_w = s_hi;
        // the row of every chunk's first byte in this round: the last entry that begins at or before it
        uint64_t xa[FG_CHUNKS], xb[FG_CHUNKS];
        uint32_t lo[FG_CHUNKS], hi[FG_CHUNKS];
#pragma unroll
        for (uint32_t c = 0; c < FG_CHUNKS; c++) {
            const uint64_t x0 = T0 + 16ull * (c * FILTER_THREADS + threadIdx.x);
            xa[c] = std::max(x0, lo_w);
            xb[c] = std::min(x0 + 16, hi_w);
            lo[c] = 0;
            hi[c] = cnt;
        }
        for (uint32_t step = 32 - __builtin_clz(cnt); step; step--) { // (cnt >= 1; an interval of cnt entries closes in that many)
#pragma unroll
            for (uint32_t c = 0; c < FG_CHUNKS; c++) {
                const uint32_t mid = (lo[c] + hi[c]) >> 1;
                const bool open = lo[c] < hi[c], le = s_o[std::min(mid, cnt - 1)] <= xa[c];
                lo[c] = open && le ? mid + 1 : lo[c];
                hi[c] = open && !le ? mid : hi[c];
            }
        }
        // The chunks that lie inside one row and whose two lines lie inside the input: their loads, all of them, first.  The
        // loads are unconditional -- a chunk that takes the other way reads the first line of this tile's own U entry (`idle`,
        // 16-byte aligned scratch of the stage) -- so that no branch, and no wait, stands between them.
        uint4 ld_lo[FG_CHUNKS], ld_hi[FG_CHUNKS];
        uint32_t sh[FG_CHUNKS];
        bool fast[FG_CHUNKS];
#pragma unroll
        for (uint32_t c = 0; c < FG_CHUNKS; c++) {
            const uint64_t x0 = T0 + 16ull * (c * FILTER_THREADS + threadIdx.x);
            const uint32_t j = lo[c] ? lo[c] - 1 : 0; // (lo[c] == 0 only where nothing of the chunk lies in this round)
            const uint64_t send = j + 1 < cnt ? s_o[j + 1] : hi_w;
            const uintptr_t a = hb + (x0 + (uint64_t)s_d[j]), a0 = a & ~(uintptr_t)15;
            const uintptr_t a1 = (a & 15) ? a0 + 16 : a0; // (an aligned chunk is its first line alone)
            fast[c] = xa[c] == x0 && xb[c] == x0 + 16 && x0 + 16 <= send && a0 >= hb && a1 + 16 <= he;
            sh[c] = (uint32_t)(a & 15);
            ld_lo[c] = *(fast[c] ? (const uint4 *)(hay + (a0 - hb)) : idle); // (through `hay`: global loads, not flat ones)
            ld_hi[c] = *(fast[c] ? (const uint4 *)(hay + (a1 - hb)) : idle);
        }
        __builtin_amdgcn_sched_barrier(0); // (no shift moves up between the loads: all of them are in flight before the first wait)
#pragma unroll
        for (uint32_t c = 0; c < FG_CHUNKS; c++) {
            if (fast[c]) {
                uint4 l = ld_lo[c], h = ld_hi[c];
                // (the lines as they were loaded: without this the shifts' selects are folded into the second load, which
                // then becomes three overlapping 8-byte loads)
                asm volatile("" : "+v"(l.x), "+v"(l.y), "+v"(l.z), "+v"(l.w), "+v"(h.x), "+v"(h.y), "+v"(h.z), "+v"(h.w));
                acc[c] = funnel16(l, h, sh[c]);
                continue;
            }
            if (xa[c] >= xb[c]) continue;
            const uint64_t x0 = T0 + 16ull * (c * FILTER_THREADS + threadIdx.x);
            uint32_t j = lo[c] - 1;
            uint4 w = acc[c];
#pragma unroll 1
            for (uint64_t x = xa[c]; x < xb[c]; x++) {
                while (j + 1 < cnt && s_o[j + 1] <= x) j++; // (kept empty rows are stepped over here)
                uint32_t v = hay[x + (uint64_t)s_d[j]];
                const uint32_t q = (uint32_t)(x - x0), s8 = 8 * (q & 3), keep = ~(0xFFu << s8), word = q >> 2;
                v <<= s8; // (the byte into word `word`: selects, not an indexed register array)
                w.x = word == 0 ? (w.x & keep) | v : w.x; w.y = word == 1 ? (w.y & keep) | v : w.y;
                w.z = word == 2 ? (w.z & keep) | v : w.z; w.w = word == 3 ? (w.w & keep) | v : w.w;
            }
            acc[c] = w;
        }
    }
#pragma unroll
    for (uint32_t c = 0; c < FG_CHUNKS; c++) {
        const uint64_t x0 = T0 + 16ull * (c * FILTER_THREADS + threadIdx.x);
        if (x0 < T1) *(uint4 *)(out + x0) = acc[c];
    }
}

uint64_t filter_tile_words(uint64_t total) { return out_tile_words(total, FILTER_TILE); }

hipError_t filter_gather(const uint8_t *hay, uint64_t len, const int64_t *offsets, const uint64_t *src, uint64_t k,
                         uint64_t *tiles, uint8_t *out, uint64_t total, hipStream_t st) {
    if (!total || !k) return hipSuccess;
    const uint64_t ntiles = tiles_of(total, FILTER_TILE);
    if (ntiles >= (1ull << 31)) return hipErrorInvalidValue;
    uint64_t *U = tiles, *L = tiles + ntiles + 1;
    hipLaunchKernelGGL(k_filter_tiles, dim3((uint32_t)((ntiles + 1 + 255) / 256)), dim3(256), 0, st, offsets, k, total, ntiles, U,
                       L);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_filter_gather, dim3((uint32_t)ntiles), dim3(FILTER_THREADS), 0, st, hay, len, offsets, src,
                       (const uint64_t *)U, (const uint64_t *)L, out, total);
    return hipGetLastError();
}

} // namespace acx
