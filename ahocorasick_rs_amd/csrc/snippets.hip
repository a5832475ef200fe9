// snippets.hip -- the snippet kernels behind acx_snippets_device / acx_snippets_rows_device (snippets.hpp says what each step
// computes, and states the definition).  The find pipeline (kernels.hip) and the other stages are not touched: the scan is
// replace_scan's.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "snippets.hpp"

namespace acx {

__device__ inline bool snip_continuation(uint8_t b) { return (b & 0xC0) == 0x80; }

// ---------------------------------------------------------------------------
// 1. one thread per record: the definition
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_snip_sizes(const acx_match_t *__restrict__ m, uint64_t n,
                                                    const int64_t *__restrict__ rec_off, RowCut R,
                                                    const uint8_t *__restrict__ hay, uint64_t context, uint32_t flags,
                                                    uint64_t *__restrict__ seg_len, uint64_t *__restrict__ src,
                                                    int64_t *__restrict__ lead, int64_t *__restrict__ pattern) {
    // A record's row is the last one whose records begin at or before it (empty rows share a begin: all but the last are
    // stepped over); rec_off[R.n] == n, so the row is below R.n.  One thread finds the rows of the tile's first and last
    // record in all of rec_off; every thread then searches between the two -- a tile of 256 records seldom holds more than a
    // few rows, so that search is a step or two instead of log2(rows).
    __shared__ uint64_t s_h[2];
    const uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x, i = i0 + threadIdx.x;
    if (threadIdx.x == 0) {
        const uint64_t a = count_le(rec_off, R.n + 1, i0), h_first = std::min(a ? a - 1 : 0, R.n - 1);
        const uint64_t b = h_first + count_le(rec_off + h_first, R.n + 1 - h_first, std::min(i0 + blockDim.x - 1, n - 1));
        s_h[0] = h_first;
        s_h[1] = std::min(b > h_first ? b - 1 : h_first, R.n - 1);
    }
    __syncthreads();
    if (i >= n) return;
    const uint64_t h0 = s_h[0], in_tile = count_le(rec_off + h0, s_h[1] - h0 + 1, i);
    const uint64_t h = h0 + (in_tile ? in_tile - 1 : 0);
    // (offsets between the first and the last are the caller's word: no byte is read beyond len)
    const uint64_t rb = std::min(row_begin(R, h), R.len), re = std::max(std::min(row_begin(R, h + 1), R.len), rb), L = re - rb;
    const uint64_t s = std::min<uint64_t>(m[i].start, L), e = std::min(std::max<uint64_t>(m[i].end, s), L);
    uint64_t lo = s - std::min(s, context), hi = e + std::min(context, L - e);
    if (flags & SNIP_UTF8) {
        const uint8_t *B = hay + rb;
#pragma unroll
        for (int k = 0; k < 3; k++)
            if (lo < s && snip_continuation(B[lo])) lo++;
#pragma unroll
        for (int k = 0; k < 3; k++)
            if (e < hi && hi < L && snip_continuation(B[hi])) hi--;
    }
    seg_len[i] = hi - lo;
    src[i] = rb + lo;
    lead[i] = (int64_t)(s - lo);
    pattern[i] = (int64_t)m[i].pattern;
}

hipError_t snip_sizes(const acx_match_t *m, uint64_t n, const int64_t *rec_off, const RowCut &R, const uint8_t *hay,
                      uint64_t context, uint32_t flags, uint64_t *seg_len, uint64_t *src, int64_t *lead, int64_t *pattern,
                      hipStream_t st) {
    if (!n || !R.n) return hipSuccess;
    if (n >= (1ull << 39)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_snip_sizes, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, m, n, rec_off, R, hay, context, flags,
                       seg_len, src, lead, pattern);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// 2. the segments that begin at or before, and before, every boundary of the output's tiles (stage_device.hpp)
// ---------------------------------------------------------------------------
__global__ void k_snip_tiles(const int64_t *__restrict__ offsets, uint64_t n, uint64_t total, uint64_t ntiles, uint64_t *U,
                             uint64_t *L) {
    out_tile_bounds<SNIP_TILE>(offsets, n, total, ntiles, U, L);
}

// ---------------------------------------------------------------------------
// 3. the gather, output side.  Segment i's bytes are output bytes offsets[i] .. offsets[i + 1]; output byte x of segment i is
//    hay[x + (src[i] - offsets[i])].  A thread owns ONE 16-byte chunk of the tile and keeps it in four registers through the
//    rounds of the window; within a round it walks the segments that intersect the chunk, first to last, and merges every
//    piece into the chunk under a byte mask.
// ---------------------------------------------------------------------------
static_assert(SNIP_TILE == 16 * SNIP_THREADS, "a thread owns one chunk of its tile");

// the aligned word at absolute address a when it straddles an end of the input: its bytes inside [hb, he), zeros outside
__device__ inline uint32_t snip_edge_word(const uint8_t *hay, uintptr_t hb, uintptr_t he, uintptr_t a) {
    uint32_t v = 0;
#pragma unroll
    for (uint32_t b = 0; b < 4; b++) {
        const uintptr_t p = a + b;
        if (p >= hb && p < he) v |= (uint32_t)hay[p - hb] << (8 * b);
    }
    return v;
}

// 0xFF in the lowest `nbytes` bytes of a word (nbytes <= 0: none, >= 4: all)
__device__ inline uint32_t snip_below(int32_t nbytes) {
    return nbytes <= 0 ? 0u : nbytes >= 4 ? ~0u : (1u << (8 * nbytes)) - 1u;
}

__global__ __launch_bounds__(SNIP_THREADS) void k_snip_gather(const uint8_t *__restrict__ hay, uint64_t len,
                                                              const int64_t *__restrict__ offsets,
                                                              const uint64_t *__restrict__ src, const uint64_t *__restrict__ U,
                                                              const uint64_t *__restrict__ L, uint8_t *__restrict__ out,
                                                              uint64_t total) {
    __shared__ uint64_t s_o[SNIP_WIN];
    __shared__ int64_t s_d[SNIP_WIN];
    __shared__ uint64_t s_hi;
    const uint64_t T0 = (uint64_t)blockIdx.x * SNIP_TILE, T1 = std::min<uint64_t>(T0 + SNIP_TILE, total);
    const uint64_t base = U[blockIdx.x] - 1, kend = L[blockIdx.x + 1];
    const uintptr_t hb = (uintptr_t)hay, he = hb + len;
    const uint64_t x0 = T0 + 16ull * threadIdx.x;
    uint32_t c0 = 0, c1 = 0, c2 = 0, c3 = 0; // the chunk
    for (uint64_t wb = base; wb < kend; wb += SNIP_WIN) {
        const uint64_t we = std::min<uint64_t>(wb + SNIP_WIN, kend);
        const uint32_t cnt = (uint32_t)(we - wb);
        if (wb != base) __syncthreads(); // (the last round's readers are done with the window)
        for (uint32_t t = threadIdx.x; t < cnt; t += SNIP_THREADS) {
            const uint64_t o = (uint64_t)offsets[wb + t];
            s_o[t] = o;
            s_d[t] = (int64_t)(src[wb + t] - o);
        }
        if (threadIdx.x == 0) s_hi = we == kend ? T1 : (uint64_t)offsets[we];
        __syncthreads();
        const uint64_t lo_w = wb == base ? T0 : s_o[0], hi_w = s_hi;
        const uint64_t xa = std::max(x0, lo_w), xb = std::min(x0 + 16, hi_w);
        if (xa >= xb) continue; // (nothing of the chunk lies in this round; no barrier stands inside the rest of the body)
        // the segment of the chunk's first byte in this round: the last entry that begins at or before it
        uint32_t lo = 0, hi = cnt;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (s_o[mid] <= xa) lo = mid + 1; else hi = mid;
        }
        uint32_t j = lo ? lo - 1 : 0; // (lo >= 1: the window's first entry begins at or before xa)
        // The pieces of the chunk, ascending in the output.  Records are ordered by row and within a row `end` never decreases
        // (spans.hpp, "RELIED ON"), so within a tile the source addresses are nearly ascending as well: a piece and the next
        // one, and the pieces of the neighbouring lanes, share cache lines.  The walk therefore goes first to last, and every
        // piece's words are loaded lowest address first.
#pragma unroll 1
        for (uint64_t x = xa; x < xb;) {
            while (j + 1 < cnt && s_o[j + 1] <= x) j++; // (empty segments are stepped over here)
            const uint64_t pe = std::min(j + 1 < cnt ? s_o[j + 1] : hi_w, xb);
            const uint32_t q = (uint32_t)(x - x0), pl = (uint32_t)(pe - x);
            const uintptr_t A = hb + (x + (uint64_t)s_d[j]); // where output byte x lies in the input
            if (pl >= 4) {
                // bytes [V, V + 16) would fill the whole chunk from this segment; of its five aligned words those that hold a
                // byte of [A, A + pl) are loaded, the others are zero.  A word that straddles an end of the input (hay at
                // an odd address, or its last bytes) is put together of its bytes inside.
                const uintptr_t V = A - q, V0 = V & ~(uintptr_t)3;
                const uint32_t sh = (uint32_t)(V & 3);
                uint32_t w[5];
#pragma unroll
                for (uint32_t k = 0; k < 5; k++) {
                    const uintptr_t wa = V0 + 4 * k;
                    const bool need = wa + 4 > A && wa < A + pl, inside = wa >= hb && wa + 4 <= he;
                    w[k] = !need ? 0u
                           : inside ? *(const uint32_t *)(hay + (wa - hb)) // (through `hay`: a global load, not a flat one)
                                    : snip_edge_word(hay, hb, he, wa);
                }
                const uint32_t v0 = __builtin_amdgcn_alignbyte(w[1], w[0], sh), v1 = __builtin_amdgcn_alignbyte(w[2], w[1], sh),
                               v2 = __builtin_amdgcn_alignbyte(w[3], w[2], sh), v3 = __builtin_amdgcn_alignbyte(w[4], w[3], sh);
                const int32_t b = (int32_t)q, e = (int32_t)(q + pl);
                const uint32_t m0 = snip_below(e) & ~snip_below(b), m1 = snip_below(e - 4) & ~snip_below(b - 4),
                               m2 = snip_below(e - 8) & ~snip_below(b - 8), m3 = snip_below(e - 12) & ~snip_below(b - 12);
                c0 = (c0 & ~m0) | (v0 & m0); c1 = (c1 & ~m1) | (v1 & m1);
                c2 = (c2 & ~m2) | (v2 & m2); c3 = (c3 & ~m3) | (v3 & m3);
            } else {
#pragma unroll 1
                for (uint32_t k = 0; k < pl; k++) {
                    uint32_t v = hay[(A - hb) + k];
                    const uint32_t p = q + k, s8 = 8 * (p & 3), keep = ~(0xFFu << s8), word = p >> 2;
                    v <<= s8; // (the byte into word `word`: selects, not an indexed register array)
                    c0 = word == 0 ? (c0 & keep) | v : c0; c1 = word == 1 ? (c1 & keep) | v : c1;
                    c2 = word == 2 ? (c2 & keep) | v : c2; c3 = word == 3 ? (c3 & keep) | v : c3;
                }
            }
            x = pe;
        }
    }
    if (x0 + 16 <= total) {
        *(uint4 *)(out + x0) = make_uint4(c0, c1, c2, c3);
    } else if (x0 < total) { // the output's last chunk: nothing is stored at or behind `total`
        const uint32_t rest = (uint32_t)(total - x0);
#pragma unroll
        for (uint32_t p = 0; p < 15; p++) {
            const uint32_t word = p >> 2 == 0 ? c0 : p >> 2 == 1 ? c1 : p >> 2 == 2 ? c2 : c3;
            if (p < rest) out[x0 + p] = (uint8_t)(word >> (8 * (p & 3)));
        }
    }
}

uint64_t snip_tile_words(uint64_t total) { return out_tile_words(total, SNIP_TILE); }

hipError_t snip_gather(const uint8_t *hay, uint64_t len, const int64_t *offsets, const uint64_t *src, uint64_t n, uint64_t *tiles,
                       uint8_t *out, uint64_t total, hipStream_t st) {
    if (!total || !n) return hipSuccess;
    const uint64_t ntiles = tiles_of(total, SNIP_TILE);
    if (ntiles >= (1ull << 31)) return hipErrorInvalidValue;
    uint64_t *U = tiles, *L = tiles + ntiles + 1;
    hipLaunchKernelGGL(k_snip_tiles, dim3((uint32_t)((ntiles + 1 + 255) / 256)), dim3(256), 0, st, offsets, n, total, ntiles, U, L);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_snip_gather, dim3((uint32_t)ntiles), dim3(SNIP_THREADS), 0, st, hay, len, offsets, src,
                       (const uint64_t *)U, (const uint64_t *)L, out, total);
    return hipGetLastError();
}

} // namespace acx
