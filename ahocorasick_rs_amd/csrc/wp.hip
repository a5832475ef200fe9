// wp.hip -- the WordPiece kernels behind acx_wordpiece / acx_wordpiece_device / acx_wordpiece_into_device (wp.hpp has the
// definition and says what each kernel computes).  The find pipeline (kernels.hip), the post-find stages and the segmenter
// (seg.hip) are not touched: the walk is k_at's over tables every handle has, the workgroup's steps around it -- the row marks,
// the suffix minimum, the ranks -- are the walkers' shared ones (at_walk.hpp), the scan over the tiles is replace_scan's.
//
// RELIED ON: k_wp<COUNT> and k_wp<EMIT> compute the same words and the same piece counts from the same bytes, so the bases of
// the emit pass add up to the counts the scan was made from.  A caller who writes the data between the two gets wrong pieces,
// but no store at or behind T: every index is compared with the total the result was sized by, and a word never stores
// more entries than the count its base was made from.  A piece is at least one byte long: every chain ends.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "at_walk.hpp"
#include "replace.hpp"
#include "wp.hpp"

namespace acx {

constexpr uint32_t WP_BPT = WP_TILE / WP_THREADS; // consecutive bytes of one thread
constexpr uint32_t WP_WAVES = WP_THREADS / 64;
constexpr uint32_t WP_FAR16 = 0xFFFFu;            // no boundary behind this byte inside the tile (WALK_FAR), as a word's end in LDS
constexpr uint32_t WP_UNK = 0x8000u;              // a word's count in LDS: the word is one unknown piece
constexpr uint64_t WP_NONE = ~0ull;               // bound[tile]: the tile has no boundary
constexpr uint64_t WP_PIECE = (uint64_t)WP_CARRY_THREADS * WP_CARRY_PER; // the tiles of one step of k_wp_carry
constexpr int WP_MODE_COUNT = 0, WP_MODE_EMIT = 1;
static_assert(WP_THREADS == 256, "root_next and cont_next are filled a word per thread");
static_assert(WP_BPT == 16, "a thread's bytes are one 16-byte load; a word of the bitmap holds the bits of two threads");
static_assert(WP_TILE + WP_MAX_WORD < WP_UNK && WP_TILE < WP_FAR16, "slots, ends, counts and bases are 16 bits wide");
static_assert((WP_CARRY_THREADS & (WP_CARRY_THREADS - 1)) == 0, "the carry's doubling steps");

// the 16 bytes at data position P, hay + P being 16-byte aligned; a position outside [0, len) is not read and gives 0
__device__ inline uint4 wp_granule(const uint8_t *__restrict__ hay, uint64_t len, int64_t P) {
    if (P >= 0 && (uint64_t)P + 16 <= len) return *(const uint4 *)(hay + P);
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (uint32_t j = 0; j < 16; j++) {
        const int64_t q = P + (int64_t)j;
        if (q >= 0 && (uint64_t)q < len) w[j >> 2] |= (uint32_t)hay[q] << (8 * (j & 3));
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

__device__ inline uint32_t wp_class(const uint32_t *s_cls, uint32_t b) { return (s_cls[b >> 4] >> (2 * (b & 15))) & 3u; }

// The chain of the word [ws, we), we - ws <= M: its pieces, or 0 when a step finds nothing.  STORE: the pieces go to
// at .. at + n - 1 -- n: the count the base was made from -- and never to an index at or behind total.
template <bool STORE>
__device__ inline uint32_t wp_chain(const AtTrie &T, const uint8_t *__restrict__ hay, uint64_t ws, uint64_t we, bool fold, int kind,
                                    const uint32_t *s_root, const uint32_t *s_cont, uint64_t at, uint32_t n, uint64_t total,
                                    int64_t *__restrict__ id, int64_t *__restrict__ start, int64_t *__restrict__ end,
                                    uint8_t *__restrict__ first) {
    uint32_t k = 0;
    for (uint64_t p = ws; p < we; k++) {
        if (STORE && k >= n) break;
        const uint8_t b = hay[p]; // (p < we <= len)
        const uint32_t fb = fold ? fold_byte(b) : b;
        const uint32_t s = p == ws ? s_root[fb] : s_cont[fb];
        if (!s) return 0;
        uint32_t best, best_len;
        at_best(T, hay, p, (uint32_t)(we - p), s, fold, kind, best, best_len);
        if (best == AT_NONE) return 0;
        if (STORE && at + k < total) {
            id[at + k] = (int64_t)best;
            start[at + k] = (int64_t)p;
            end[at + k] = (int64_t)(p + best_len);
            first[at + k] = k == 0;
        }
        p += best_len; // (1 <= best_len <= we - p)
    }
    return k;
}

// COUNT: counts[tile], bound[tile].  EMIT: tbase[tile]: the index of the tile's first piece; carry[tile]: the first boundary
// at or behind the tile's end; id, start, end, first: the result's columns, sized by `total`.
template <int MODE>
__global__ __launch_bounds__(WP_THREADS) void k_wp(const AtTrie T, const uint8_t *__restrict__ hay, const RowCut R, const WpArgs A,
                                                   uint64_t *__restrict__ counts, uint64_t *__restrict__ bound,
                                                   const int64_t *__restrict__ tbase, const uint64_t *__restrict__ carry,
                                                   const uint64_t total, int64_t *__restrict__ id, int64_t *__restrict__ start,
                                                   int64_t *__restrict__ end, uint8_t *__restrict__ first) {
    __shared__ uint32_t s_root[256], s_cont[256];
    __shared__ uint32_t s_cls[16];
    __shared__ uint16_t s_list[WP_TILE]; // the word starts' slots, in position order
    __shared__ uint16_t s_wend[WP_TILE]; // a word's end as a slot, or WP_FAR16
    __shared__ uint16_t s_cnt[WP_TILE];  // a word's pieces, WP_UNK | 1: one unknown piece
    __shared__ uint16_t s_base[MODE == WP_MODE_EMIT ? WP_TILE : 1]; // the pieces of the tile's words before this one
    __shared__ uint32_t s_bits[WP_TILE / 32]; // the row starts inside the tile
    __shared__ uint16_t s_wb[WP_THREADS];     // every thread's WORD bits
    __shared__ uint32_t s_wmin[WP_WAVES], s_wsum[WP_WAVES];
    __shared__ uint64_t s_cut[2];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t tile = (uint64_t)blockIdx.x * WP_TILE;
    const uint32_t in_tile = (uint32_t)std::min<uint64_t>(R.len - tile, WP_TILE); // the tile's bytes of the data (tile < R.len)
    const uint64_t tile_end = tile + in_tile;
    const bool fold = (A.flags & WP_FOLD) != 0;
    const uint32_t M = A.max_word;
    s_root[tid] = T.root_next[tid];
    s_cont[tid] = A.cont_node == WP_NO_NODE ? 0u : at_child(T, A.cont_node, tid);
    if (tid < 16) {
        uint32_t w = 0;
#pragma unroll
        for (uint32_t k = 0; k < 16; k++) w = tid == k ? A.cls.w[k] : w;
        s_cls[tid] = w;
    }
    if (tid < WP_TILE / 32) s_bits[tid] = 0;
    walk_row_range<true>(R, tile, tile_end, tid, s_cut);
    __syncthreads();

    // ---- A: the row starts at or behind the tile's first byte as marks, the data's first byte among them (walk_row_marks);
    // `tail`: where the row of a byte without a mark behind it ends
    const uint64_t tail = walk_row_marks<true, WP_THREADS, WP_TILE>(R, tile, tile_end, tid, s_cut, s_bits);

    // ... the thread's 16 bytes and their classes as bit masks (bit j: byte q0 + j)
    const uint32_t q0 = tid * WP_BPT;
    const uint32_t nvalid = in_tile > q0 ? std::min(in_tile - q0, WP_BPT) : 0u;
    const uint32_t valid = (1u << nvalid) - 1u;
    uint32_t wordb = 0, spaceb = 0;
    {
        const uint32_t sh = (uint32_t)((uintptr_t)(hay + tile) & 15);
        const int64_t P0 = (int64_t)tile - (int64_t)sh + (int64_t)q0;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (nvalid) {
            const uint4 lo = wp_granule(hay, R.len, P0);
            const uint4 hi = sh ? wp_granule(hay, R.len, P0 + 16) : lo;
            v = funnel16(lo, hi, sh);
        }
        const uint32_t vw[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (uint32_t j = 0; j < WP_BPT; j++) {
            const uint32_t c = wp_class(s_cls, (vw[j >> 2] >> (8 * (j & 3))) & 0xFFu);
            wordb |= (uint32_t)(c == WP_WORD) << j;
            spaceb |= (uint32_t)(c == WP_SPACE) << j;
        }
        wordb &= valid;
        spaceb &= valid;
    }
    const uint32_t aloneb = valid & ~wordb & ~spaceb;
    s_wb[tid] = (uint16_t)wordb;
    __syncthreads();
    const uint32_t rowb = (s_bits[tid >> 1] >> (16 * (tid & 1))) & 0xFFFFu;
    uint32_t prevw; // is the byte in front of the thread's first one a WORD byte
    if (tid) prevw = (s_wb[tid - 1] >> 15) & 1u;
    else prevw = tile ? wp_class(s_cls, hay[tile - 1]) == WP_WORD : 0u;
    const uint32_t bnd = (~wordb | rowb) & 0xFFFFu; // the boundaries; a slot behind the data is one
    const uint32_t startb = valid & ~spaceb & (rowb | aloneb | ~((wordb << 1) | prevw));

    // ... every thread's first boundary, a suffix minimum over the workgroup (walk_behind); the word starts ranked in position
    // order (walk_rank); both around one barrier
    const uint32_t c = (uint32_t)__popc(startb);
    uint32_t behind = walk_behind_wave(bnd ? q0 + (uint32_t)__builtin_ctz(bnd) : WALK_FAR, lane, wave, s_wmin);
    const uint32_t inc = walk_rank_wave(c, lane, wave, s_wsum);
    __syncthreads();
    behind = walk_behind<WP_WAVES>(behind, wave, s_wmin); // the first boundary behind this thread's bytes
    uint32_t n_words = 0, tile_first = WALK_FAR;
#pragma unroll
    for (uint32_t w = 0; w < WP_WAVES; w++) {
        n_words += s_wsum[w];
        tile_first = std::min(tile_first, s_wmin[w]);
    }
    {
        uint32_t k = walk_rank<WP_WAVES>(inc, c, wave, s_wsum);
        for (uint32_t m = startb; m; m &= m - 1, k++) {
            const uint32_t j = (uint32_t)__builtin_ctz(m), q = q0 + j;
            const uint32_t later = bnd >> (j + 1);
            const uint32_t e = (aloneb >> j) & 1u ? q + 1 : later ? q + 1 + (uint32_t)__builtin_ctz(later) : behind;
            s_list[k] = (uint16_t)q; // (k < n_words <= WP_TILE: the ranks of distinct slots)
            s_wend[k] = (uint16_t)(e == WALK_FAR ? WP_FAR16 : e);
        }
    }
    __syncthreads();

    // ---- B: a word per lane.  word_end: the word's end and whether it is longer than M
    auto word_end = [&](uint32_t j, uint64_t &we) -> bool {
        const uint32_t q = s_list[j], e = s_wend[j];
        const uint64_t ws = tile + q;
        if (e != WP_FAR16) {
            we = tile + e;
            return e - q > M;
        }
        // no boundary behind it in the tile (in_tile == WP_TILE): at most M + 1 bytes from its start, inside the row
        const uint64_t lim = std::min<uint64_t>(tail, ws + M + 1); // (tail <= len)
        uint64_t x = tile_end;
        while (x < lim && wp_class(s_cls, hay[x]) == WP_WORD) x++;
        we = x;
        if (x - ws <= M) return false;
        if (MODE == WP_MODE_EMIT) we = std::max<uint64_t>(std::min<uint64_t>(carry[blockIdx.x], R.len), ws + 1);
        return true;
    };
    uint32_t mine = 0;
    for (uint32_t j = tid; j < n_words; j += WP_THREADS) {
        uint64_t we;
        uint32_t n = 0;
        if (!word_end(j, we)) n = wp_chain<false>(T, hay, tile + s_list[j], we, fold, A.kind, s_root, s_cont, 0, 0, 0, nullptr, nullptr, nullptr, nullptr);
        s_cnt[j] = (uint16_t)(n ? n : WP_UNK | 1u);
        mine += n ? n : 1u;
    }

    if (MODE == WP_MODE_COUNT) {
        // ---- C: the tile's pieces and its first boundary
#pragma unroll
        for (uint32_t d = 32; d; d >>= 1) mine += __shfl_down(mine, d);
        __syncthreads(); // (s_wsum's ranks were read above)
        if (lane == 0) s_wsum[wave] = mine;
        __syncthreads();
        if (tid == 0) {
            uint32_t sum = 0;
            for (uint32_t w = 0; w < WP_WAVES; w++) sum += s_wsum[w];
            counts[blockIdx.x] = sum;
            bound[blockIdx.x] = tile_first == WALK_FAR ? WP_NONE : tile + tile_first;
        }
        return;
    }

    // ---- EMIT: the words' bases -- every thread sums 16 consecutive words of the list, the sums are ranked (walk_rank) -- and
    // the stores
    __syncthreads();
    {
        uint32_t sum = 0;
        for (uint32_t k = 0; k < WP_BPT; k++) sum += q0 + k < n_words ? (s_cnt[q0 + k] & (WP_UNK - 1u)) : 0u;
        const uint32_t run = walk_rank_wave(sum, lane, wave, s_wsum);
        __syncthreads();
        uint32_t at = walk_rank<WP_WAVES>(run, sum, wave, s_wsum);
        for (uint32_t k = 0; k < WP_BPT && q0 + k < n_words; k++) {
            s_base[q0 + k] = (uint16_t)at; // (at most WP_TILE + WP_MAX_WORD)
            at += s_cnt[q0 + k] & (WP_UNK - 1u);
        }
    }
    __syncthreads();
    const uint64_t tb = (uint64_t)tbase[blockIdx.x];
    for (uint32_t j = tid; j < n_words; j += WP_THREADS) {
        const uint64_t ws = tile + s_list[j], at = tb + s_base[j];
        const uint32_t cnt = s_cnt[j];
        uint64_t we;
        (void)word_end(j, we);
        if (cnt & WP_UNK) {
            if (at < total) {
                id[at] = A.unk_id;
                start[at] = (int64_t)ws;
                end[at] = (int64_t)we;
                first[at] = 1;
            }
        } else {
            (void)wp_chain<true>(T, hay, ws, we, fold, A.kind, s_root, s_cont, at, cnt, total, id, start, end, first);
        }
    }
}

// carry[t] for t = T - 1 .. 0: the smallest bound[u] of the tiles u > t, clamped to len -- the first boundary at or behind
// tile t's end.  One workgroup; the tiles in pieces of WP_CARRY_THREADS * WP_CARRY_PER from the last piece to the first: a
// thread takes the minimum of its WP_CARRY_PER consecutive tiles, the threads' minima are scanned by doubling through LDS,
// `behind` is what the pieces already done give, and the thread walks its tiles once more from the last to the first.
__global__ __launch_bounds__(WP_CARRY_THREADS) void k_wp_carry(const uint64_t *__restrict__ bound, const uint64_t T, const uint64_t len,
                                                              uint64_t *__restrict__ carry) {
    __shared__ uint64_t s_a[WP_CARRY_THREADS];
    const uint32_t tid = threadIdx.x;
    uint64_t behind = WP_NONE;
    for (uint64_t hi = T; hi > 0;) {
        const uint64_t lo = hi > WP_PIECE ? hi - WP_PIECE : 0, t0 = lo + (uint64_t)tid * WP_CARRY_PER;
        uint64_t v[WP_CARRY_PER];
        uint64_t a = WP_NONE;
#pragma unroll
        for (uint32_t k = 0; k < WP_CARRY_PER; k++) {
            v[k] = t0 + k < hi ? bound[t0 + k] : WP_NONE;
            a = std::min(a, v[k]);
        }
        for (uint32_t d = 1; d < WP_CARRY_THREADS; d <<= 1) { // a: the tiles of threads tid .. tid + 2 d - 1
            s_a[tid] = a;
            __syncthreads();
            if (tid + d < WP_CARRY_THREADS) a = std::min(a, s_a[tid + d]);
            __syncthreads();
        }
        s_a[tid] = a;
        __syncthreads();
        uint64_t x = std::min(tid + 1 < WP_CARRY_THREADS ? s_a[tid + 1] : WP_NONE, behind); // behind the thread's last tile
#pragma unroll
        for (int k = WP_CARRY_PER - 1; k >= 0; k--) {
            if (t0 + k < hi) carry[t0 + k] = std::min(x, len);
            x = std::min(x, v[k]);
        }
        behind = std::min(behind, s_a[0]);
        __syncthreads();
        hi = lo;
    }
}

WpPlan wp_plan(uint64_t len) {
    WpPlan P;
    P.ntiles = tiles_of(len, WP_TILE);
    Carver C;
    P.counts = C.part(P.ntiles);
    P.bound = C.part(P.ntiles);
    P.carry = C.part(P.ntiles);
    P.base = C.part(P.ntiles + 1);
    P.scan = C.part(replace_scan_words(P.ntiles));
    P.words = C.words();
    return P;
}

namespace {
inline bool plan_ok(const WpPlan &P, const RowCut &R, const WpArgs &A, const uint8_t *hay, const uint64_t *scratch) {
    return hay && scratch && R.len && P.ntiles == tiles_of(R.len, WP_TILE) && P.ntiles <= WP_MAX_TILES && A.max_word >= 1 &&
           A.max_word <= WP_MAX_WORD && R.n < (1ull << 38);
}
} // namespace

hipError_t wp_count(const AtTrie &T, const uint8_t *hay, const RowCut &R, const WpArgs &A, const WpPlan &P, uint64_t *scratch,
                    hipStream_t st) {
    if (!plan_ok(P, R, A, hay, scratch)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_wp<WP_MODE_COUNT>, dim3((uint32_t)P.ntiles), dim3(WP_THREADS), 0, st, T, hay, R, A, scratch + P.counts,
                       scratch + P.bound, nullptr, nullptr, 0ull, nullptr, nullptr, nullptr, nullptr);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if ((e = replace_scan(nullptr, nullptr, scratch + P.counts, P.ntiles, (int64_t *)(scratch + P.base), scratch + P.scan, st)) != hipSuccess)
        return e;
    hipLaunchKernelGGL(k_wp_carry, dim3(1), dim3(WP_CARRY_THREADS), 0, st, (const uint64_t *)(scratch + P.bound), P.ntiles, R.len,
                       scratch + P.carry);
    return hipGetLastError();
}

hipError_t wp_emit(const AtTrie &T, const uint8_t *hay, const RowCut &R, const WpArgs &A, const WpPlan &P, const uint64_t *scratch,
                   uint64_t total, int64_t *id, int64_t *start, int64_t *end, uint8_t *first, int64_t *row_offsets, hipStream_t st) {
    if (!plan_ok(P, R, A, hay, scratch) || !id || !start || !end || !first) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_wp<WP_MODE_EMIT>, dim3((uint32_t)P.ntiles), dim3(WP_THREADS), 0, st, T, hay, R, A, nullptr, nullptr,
                       (const int64_t *)(scratch + P.base), scratch + P.carry, total, id, start, end, first);
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? e : piece_rows(R, start, total, row_offsets, st);
}

} // namespace acx
