// seg.hip -- the segmenter's kernels behind acx_segment / acx_segment_device / acx_segment_into_device (seg.hpp has the
// definition and says what each kernel computes).  The find pipeline (kernels.hip) and the post-find stages are not touched:
// the walk is k_at's over tables every handle has, and the workgroup's steps around it -- the row marks, the suffix minimum, the
// survivors' list, the rank -- are the walkers' shared ones (at_walk.hpp).
//
// RELIED ON: k_seg<COUNT> and k_seg<EMIT> compute the same step[] from the same bytes, so the ranks of the emit pass add up
// to the counts the tree was built from.  A caller who writes the data between the two gets wrong pieces, but no store at or
// behind pattern[T] / offsets[T + 1]: every index is compared with the total the result was sized by.  A step is at least 1
// and at most E, and p + step never passes len: every chase ends, and an exit is an entry of the next tile.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "at_walk.hpp"
#include "seg.hpp"

namespace acx {

constexpr uint32_t SEG_BPT = SEG_TILE / SEG_THREADS; // consecutive bytes of one thread in the limits and in the ranking
constexpr uint32_t SEG_IPT = SEG_TILE / SEG_THREADS; // bytes of one thread, SEG_THREADS apart, in phase A's loads
constexpr uint32_t SEG_WAVES = SEG_THREADS / 64;
constexpr int SEG_MODE_COUNT = 0, SEG_MODE_EMIT = 1;
static_assert(SEG_THREADS == 256, "root_next is copied to LDS a word per thread; the entry map has a thread per entry");
static_assert(SEG_BPT == 16, "a word of the bitmap holds the bits of two threads");
static_assert(SEG_TILE <= 32768 && SEG_MAX_STEP <= SEG_THREADS && SEG_TILE + SEG_MAX_STEP < 65536,
              "slots, steps and limits are 16 bits wide, a tile's count shares a word with its exit");

// the unknown unit at p (seg.hpp): b = hay[p], lim >= 1 bytes remain in the row
__device__ inline uint32_t seg_unit(const uint8_t *__restrict__ hay, uint64_t p, uint32_t lim, uint8_t b, bool utf8) {
    if (!utf8 || b < 0xC0 || b > 0xF7) return 1;
    const uint32_t want = b < 0xE0 ? 2 : b < 0xF0 ? 3 : 4;
    uint32_t u = 1;
    while (u < want && u < lim && (hay[p + u] & 0xC0) == 0x80) u++; // (p + u < p + lim <= L)
    return u;
}

// COUNT: map0[tile * E + e] = pieces << 16 | exit.  EMIT: entry0 / base0: the tile's true entry and the index of its first
// piece; pattern, offsets: the result's columns, sized by `total`.
template <int MODE>
__global__ __launch_bounds__(SEG_THREADS) void k_seg(const AtTrie T, const uint8_t *__restrict__ hay, const RowCut R, const int kind,
                                                     const uint32_t flags, const uint32_t E, uint32_t *__restrict__ map0,
                                                     const uint32_t *__restrict__ entry0, const uint64_t *__restrict__ base0,
                                                     const uint64_t total, int64_t *__restrict__ pattern,
                                                     int64_t *__restrict__ offsets) {
    __shared__ uint32_t s_root[256];
    __shared__ uint16_t s_half[2][SEG_TILE]; // the two below; EMIT's jumps swing between them
    __shared__ uint32_t s_pid[SEG_TILE];     // A: a survivor's depth-1 state; then the pattern or AT_NONE; COUNT: then the jumps
    uint16_t(&s_step)[SEG_TILE] = s_half[0]; // A: the bytes the walk may read, min(L - p, 65535); then the step
    uint16_t(&s_list)[SEG_TILE] = s_half[1]; // the survivors' slots
    __shared__ uint32_t s_bits[SEG_TILE / 32]; // the row starts inside the tile; EMIT: then the piece starts
    __shared__ uint32_t s_w[SEG_WAVES];
    __shared__ uint64_t s_cut[2];
    __shared__ uint32_t s_n;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t tile = (uint64_t)blockIdx.x * SEG_TILE;
    const uint32_t in_tile = (uint32_t)std::min<uint64_t>(R.len - tile, SEG_TILE); // the tile's bytes of the data (tile < R.len)
    const uint64_t tile_end = tile + in_tile;
    const bool fold = (flags & SEG_FOLD) != 0, utf8 = (flags & SEG_UTF8) != 0;
    s_root[tid] = T.root_next[tid];
    if (tid < SEG_TILE / 32) s_bits[tid] = 0;
    if (tid == 0) s_n = 0;
    walk_row_range<false>(R, tile, tile_end, tid, s_cut);
    __syncthreads();

    // ---- A: the row starts strictly behind the tile's first byte as marks (walk_row_marks); `tail`: where the row of a byte
    // without a mark behind it ends
    const uint64_t tail = walk_row_marks<false, SEG_THREADS, SEG_TILE>(R, tile, tile_end, tid, s_cut, s_bits);
    __syncthreads();

    // ... every thread's first mark, a suffix minimum over the workgroup (walk_behind), and the limit of each of its 16 bytes
    {
        const uint32_t q0 = tid * SEG_BPT;
        const uint32_t bits = (s_bits[tid >> 1] >> (16 * (tid & 1))) & 0xFFFFu;
        uint32_t behind = walk_behind_wave(bits ? q0 + (uint32_t)__builtin_ctz(bits) : WALK_FAR, lane, wave, s_w);
        __syncthreads();
        behind = walk_behind<SEG_WAVES>(behind, wave, s_w); // the first mark behind this thread's bytes
#pragma unroll
        for (uint32_t j = 0; j < SEG_BPT; j++) {
            const uint32_t q = q0 + j;
            uint32_t lim = 0;
            if (q < in_tile) {
                const uint32_t m = bits >> (j + 1);
                const uint32_t next = m ? q + 1 + (uint32_t)__builtin_ctz(m) : behind;
                const uint64_t p = tile + q;
                // (a mark lies inside the data; tail <= len; wrong offsets may leave tail <= p: one byte, p + 1 <= len)
                lim = next != WALK_FAR ? next - q : tail > p ? (uint32_t)std::min<uint64_t>(tail - p, 65535) : 1u;
            }
            s_step[q] = (uint16_t)lim;
        }
    }
    __syncthreads();
    if (MODE == SEG_MODE_EMIT && tid < SEG_TILE / 32) s_bits[tid] = 0; // (the marks are spent: the flags of the piece starts)

    // ... the first byte of every position; the survivors into the list (walk_push)
#pragma unroll
    for (uint32_t k = 0; k < SEG_IPT; k++) {
        const uint32_t slot = k * SEG_THREADS + tid;
        const uint32_t lim = s_step[slot];
        uint32_t s1 = 0;
        if (lim) { // (tile + slot < len)
            const uint8_t b = hay[tile + slot];
            s1 = s_root[fold ? fold_byte(b) : b];
            if (!s1) s_step[slot] = (uint16_t)seg_unit(hay, tile + slot, lim, b, utf8);
        } else {
            s_step[slot] = 1; // (behind the data: never chased)
        }
        const bool survive = s1 != 0;
        s_pid[slot] = survive ? s1 : AT_NONE;
        walk_push(survive, slot, lane, &s_n, s_list);
    }
    __syncthreads();

    // ... the walks, a survivor per lane: the match kind's choice (at_best), or the unknown unit
    const uint32_t n_live = s_n; // (<= SEG_TILE: every slot is listed at most once)
    for (uint32_t j = tid; j < n_live; j += SEG_THREADS) {
        const uint32_t slot = s_list[j];
        const uint64_t p = tile + slot;
        const uint32_t lim = s_step[slot];
        uint32_t best, best_len;
        at_best(T, hay, p, lim, s_pid[slot], fold, kind, best, best_len);
        if (best == AT_NONE) best_len = seg_unit(hay, p, lim, hay[p], utf8);
        s_step[slot] = (uint16_t)best_len; // (1 <= best_len <= min(lim, E))
        s_pid[slot] = best;
    }
    __syncthreads();

    if (MODE == SEG_MODE_COUNT) {
        // ---- B: the entry map.  jump[q] = hops << 16 | target: `hops` steps from q land at `target`.  A round replaces it
        // by the jump of its target on top of its own; every word is written by its owner alone and ANY word read is a
        // true pair, so the rounds need no second buffer.  A round at least doubles every chain's hops: 13 rounds at most.
        uint32_t *jump = s_pid; // (COUNT stores no pattern: the words are free)
#pragma unroll
        for (uint32_t k = 0; k < SEG_IPT; k++) {
            const uint32_t slot = k * SEG_THREADS + tid;
            jump[slot] = 1u << 16 | (slot + s_step[slot]);
        }
        __syncthreads();
        int more;
        do {
            more = 0;
#pragma unroll
            for (uint32_t k = 0; k < SEG_IPT; k++) {
                const uint32_t slot = k * SEG_THREADS + tid;
                const uint32_t w = jump[slot];
                if ((w & 0xFFFFu) < in_tile) {
                    const uint32_t w2 = jump[w & 0xFFFFu];
                    jump[slot] = ((w & 0xFFFF0000u) + (w2 & 0xFFFF0000u)) | (w2 & 0xFFFFu);
                    more |= (w2 & 0xFFFFu) < in_tile;
                }
            }
        } while (__syncthreads_or(more));
        if (tid < E) {
            const uint32_t w = tid < in_tile ? jump[tid] : 0u; // (an entry at or beyond len exits at once)
            const uint32_t q = w & 0xFFFFu;
            uint32_t exit = q >= SEG_TILE ? q - SEG_TILE : 0u; // (the data ends in this tile: no tile takes the exit)
            if (exit >= E) exit = 0;                           // (never: a step is at most E)
            map0[(uint64_t)blockIdx.x * E + tid] = (w & 0xFFFF0000u) | exit;
        }
        return;
    }

    // ---- EMIT: the piece starts are the positions on the chain from the true entry.  Round k holds every position's
    // 2^k-th successor; the marked positions mark theirs, which doubles the marked stretch of the chain (a position marked
    // in the same round may mark too: its successor is on the chain as well); then the successors are squared into the other
    // buffer.  The workgroup ranks the marks (walk_rank) and stores.
    const uint32_t q0 = tid * SEG_BPT;
    {
#pragma unroll
        for (uint32_t k = 0; k < SEG_IPT; k++) {
            const uint32_t slot = k * SEG_THREADS + tid;
            s_half[0][slot] = (uint16_t)(slot + s_half[0][slot]); // (at most SEG_TILE + SEG_MAX_STEP)
        }
        if (tid == 0) {
            const uint32_t e0 = entry0[blockIdx.x];
            if (e0 < in_tile) s_bits[e0 >> 5] = 1u << (e0 & 31);
        }
        __syncthreads();
        uint32_t cur = 0;
        int more;
        do {
            more = 0;
            for (uint32_t m = (s_bits[tid >> 1] >> (16 * (tid & 1))) & 0xFFFFu; m; m &= m - 1) {
                const uint32_t t = s_half[cur][q0 + (uint32_t)__builtin_ctz(m)];
                if (t < in_tile) walk_mark(s_bits, t);
            }
#pragma unroll
            for (uint32_t k = 0; k < SEG_IPT; k++) {
                const uint32_t slot = k * SEG_THREADS + tid;
                const uint32_t t = s_half[cur][slot];
                const uint32_t t2 = t < in_tile ? s_half[cur][t] : t;
                s_half[cur ^ 1][slot] = (uint16_t)t2;
                more |= t2 < in_tile;
            }
            cur ^= 1;
        } while (__syncthreads_or(more));
    }
    const uint32_t bits = (s_bits[tid >> 1] >> (16 * (tid & 1))) & 0xFFFFu;
    const uint32_t c = (uint32_t)__popc(bits);
    const uint32_t inc = walk_rank_wave(c, lane, wave, s_w); // (s_w's minima were read before the barriers above)
    __syncthreads();
    uint64_t at = base0[blockIdx.x] + walk_rank<SEG_WAVES>(inc, c, wave, s_w); // the rank of this thread's first piece
    for (uint32_t t = bits; t; t &= t - 1, at++) {
        const uint32_t q = q0 + (uint32_t)__builtin_ctz(t);
        if (at >= total) break;
        const uint32_t pid = s_pid[q];
        offsets[at] = (int64_t)(tile + q);
        pattern[at] = pid == AT_NONE ? -1 : (int64_t)pid;
    }
    if (blockIdx.x == gridDim.x - 1 && tid == 0) offsets[total] = (int64_t)R.len;
}

// one step of a chain through the maps of a level: child's map at entry x -> the pieces it adds, x becomes its exit
template <bool LEAF>
__device__ inline uint64_t seg_step_map(const uint32_t *__restrict__ c_exit, const uint64_t *__restrict__ c_cnt, uint64_t child,
                                        uint32_t E, uint32_t &x) {
    const uint64_t at = child * E + x;
    uint64_t pieces;
    if (LEAF) {
        const uint32_t w = c_exit[at];
        pieces = w >> 16;
        x = w & 0xFFFFu;
    } else {
        pieces = c_cnt[at];
        x = c_exit[at];
    }
    if (x >= E) x = 0; // (never: the maps are this call's own)
    return pieces;
}

// the up-sweep: a lane per (parent, entry) folds the parent's children.  LEAF: the children are level 0's packed words
template <bool LEAF>
__global__ __launch_bounds__(SEG_THREADS) void k_seg_compose(const uint32_t *__restrict__ c_exit, const uint64_t *__restrict__ c_cnt,
                                                             const uint64_t n_child, const uint32_t E, uint32_t *__restrict__ p_exit,
                                                             uint64_t *__restrict__ p_cnt, const uint64_t n_parent) {
    const uint64_t i = (uint64_t)blockIdx.x * SEG_THREADS + threadIdx.x;
    const uint64_t parent = i / E;
    if (parent >= n_parent) return;
    uint32_t x = (uint32_t)(i % E);
    uint64_t pieces = 0;
    for (uint32_t k = 0; k < SEG_FAN; k++) {
        const uint64_t child = parent * SEG_FAN + k;
        if (child >= n_child) break;
        pieces += seg_step_map<LEAF>(c_exit, c_cnt, child, E, x);
    }
    p_exit[i] = x;
    p_cnt[i] = pieces;
}

// the down-sweep: a thread per parent gives its children their entries and bases.  p_entry == null: the root, entry 0, base 0
template <bool LEAF>
__global__ __launch_bounds__(SEG_THREADS) void k_seg_resolve(const uint32_t *__restrict__ c_exit, const uint64_t *__restrict__ c_cnt,
                                                             const uint64_t n_child, const uint32_t E,
                                                             const uint32_t *__restrict__ p_entry, const uint64_t *__restrict__ p_base,
                                                             const uint64_t n_parent, uint32_t *__restrict__ c_entry,
                                                             uint64_t *__restrict__ c_base) {
    const uint64_t parent = (uint64_t)blockIdx.x * SEG_THREADS + threadIdx.x;
    if (parent >= n_parent) return;
    uint32_t x = p_entry ? p_entry[parent] : 0u;
    uint64_t pieces = p_entry ? p_base[parent] : 0ull;
    if (x >= E) x = 0;
    for (uint32_t k = 0; k < SEG_FAN; k++) {
        const uint64_t child = parent * SEG_FAN + k;
        if (child >= n_child) break;
        c_entry[child] = x;
        c_base[child] = pieces;
        pieces += seg_step_map<LEAF>(c_exit, c_cnt, child, E, x);
    }
}

namespace {
inline uint32_t *u32_at(uint64_t *scratch, uint64_t word) { return (uint32_t *)(scratch + word); }
inline dim3 grid_of(uint64_t threads) { return dim3((uint32_t)tiles_of(threads, SEG_THREADS)); }
inline bool plan_ok(const SegPlan &P, const RowCut &R, const uint8_t *hay, const uint64_t *scratch) {
    return hay && scratch && R.len && P.ntiles == tiles_of(R.len, SEG_TILE) && P.ntiles <= SEG_MAX_TILES && P.levels >= 1 &&
           P.E >= 1 && P.E <= SEG_MAX_STEP && R.n < (1ull << 38);
}
} // namespace

hipError_t seg_count(const AtTrie &T, const uint8_t *hay, const RowCut &R, int kind, uint32_t flags, const SegPlan &P,
                     uint64_t *scratch, hipStream_t st) {
    if (!plan_ok(P, R, hay, scratch)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_seg<SEG_MODE_COUNT>, dim3((uint32_t)P.ntiles), dim3(SEG_THREADS), 0, st, T, hay, R, kind, flags, P.E,
                       u32_at(scratch, P.map0), nullptr, nullptr, 0ull, nullptr, nullptr);
    for (int l = 1; l <= P.levels; l++) {
        uint32_t *p_exit = u32_at(scratch, P.exits[l]);
        uint64_t *p_cnt = scratch + P.counts[l];
        if (l == 1)
            hipLaunchKernelGGL(k_seg_compose<true>, grid_of(P.n[1] * P.E), dim3(SEG_THREADS), 0, st, u32_at(scratch, P.map0), nullptr,
                               P.n[0], P.E, p_exit, p_cnt, P.n[1]);
        else
            hipLaunchKernelGGL(k_seg_compose<false>, grid_of(P.n[l] * P.E), dim3(SEG_THREADS), 0, st, u32_at(scratch, P.exits[l - 1]),
                               scratch + P.counts[l - 1], P.n[l - 1], P.E, p_exit, p_cnt, P.n[l]);
    }
    return hipGetLastError();
}

hipError_t seg_emit(const AtTrie &T, const uint8_t *hay, const RowCut &R, int kind, uint32_t flags, const SegPlan &P,
                    uint64_t *scratch, uint64_t total, int64_t *pattern, int64_t *offsets, int64_t *row_offsets, hipStream_t st) {
    if (!plan_ok(P, R, hay, scratch) || !pattern || !offsets) return hipErrorInvalidValue;
    for (int l = P.levels; l >= 1; l--) {
        const uint32_t *p_entry = l == P.levels ? nullptr : u32_at(scratch, P.entry[l]);
        const uint64_t *p_base = l == P.levels ? nullptr : scratch + P.base[l];
        uint32_t *c_entry = u32_at(scratch, P.entry[l - 1]);
        uint64_t *c_base = scratch + P.base[l - 1];
        if (l == 1)
            hipLaunchKernelGGL(k_seg_resolve<true>, grid_of(P.n[1]), dim3(SEG_THREADS), 0, st, u32_at(scratch, P.map0), nullptr, P.n[0],
                               P.E, p_entry, p_base, P.n[1], c_entry, c_base);
        else
            hipLaunchKernelGGL(k_seg_resolve<false>, grid_of(P.n[l]), dim3(SEG_THREADS), 0, st, u32_at(scratch, P.exits[l - 1]),
                               scratch + P.counts[l - 1], P.n[l - 1], P.E, p_entry, p_base, P.n[l], c_entry, c_base);
    }
    hipLaunchKernelGGL(k_seg<SEG_MODE_EMIT>, dim3((uint32_t)P.ntiles), dim3(SEG_THREADS), 0, st, T, hay, R, kind, flags, P.E, nullptr,
                       u32_at(scratch, P.entry[0]), scratch + P.base[0], total, pattern, offsets);
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? e : piece_rows(R, offsets, total, row_offsets, st);
}

} // namespace acx
