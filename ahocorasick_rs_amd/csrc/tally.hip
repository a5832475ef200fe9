// tally.hip -- the kernels behind acx_tally / acx_tally_device / acx_tally_rows_device (tally.hpp says what they compute).
// The find pipeline (kernels.hip) is not touched: the kernels read the records its write kernel left in HBM, and every
// prefix comes from replace.hip's scan.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "replace.hpp"
#include "tally.hpp"

namespace acx {

namespace {

constexpr uint32_t TL_SLOTS = 2 * TALLY_TILE;          // keys a workgroup has room for: 2 * TALLY_TILE - 1 staged, a power of two sorted
constexpr uint32_t TL_WORDS = TALLY_TILE / 32;         // words of a bitmap with one bit per record a row may begin at
constexpr uint32_t TL_IPT = TL_SLOTS / TALLY_THREADS;  // keys per thread at the widest staging
constexpr uint32_t TL_FLAG = 0x80000000u;
constexpr uint32_t TL_TILE_LOG2 = 11;
static_assert((1u << TL_TILE_LOG2) == TALLY_TILE, "the key's row field is log2(TALLY_TILE) bits");
static_assert(TL_WORDS <= 64 && TALLY_THREADS >= 64, "one wave scans the row-start bitmap");
static_assert(TALLY_THREADS % 64 == 0 && TL_SLOTS % TALLY_THREADS == 0, "whole waves, whole rounds of the workgroup");
static_assert(TALLY_ROW_MAX <= TALLY_TILE, "a row of the tile kernel ends inside the staged keys");

__device__ inline uint32_t bits_of(uint64_t v) { return v ? 64u - (uint32_t)__clzll((long long)v) : 0u; }

// first index i in [lo, hi] with a[i] >= x; a[hi] >= x is the caller's to know
__device__ inline uint64_t first_at_least(const int64_t *__restrict__ a, uint64_t lo, uint64_t hi, uint64_t x) {
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if ((uint64_t)a[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// first index i in [lo, hi] with a[i] > x; a[hi] > x is the caller's to know.  (minus one: the row that holds item x --
// the empty rows in front of it share its offset and lie below)
__device__ inline uint64_t first_above(const int64_t *__restrict__ a, uint64_t lo, uint64_t hi, uint64_t x) {
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if ((uint64_t)a[mid] <= x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// What the scan behind the sort carries for every sorted key i: hp = where i's run began (a maximum over "i if a run begins
// at i"), seg = the runs of i's row up to i (a sum that starts again where a row begins: TL_FLAG marks "a row began here or
// later").  Both are associative; {0, 0} is the identity (a run begins at key 0 anyway).
struct TlState { uint32_t hp, seg; };
__device__ inline TlState tl_op(TlState a, TlState b) {
    TlState r;
    r.hp = a.hp > b.hp ? a.hp : b.hp;
    r.seg = (b.seg & TL_FLAG) ? b.seg : a.seg + b.seg;
    return r;
}

} // namespace

// ---------------------------------------------------------------------------
// The tile kernel.  The record stream is cut into tiles of TALLY_TILE records; a workgroup owns the rows that BEGIN in
// its tile (binary searches in rec_off give the first and the last of them, as k_rep_tiles finds its segments).  Empty rows
// own nothing: there may be millions of them between two records, so a row is never named by its distance from the tile's
// first row -- a non-empty row is named by the record it begins at, relative to the tile: its slot, below TALLY_TILE.
//
//   rows    the threads walk the tile's rows (each row of the batch is walked by exactly one tile) and set the bit of every
//           non-empty row's slot in s_head, and in s_long when the row has more than row_max records; such a row's records
//           are added to *n_long (a 64-bit vector atomic) and left to tally_long.  One wave turns s_head into s_prev: the
//           last row start below every word of the bitmap.
//   stage   the records from the first owned row's first to the last owned row's last -- at most 2 * TALLY_TILE - 1, for
//           a row of TALLY_TILE records that begins at the tile's last record.  Of each record the pattern field alone is
//           loaded, one 8-byte load, lane l next to lane l + 1's record, all of a thread's loads before its first LDS
//           write.  The key of a record: (its row's slot) << pbits | pattern -- unique per non-empty row, monotone in the
//           row.  pbits = bits(n_patterns - 1) in the 32-bit form (log2(TALLY_TILE) + pbits <= 32), 24 in the 64-bit form.
//   pad     the keys of long rows' records and the slots up to the sort's power of two are all ones.  In the 32-bit form
//           at its limit that IS a real key (the last slot, the last pattern): a key is real by its POSITION -- the real
//           keys are counted while they are staged (n_real) and are the first n_real of the sorted keys, whatever an equal
//           pad behind them looks like.
//   sort    bitonic, in LDS, over the smallest power of two that holds the staged keys (at least one key per thread).
//   count   thread t takes sorted keys [t * ipt, (t + 1) * ipt): a run begins where key[i] != key[i - 1], a row where the
//           row fields differ.  One block scan (TlState) gives every key the start of its run and the rank of its run in
//           its row; the thread that holds a run's LAST key writes pattern and count (= last - start + 1) to the
//           temporaries at (row's first record) + rank, and the one that holds a row's last key writes nnz_row[h] = rank +
//           1, h from one more binary search among the tile's rows.  A row never has more runs than records: the slots of
//           two rows cannot collide.
//
// Tile numbers and record indexes are 64-bit, indexes within a tile 32-bit.  Stores are ordinary vector stores.
// ---------------------------------------------------------------------------
template <typename K>
__global__ __launch_bounds__(TALLY_THREADS) void k_tally_tiles(const uint64_t *__restrict__ w, uint64_t n,
                                                               const int64_t *__restrict__ rec_off, uint64_t rows,
                                                               uint32_t pbits, uint32_t row_max,
                                                               int64_t *__restrict__ tmp_pattern, int64_t *__restrict__ tmp_count,
                                                               uint64_t *__restrict__ nnz_row, unsigned long long *__restrict__ n_long) {
    __shared__ K s_key[TL_SLOTS];
    __shared__ uint32_t s_head[TL_WORDS], s_long[TL_WORDS];
    __shared__ int32_t s_prev[TL_WORDS + 1];
    __shared__ uint32_t s_real;
    __shared__ TlState s_wave[TALLY_THREADS / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const K PAD = (K) ~(K)0;
    const K pmask = (K)(((K)1 << pbits) - 1);
    const uint64_t n_tiles = (n + TALLY_TILE - 1) / TALLY_TILE;
    for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const uint64_t base = t * TALLY_TILE, end = std::min<uint64_t>(base + TALLY_TILE, n);
        // rows h_lo .. h_hi - 1 begin in [base, end) (rec_off[rows] = n >= end bounds both searches)
        const uint64_t h_lo = first_at_least(rec_off, 0, rows, base);
        const uint64_t h_hi = first_at_least(rec_off, h_lo, rows, end);
        if (h_lo == h_hi) continue; // (no row begins here: the tile lies inside a row.  The same for every thread)
        const uint64_t first = (uint64_t)rec_off[h_lo];
        const uint64_t last = std::min<uint64_t>((uint64_t)rec_off[h_hi], base + TL_SLOTS - 1);
        const uint32_t lo_slot = (uint32_t)(first - base), staged = (uint32_t)(last - first);
        if (!staged) continue; // (empty rows only)

        if (tid < TL_WORDS) { s_head[tid] = 0; s_long[tid] = 0; }
        if (tid == 0) s_real = 0;
        __syncthreads();
        for (uint64_t h = h_lo + tid; h < h_hi; h += TALLY_THREADS) {
            const uint64_t s = (uint64_t)rec_off[h], e = (uint64_t)rec_off[h + 1];
            if (e > s) {
                const uint32_t slot = (uint32_t)(s - base);
                atomicOr(&s_head[slot >> 5], 1u << (slot & 31));
                if (e - s > row_max) {
                    atomicOr(&s_long[slot >> 5], 1u << (slot & 31));
                    atomicAdd(n_long, (unsigned long long)(e - s));
                }
            }
        }
        __syncthreads();
        if (wave == 0) {
            int32_t v = -1;
            if (lane < TL_WORDS && s_head[lane]) v = (int32_t)((lane << 5) | (31u - (uint32_t)__clz((int)s_head[lane])));
#pragma unroll
            for (uint32_t d = 1; d < 64; d <<= 1) {
                const int32_t u = __shfl_up(v, d);
                if (lane >= d && u > v) v = u;
            }
            if (lane < TL_WORDS) s_prev[lane + 1] = v;
            if (lane == 0) s_prev[0] = -1;
        }
        __syncthreads();

        uint32_t m_sort = TALLY_THREADS;
        while (m_sort < staged) m_sort <<= 1; // (staged <= TL_SLOTS - 1)
        uint64_t pat[TL_IPT];
#pragma unroll
        for (uint32_t k = 0; k < TL_IPT; k++) {
            const uint32_t j = tid + k * TALLY_THREADS;
            pat[k] = 0;
            if (j < staged) pat[k] = w[3 * (first + j)];
        }
        uint32_t real = 0;
#pragma unroll
        for (uint32_t k = 0; k < TL_IPT; k++) {
            const uint32_t j = tid + k * TALLY_THREADS;
            if (j < m_sort) {
                K key = PAD;
                if (j < staged) {
                    // the row of record lo_slot + j begins at the last set bit of s_head at or below it (there is one:
                    // lo_slot itself is a row's slot)
                    const uint32_t at = lo_slot + j;
                    uint32_t r;
                    if (at >= TALLY_TILE) {
                        r = (uint32_t)s_prev[TL_WORDS];
                    } else {
                        const uint32_t below = s_head[at >> 5] & (0xFFFFFFFFu >> (31u - (at & 31)));
                        r = below ? ((at & ~31u) | (31u - (uint32_t)__clz((int)below))) : (uint32_t)s_prev[at >> 5];
                    }
                    if (!((s_long[r >> 5] >> (r & 31)) & 1u)) {
                        key = (K)(((K)r << pbits) | ((K)pat[k] & pmask));
                        real++;
                    }
                }
                s_key[j] = key;
            }
        }
        if (real) atomicAdd(&s_real, real);
        __syncthreads();
        const uint32_t n_real = s_real;
        if (n_real) {
            // ---- bitonic sort of s_key[0 .. m_sort)
            for (uint32_t k = 2; k <= m_sort; k <<= 1) {
                for (uint32_t j = k >> 1; j > 0; j >>= 1) {
                    for (uint32_t q = tid; q < m_sort / 2; q += TALLY_THREADS) {
                        const uint32_t i = ((q & ~(j - 1)) << 1) | (q & (j - 1)), p = i | j;
                        const K a = s_key[i], b = s_key[p];
                        if ((a > b) == ((i & k) == 0)) { s_key[i] = b; s_key[p] = a; }
                    }
                    __syncthreads();
                }
            }
            // ---- runs: where each began, and their rank in their row
            const uint32_t ipt = m_sort / TALLY_THREADS, i0 = tid * ipt;
            auto item = [&](uint32_t i) -> TlState {
                const K key = s_key[i], before = i ? s_key[i - 1] : key;
                const bool head = i == 0 || key != before, row_head = i == 0 || (key >> pbits) != (before >> pbits);
                return TlState{head ? i : 0u, (row_head ? TL_FLAG : 0u) | (head ? 1u : 0u)};
            };
            TlState agg{0, 0};
            for (uint32_t q = 0; q < ipt; q++)
                if (i0 + q < n_real) agg = tl_op(agg, item(i0 + q));
            TlState inc = agg;
#pragma unroll
            for (uint32_t d = 1; d < 64; d <<= 1) {
                TlState u;
                u.hp = __shfl_up(inc.hp, d);
                u.seg = __shfl_up(inc.seg, d);
                if (lane >= d) inc = tl_op(u, inc);
            }
            if (lane == 63) s_wave[wave] = inc;
            TlState run;
            run.hp = __shfl_up(inc.hp, 1u);
            run.seg = __shfl_up(inc.seg, 1u);
            if (lane == 0) run = TlState{0, 0};
            __syncthreads();
            TlState pre{0, 0};
            for (uint32_t v = 0; v < wave; v++) pre = tl_op(pre, s_wave[v]);
            run = tl_op(pre, run);
            for (uint32_t q = 0; q < ipt; q++) {
                const uint32_t i = i0 + q;
                if (i >= n_real) break;
                run = tl_op(run, item(i));
                const K key = s_key[i];
                const bool is_last = i + 1 == n_real;
                const K next = is_last ? key : s_key[i + 1];
                if (is_last || next != key) {
                    const uint32_t rank = (run.seg & ~TL_FLAG) - 1, slot = (uint32_t)(key >> pbits);
                    const uint64_t g = base + slot + rank;
                    tmp_pattern[g] = (int64_t)(key & pmask);
                    tmp_count[g] = (int64_t)(i - run.hp + 1);
                    if (is_last || (uint32_t)(next >> pbits) != slot) {
                        const uint64_t h = first_above(rec_off, h_lo, h_hi, base + slot) - 1;
                        nnz_row[h] = rank + 1;
                    }
                }
            }
        }
        __syncthreads(); // (the next tile's bitmaps and keys go where these were read)
    }
}

bool tally_keys32(uint64_t n_patterns) {
    uint32_t bits = 0;
    while (bits < 64 && n_patterns > 1 && ((n_patterns - 1) >> bits)) bits++;
    return TL_TILE_LOG2 + bits <= 32;
}

uint32_t tally_tiles_grid(uint64_t n) {
    const uint64_t tiles = (n + TALLY_TILE - 1) / TALLY_TILE;
    return (uint32_t)std::min<uint64_t>(tiles, TALLY_MAX_GRID);
}

hipError_t tally_tiles(const acx_match_t *m, uint64_t n, const int64_t *rec_off, uint64_t rows, uint64_t n_patterns,
                       uint32_t row_max, int64_t *tmp_pattern, int64_t *tmp_count, uint64_t *nnz_row, uint64_t *n_long,
                       hipStream_t st) {
    if (!n) return hipSuccess;
    if (n > UINT64_MAX / sizeof(acx_match_t) || n_patterns > (1ull << TALLY_PATTERN_BITS) || row_max > TALLY_ROW_MAX)
        return hipErrorInvalidValue;
    const uint32_t grid = tally_tiles_grid(n);
    // (a workgroup's passes: the tile numbers are 64-bit, and no workgroup makes 2^32 of them)
    if (((n + TALLY_TILE - 1) / TALLY_TILE + grid - 1) / grid >= (1ull << 32)) return hipErrorInvalidValue;
    const uint64_t *w = reinterpret_cast<const uint64_t *>(m);
    unsigned long long *nl = reinterpret_cast<unsigned long long *>(n_long);
    if (tally_keys32(n_patterns)) {
        uint32_t pbits = 0;
        while (n_patterns > 1 && ((n_patterns - 1) >> pbits)) pbits++;
        hipLaunchKernelGGL(k_tally_tiles<uint32_t>, dim3(grid), dim3(TALLY_THREADS), 0, st, w, n, rec_off, rows, pbits, row_max,
                           tmp_pattern, tmp_count, nnz_row, nl);
    } else {
        hipLaunchKernelGGL(k_tally_tiles<uint64_t>, dim3(grid), dim3(TALLY_THREADS), 0, st, w, n, rec_off, rows,
                           TALLY_PATTERN_BITS, row_max, tmp_pattern, tmp_count, nnz_row, nl);
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Rows of more than row_max records: one 100 MB document in the batch, a dense haystack -- or every row, when the caller
// lowered row_max to 0.  The last-resort form, a handful of plain passes around rocPRIM's radix sort:
//   k_tally_classify   per row: is it long, and its records if it is; two scans give every long row its rank among the
//                      long rows and the place of its keys
//   k_tally_long_keys  per record of a long row: (rank << 24) | pattern, and per long row: rank -> row
//   radix_sort_keys    over rank and pattern bits
//   k_tally_heads      per sorted key: does a run begin here (as a word, for the scan that numbers the runs)
//   k_tally_run_pos    per run: where it begins
//   k_tally_rle        per run: its pattern, its length (the next run's start minus its own) and its rank in its row (the
//                      runs before it minus the runs before its row's first key) into the temporaries; per row: nnz_row
// Every index is 64-bit; every kernel is a grid-stride loop of TL1_THREADS threads.
// ---------------------------------------------------------------------------
namespace {

constexpr uint32_t TL1_THREADS = 256, TL1_MAX_GRID = 4096;
constexpr uint64_t TL_PMASK = (1ull << TALLY_PATTERN_BITS) - 1;

uint32_t grid1(uint64_t n) { return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n + TL1_THREADS - 1) / TL1_THREADS, TL1_MAX_GRID)); }

// where the parts of tally_long's scratch begin, in words
struct LongLayout {
    uint64_t is_long, long_len, long_rank, long_off, scan_rows, keys_in, keys_out, hx, pos, long_row, scan_keys, sort, words;
    size_t sort_bytes;
    unsigned end_bit;
    LongLayout(uint64_t rows, uint64_t n_long, uint32_t row_max) {
        const uint64_t max_long_rows = std::min<uint64_t>(rows, n_long / ((uint64_t)row_max + 1)) + 1;
        unsigned rank_bits = 0;
        while (rank_bits < 40 && (max_long_rows >> rank_bits)) rank_bits++;
        end_bit = TALLY_PATTERN_BITS + rank_bits;
        sort_bytes = 0;
        (void)rocprim::radix_sort_keys(nullptr, sort_bytes, (const uint64_t *)nullptr, (uint64_t *)nullptr, (size_t)n_long, 0u,
                                       end_bit, (hipStream_t)0);
        uint64_t at = 0;
        auto part = [&](uint64_t w) { const uint64_t here = at; at += (w + 31) / 32 * 32; return here; };
        is_long = part(rows);
        long_len = part(rows);
        long_rank = part(rows + 1);
        long_off = part(rows + 1);
        scan_rows = part(replace_scan_words(rows));
        keys_in = part(n_long);
        keys_out = part(n_long);
        hx = part(n_long + 1);
        pos = part(n_long);
        long_row = part(max_long_rows);
        scan_keys = part(replace_scan_words(n_long));
        sort = part((sort_bytes + 7) / 8);
        words = at;
    }
};

__global__ __launch_bounds__(TL1_THREADS) void k_tally_classify(const int64_t *__restrict__ rec_off, uint64_t rows, uint32_t row_max,
                                                                uint64_t *__restrict__ is_long, uint64_t *__restrict__ long_len) {
    const uint64_t stride = (uint64_t)gridDim.x * TL1_THREADS;
    for (uint64_t h = (uint64_t)blockIdx.x * TL1_THREADS + threadIdx.x; h < rows; h += stride) {
        const uint64_t len = (uint64_t)(rec_off[h + 1] - rec_off[h]);
        const bool lng = len > row_max;
        is_long[h] = lng ? 1 : 0;
        long_len[h] = lng ? len : 0;
    }
}

__global__ __launch_bounds__(TL1_THREADS) void k_tally_long_keys(const uint64_t *__restrict__ w, const int64_t *__restrict__ rec_off,
                                                                 uint64_t rows, const int64_t *__restrict__ long_off,
                                                                 const int64_t *__restrict__ long_rank, uint64_t n_long,
                                                                 uint64_t *__restrict__ keys, uint64_t *__restrict__ long_row) {
    const uint64_t stride = (uint64_t)gridDim.x * TL1_THREADS;
    const uint64_t nl = std::min<uint64_t>(n_long, (uint64_t)long_off[rows]); // (the same number, counted twice)
    for (uint64_t g = (uint64_t)blockIdx.x * TL1_THREADS + threadIdx.x; g < nl; g += stride) {
        const uint64_t h = first_above(long_off, 0, rows, g) - 1; // (long_off[rows] = nl > g)
        const uint64_t in_row = g - (uint64_t)long_off[h], rank = (uint64_t)long_rank[h];
        keys[g] = (rank << TALLY_PATTERN_BITS) | (w[3 * ((uint64_t)rec_off[h] + in_row)] & TL_PMASK);
        if (in_row == 0) long_row[rank] = h;
    }
}

__global__ __launch_bounds__(TL1_THREADS) void k_tally_heads(const uint64_t *__restrict__ sorted, uint64_t n,
                                                             uint64_t *__restrict__ heads) {
    const uint64_t stride = (uint64_t)gridDim.x * TL1_THREADS;
    for (uint64_t i = (uint64_t)blockIdx.x * TL1_THREADS + threadIdx.x; i < n; i += stride)
        heads[i] = (i == 0 || sorted[i] != sorted[i - 1]) ? 1 : 0;
}

__global__ __launch_bounds__(TL1_THREADS) void k_tally_run_pos(const uint64_t *__restrict__ heads, const int64_t *__restrict__ hx,
                                                               uint64_t n, uint64_t *__restrict__ pos) {
    const uint64_t stride = (uint64_t)gridDim.x * TL1_THREADS;
    for (uint64_t i = (uint64_t)blockIdx.x * TL1_THREADS + threadIdx.x; i < n; i += stride)
        if (heads[i]) pos[hx[i]] = i;
}

__global__ __launch_bounds__(TL1_THREADS) void k_tally_rle(const uint64_t *__restrict__ sorted, uint64_t n,
                                                           const int64_t *__restrict__ hx, const uint64_t *__restrict__ pos,
                                                           const uint64_t *__restrict__ long_row, const int64_t *__restrict__ long_off,
                                                           const int64_t *__restrict__ rec_off, int64_t *__restrict__ tmp_pattern,
                                                           int64_t *__restrict__ tmp_count, uint64_t *__restrict__ nnz_row) {
    const uint64_t stride = (uint64_t)gridDim.x * TL1_THREADS;
    const uint64_t n_runs = (uint64_t)hx[n];
    for (uint64_t g = (uint64_t)blockIdx.x * TL1_THREADS + threadIdx.x; g < n_runs; g += stride) {
        const uint64_t i = pos[g], next = g + 1 < n_runs ? pos[g + 1] : n;
        const uint64_t key = sorted[i];
        const uint64_t h = long_row[key >> TALLY_PATTERN_BITS];
        const uint64_t seg = (uint64_t)long_off[h], at = (uint64_t)rec_off[h], len = (uint64_t)rec_off[h + 1] - at;
        const uint64_t rank = g - (uint64_t)hx[seg]; // (the row's first key begins a run)
        tmp_pattern[at + rank] = (int64_t)(key & TL_PMASK);
        tmp_count[at + rank] = (int64_t)(next - i);
        if (next == seg + len) nnz_row[h] = rank + 1;
    }
}

} // namespace

uint64_t tally_long_words(uint64_t rows, uint64_t n_long, uint32_t row_max) { return LongLayout(rows, n_long, row_max).words; }

hipError_t tally_long(const acx_match_t *m, const int64_t *rec_off, uint64_t rows, uint32_t row_max, uint64_t n_long,
                      uint64_t *scratch, int64_t *tmp_pattern, int64_t *tmp_count, uint64_t *nnz_row, hipStream_t st) {
    if (!n_long || !rows) return hipSuccess;
    const LongLayout L(rows, n_long, row_max);
    const uint64_t *w = reinterpret_cast<const uint64_t *>(m);
    uint64_t *is_long = scratch + L.is_long, *long_len = scratch + L.long_len, *keys_in = scratch + L.keys_in;
    uint64_t *keys_out = scratch + L.keys_out, *pos = scratch + L.pos, *long_row = scratch + L.long_row;
    int64_t *long_rank = (int64_t *)(scratch + L.long_rank), *long_off = (int64_t *)(scratch + L.long_off);
    int64_t *hx = (int64_t *)(scratch + L.hx);
    hipLaunchKernelGGL(k_tally_classify, dim3(grid1(rows)), dim3(TL1_THREADS), 0, st, rec_off, rows, row_max, is_long, long_len);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = replace_scan(nullptr, nullptr, is_long, rows, long_rank, scratch + L.scan_rows, st);
    if (e == hipSuccess) e = replace_scan(nullptr, nullptr, long_len, rows, long_off, scratch + L.scan_rows, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_tally_long_keys, dim3(grid1(n_long)), dim3(TL1_THREADS), 0, st, w, rec_off, rows, long_off, long_rank,
                       n_long, keys_in, long_row);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    size_t bytes = L.sort_bytes;
    e = rocprim::radix_sort_keys((void *)(scratch + L.sort), bytes, (const uint64_t *)keys_in, keys_out, (size_t)n_long, 0u,
                                 L.end_bit, st);
    if (e != hipSuccess) return e;
    uint64_t *heads = keys_in; // (the unsorted keys are not read again)
    hipLaunchKernelGGL(k_tally_heads, dim3(grid1(n_long)), dim3(TL1_THREADS), 0, st, keys_out, n_long, heads);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = replace_scan(nullptr, nullptr, heads, n_long, hx, scratch + L.scan_keys, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_tally_run_pos, dim3(grid1(n_long)), dim3(TL1_THREADS), 0, st, heads, hx, n_long, pos);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_tally_rle, dim3(grid1(n_long)), dim3(TL1_THREADS), 0, st, keys_out, n_long, hx, pos, long_row, long_off,
                       rec_off, tmp_pattern, tmp_count, nnz_row);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// out[row_offsets[h] + j] = tmp[rec_off[h] + j] for j < nnz_row[h] = row_offsets[h + 1] - row_offsets[h]: a thread per
// entry of the result, its row from a binary search in row_offsets (however long or empty the rows are, the threads have
// the same work).
// ---------------------------------------------------------------------------
namespace {

__global__ __launch_bounds__(TL1_THREADS) void k_tally_compact(const int64_t *__restrict__ row_offsets, uint64_t rows,
                                                               const int64_t *__restrict__ rec_off, uint64_t nnz,
                                                               const int64_t *__restrict__ tmp_pattern,
                                                               const int64_t *__restrict__ tmp_count, int64_t *__restrict__ pattern,
                                                               int64_t *__restrict__ count) {
    const uint64_t stride = (uint64_t)gridDim.x * TL1_THREADS;
    const uint64_t total = std::min<uint64_t>(nnz, (uint64_t)row_offsets[rows]);
    for (uint64_t q = (uint64_t)blockIdx.x * TL1_THREADS + threadIdx.x; q < total; q += stride) {
        const uint64_t h = first_above(row_offsets, 0, rows, q) - 1; // (row_offsets[rows] = total > q)
        const uint64_t src = (uint64_t)rec_off[h] + (q - (uint64_t)row_offsets[h]);
        pattern[q] = tmp_pattern[src];
        count[q] = tmp_count[src];
    }
}

} // namespace

hipError_t tally_compact(const int64_t *row_offsets, uint64_t rows, const int64_t *rec_off, uint64_t nnz,
                         const int64_t *tmp_pattern, const int64_t *tmp_count, int64_t *pattern, int64_t *count, hipStream_t st) {
    if (!nnz || !rows) return hipSuccess;
    hipLaunchKernelGGL(k_tally_compact, dim3(grid1(nnz)), dim3(TL1_THREADS), 0, st, row_offsets, rows, rec_off, nnz, tmp_pattern,
                       tmp_count, pattern, count);
    return hipGetLastError();
}

} // namespace acx
