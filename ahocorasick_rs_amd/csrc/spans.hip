// spans.hip -- the span kernels behind acx_spans_device / acx_spans_rows_device (spans.hpp says what each step computes and
// what it relies on).  The find pipeline (kernels.hip) and the other stages are not touched: both scans are replace_scan's.
//
// The reverse segmented min-scan, in all three places it is made (the tile heads, a thread's records, a tile's threads), is
// the composition of functions x -> min(a, pass ? x : +inf), written (a, pass): x is what lies BEHIND an element in its row,
// a the element's own smallest live start, pass whether the row goes on behind it.
//   (a, p) o (b, q) = (min(a, p ? b : +inf), p && q)          identity: (+inf, true)
// It is associative and not commutative: the left operand is always the EARLIER element.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "spans.hpp"
#include "stage_device.hpp"

namespace acx {

constexpr uint32_t SP_IPT = SPANS_TILE / SPANS_THREADS; // records of one thread, consecutive
constexpr uint32_t SP_WAVES = SPANS_THREADS / 64;
constexpr uint64_t SP_INF = ~0ull;                       // never a live record's start: start < end
constexpr uint64_t SP_FRESH = 1, SP_WHOLE = 2;           // a tile's flags
constexpr uint64_t SP_PIECE = (uint64_t)SPANS_CARRY_THREADS * SPANS_CARRY_PER; // the tiles of one step of k_span_carry
static_assert(SP_IPT * SPANS_THREADS == SPANS_TILE && SP_IPT == 4, "a thread reads its 4 marks as one 16-byte LDS load");
static_assert(SPANS_THREADS % 64 == 0 && SPANS_CARRY_THREADS % 64 == 0, "whole waves");
static_assert((SPANS_CARRY_THREADS & (SPANS_CARRY_THREADS - 1)) == 0, "the carry's doubling steps");

__device__ inline uint64_t span_after(uint64_t a, uint32_t pass, uint64_t x) { return std::min(a, pass ? x : SP_INF); }
// does a live record that ends at `end` close its span, `next` being the smallest live start behind it in its row
__device__ inline bool span_closes(uint64_t end, uint64_t next, uint64_t gap) {
    return next == SP_INF || (next > end && next - end > gap); // (no difference wraps)
}

// Per tile t of records [base, base + cnt): LO[t] .. HI[t] - 1 are the rows h with base <= rec_off[h] < base + cnt -- the
// rows whose first record lies in the tile, empty ones included -- HI[t] <= rows; HEAD[t] the smallest live start among the
// tile's records in the row of record `base`; META[t]: SP_FRESH, record `base` is its row's first one (a row that is not
// empty begins there), SP_WHOLE, that row reaches the tile's end.  rec_off[0] = 0 and rec_off[rows] = n bound the searches;
// the clamps keep a caller's wrong offsets inside the rows.
__global__ __launch_bounds__(SPANS_THREADS) void k_span_tiles(const uint64_t *__restrict__ w, uint64_t n,
                                                              const int64_t *__restrict__ rec_off, uint64_t rows,
                                                              uint64_t *__restrict__ LO, uint64_t *__restrict__ HI,
                                                              uint64_t *__restrict__ HEAD, uint64_t *__restrict__ META) {
    __shared__ uint32_t s_stop;
    __shared__ uint64_t s_min[SP_WAVES];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t t = blockIdx.x, base = t * SPANS_TILE;
    const uint32_t cnt = (uint32_t)std::min<uint64_t>(SPANS_TILE, n - base);
    if (tid == 0) {
        const uint64_t lo = std::min(count_lt(rec_off, rows + 1, base), rows);
        const uint64_t up = std::min(count_le(rec_off, rows + 1, base), rows); // the first entry beyond `base`
        const uint64_t hi = std::min(count_le(rec_off, rows + 1, base + cnt - 1), rows);
        const uint64_t row_end = (uint64_t)rec_off[up];
        const uint32_t stop = row_end > base ? (uint32_t)std::min<uint64_t>(row_end - base, cnt) : cnt;
        LO[t] = lo;
        HI[t] = std::max(hi, lo);
        META[t] = (up > lo || t == 0 ? SP_FRESH : 0) | (stop == cnt ? SP_WHOLE : 0);
        s_stop = stop;
    }
    __syncthreads();
    const uint32_t stop = s_stop;
    uint64_t mn = SP_INF;
#pragma unroll
    for (uint32_t k = 0; k < SP_IPT; k++) {
        const uint32_t j = tid + k * SPANS_THREADS;
        if (j < stop) {
            const uint64_t s = w[(base + j) * 3 + 1], e = w[(base + j) * 3 + 2];
            if (s < e) mn = std::min(mn, s);
        }
    }
#pragma unroll
    for (uint32_t d = 32; d; d >>= 1) mn = std::min(mn, (uint64_t)__shfl_down((unsigned long long)mn, d));
    if (lane == 0) s_min[wave] = mn;
    __syncthreads();
    if (tid == 0) {
        for (uint32_t q = 1; q < SP_WAVES; q++) mn = std::min(mn, s_min[q]);
        HEAD[t] = mn;
    }
}

// CARRY[t] for t = T - 1 .. 0: what lies behind tile t's last record in that record's row.  Tile u as a function of what
// lies behind ITS last record: fresh, +inf whatever follows (the row of tile u - 1's last record ends there); else
// (HEAD[u], whole).  CARRY[t] = (tile t + 1 o tile t + 2 o ... o tile T - 1)(+inf).  One workgroup; the tiles in pieces of
// SPANS_CARRY_THREADS * SPANS_CARRY_PER from the last piece to the first: a thread composes its SPANS_CARRY_PER consecutive
// tiles, the threads' results are scanned by doubling through LDS, `behind` is what the pieces already done give, and the
// thread walks its tiles once more from the last to the first.
__global__ __launch_bounds__(SPANS_CARRY_THREADS) void k_span_carry(const uint64_t *__restrict__ HEAD,
                                                                    const uint64_t *__restrict__ META, uint64_t T,
                                                                    uint64_t *__restrict__ CARRY) {
    __shared__ uint64_t s_a[SPANS_CARRY_THREADS];
    __shared__ uint32_t s_p[SPANS_CARRY_THREADS];
    const uint32_t tid = threadIdx.x;
    uint64_t behind = SP_INF;
    for (uint64_t hi = T; hi > 0;) {
        const uint64_t lo = hi > SP_PIECE ? hi - SP_PIECE : 0, t0 = lo + (uint64_t)tid * SPANS_CARRY_PER;
        uint64_t ta[SPANS_CARRY_PER], fl[SPANS_CARRY_PER]; // the thread's own tiles, all loads before anything depends on them
        uint32_t tp[SPANS_CARRY_PER];
#pragma unroll
        for (uint32_t k = 0; k < SPANS_CARRY_PER; k++) {
            fl[k] = t0 + k < hi ? META[t0 + k] : SP_FRESH;
            ta[k] = t0 + k < hi ? HEAD[t0 + k] : SP_INF;
        }
        uint64_t a = SP_INF;
        uint32_t p = 1;
#pragma unroll
        for (int k = SPANS_CARRY_PER - 1; k >= 0; k--) {
            const bool in = t0 + k < hi; // (behind the piece: the identity)
            tp[k] = in ? (!(fl[k] & SP_FRESH) && (fl[k] & SP_WHOLE)) : 1;
            ta[k] = in && !(fl[k] & SP_FRESH) ? ta[k] : SP_INF;
            a = span_after(ta[k], tp[k], a);
            p = tp[k] && p;
        }
        for (uint32_t d = 1; d < SPANS_CARRY_THREADS; d <<= 1) { // (a, p): the tiles of threads tid .. tid + 2 d - 1
            s_a[tid] = a;
            s_p[tid] = p;
            __syncthreads();
            if (tid + d < SPANS_CARRY_THREADS) {
                a = span_after(a, p, s_a[tid + d]);
                p = p && s_p[tid + d];
            }
            __syncthreads();
        }
        s_a[tid] = a;
        s_p[tid] = p;
        __syncthreads();
        const bool last = tid + 1 == SPANS_CARRY_THREADS;
        uint64_t x = span_after(last ? SP_INF : s_a[tid + 1], last ? 1u : s_p[tid + 1], behind); // behind the thread's last tile
#pragma unroll
        for (int k = SPANS_CARRY_PER - 1; k >= 0; k--) {
            if (t0 + k < hi) CARRY[t0 + k] = x;
            x = span_after(ta[k], tp[k], x);
        }
        behind = span_after(s_a[0], s_p[0], behind);
        __syncthreads();
        hi = lo;
    }
}

// ---------------------------------------------------------------------------
// The tile pass, made twice: EMIT = false counts the tile's closers, EMIT = true stores its spans and row offsets.  Tile t
// is records [base, base + cnt); thread `tid` owns the consecutive slots 4 tid .. 4 tid + 3.
//
//   marks   the threads walk the rows LO[t] .. HI[t] - 1, SPANS_THREADS rows at a step, each row once: a row that is not
//           empty marks the slot of its first record in s_mark.  Empty rows cost this walk and nothing else.
//   records the start and end words of the thread's four records (8-byte loads), thread 0 those of record base - 1 too.
//   sufmin  a record's element is (its live start or +inf, no mark on the NEXT slot); the thread composes its four, the
//           wave's lanes scan from lane 63 down (__shfl_down), the waves' results go through LDS, CARRY[t] is what lies
//           behind the tile.  after[k] = sufmin(i + 1), sm[k] = sufmin(i).
//   close   span_closes() for every live record.
//   count   (EMIT = false) the closers of the tile, one word.
//   ranks   (EMIT = true) the closers before every slot (in the thread, __shfl_up, the waves' sums through LDS); the
//           closer's `end` and the opener's sufmin go to base[t] + rank; the ranks replace the marks in s_mark.
//   rows    (EMIT = true) row_off[h] = base[t] + the rank of slot rec_off[h] - base for the rows LO[t] .. HI[t] - 1; the
//           last tile goes on to h = rows: their slot is `cnt`, their value S.
// ---------------------------------------------------------------------------
template <bool EMIT>
__device__ __forceinline__ void span_tile(const uint64_t *__restrict__ w, uint64_t n, const int64_t *__restrict__ rec_off,
                                          uint64_t rows, uint64_t gap, const uint64_t *__restrict__ LO,
                                          const uint64_t *__restrict__ HI, const uint64_t *__restrict__ CARRY,
                                          uint64_t *__restrict__ counts, const int64_t *__restrict__ tbase, uint64_t S,
                                          int64_t *__restrict__ row_off, int64_t *__restrict__ start,
                                          int64_t *__restrict__ end) {
    __shared__ __attribute__((aligned(16))) uint32_t s_mark[SPANS_TILE];
    __shared__ uint64_t s_wa[SP_WAVES];
    __shared__ uint32_t s_wp[SP_WAVES], s_wcnt[SP_WAVES], s_wclose[SP_WAVES];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t t = blockIdx.x, base = t * SPANS_TILE;
    const uint32_t cnt = (uint32_t)std::min<uint64_t>(SPANS_TILE, n - base);
    const uint64_t lo = LO[t], hi = HI[t];

#pragma unroll
    for (uint32_t k = 0; k < SP_IPT; k++) s_mark[tid + k * SPANS_THREADS] = 0;
    __syncthreads();

    const uint32_t j0 = tid * SP_IPT;
    uint64_t rs[SP_IPT], re[SP_IPT];
#pragma unroll
    for (uint32_t k = 0; k < SP_IPT; k++) {
        const uint32_t j = j0 + k;
        rs[k] = j < cnt ? w[(base + j) * 3 + 1] : 0;
        re[k] = j < cnt ? w[(base + j) * 3 + 2] : 0;
    }
    uint64_t ps = 0, pe = 0; // record base - 1
    if (EMIT && tid == 0 && base) {
        ps = w[(base - 1) * 3 + 1];
        pe = w[(base - 1) * 3 + 2];
    }

    for (uint64_t h = lo + tid; h < hi; h += SPANS_THREADS) { // (hi <= rows: h + 1 is an entry)
        const uint64_t s = (uint64_t)rec_off[h], e = (uint64_t)rec_off[h + 1];
        if (e > s && s >= base && s - base < cnt) s_mark[s - base] = 1;
    }
    __syncthreads();

    const uint4 mk = *(const uint4 *)&s_mark[j0];
    uint32_t f[SP_IPT + 1] = {mk.x, mk.y, mk.z, mk.w, 0};
    if (j0 + SP_IPT < SPANS_TILE) f[SP_IPT] = s_mark[j0 + SP_IPT]; // (the last thread: CARRY[t] knows where the row ends)
    if (base == 0 && tid == 0) f[0] = 1;

    uint64_t v[SP_IPT];
    uint64_t ta = SP_INF;
    uint32_t tp = 1;
#pragma unroll
    for (int k = SP_IPT - 1; k >= 0; k--) {
        v[k] = rs[k] < re[k] ? rs[k] : SP_INF; // (a slot behind the tile's records: 0 < 0 is false)
        ta = span_after(v[k], !f[k + 1], ta);
        tp = tp && !f[k + 1];
    }
    // the wave: (ia, ip) becomes this thread's composed with every later lane's
    uint64_t ia = ta;
    uint32_t ip = tp;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint64_t a2 = (uint64_t)__shfl_down((unsigned long long)ia, d);
        const uint32_t p2 = __shfl_down(ip, d);
        if (lane + d < 64) {
            ia = span_after(ia, ip, a2);
            ip = ip && p2;
        }
    }
    if (lane == 0) {
        s_wa[wave] = ia;
        s_wp[wave] = ip;
    }
    uint64_t xa = (uint64_t)__shfl_down((unsigned long long)ia, 1); // the later lanes alone
    uint32_t xp = __shfl_down(ip, 1);
    if (lane == 63) {
        xa = SP_INF;
        xp = 1;
    }
    __syncthreads();
    uint64_t behind = CARRY[t];
    for (uint32_t q = SP_WAVES - 1; q > wave; q--) behind = span_after(s_wa[q], s_wp[q], behind);
    uint64_t nxt = span_after(xa, xp, behind); // what lies behind the thread's last record

    uint64_t sm[SP_IPT];
    uint32_t cl[SP_IPT], c = 0;
#pragma unroll
    for (int k = SP_IPT - 1; k >= 0; k--) {
        const uint64_t after = f[k + 1] ? SP_INF : nxt;
        sm[k] = std::min(v[k], after);
        cl[k] = v[k] != SP_INF && span_closes(re[k], after, gap);
        c += cl[k];
        nxt = sm[k];
    }

    uint32_t inc = c; // the closers up to and with this thread's, in its wave
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(inc, d);
        if (lane >= d) inc += up;
    }
    uint32_t prev = __shfl_up(cl[SP_IPT - 1], 1); // does the record before the thread's first close
    if (lane == 63) {
        s_wcnt[wave] = inc;
        s_wclose[wave] = cl[SP_IPT - 1];
    }
    __syncthreads();
    uint32_t before = 0, total = 0;
    for (uint32_t q = 0; q < SP_WAVES; q++) {
        if (q < wave) before += s_wcnt[q];
        total += s_wcnt[q];
    }
    if (!EMIT) {
        if (tid == 0) counts[t] = total;
        return;
    }

    if (lane == 0) prev = wave ? s_wclose[wave - 1] : (base == 0 || (ps < pe && span_closes(pe, sm[0], gap)));
    const uint64_t tb = (uint64_t)tbase[t];
    uint32_t r = before + inc - c;
#pragma unroll
    for (uint32_t k = 0; k < SP_IPT; k++) {
        const uint32_t j = j0 + k;
        s_mark[j] = r; // (every thread has read its marks before the barriers above)
        const uint64_t at = tb + r;
        const bool opens = (f[k] || (k ? cl[k ? k - 1 : 0] : prev)) && sm[k] != SP_INF && j < cnt;
        if (opens && at < S) start[at] = (int64_t)sm[k];
        if (cl[k] && at < S) end[at] = (int64_t)re[k];
        r += cl[k];
    }
    if (!row_off) return;
    __syncthreads();
    const uint64_t stop = t + 1 == gridDim.x ? rows + 1 : hi;
    for (uint64_t h = lo + tid; h < stop; h += SPANS_THREADS) {
        const uint64_t s = (uint64_t)rec_off[h];
        row_off[h] = (int64_t)(tb + (s >= base && s - base < cnt ? s_mark[s - base] : total));
    }
}

__global__ __launch_bounds__(SPANS_THREADS) void k_span_count(const uint64_t *__restrict__ w, uint64_t n,
                                                              const int64_t *__restrict__ rec_off, uint64_t rows, uint64_t gap,
                                                              const uint64_t *__restrict__ LO, const uint64_t *__restrict__ HI,
                                                              const uint64_t *__restrict__ CARRY, uint64_t *__restrict__ counts) {
    span_tile<false>(w, n, rec_off, rows, gap, LO, HI, CARRY, counts, nullptr, 0, nullptr, nullptr, nullptr);
}

__global__ __launch_bounds__(SPANS_THREADS) void k_span_emit(const uint64_t *__restrict__ w, uint64_t n,
                                                             const int64_t *__restrict__ rec_off, uint64_t rows, uint64_t gap,
                                                             const uint64_t *__restrict__ LO, const uint64_t *__restrict__ HI,
                                                             const uint64_t *__restrict__ CARRY, const int64_t *__restrict__ tbase,
                                                             uint64_t S, int64_t *__restrict__ row_off,
                                                             int64_t *__restrict__ start, int64_t *__restrict__ end) {
    span_tile<true>(w, n, rec_off, rows, gap, LO, HI, CARRY, nullptr, tbase, S, row_off, start, end);
}

uint64_t spans_tiles(uint64_t n) { return (n + SPANS_TILE - 1) / SPANS_TILE; }
uint64_t spans_temp_words(uint64_t n) { return 5 * spans_tiles(n); }

hipError_t spans_count(const acx_match_t *m, uint64_t n, const int64_t *rec_off, uint64_t rows, uint64_t gap, uint64_t *temp,
                       uint64_t *counts, hipStream_t st) {
    const uint64_t T = spans_tiles(n);
    if (!n || !rows || T >= (1ull << 31)) return hipErrorInvalidValue;
    uint64_t *LO = temp, *HI = temp + T, *HEAD = temp + 2 * T, *META = temp + 3 * T, *CARRY = temp + 4 * T;
    hipLaunchKernelGGL(k_span_tiles, dim3((uint32_t)T), dim3(SPANS_THREADS), 0, st, (const uint64_t *)m, n, rec_off, rows, LO, HI,
                       HEAD, META);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_span_carry, dim3(1), dim3(SPANS_CARRY_THREADS), 0, st, (const uint64_t *)HEAD, (const uint64_t *)META, T,
                       CARRY);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_span_count, dim3((uint32_t)T), dim3(SPANS_THREADS), 0, st, (const uint64_t *)m, n, rec_off, rows, gap,
                       (const uint64_t *)LO, (const uint64_t *)HI, (const uint64_t *)CARRY, counts);
    return hipGetLastError();
}

hipError_t spans_emit(const acx_match_t *m, uint64_t n, const int64_t *rec_off, uint64_t rows, uint64_t gap, const uint64_t *temp,
                      const int64_t *base, uint64_t S, int64_t *row_off, int64_t *start, int64_t *end, hipStream_t st) {
    const uint64_t T = spans_tiles(n);
    if (!n || !rows || T >= (1ull << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_span_emit, dim3((uint32_t)T), dim3(SPANS_THREADS), 0, st, (const uint64_t *)m, n, rec_off, rows, gap, temp,
                       temp + T, temp + 4 * T, base, S, row_off, start, end);
    return hipGetLastError();
}

} // namespace acx
