// replace.hip -- the splice kernels behind acx_replace / acx_replace_device (replace.hpp says what each step computes).
// The find pipeline (kernels.hip) is not touched: these kernels read the records its write kernel left in HBM.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "replace.hpp"

namespace acx {

// ---------------------------------------------------------------------------
// 1. exclusive scan of signed 64-bit values, two launches per level (the shape of kernels.hip's k_block_partials /
//    k_block_prefix): a workgroup per RS_ITEMS values, RS_PER consecutive values per thread.  More than RS_ITEMS
//    workgroups: the partials are scanned the same way before the second launch reads its own entry of their prefix.
// ---------------------------------------------------------------------------
constexpr uint32_t RS_THREADS = 256, RS_PER = 8, RS_ITEMS = RS_THREADS * RS_PER;

struct GetI64 { // counts of a batch, or the partials of a level below
    const int64_t *v;
    __device__ int64_t operator()(uint64_t i) const { return v[i]; }
};
struct GetDelta { // what match i adds to the output's length
    const acx_match_t *m;
    const uint64_t *roff;
    __device__ int64_t operator()(uint64_t i) const {
        const acx_match_t x = m[i];
        return (int64_t)(roff[x.pattern + 1] - roff[x.pattern]) - (int64_t)(x.end - x.start);
    }
};

// exclusive scan of one value per thread over the workgroup; *total = the workgroup's sum
__device__ inline int64_t block_excl_scan(int64_t v, int64_t *s_wave, int64_t *total) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const long long t = __shfl_up(inc, (unsigned)d);
        if (lane >= (uint32_t)d) inc += t;
    }
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    int64_t before = 0, tot = 0;
#pragma unroll
    for (uint32_t w = 0; w < RS_THREADS / 64; w++) {
        if (w < wave) before += s_wave[w];
        tot += s_wave[w];
    }
    *total = tot;
    return before + inc - v;
}

template <typename Get>
__global__ __launch_bounds__(RS_THREADS) void k_rep_partials(Get get, uint64_t n, int64_t *partial) {
    __shared__ int64_t s_wave[RS_THREADS / 64];
    const uint64_t i0 = (uint64_t)blockIdx.x * RS_ITEMS + (uint64_t)threadIdx.x * RS_PER;
    int64_t sum = 0;
#pragma unroll
    for (uint32_t k = 0; k < RS_PER; k++)
        if (i0 + k < n) sum += get(i0 + k);
    int64_t tot;
    (void)block_excl_scan(sum, s_wave, &tot);
    if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

// pre: exclusive prefix of the partials (null: one workgroup); out[i] for i < n, and out[n] by the last workgroup
template <typename Get>
__global__ __launch_bounds__(RS_THREADS) void k_rep_prefix(Get get, uint64_t n, const int64_t *pre, int64_t *out) {
    __shared__ int64_t s_wave[RS_THREADS / 64];
    const uint64_t i0 = (uint64_t)blockIdx.x * RS_ITEMS + (uint64_t)threadIdx.x * RS_PER;
    int64_t v[RS_PER], sum = 0;
#pragma unroll
    for (uint32_t k = 0; k < RS_PER; k++) { v[k] = i0 + k < n ? get(i0 + k) : 0; sum += v[k]; }
    int64_t tot;
    const int64_t excl = block_excl_scan(sum, s_wave, &tot);
    const int64_t base = pre ? pre[blockIdx.x] : 0;
    int64_t run = base + excl;
#pragma unroll
    for (uint32_t k = 0; k < RS_PER; k++) { if (i0 + k < n) out[i0 + k] = run; run += v[k]; }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) out[n] = base + tot;
}

uint64_t replace_scan_words(uint64_t n) {
    if (n <= RS_ITEMS) return 0;
    const uint64_t nwg = (n + RS_ITEMS - 1) / RS_ITEMS;
    return nwg + (nwg + 1) + replace_scan_words(nwg);
}

template <typename Get>
hipError_t scan_level(Get get, uint64_t n, int64_t *out, int64_t *temp, hipStream_t st) {
    if (n == 0) return hipMemsetAsync(out, 0, 8, st);
    const uint64_t nwg = (n + RS_ITEMS - 1) / RS_ITEMS;
    if (nwg == 1) {
        hipLaunchKernelGGL(k_rep_prefix<Get>, dim3(1), dim3(RS_THREADS), 0, st, get, n, (const int64_t *)nullptr, out);
        return hipGetLastError();
    }
    int64_t *partial = temp, *pre = temp + nwg;
    hipLaunchKernelGGL(k_rep_partials<Get>, dim3((uint32_t)nwg), dim3(RS_THREADS), 0, st, get, n, partial);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = scan_level(GetI64{partial}, nwg, pre, temp + nwg + (nwg + 1), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_rep_prefix<Get>, dim3((uint32_t)nwg), dim3(RS_THREADS), 0, st, get, n, (const int64_t *)pre, out);
    return hipGetLastError();
}

hipError_t replace_scan(const acx_match_t *m, const uint64_t *roff, const uint64_t *counts, uint64_t n, int64_t *out,
                        uint64_t *temp, hipStream_t st) {
    if (m) return scan_level(GetDelta{m, roff}, n, out, (int64_t *)temp, st);
    return scan_level(GetI64{(const int64_t *)counts}, n, out, (int64_t *)temp, st);
}

// ---------------------------------------------------------------------------
// 2. where every replacement starts in the output, and every haystack's output bounds
// ---------------------------------------------------------------------------
__global__ void k_rep_positions(const acx_match_t *__restrict__ m, uint64_t n, const int64_t *__restrict__ P, RepSegs S,
                                uint64_t *o, uint64_t *out_off) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        uint64_t h = 0;
        if (S.first) { // the last haystack whose first match is at or before i (empty ones share their successor's)
            uint64_t lo = 0, hi = S.cut.n + 1;
            while (lo < hi) {
                const uint64_t mid = (lo + hi) >> 1;
                if (S.first[mid] <= i) lo = mid + 1; else hi = mid;
            }
            h = lo - 1;
        }
        o[i] = row_begin(S.cut, h) + m[i].start + (uint64_t)P[i];
    }
    if (i <= S.cut.n) {
        const uint64_t f = S.first ? S.first[i] : (i ? n : 0);
        out_off[i] = row_begin(S.cut, i) + (uint64_t)P[f];
    }
}

hipError_t replace_positions(const acx_match_t *m, uint64_t n, const int64_t *P, const RepSegs &S, uint64_t *o,
                             uint64_t *out_off, hipStream_t st) {
    const uint64_t threads = std::max(n, S.cut.n + 1);
    hipLaunchKernelGGL(k_rep_positions, dim3((uint32_t)((threads + 255) / 256)), dim3(256), 0, st, m, n, P, S, o, out_off);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// 3. the gather, output side.  Segment j (j = -1 .. n-1) of the output begins at o[j] (o[-1] = 0): replacement j
//    (r_j bytes of the blob), then the haystack up to the next segment at the shift P[j + 1] (input = output - shift).
//    A workgroup owns RG_TILE output bytes; its segments -- from the last one that begins at or before the tile up to
//    the last one that begins inside it -- are staged in LDS, RG_WIN at a time (a tile every byte of which is a
//    replacement of one byte holds 16 384 of them: rounds, each thread keeps its chunks in registers between them).
//    A thread owns RG_CHUNKS 16-byte chunks, one aligned 16-byte store each.  A chunk inside one segment's replacement
//    or haystack part is two aligned 16-byte loads and a funnel shift; a chunk that straddles a segment boundary (or a
//    round's) is assembled byte by byte.
// ---------------------------------------------------------------------------
constexpr uint32_t RG_THREADS = 256, RG_TILE = 16384, RG_CHUNKS = RG_TILE / 16 / RG_THREADS, RG_WIN = 1024;

// the replacements that begin at or before, and before, every boundary of the output's tiles (stage_device.hpp)
__global__ void k_rep_tiles(const uint64_t *__restrict__ o, uint64_t n, uint64_t total, uint64_t ntiles, uint64_t *U,
                            uint64_t *L) {
    out_tile_bounds<RG_TILE>(o, n, total, ntiles, U, L);
}

// 16 bytes at base + pos (pos + 16 <= size); the two aligned loads only where both lie inside [base, base + size)
__device__ inline uint4 load16(const uint8_t *base, uint64_t size, uint64_t pos) {
    const uintptr_t b = (uintptr_t)base, a = b + pos, a0 = a & ~(uintptr_t)15;
    if (a0 >= b && a0 + 32 <= b + size)
        return funnel16(*(const uint4 *)a0, *(const uint4 *)(a0 + 16), (uint32_t)(a & 15));
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 16; k++) w[k >> 2] |= (uint32_t)base[pos + k] << (8 * (k & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

__global__ __launch_bounds__(RG_THREADS) void k_rep_gather(const uint8_t *__restrict__ hay, uint64_t len,
                                                           const acx_match_t *__restrict__ m, const uint64_t *__restrict__ o,
                                                           const int64_t *__restrict__ P, const uint8_t *__restrict__ blob,
                                                           uint64_t blob_len, const uint64_t *__restrict__ roff,
                                                           const uint64_t *__restrict__ U, const uint64_t *__restrict__ L,
                                                           uint8_t *out, uint64_t total) {
    __shared__ uint64_t s_o[RG_WIN], s_roff[RG_WIN];
    __shared__ int64_t s_d[RG_WIN];
    __shared__ uint32_t s_r[RG_WIN];
    __shared__ uint64_t s_hi;
    const uint64_t T0 = (uint64_t)blockIdx.x * RG_TILE, T1 = std::min<uint64_t>(T0 + RG_TILE, total);
    const int64_t base = (int64_t)U[blockIdx.x] - 1, kend = (int64_t)L[blockIdx.x + 1];
    uint4 acc[RG_CHUNKS];
#pragma unroll
    for (uint32_t c = 0; c < RG_CHUNKS; c++) acc[c] = make_uint4(0, 0, 0, 0);
    for (int64_t wb = base; wb < kend; wb += RG_WIN) {
        const int64_t we = std::min<int64_t>(wb + RG_WIN, kend);
        const uint32_t cnt = (uint32_t)(we - wb);
        if (wb != base) __syncthreads(); // (the last round's readers are done with the window)
        for (uint32_t t = threadIdx.x; t < cnt; t += RG_THREADS) {
            const int64_t j = wb + (int64_t)t;
            if (j < 0) {
                s_o[t] = 0; s_d[t] = 0; s_r[t] = 0; s_roff[t] = 0;
            } else {
                const uint64_t p = m[j].pattern, r0 = roff[p];
                s_o[t] = o[j]; s_d[t] = P[j + 1]; s_roff[t] = r0; s_r[t] = (uint32_t)(roff[p + 1] - r0);
            }
        }
        if (threadIdx.x == 0) s_hi = we == kend ? T1 : o[we];
        __syncthreads();
        const uint64_t lo_w = wb == base ? T0 : s_o[0], hi_w = s_hi;
#pragma unroll
        for (uint32_t c = 0; c < RG_CHUNKS; c++) {
            const uint64_t x0 = T0 + 16ull * (c * RG_THREADS + threadIdx.x);
            const uint64_t a = std::max(x0, lo_w), b = std::min(x0 + 16, hi_w);
            if (a >= b) continue;
            uint32_t lo = 0, hi = cnt; // the segment of byte a: the last entry that begins at or before it
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (s_o[mid] <= a) lo = mid + 1; else hi = mid;
            }
            uint32_t j = lo - 1;
            const uint64_t oj = s_o[j], rend = oj + s_r[j], send = j + 1 < cnt ? s_o[j + 1] : hi_w;
            const bool whole = a == x0 && b == x0 + 16;
            if (whole && x0 + 16 <= rend) {
                acc[c] = load16(blob, blob_len, s_roff[j] + (x0 - oj));
            } else if (whole && x0 >= rend && x0 + 16 <= send) {
                acc[c] = load16(hay, len, x0 - (uint64_t)s_d[j]);
            } else {
                uint4 w = acc[c];
#pragma unroll 1
                for (uint64_t x = a; x < b; x++) {
                    while (j + 1 < cnt && s_o[j + 1] <= x) j++;
                    const uint64_t oo = s_o[j];
                    uint32_t v = x < oo + s_r[j] ? blob[s_roff[j] + (x - oo)] : hay[x - (uint64_t)s_d[j]];
                    const uint32_t k = (uint32_t)(x - x0), sh = 8 * (k & 3), keep = ~(0xFFu << sh), q = k >> 2;
                    v <<= sh; // (the byte into word q: selects, not an indexed register array)
                    w.x = q == 0 ? (w.x & keep) | v : w.x; w.y = q == 1 ? (w.y & keep) | v : w.y;
                    w.z = q == 2 ? (w.z & keep) | v : w.z; w.w = q == 3 ? (w.w & keep) | v : w.w;
                }
                acc[c] = w;
            }
        }
    }
#pragma unroll
    for (uint32_t c = 0; c < RG_CHUNKS; c++) {
        const uint64_t x0 = T0 + 16ull * (c * RG_THREADS + threadIdx.x);
        if (x0 < T1) *(uint4 *)(out + x0) = acc[c];
    }
}

hipError_t replace_gather(const uint8_t *hay, uint64_t len, const acx_match_t *m, uint64_t n, const uint64_t *o,
                          const int64_t *P, const uint8_t *blob, uint64_t blob_len, const uint64_t *roff, uint64_t *tiles,
                          uint8_t *out, uint64_t total, hipStream_t st) {
    if (!total) return hipSuccess;
    const uint64_t ntiles = tiles_of(total, RG_TILE);
    uint64_t *U = tiles, *L = tiles + ntiles + 1;
    hipLaunchKernelGGL(k_rep_tiles, dim3((uint32_t)((ntiles + 1 + 255) / 256)), dim3(256), 0, st, o, n, total, ntiles, U, L);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_rep_gather, dim3((uint32_t)ntiles), dim3(RG_THREADS), 0, st, hay, len, m, o, P, blob, blob_len, roff,
                       (const uint64_t *)U, (const uint64_t *)L, out, total);
    return hipGetLastError();
}

uint64_t replace_tile_words(uint64_t total) { return out_tile_words(total, RG_TILE); }

} // namespace acx
