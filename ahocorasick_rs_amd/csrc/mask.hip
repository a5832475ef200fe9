// mask.hip -- the cover kernels behind acx_mask_device / acx_mask_rows_device (mask.hpp says what each step computes).  The
// find pipeline (kernels.hip) and the other stages are not touched: the scan of the counts is replace_scan's.
//
// RELIED ON: every store of k_mask_paint writes the same byte value, `fill`.  Two records that overlap -- nested, identical,
// chained, in one tile or in two workgroups -- therefore need no order and no atomic: whichever store lands last, the byte
// holds `fill`.  The one order that matters is the stream's: the copy or the clear of `out` is complete before the paint.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "mask.hpp"

namespace acx {

constexpr uint32_t MK_IPT = MASK_TILE / MASK_THREADS; // records of one thread
constexpr uint32_t MK_WAVES = MASK_THREADS / 64;
static_assert(MK_IPT * MASK_THREADS == MASK_TILE && MK_IPT == 4, "a thread reads its 4 row-start slots as one 16-byte LDS load");
static_assert(MASK_THREADS % 64 == 0 && MASK_THREADS >= 48, "whole waves; threads 0 .. 15 and 32 .. 47 store a sweep's edge bytes");
static_assert(MASK_LONG >= 32, "a swept record holds a 16-byte boundary before its last one");

// per tile of MASK_TILE records the rows that hold its first and its last record (stage_device.hpp)
__global__ void k_mask_tiles(const int64_t *__restrict__ rec_off, uint64_t rows, uint64_t n, uint64_t ntiles,
                             uint64_t *__restrict__ U, uint64_t *__restrict__ L) {
    rec_tile_bounds<MASK_TILE>(rec_off, rows, n, ntiles, U, L);
}

// n bytes of the value f4 repeats, at p (global memory, any alignment): every store naturally aligned and inside [p, p + n).
// Pieces of 1, 2, 4, 8 bytes up to the first 16-byte boundary, 16-byte stores, pieces of 8, 4, 2, 1 behind the last one.  A
// piece that does not fit any more (n is short) leaves p aligned for every smaller piece that follows.
__device__ inline void mask_fill(uint8_t *p, uint64_t n, uint32_t f4) {
    if (((uintptr_t)p & 1) && n >= 1) { *p = (uint8_t)f4; p += 1; n -= 1; }
    if (((uintptr_t)p & 2) && n >= 2) { *(uint16_t *)p = (uint16_t)f4; p += 2; n -= 2; }
    if (((uintptr_t)p & 4) && n >= 4) { *(uint32_t *)p = f4; p += 4; n -= 4; }
    if (((uintptr_t)p & 8) && n >= 8) { *(uint2 *)p = make_uint2(f4, f4); p += 8; n -= 8; }
    for (; n >= 16; p += 16, n -= 16) *(uint4 *)p = make_uint4(f4, f4, f4, f4);
    if (n & 8) { *(uint2 *)p = make_uint2(f4, f4); p += 8; }
    if (n & 4) { *(uint32_t *)p = f4; p += 4; }
    if (n & 2) { *(uint16_t *)p = (uint16_t)f4; p += 2; }
    if (n & 1) *p = (uint8_t)f4;
}

// ---------------------------------------------------------------------------
// The tile kernel.  Tile t is records [base, base + cnt); its rows are r0 = U[t] .. r1 = L[t].  A non-empty row is named
// by the record it begins at, relative to the tile -- its slot, below MASK_TILE -- never by its distance from r0: there
// may be millions of empty rows between two records.
//
//   records the start and end words of every record (two 8-byte loads, lane l next to lane l + 1's record), all of a
//           thread's loads before anything depends on them.
//   rows    the threads walk r0 .. r1, MASK_THREADS rows at a step, each row once: a non-empty one writes its slot into
//           s_head[slot] and leaves its index in s_row[slot].  r0 begins at or before the tile: its slot is 0.  Empty rows
//           cost this walk and nothing else; those that sit exactly on a tile boundary belong to no tile at all.
//   owner   s_head[j] becomes the largest marked slot <= j, the slot of record j's row: thread t owns slots 4 t .. 4 t + 3,
//           an inclusive running maximum across the wave's lanes (__shfl_up), the waves' maxima through LDS.
//   paint   record j's row h = s_row[s_head[j]], the row's first byte and length (64-bit: rows and haystacks pass 2^32
//           bytes), the clip, and -- shorter than MASK_LONG -- the thread's own stores; else an entry of s_long.
//   sweep   every listed record by the whole workgroup: the bytes up to its first 16-byte boundary and behind its last one
//           by threads 0 .. 15 and 32 .. 47, the 16-byte words between 16 bytes per lane.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(MASK_THREADS) void k_mask_paint(const uint64_t *__restrict__ w, uint64_t n,
                                                             const int64_t *__restrict__ rec_off, RowCut R,
                                                             const uint64_t *__restrict__ U, const uint64_t *__restrict__ L,
                                                             uint32_t f4, uint8_t *out) {
    __shared__ uint64_t s_row[MASK_TILE];
    __shared__ __attribute__((aligned(16))) int32_t s_head[MASK_TILE];
    __shared__ uint64_t s_long[MASK_TILE][2];
    __shared__ int32_t s_wmax[MK_WAVES];
    __shared__ uint32_t s_nlong;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t base = (uint64_t)blockIdx.x * MASK_TILE;
    const uint32_t cnt = (uint32_t)std::min<uint64_t>(MASK_TILE, n - base);
    const uint64_t r0 = U[blockIdx.x], r1 = L[blockIdx.x];

#pragma unroll
    for (uint32_t k = 0; k < MK_IPT; k++) s_head[tid + k * MASK_THREADS] = -1;
    if (tid == 0) s_nlong = 0;
    __syncthreads();

    uint64_t rs[MK_IPT], re[MK_IPT];
#pragma unroll
    for (uint32_t k = 0; k < MK_IPT; k++) {
        const uint32_t j = tid + k * MASK_THREADS;
        rs[k] = j < cnt ? w[(base + j) * 3 + 1] : 0;
        re[k] = j < cnt ? w[(base + j) * 3 + 2] : 0;
    }

    for (uint64_t h = r0 + tid; h <= r1; h += MASK_THREADS) {
        const uint64_t s = (uint64_t)rec_off[h], e = (uint64_t)rec_off[h + 1];
        if (e > s) {
            const uint64_t slot = s > base ? s - base : 0;
            if (slot < cnt) { // (always, for offsets that rise)
                s_head[slot] = (int32_t)slot;
                s_row[slot] = h;
            }
        }
    }
    __syncthreads();

    // the running maximum of the marks; -1: no row start so far (never at slot 0 for offsets that rise)
    const uint32_t j0 = tid * MK_IPT;
    int4 v = *(const int4 *)&s_head[j0];
    v.y = std::max(v.x, v.y);
    v.z = std::max(v.y, v.z);
    v.w = std::max(v.z, v.w);
    int32_t inc = v.w;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const int32_t up = __shfl_up(inc, d);
        if (lane >= d) inc = std::max(inc, up);
    }
    if (lane == 63) s_wmax[wave] = inc;
    int32_t run = __shfl_up(inc, 1); // what lies before this thread in its wave ...
    if (lane == 0) run = -1;
    __syncthreads();
    for (uint32_t q = 0; q < wave; q++) run = std::max(run, s_wmax[q]); // ... and before the wave
    v.x = std::max(v.x, run);
    v.y = std::max(v.y, run);
    v.z = std::max(v.z, run);
    v.w = std::max(v.w, run);
    *(int4 *)&s_head[j0] = v;
    __syncthreads();

#pragma unroll
    for (uint32_t k = 0; k < MK_IPT; k++) {
        const uint32_t j = tid + k * MASK_THREADS;
        if (j >= cnt) continue;
        const int32_t hs = s_head[j];
        if (hs < 0) continue;
        const uint64_t h = s_row[hs];
        uint64_t b0 = 0, rl = R.len; // the row's first byte and its length
        if (R.off) {
            const uint64_t e0 = R.off[h + 1];
            b0 = R.off[h];
            rl = e0 > b0 ? e0 - b0 : 0;
        } else if (R.uniform_len) {
            b0 = h * R.uniform_len;
            rl = R.uniform_len;
        }
        b0 = std::min(b0, R.len); // (a caller's wrong offsets: every store stays inside [0, len))
        rl = std::min(rl, R.len - b0);
        const uint64_t e = std::min(re[k], rl), s = std::min(rs[k], e); // the record, clipped to its row
        if (e <= s) continue;
        if (e - s < MASK_LONG) {
            mask_fill(out + b0 + s, e - s, f4);
        } else {
            const uint32_t q = atomicAdd(&s_nlong, 1u);
            s_long[q][0] = b0 + s;
            s_long[q][1] = b0 + e;
        }
    }
    __syncthreads();

    const uint32_t nlong = s_nlong;
    const uint4 f16 = make_uint4(f4, f4, f4, f4);
    for (uint32_t q = 0; q < nlong; q++) {
        uint8_t *pa = out + s_long[q][0], *pb = out + s_long[q][1];
        const uint32_t head = (16 - ((uint32_t)(uintptr_t)pa & 15)) & 15, tail = (uint32_t)(uintptr_t)pb & 15; // (pb - pa >= 32)
        uint8_t *A = pa + head, *B = pb - tail;
        if (tid < head) pa[tid] = (uint8_t)f4;
        if (tid >= 32 && tid - 32 < tail) B[tid - 32] = (uint8_t)f4;
        for (uint8_t *x = A + (uint64_t)tid * 16; x < B; x += (uint64_t)MASK_THREADS * 16) *(uint4 *)x = f16;
    }
}

__global__ void k_mask_offsets(RowCut R, int64_t *__restrict__ o) {
    const uint64_t h = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (h > R.n) return;
    o[h] = (int64_t)row_begin(R, h);
}

uint64_t mask_tile_words(uint64_t n) { return rec_tile_words(n, MASK_TILE); }

hipError_t mask_paint(const acx_match_t *m, uint64_t n, const int64_t *rec_off, const RowCut &R, uint8_t fill, uint64_t *tiles,
                      uint8_t *out, hipStream_t st) {
    if (!n || !R.n || !R.len) return hipSuccess;
    const uint64_t ntiles = tiles_of(n, MASK_TILE);
    if (ntiles >= (1ull << 31)) return hipErrorInvalidValue;
    uint64_t *U = tiles, *L = tiles + ntiles;
    hipLaunchKernelGGL(k_mask_tiles, dim3((uint32_t)((ntiles + 255) / 256)), dim3(256), 0, st, rec_off, R.n, n, ntiles, U, L);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_mask_paint, dim3((uint32_t)ntiles), dim3(MASK_THREADS), 0, st, (const uint64_t *)m, n, rec_off, R,
                       (const uint64_t *)U, (const uint64_t *)L, (uint32_t)fill * 0x01010101u, out);
    return hipGetLastError();
}

hipError_t mask_offsets(const RowCut &R, int64_t *o, hipStream_t st) {
    if ((R.n + 256) / 256 >= (1ull << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_mask_offsets, dim3((uint32_t)((R.n + 256) / 256)), dim3(256), 0, st, R, o);
    return hipGetLastError();
}

} // namespace acx
