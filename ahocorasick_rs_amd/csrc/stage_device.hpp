// stage_device.hpp -- what the device stages behind the find pipeline (replace, filter, score, mask, spans, snippets) share:
// how a byte range is cut into rows, the searches in an ascending array, the funnel shift of the gathers, and the bounds of
// a tile -- of the output's bytes, or of the records -- with the size of the scratch that holds them, and the carver of a
// stage's temporaries (the walkers' plans, at.hpp .. wp.hpp, use it as the stages' API units do).  Everything here is
// inline or constexpr: any number of units include it, and a .cpp takes the struct and the sizes (the device functions are
// the HIP compiler's).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

namespace acx {

// How `len` bytes are cut into n rows, three ways: off != null (n + 1 device offsets from 0 to len), uniform_len > 0 (row h
// begins at h * uniform_len), or neither (one row of `len` bytes: n = 1).
struct RowCut {
    const uint64_t *off;
    uint64_t uniform_len;
    uint64_t n;
    uint64_t len;
};

// The scratch of a tile kernel, in u64 words: U then L.  Output side: an entry per tile BOUNDARY of `total` output bytes (one
// more than tiles); record side: an entry per tile of n records.
constexpr uint64_t tiles_of(uint64_t n, uint64_t tile) { return (n + tile - 1) / tile; }
constexpr uint64_t out_tile_words(uint64_t total, uint64_t tile) { return 2 * (tiles_of(total, tile) + 1); }
constexpr uint64_t rec_tile_words(uint64_t n, uint64_t tile) { return 2 * tiles_of(n, tile); }

// Carves one block of the buffer cache into a stage's temporaries, in u64 words: every part a multiple of 256 bytes behind the
// previous one, the block at least 256 bytes.
struct Carver {
    uint64_t at = 0;
    uint64_t part(uint64_t words) {
        const uint64_t here = at;
        at += (words + 31) / 32 * 32;
        return here;
    }
    uint64_t words() const { return std::max<uint64_t>(at, 32); }
    uint64_t bytes() const { return words() * 8; }
};

#ifdef __HIPCC__

// where row h begins (h = R.n: where the last one ends).  Offsets are the caller's word: nothing is clamped here.
__device__ inline uint64_t row_begin(const RowCut &R, uint64_t h) {
    if (R.off) return R.off[h];
    if (R.uniform_len) return h * R.uniform_len;
    return h ? R.len : 0;
}

// entries <= x / < x of o[0 .. n), o ascending (T: int64_t or uint64_t words, compared unsigned)
template <typename T>
__device__ inline uint64_t count_le(const T *o, uint64_t n, uint64_t x) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if ((uint64_t)o[mid] <= x) lo = mid + 1; else hi = mid;
    }
    return lo;
}
template <typename T>
__device__ inline uint64_t count_lt(const T *o, uint64_t n, uint64_t x) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if ((uint64_t)o[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__device__ inline uint4 funnel16(uint4 lo, uint4 hi, uint32_t s) { // bytes s .. s + 15 of lo:hi
    uint32_t v0 = lo.x, v1 = lo.y, v2 = lo.z, v3 = lo.w, v4 = hi.x, v5 = hi.y, v6 = hi.z, v7 = hi.w;
    if (s & 8) { v0 = v2; v1 = v3; v2 = v4; v3 = v5; v4 = v6; v5 = v7; }
    if (s & 4) { v0 = v1; v1 = v2; v2 = v3; v3 = v4; v4 = v5; }
    const uint32_t sh = s & 3;
    return make_uint4(__builtin_amdgcn_alignbyte(v1, v0, sh), __builtin_amdgcn_alignbyte(v2, v1, sh),
                      __builtin_amdgcn_alignbyte(v3, v2, sh), __builtin_amdgcn_alignbyte(v4, v3, sh));
}

// Output side, one thread per tile boundary t = 0 .. ntiles of `total` output bytes whose segments begin at o[0 .. n):
// U[t] = the segments that begin at or before t * TILE, L[t] = those that begin before it (clamped to the output's end) --
// tile t stages segments U[t] - 1 .. L[t + 1] - 1: from the last one that begins at or before the tile (it covers the tile's
// first byte: of several segments with one start, all but the last are empty) to the last one that begins inside it.
template <uint32_t TILE, typename T>
__device__ inline void out_tile_bounds(const T *o, uint64_t n, uint64_t total, uint64_t ntiles, uint64_t *U, uint64_t *L) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t > ntiles) return;
    const uint64_t x = std::min<uint64_t>(t * TILE, total);
    U[t] = count_le(o, n, x);
    L[t] = x ? count_le(o, n, x - 1) : 0;
}

// Record side, one thread per tile t < ntiles of TILE records: U[t] = the row that holds record t * TILE, L[t] = the row that
// holds the tile's last record -- the LAST row that begins at or before the record (of several rows with one start all but
// the last are empty).  rec_off[0] = 0 and rec_off[rows] = n bound both; the clamp keeps a caller's wrong offsets inside
// the rows.
template <uint32_t TILE>
__device__ inline void rec_tile_bounds(const int64_t *rec_off, uint64_t rows, uint64_t n, uint64_t ntiles, uint64_t *U,
                                       uint64_t *L) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ntiles) return;
    const uint64_t base = t * TILE, last = std::min<uint64_t>(base + TILE, n) - 1;
    U[t] = std::min<uint64_t>(std::max<uint64_t>(count_le(rec_off, rows + 1, base), 1) - 1, rows - 1);
    L[t] = std::min<uint64_t>(std::max<uint64_t>(count_le(rec_off, rows + 1, last), 1) - 1, rows - 1);
}

#endif // __HIPCC__

} // namespace acx
