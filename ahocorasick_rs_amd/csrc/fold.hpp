// fold.hpp -- ASCII case folding of a haystack (acx_build_ex with ACX_BUILD_ASCII_CASE_INSENSITIVE).
//
// The crate's ascii_case_insensitive adds the opposite-case edge of every ASCII letter to the same trie node, so the
// case-insensitive automaton over P is the case-sensitive automaton over fold(P), fold: A-Z -> a-z, every other byte as
// it is.  A case-insensitive handle is compiled from the folded patterns and searches a folded copy of the haystack with
// the unchanged pipeline; the fold keeps byte lengths and never makes or unmakes a UTF-8 continuation byte, so offsets
// and code-point indexes are the caller's.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace acx {

// the four bytes of w folded: a byte gets 0x20 when its low seven bits lie in 'A' .. 'Z' and its top bit is clear (the
// two adds cannot carry out of a byte: seven bits + 0x3F / 0x25 < 0x100)
__host__ __device__ inline uint32_t fold_word(uint32_t w) {
    const uint32_t low7 = w & 0x7F7F7F7Fu;
    const uint32_t ge_a = low7 + 0x3F3F3F3Fu; // top bit: byte >= 'A' (0x41)
    const uint32_t gt_z = low7 + 0x25252525u; // top bit: byte > 'Z' (0x5A)
    return w | (((ge_a & ~gt_z & ~w) & 0x80808080u) >> 2);
}

__host__ __device__ inline uint8_t fold_byte(uint8_t b) { return (b >= 'A' && b <= 'Z') ? (uint8_t)(b | 0x20) : b; }

// host: dst[0 .. len) = fold(src[0 .. len)); dst == src folds in place
inline void fold_host(uint8_t *dst, const uint8_t *src, uint64_t len) {
    uint64_t i = 0;
    for (; i + 4 <= len; i += 4) {
        uint32_t w;
        __builtin_memcpy(&w, src + i, 4);
        w = fold_word(w);
        __builtin_memcpy(dst + i, &w, 4);
    }
    for (; i < len; i++) dst[i] = fold_byte(src[i]);
}

// device: dst[0 .. len) = fold(src[0 .. len)) in one launch on `st` (dst == src: in place).  Both pointers must have
// the same address modulo 16 (the body moves aligned 16-byte pieces); ranges that overlap other than exactly are not
// allowed.  n_cus sizes the grid.
hipError_t fold_device(const uint8_t *src, uint8_t *dst, uint64_t len, int n_cus, hipStream_t st);

} // namespace acx
