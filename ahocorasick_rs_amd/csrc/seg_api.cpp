// seg_api.cpp -- greedy segmentation by the dictionary (seg.hpp has the definition): the host form of the definition, the
// device stage, the acx_segment* entry points and the accessors of their result.  No find runs: the chain reads the trie
// edges and the own lists every handle has.  The entries' preambles, the two-pass frames, the staged route and the host twin
// are the walkers' shared ones (result_block.hpp), the match kind's choice on the host is HostTrie::pick.
#include "seg.hpp"
#include "host_trie.hpp"
#include "result_block.hpp"

using namespace acxh;

// acx_segment / acx_segment_device: the patterns (`pieces` int64 words), the boundaries (pieces + 1) and the rows' offsets
// (rows + 1) in ONE block (result_block.hpp).  Device route: the stage's temporaries go back to the cache behind its kernels.
struct ACX_HIDDEN acx_seg : ResultBlock {
    enum { PATTERN, OFFSETS, ROW_OFFSETS, N_PARTS };
    uint64_t pieces = 0, rows = 0;

    int alloc() { return alloc_parts({pieces * 8, (pieces + 1) * 8, (rows + 1) * 8}); }
    int64_t *pattern() const { return at<int64_t>(PATTERN); }
    int64_t *offsets() const { return at<int64_t>(OFFSETS); }
    int64_t *row_offsets() const { return at<int64_t>(ROW_OFFSETS); }
    void shaped_like(const acx_seg &D) { pieces = D.pieces; rows = D.rows; }
};

namespace {

// what every entry point refuses before any device work, in this order (the offsets' checks stand between the two halves)
int seg_flags(uint32_t flags) { return flags & ~ACX_SEG_UTF8 ? fail(ACX_EINVAL, "unknown flags") : ACX_OK; }
int seg_sizes(uint32_t max_len, uint64_t len, uint64_t rows) {
    if (max_len > acx::SEG_MAX_STEP) return fail(ACX_ETOOBIG, "segment takes patterns of up to 256 bytes");
    if (acx::tiles_of(len, acx::SEG_TILE) > acx::SEG_MAX_TILES) return fail(ACX_ETOOBIG, "more tiles than a 32-bit grid");
    if (rows >= (1ull << 38)) return fail(ACX_ETOOBIG, "2^38 rows or more in one call");
    return ACX_OK;
}

uint32_t kernel_flags(const acx_automaton *a, uint32_t flags) {
    return ((flags & ACX_SEG_UTF8) ? acx::SEG_UTF8 : 0u) | (folds(a) ? acx::SEG_FOLD : 0u);
}

// The device stage on st as the two passes of two_pass / two_pass_raw.  count: k_seg<COUNT>, the tree, and T -- 8 bytes cross
// the bus, the stream is waited for; *temp: the stage's scratch, one block of the buffer cache.  emit: into columns sized by
// `total`, every word of the three is written.
struct SegStage {
    acx_automaton *a;
    const uint8_t *d_hay;
    acx::RowCut R;
    uint32_t kf;
    acx::SegPlan P{};

    int count(hipStream_t st, void **temp, uint64_t *total) {
        *total = 0;
        if (!R.len) return ACX_OK;
        P = acx::seg_plan(R.len, a->host.max_len, kf);
        HIPCHK(g_bufs.get(temp, P.words * 8, a->device));
        uint64_t *scratch = (uint64_t *)*temp;
        HIPCHK(acx::seg_count(acx::at_trie(a->dev), d_hay, R, a->host.match_kind, kf, P, scratch, st));
        HIPCHK(hipMemcpyAsync(total, acx::seg_total(P, scratch), 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        return *total > R.len ? fail(ACX_EDEVICE, "the tiles' counts do not sum to a number of pieces") : ACX_OK;
    }
    int emit(hipStream_t st, void *temp, uint64_t total, int64_t *pattern, int64_t *offsets, int64_t *row_offsets) const {
        if (!R.len) { // no piece: offsets[0] = len = 0, every row begins at piece 0
            HIPCHK(hipMemsetAsync(offsets, 0, 8, st));
            HIPCHK(hipMemsetAsync(row_offsets, 0, (R.n + 1) * 8, st));
            return ACX_OK;
        }
        HIPCHK(acx::seg_emit(acx::at_trie(a->dev), d_hay, R, a->host.match_kind, kf, P, (uint64_t *)temp, total, pattern, offsets,
                             row_offsets, st));
        return ACX_OK;
    }
};

// The device route under a lease: the stage on the context's stream, a device result.  Returns when T is known, with the
// emitting half in flight (Z->done).  d_hay and the offsets must stay valid until then.
int run_seg(acx_automaton *a, Ctx *c, const uint8_t *d_hay, uint64_t len, const Segments &G, uint32_t flags, acx_seg **out) {
    *out = nullptr;
    SegStage S{a, d_hay, row_cut(G, len), kernel_flags(a, flags)};
    acx_seg *Z = new_result<acx_seg>(a->device, true);
    if (!Z) return ACX_ENOMEM;
    Z->rows = S.R.n;
    return two_pass(
        c->stream, Z, &Z->pieces, nullptr, out, [&](hipStream_t st, void **temp, uint64_t *total) { return S.count(st, temp, total); },
        [&](hipStream_t st, void *temp, uint64_t total) { return S.emit(st, temp, total, Z->pattern(), Z->offsets(), Z->row_offsets()); });
}

// ... and of step 3: the unknown unit at p < L
uint64_t host_unit(const uint8_t *h, uint64_t p, uint64_t L, bool utf8) {
    const uint8_t b = h[p];
    if (!utf8 || b < 0xC0 || b > 0xF7) return 1;
    const uint64_t want = b < 0xE0 ? 2 : b < 0xF0 ? 3 : 4;
    uint64_t u = 1;
    while (u < want && p + u < L && (h[p + u] & 0xC0) == 0x80) u++;
    return u;
}

} // namespace

extern "C" {

int acx_segment_host(const acx_host_automaton_t *h, const uint8_t *hay, uint64_t len, const uint64_t *offsets, uint64_t n_hay,
                     uint32_t flags, int match_kind, uint64_t cap, int64_t *pattern, int64_t *offsets_out, int64_t *row_offsets,
                     uint64_t *n_pieces) {
    if (n_pieces) *n_pieces = 0;
    int rc = host_form_args(h && n_pieces, [&] { return seg_flags(flags); }, match_kind, any_kind, hay, len, offsets, &n_hay);
    if (rc != ACX_OK) return rc;
    if (cap && (!pattern || !offsets_out || !row_offsets)) return fail(ACX_EINVAL, "null argument");
    if ((rc = seg_sizes(h->host.max_len, len, n_hay)) != ACX_OK) return rc;
    const HostTrie T{h->host, (h->flags & ACX_BUILD_ASCII_CASE_INSENSITIVE) != 0};
    const bool utf8 = (flags & ACX_SEG_UTF8) != 0;
    // two passes of the loop: the count, then -- it fits -- the pieces
    for (int pass = 0; pass < 2; pass++) {
        uint64_t t = 0;
        for (uint64_t r = 0; r < n_hay; r++) {
            const uint64_t b = offsets ? offsets[r] : 0, L = offsets ? offsets[r + 1] : len;
            if (pass) row_offsets[r] = (int64_t)t;
            for (uint64_t p = b; p < L; t++) {
                int64_t pid;
                uint64_t e;
                if (!T.pick(hay, p, L, 0, match_kind, false, &pid, &e)) e = p + host_unit(hay, p, L, utf8);
                if (pass) { pattern[t] = pid; offsets_out[t] = (int64_t)p; }
                p = e;
            }
        }
        *n_pieces = t;
        if (t > cap || !pattern || !offsets_out || !row_offsets) return ACX_OK; // (nothing is written)
        if (pass) { offsets_out[t] = (int64_t)len; row_offsets[n_hay] = (int64_t)t; }
    }
    return ACX_OK;
}

int acx_segment_device(acx_automaton_t *a, const void *d_hay, uint64_t len, const uint64_t *d_offsets, uint64_t n_hay,
                       uint64_t uniform_len, uint32_t flags, acx_seg_t **out) {
    if (!a || !out) return fail(ACX_EINVAL, "null argument");
    *out = nullptr;
    int rc = seg_flags(flags);
    if (rc != ACX_OK) return rc;
    Segments G;
    rc = walk_device_args(d_hay, len, d_offsets, n_hay, uniform_len,
                          [&] { return (uintptr_t)d_offsets & 7 ? fail(ACX_EINVAL, "offsets must be 8-byte aligned") : ACX_OK; }, &G);
    if (rc != ACX_OK || (rc = seg_sizes(a->host.max_len, len, rows_of(G).n)) != ACX_OK) return rc;
    return leased(a, [&](Ctx *c) { return run_seg(a, c, (const uint8_t *)d_hay, len, G, flags, out); });
}

int acx_segment_into_device(acx_automaton_t *a, const void *d_hay, uint64_t len, const uint64_t *d_offsets, uint64_t n_hay,
                            uint64_t uniform_len, uint32_t flags, uint64_t cap, int64_t *d_pattern, int64_t *d_offsets_out,
                            int64_t *d_row_offsets, uint64_t *n_pieces) {
    if (!a || !n_pieces) return fail(ACX_EINVAL, "null argument");
    *n_pieces = 0;
    int rc = seg_flags(flags);
    if (rc != ACX_OK) return rc;
    Segments G;
    rc = walk_device_args(d_hay, len, d_offsets, n_hay, uniform_len, [&] {
        if (((uintptr_t)d_offsets | (uintptr_t)d_pattern | (uintptr_t)d_offsets_out | (uintptr_t)d_row_offsets) & 7)
            return fail(ACX_EINVAL, "offsets and the three columns must be 8-byte aligned");
        return !d_offsets_out || !d_row_offsets || (cap && !d_pattern) ? fail(ACX_EINVAL, "null argument") : ACX_OK;
    }, &G);
    if (rc != ACX_OK) return rc;
    SegStage S{a, (const uint8_t *)d_hay, row_cut(G, len), kernel_flags(a, flags)};
    if ((rc = seg_sizes(a->host.max_len, len, S.R.n)) != ACX_OK) return rc;
    return leased(a, [&](Ctx *c) {
        return two_pass_raw(
            a->device, c->stream, cap, n_pieces, [&](hipStream_t st, void **temp, uint64_t *total) { return S.count(st, temp, total); },
            [&](hipStream_t st, void *temp, uint64_t total) { return S.emit(st, temp, total, d_pattern, d_offsets_out, d_row_offsets); });
    });
}

int acx_segment(acx_automaton_t *a, const uint8_t *hay, uint64_t len, const uint64_t *offsets, uint64_t n_hay, uint32_t flags,
                int codepoints, acx_seg_t **out) {
    if (!a || !out) return fail(ACX_EINVAL, "null argument");
    *out = nullptr;
    int rc = seg_flags(flags);
    if (rc != ACX_OK) return rc;
    if (codepoints) flags |= ACX_SEG_UTF8;
    if ((rc = host_rows(hay, len, offsets, &n_hay, "null haystack")) != ACX_OK) return rc;
    if ((rc = seg_sizes(a->host.max_len, len, n_hay)) != ACX_OK) return rc;
    // the data (and, for a batch, its offsets) through the context's staging buffers; the same kernels; the block comes home
    // in one copy
    acx_seg *D = nullptr;
    rc = staged_walk(a, hay, len, offsets, n_hay, &D,
                     [&](Ctx *c, const Segments &G, acx_seg **dev) { return run_seg(a, c, c->ws.hay, len, G, flags, dev); });
    if ((rc = host_twin(rc, D, "the segments' copy", out)) != ACX_OK) return rc;
    if (!codepoints) return ACX_OK;
    acx_seg *Z = *out;
    // boundaries in characters: the characters that begin before each
    std::vector<uint64_t> cs;
    if ((rc = char_starts(hay, len, &cs)) != ACX_OK) { free_result(Z); *out = nullptr; return rc; }
    int64_t *off = Z->offsets();
    for (uint64_t k = 0; k <= Z->pieces; k++) off[k] = (int64_t)char_of(cs, (uint64_t)off[k]);
    return ACX_OK;
}

uint64_t acx_seg_count(const acx_seg_t *r) { return r ? r->pieces : 0; }
uint64_t acx_seg_rows(const acx_seg_t *r) { return r ? r->rows : 0; }
int acx_seg_on_device(const acx_seg_t *r) { return r ? r->on_device : 0; }

const int64_t *acx_seg_pattern(const acx_seg_t *r) { return (const int64_t *)part_ptr(r, acx_seg::PATTERN, acx_seg::N_PARTS); }
const int64_t *acx_seg_offsets(const acx_seg_t *r) { return (const int64_t *)part_ptr(r, acx_seg::OFFSETS, acx_seg::N_PARTS); }
const int64_t *acx_seg_row_offsets(const acx_seg_t *r) { return (const int64_t *)part_ptr(r, acx_seg::ROW_OFFSETS, acx_seg::N_PARTS); }
int acx_seg_copy(const acx_seg_t *r, int which, void *host_dst) {
    return part_copy(r, which, acx_seg::N_PARTS, host_dst, "no such part of a segment result");
}

void acx_free_seg(acx_seg_t *r) { free_result(r); }

} // extern "C"
