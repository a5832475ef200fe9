// seg_api.cpp -- greedy segmentation by the dictionary (seg.hpp has the definition): the host form of the definition, the
// device stage, the acx_segment* entry points and the accessors of their result.  No find runs: the chain reads the trie
// edges and the own lists every handle has.
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

// The counting half of the device stage on st: k_seg<COUNT>, the tree, and T -- 8 bytes cross the bus, the stream is waited
// for.  *temp: the stage's scratch, one block of the buffer cache -- the caller's to return, behind the stage's kernels.
int seg_count_stage(acx_automaton *a, hipStream_t st, const uint8_t *d_hay, const acx::RowCut &R, uint32_t kf, acx::SegPlan *P,
                    void **temp, uint64_t *total) {
    *total = 0;
    if (!R.len) return ACX_OK;
    *P = acx::seg_plan(R.len, a->host.max_len, kf);
    HIPCHK(g_bufs.get(temp, P->words * 8, a->device));
    uint64_t *scratch = (uint64_t *)*temp;
    HIPCHK(acx::seg_count(acx::at_trie(a->dev), d_hay, R, a->host.match_kind, kf, *P, scratch, st));
    HIPCHK(hipMemcpyAsync(total, acx::seg_total(*P, scratch), 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (*total > R.len) return fail(ACX_EDEVICE, "the tiles' counts do not sum to a number of pieces");
    return ACX_OK;
}

// ... and the emitting half into columns sized by `total`: every word of the three is written
int seg_emit_stage(acx_automaton *a, hipStream_t st, const uint8_t *d_hay, const acx::RowCut &R, uint32_t kf, const acx::SegPlan &P,
                   void *temp, uint64_t total, int64_t *pattern, int64_t *offsets, int64_t *row_offsets) {
    if (!R.len) { // no piece: offsets[0] = len = 0, every row begins at piece 0
        HIPCHK(hipMemsetAsync(offsets, 0, 8, st));
        HIPCHK(hipMemsetAsync(row_offsets, 0, (R.n + 1) * 8, st));
        return ACX_OK;
    }
    HIPCHK(acx::seg_emit(acx::at_trie(a->dev), d_hay, R, a->host.match_kind, kf, P, (uint64_t *)temp, total, pattern, offsets,
                         row_offsets, st));
    return ACX_OK;
}

// The device route under a lease: the stage on the context's stream, a device result.  Returns when T is known, with the
// emitting half in flight (Z->done).  d_hay and the offsets must stay valid until then.
int run_seg(acx_automaton *a, Ctx *c, const uint8_t *d_hay, uint64_t len, const Segments &G, uint32_t flags, acx_seg **out) {
    *out = nullptr;
    const acx::RowCut R = row_cut(G, len);
    acx_seg *Z = new_result<acx_seg>(a->device, true);
    if (!Z) return ACX_ENOMEM;
    Z->rows = R.n;
    const uint32_t kf = kernel_flags(a, flags);
    acx::SegPlan P;
    void *temp = nullptr;
    int queued = seg_count_stage(a, c->stream, d_hay, R, kf, &P, &temp, &Z->pieces);
    if (queued == ACX_OK) queued = Z->alloc();
    if (queued == ACX_OK) queued = seg_emit_stage(a, c->stream, d_hay, R, kf, P, temp, Z->pieces, Z->pattern(), Z->offsets(), Z->row_offsets());
    const int rc = retire_find(queued, c->stream, nullptr, Z, temp);
    if (rc != ACX_OK) { free_result(Z); return rc; }
    *out = Z;
    return ACX_OK;
}

// the host form of step 1: the match_at result of the anchor (p, L) under `kind`; false: no pattern begins at p
bool host_pick(const HostTrie &T, const uint8_t *h, uint64_t p, uint64_t L, int kind, int64_t *pid, uint64_t *end) {
    const acx::Automaton &H = T.A;
    int64_t best = -1;
    uint64_t best_end = 0;
    T.walk(h, p, L, [&](uint32_t s, uint64_t d) {
        const int64_t i = (int64_t)H.own_pid[H.own_off[s]]; // (the lists are in id order)
        if (kind == ACX_MATCH_LEFTMOST_FIRST && best >= 0 && best < i) return true;
        best = i;
        best_end = p + d;
        return kind != ACX_MATCH_STANDARD;
    });
    *pid = best;
    *end = best_end;
    return best >= 0;
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
    if (!h || !n_pieces) return fail(ACX_EINVAL, "null argument");
    *n_pieces = 0;
    int rc = seg_flags(flags);
    if (rc != ACX_OK) return rc;
    if (match_kind < ACX_MATCH_STANDARD || match_kind > ACX_MATCH_LEFTMOST_LONGEST) return fail(ACX_EINVAL, "unknown match kind");
    if (len && !hay) return fail(ACX_EINVAL, "null argument");
    if (!offsets) {
        if (n_hay > 1) return fail(ACX_EINVAL, "several haystacks need offsets");
        n_hay = 1;
    } else if ((rc = offsets_span(offsets, n_hay, len)) != ACX_OK) {
        return rc;
    }
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
                if (!host_pick(T, hay, p, L, match_kind, &pid, &e)) e = p + host_unit(hay, p, L, utf8);
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
    if (len && !d_hay) return fail(ACX_EINVAL, "null haystack");
    if (d_offsets && uniform_len) return fail(ACX_EINVAL, "offsets and uniform_len exclude one another");
    if ((uintptr_t)d_offsets & 7) return fail(ACX_EINVAL, "offsets must be 8-byte aligned");
    Segments G;
    if ((rc = make_segments(d_offsets, n_hay, uniform_len, len, &G)) != ACX_OK) return rc;
    if ((rc = seg_sizes(a->host.max_len, len, rows_of(G).n)) != ACX_OK) return rc;
    Lease lease(a);
    if (!lease.c) return fail(ACX_EDEVICE, "could not create a stream for the call");
    // (a case-insensitive handle folds in the walk's loads: no folded copy of the data)
    return run_seg(a, lease.c, (const uint8_t *)d_hay, len, G, flags, out);
}

int acx_segment_into_device(acx_automaton_t *a, const void *d_hay, uint64_t len, const uint64_t *d_offsets, uint64_t n_hay,
                            uint64_t uniform_len, uint32_t flags, uint64_t cap, int64_t *d_pattern, int64_t *d_offsets_out,
                            int64_t *d_row_offsets, uint64_t *n_pieces) {
    if (!a || !n_pieces) return fail(ACX_EINVAL, "null argument");
    *n_pieces = 0;
    int rc = seg_flags(flags);
    if (rc != ACX_OK) return rc;
    if (len && !d_hay) return fail(ACX_EINVAL, "null haystack");
    if (d_offsets && uniform_len) return fail(ACX_EINVAL, "offsets and uniform_len exclude one another");
    if (((uintptr_t)d_offsets | (uintptr_t)d_pattern | (uintptr_t)d_offsets_out | (uintptr_t)d_row_offsets) & 7)
        return fail(ACX_EINVAL, "offsets and the three columns must be 8-byte aligned");
    if (!d_offsets_out || !d_row_offsets || (cap && !d_pattern)) return fail(ACX_EINVAL, "null argument");
    Segments G;
    if ((rc = make_segments(d_offsets, n_hay, uniform_len, len, &G)) != ACX_OK) return rc;
    const acx::RowCut R = row_cut(G, len);
    if ((rc = seg_sizes(a->host.max_len, len, R.n)) != ACX_OK) return rc;
    Lease lease(a);
    if (!lease.c) return fail(ACX_EDEVICE, "could not create a stream for the call");
    const hipStream_t st = lease.c->stream;
    const uint32_t kf = kernel_flags(a, flags);
    acx::SegPlan P;
    void *temp = nullptr;
    rc = seg_count_stage(a, st, (const uint8_t *)d_hay, R, kf, &P, &temp, n_pieces);
    if (rc == ACX_OK && *n_pieces <= cap)
        rc = seg_emit_stage(a, st, (const uint8_t *)d_hay, R, kf, P, temp, *n_pieces, d_pattern, d_offsets_out, d_row_offsets);
    const hipError_t s = hipStreamSynchronize(st); // (complete when it returns, whatever the launches said)
    g_bufs.put(temp, a->device);
    if (rc != ACX_OK) return rc;
    return s == hipSuccess ? ACX_OK : hipfail(s, "hipStreamSynchronize");
}

int acx_segment(acx_automaton_t *a, const uint8_t *hay, uint64_t len, const uint64_t *offsets, uint64_t n_hay, uint32_t flags,
                int codepoints, acx_seg_t **out) {
    if (!a || !out) return fail(ACX_EINVAL, "null argument");
    *out = nullptr;
    int rc = seg_flags(flags);
    if (rc != ACX_OK) return rc;
    if (codepoints) flags |= ACX_SEG_UTF8;
    if (len && !hay) return fail(ACX_EINVAL, "null haystack");
    const bool batch = offsets != nullptr;
    if (!batch) {
        if (n_hay > 1) return fail(ACX_EINVAL, "several haystacks need offsets");
        n_hay = 1;
    } else if ((rc = offsets_span(offsets, n_hay, len)) != ACX_OK) {
        return rc;
    }
    if ((rc = seg_sizes(a->host.max_len, len, n_hay)) != ACX_OK) return rc;
    // the data (and, for a batch, its offsets) through the context's staging buffers; the same kernels; the block comes home
    // in one copy
    acx_seg *D = nullptr;
    {
        Lease lease(a);
        Ctx *c = lease.c;
        if (!c) return fail(ACX_EDEVICE, "could not create a stream for the call");
        if ((rc = stage_host(a, c, hay, len, batch ? offsets : nullptr, batch ? n_hay + 1 : 0, false)) != ACX_OK) return rc;
        const Segments G = batch ? Segments{c->ws.offsets, n_hay, 0} : Segments{nullptr, 1, 0};
        rc = run_seg(a, c, c->ws.hay, len, G, flags, &D);
        if (rc == ACX_OK) rc = D->wait(); // (the staging buffers are the context's)
        else (void)hipStreamSynchronize(c->stream);
    }
    acx_seg *Z = rc == ACX_OK ? new_result<acx_seg>(a->device, false) : nullptr;
    if (Z) {
        Z->pieces = D->pieces;
        Z->rows = D->rows;
        if ((rc = Z->alloc()) != ACX_OK) { free_result(Z); free_result(D); return rc; }
    }
    if ((rc = copy_down(rc, D, Z, D ? D->block_bytes : 0, "the segments' copy", out)) != ACX_OK) return rc;
    if (!codepoints) return ACX_OK;
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
