// snippets_api.cpp -- the matched text and its context (snippets.hpp): the host form, the device stage behind the find
// pipeline, the acx_snippets* entry points and the accessors of their result.
#include "snippets.hpp"
#include "replace.hpp"
#include "result_block.hpp"

using namespace acxh;

// acx_snippets / acx_snippets_device: the snippets' bytes, their n + 1 offsets, two columns of n words and, for a batch,
// rows + 1 row offsets, in ONE block (result_block.hpp).  Device route: the find's records and the stage's temporaries have
// gone back to the cache behind the stage's kernels; the gather's tile words are kept until acx_free_snippets.
struct ACX_HIDDEN acx_snippets : ResultBlock {
    bool batch = false;
    uint64_t n = 0, rows = 0, bytes = 0;

    // the block (by on_device) and its parts, ACX_SNIP_*; the single form has no row offsets
    int alloc() {
        return batch ? alloc_parts({bytes, (n + 1) * 8, n * 8, n * 8, (rows + 1) * 8}) : alloc_parts({bytes, (n + 1) * 8, n * 8, n * 8});
    }
    uint8_t *data() const { return at<uint8_t>(ACX_SNIP_DATA); }
    int64_t *words(int which) const { return at<int64_t>(which); }
};

namespace {

constexpr int N_PARTS = ACX_SNIP_ROW_OFFSETS + 1;

constexpr uint64_t CONTEXT_LIMIT = 1ull << 63;

int check_args(uint64_t context, uint32_t flags) {
    if (context >= CONTEXT_LIMIT) return fail(ACX_EINVAL, "context must be below 2^63");
    return flags & ~(uint32_t)ACX_SNIPPET_UTF8 ? fail(ACX_EINVAL, "unknown snippet flags") : ACX_OK;
}

bool continuation(uint8_t b) { return (b & 0xC0) == 0x80; }

// The definition (snippets.hpp) for one record in a row of L bytes at B: the snippet is B[*lo .. *hi), the match begins at *s.
void cut(const uint8_t *B, uint64_t L, const acx_match_t &r, uint64_t context, bool utf8, uint64_t *lo, uint64_t *hi, uint64_t *s) {
    const uint64_t s1 = std::min<uint64_t>(r.start, L), e1 = std::min(std::max<uint64_t>(r.end, s1), L);
    uint64_t a = s1 - std::min(s1, context), b = e1 + std::min(context, L - e1);
    if (utf8) {
        for (int k = 0; k < 3; k++)
            if (a < s1 && continuation(B[a])) a++;
        for (int k = 0; k < 3; k++)
            if (e1 < b && b < L && continuation(B[b])) b--;
    }
    *lo = a;
    *hi = b;
    *s = s1;
}

// The temporaries of one run of the device stage: one block of the buffer cache, and the gather's tile words (another).
struct Stage {
    void *block = nullptr, *tiles = nullptr;
    const int64_t *rec_off = nullptr; // rows + 1
    uint64_t *src = nullptr;          // n: where every snippet begins in the haystack
    int64_t *offsets = nullptr, *pattern = nullptr, *lead = nullptr; // the caller's, or parts of the block
    uint64_t total = 0;
};

// The stage up to the point where the output's size is known (n > 0, R.n > 0): where the rows' records begin, every
// record's cut, the scan of the lengths, and the 8 bytes that cross the bus.  d_counts: R.n words that sum to n (check_sum:
// record_offsets).  offsets (n + 1), pattern, lead (n each): where they are wanted, or null: parts of the block.
int stage_sizes(int device, hipStream_t st, const acx_match_t *d_m, uint64_t n, const uint64_t *d_counts, const acx::RowCut &R,
                bool check_sum, const uint8_t *d_hay, uint64_t context, uint32_t flags, int64_t *offsets, int64_t *pattern,
                int64_t *lead, Stage *G) {
    if (n >= (1ull << 39)) return fail(ACX_ETOOBIG, "too many records to be cut in one call");
    // [rec_off: rows + 1][scan of the rows][len: n][src: n][scan of the lengths]([offsets: n + 1][pattern: n][lead: n])
    Carver C;
    const uint64_t o_rec = C.part(R.n + 1), o_scan = C.part(replace_scan_words(R.n)), o_len = C.part(n), o_src = C.part(n),
                   o_scan2 = C.part(replace_scan_words(n));
    const uint64_t o_off = offsets ? 0 : C.part(n + 1), o_pat = pattern ? 0 : C.part(n), o_lead = lead ? 0 : C.part(n);
    HIPCHK(g_bufs.get(&G->block, C.bytes(), device));
    uint64_t *b = (uint64_t *)G->block;
    int64_t *rec_off = (int64_t *)(b + o_rec);
    G->rec_off = rec_off;
    G->src = b + o_src;
    G->offsets = offsets ? offsets : (int64_t *)(b + o_off);
    G->pattern = pattern ? pattern : (int64_t *)(b + o_pat);
    G->lead = lead ? lead : (int64_t *)(b + o_lead);
    if (int rc = record_offsets(d_counts, R.n, n, check_sum, rec_off, b + o_scan, st)) return rc;
    HIPCHK(acx::snip_sizes(d_m, n, rec_off, R, d_hay, context, flags, b + o_len, G->src, G->lead, G->pattern, st));
    HIPCHK(acx::replace_scan(nullptr, nullptr, b + o_len, n, G->offsets, b + o_scan2, st));
    uint64_t total = 0; // all that crosses the bus
    HIPCHK(hipMemcpyAsync(&total, G->offsets + n, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    G->total = total;
    return ACX_OK;
}

// ... and the gather into d_data (G->total bytes, 16-byte aligned)
int stage_gather(int device, hipStream_t st, const uint8_t *d_hay, uint64_t len, uint64_t n, uint8_t *d_data, Stage *G) {
    if (!G->total) return ACX_OK;
    if ((G->total + acx::SNIP_TILE - 1) / acx::SNIP_TILE >= (1ull << 31)) return fail(ACX_ETOOBIG, "too many bytes to be cut in one call");
    HIPCHK(g_bufs.get(&G->tiles, std::max<uint64_t>(acx::snip_tile_words(G->total), 32) * 8, device));
    HIPCHK(acx::snip_gather(d_hay, len, G->offsets, G->src, n, (uint64_t *)G->tiles, d_data, G->total, st));
    return ACX_OK;
}

// The device route: the find pipeline as acx_find_device runs it (byte ranges, batch splits and the expansion of copies
// included; byte offsets) on d_search, then the stage on the same stream over d_hay -- the caller's own bytes.  Returns when
// the output's size is known; the gather may still run (out->done).  d_hay, d_search and G.offsets must stay valid until then.
int run_snippets(acx_automaton *a, Ctx *x, const uint8_t *d_hay, const uint8_t *d_search, uint64_t len, const Segments &G,
                 int overlapping, uint64_t context, uint32_t flags, acx_snippets_t **out) {
    const bool segmented = rows_of(G).segmented;
    // (an empty batch: nothing to search, one row offset)
    return find_stage(a, x, d_search, len, G, overlapping, 0, !(segmented && G.n_hay == 0), out, [&](FindStage<acx_snippets_t> &F) -> int {
        acx_snippets_t *R = F.R;
        acx_result *r = F.r;
        hipStream_t st = F.st;
        R->batch = segmented;
        R->rows = segmented ? G.n_hay : 0;
        int rc;
        const uint64_t n = r ? r->n : 0;
        if (!n) { // no record: no snippet, and every offset is zero
            if ((rc = R->alloc()) != ACX_OK) return rc;
            HIPCHK(hipMemsetAsync(R->words(ACX_SNIP_OFFSETS), 0, 8, st));
            if (R->batch) HIPCHK(hipMemsetAsync(R->words(ACX_SNIP_ROW_OFFSETS), 0, (R->rows + 1) * 8, st));
            return ACX_OK;
        }
        const uint64_t *d_counts = nullptr;
        if ((rc = F.counts(&d_counts)) != ACX_OK) return rc;
        const uint64_t rows = rows_of(G).n;
        const acx::RowCut SR = row_cut(G, len);
        Stage S;
        rc = stage_sizes(a->device, st, r->d_matches, n, d_counts, SR, false, d_hay, context, flags, nullptr, nullptr, nullptr, &S);
        F.temp = S.block;
        if (rc != ACX_OK) return rc;
        R->n = n;
        R->bytes = S.total;
        if ((rc = R->alloc()) != ACX_OK) return rc;
        HIPCHK(hipMemcpyAsync(R->words(ACX_SNIP_OFFSETS), S.offsets, (n + 1) * 8, hipMemcpyDeviceToDevice, st));
        HIPCHK(hipMemcpyAsync(R->words(ACX_SNIP_PATTERN), S.pattern, n * 8, hipMemcpyDeviceToDevice, st));
        HIPCHK(hipMemcpyAsync(R->words(ACX_SNIP_LEAD), S.lead, n * 8, hipMemcpyDeviceToDevice, st));
        if (R->batch) HIPCHK(hipMemcpyAsync(R->words(ACX_SNIP_ROW_OFFSETS), S.rec_off, (rows + 1) * 8, hipMemcpyDeviceToDevice, st));
        rc = stage_gather(a->device, st, d_hay, len, n, R->data(), &S);
        F.keep(S.tiles); // (kept until acx_free_snippets)
        return rc;
    });
}

} // namespace

extern "C" {

int acx_snippets_host(const acx_match_t *m, uint64_t n_m, const uint64_t *counts, uint64_t n_hay, const uint8_t *hay, uint64_t len,
                      const uint64_t *offsets, uint64_t context, uint32_t flags, int64_t *out_offsets, int64_t *pattern,
                      int64_t *lead, int64_t *row_offsets, uint8_t *data, uint64_t *total) {
    if (!total || (n_m && !m) || (len && !hay)) return fail(ACX_EINVAL, "null argument");
    *total = 0;
    int rc = check_args(context, flags);
    if (rc != ACX_OK) return rc;
    if (!offsets) {
        if (n_hay > 1) return fail(ACX_EINVAL, "several haystacks need offsets");
        n_hay = 1;
    } else if ((rc = offsets_span(offsets, n_hay, len)) != ACX_OK) {
        return rc;
    }
    if (!counts && n_hay > 1) return fail(ACX_EINVAL, "several haystacks need counts");
    if ((rc = counts_sum_to(counts, n_hay, n_m)) != ACX_OK) return rc;
    const bool utf8 = (flags & ACX_SNIPPET_UTF8) != 0;
    uint64_t at = 0, bytes = 0;
    for (uint64_t h = 0; h < n_hay; h++) {
        const uint64_t b = offsets ? offsets[h] : 0, L = (offsets ? offsets[h + 1] : len) - b;
        if (row_offsets) row_offsets[h] = (int64_t)at;
        for (const uint64_t end = counts ? at + counts[h] : n_m; at < end; at++) {
            uint64_t lo, hi, s;
            cut(hay + b, L, m[at], context, utf8, &lo, &hi, &s);
            if (out_offsets) out_offsets[at] = (int64_t)bytes;
            if (pattern) pattern[at] = (int64_t)m[at].pattern;
            if (lead) lead[at] = (int64_t)(s - lo);
            if (data && hi > lo) std::memcpy(data + bytes, hay + b + lo, (size_t)(hi - lo));
            bytes += hi - lo;
        }
    }
    if (row_offsets) row_offsets[n_hay] = (int64_t)at;
    if (out_offsets) out_offsets[n_m] = (int64_t)bytes;
    *total = bytes;
    return ACX_OK;
}

int acx_snippets(acx_automaton_t *a, const uint8_t *hay, uint64_t len, const uint64_t *offsets, uint64_t n_hay, int overlapping,
                 uint64_t context, uint32_t flags, acx_snippets_t **out) {
    if (!a || !out) return fail(ACX_EINVAL, "null argument");
    *out = nullptr;
    int rc = check_args(context, flags);
    if (rc == ACX_OK && overlapping) rc = check_overlapping(a); // (the error, no device state)
    if (rc != ACX_OK) return rc;
    HostBatch B;
    if ((rc = host_batch(hay, &len, offsets, &n_hay, &B)) != ACX_OK) return rc;
    // the find entry points as they are (K0, the resident K0, the in-place read, the staged pipeline), each under its lease,
    // with byte offsets: the records cross the bus, the snippets are cut of the caller's own bytes here
    HostFind f;
    const bool search = n_hay && len; // (an empty batch, or empty rows only: nothing to search)
    if ((rc = f.find(a, B.hay, len, offsets ? B.rel.data() : nullptr, n_hay, overlapping, 0, search)) != ACX_OK) return rc;
    acx_snippets_t *R = new_result<acx_snippets_t>(a->device, false);
    if (!R) return ACX_ENOMEM;
    R->batch = offsets != nullptr;
    R->rows = R->batch ? n_hay : 0;
    R->n = f.nm;
    const uint64_t *rel = R->batch ? B.rel.data() : nullptr;
    rc = acx_snippets_host(f.m, f.nm, f.counts.data(), n_hay, B.hay, len, rel, context, flags, nullptr, nullptr, nullptr, nullptr,
                           nullptr, &R->bytes);
    if (rc == ACX_OK) rc = R->alloc();
    if (rc == ACX_OK)
        rc = acx_snippets_host(f.m, f.nm, f.counts.data(), n_hay, B.hay, len, rel, context, flags, R->words(ACX_SNIP_OFFSETS),
                               R->words(ACX_SNIP_PATTERN), R->words(ACX_SNIP_LEAD), R->batch ? R->words(ACX_SNIP_ROW_OFFSETS) : nullptr,
                               R->data(), &R->bytes);
    if (rc != ACX_OK) { free_result(R); return rc; }
    *out = R;
    return ACX_OK;
}

int acx_snippets_device(acx_automaton_t *a, const void *d_hay, uint64_t len, const uint64_t *d_offsets, uint64_t n_hay,
                        uint64_t uniform_len, int overlapping, uint64_t context, uint32_t flags, acx_snippets_t **out) {
    if (!a || !out) return fail(ACX_EINVAL, "null argument");
    *out = nullptr;
    int rc = check_args(context, flags);
    if (rc != ACX_OK) return rc;
    // (a case-insensitive handle: the folded copy is searched, the caller's bytes are cut)
    return device_call(a, d_hay, len, d_offsets, n_hay, uniform_len, overlapping, [&](Ctx *c, const uint8_t *d_search, const Segments &G) {
        return run_snippets(a, c, (const uint8_t *)d_hay, d_search, len, G, overlapping, context, flags, out);
    });
}

int acx_snippets_rows_device(const acx_match_t *d_records, uint64_t n, const uint64_t *d_counts, uint64_t n_hay, const void *d_hay,
                             uint64_t len, const uint64_t *d_offsets, uint64_t uniform_len, uint64_t context, uint32_t flags,
                             int64_t *d_out_offsets, int64_t *d_pattern, int64_t *d_lead, int64_t *d_row_offsets, uint8_t *d_data,
                             uint64_t data_capacity, uint64_t *total) {
    if (!total) return fail(ACX_EINVAL, "null argument");
    *total = 0;
    int rc = check_args(context, flags);
    if (rc != ACX_OK) return rc;
    if ((rc = device_rows_args(d_offsets, &n_hay, uniform_len, len)) != ACX_OK) return rc;
    if (!d_out_offsets || !d_row_offsets || (len && !d_hay) || (data_capacity && !d_data) ||
        (n && (!d_records || !d_counts || !d_pattern || !d_lead)))
        return fail(ACX_EINVAL, "null argument");
    if (!n_hay && n) return fail(ACX_EINVAL, "the counts do not sum to the number of records");
    if (((uintptr_t)d_records | (uintptr_t)d_counts | (uintptr_t)d_offsets | (uintptr_t)d_out_offsets | (uintptr_t)d_pattern |
         (uintptr_t)d_lead | (uintptr_t)d_row_offsets) & 7)
        return fail(ACX_EINVAL, "records, counts, offsets and columns must be 8-byte aligned");
    if ((uintptr_t)d_data & 15) return fail(ACX_EINVAL, "the data must be 16-byte aligned");
    return rows_call(d_out_offsets, [&](int device, void **block, void **tiles) -> int {
        if (!n) { // no record: no snippet, and every offset is zero
            HIPCHK(hipMemsetAsync(d_out_offsets, 0, 8, nullptr));
            HIPCHK(hipMemsetAsync(d_row_offsets, 0, (n_hay + 1) * 8, nullptr));
            return ACX_OK;
        }
        const int span = device_offsets_span(d_offsets, n_hay, len);
        if (span != ACX_OK) return span;
        const acx::RowCut SR{d_offsets, uniform_len, n_hay, len};
        Stage S;
        const int sized = stage_sizes(device, nullptr, d_records, n, d_counts, SR, true, (const uint8_t *)d_hay, context, flags,
                                      d_out_offsets, d_pattern, d_lead, &S);
        *block = S.block;
        if (sized != ACX_OK) return sized;
        *total = S.total;
        HIPCHK(hipMemcpyAsync(d_row_offsets, S.rec_off, (n_hay + 1) * 8, hipMemcpyDeviceToDevice, nullptr));
        if (S.total > data_capacity) return fail(ACX_ETOOBIG, "the snippets need more bytes than the data holds");
        const int rc2 = stage_gather(device, nullptr, (const uint8_t *)d_hay, len, n, d_data, &S);
        *tiles = S.tiles;
        return rc2;
    });
}

uint64_t acx_snippets_count(const acx_snippets_t *s) { return s ? s->n : 0; }
uint64_t acx_snippets_rows(const acx_snippets_t *s) { return s ? s->rows : 0; }
uint64_t acx_snippets_nbytes(const acx_snippets_t *s) { return s ? s->bytes : 0; }
int acx_snippets_on_device(const acx_snippets_t *s) { return s ? s->on_device : 0; }

const void *acx_snippets_data(const acx_snippets_t *s, int which) { return part_ptr(s, which, N_PARTS); }
int acx_snippets_copy(const acx_snippets_t *s, int which, void *host_dst) {
    return part_copy(s, which, N_PARTS, host_dst, "no such part", "the single form has no row offsets");
}

void acx_free_snippets(acx_snippets_t *s) { free_result(s); }

} // extern "C"
