// tokens_api.cpp -- a search's matches mapped onto token boundaries (tokens.hpp has the definition): the host form, the device
// stage behind the find pipeline, the acx_tokens* entry points and the accessors of their result.
#include "tokens.hpp"
#include "replace.hpp"
#include "result_block.hpp"

using namespace acxh;

// acx_tokens / acx_tokens_device: the owner's pattern (T int64 words) and the begin flags (T bytes) in ONE block
// (result_block.hpp).  Device route: the find's records and the stage's temporaries have gone back to the cache behind the
// stage's kernels.
struct ACX_HIDDEN acx_token_labels : ResultBlock {
    enum { PATTERN, BEGIN, N_PARTS };
    uint64_t n = 0; // T

    int alloc() { return alloc_parts({n * 8, n}); } // the block (by on_device) and its two parts
    int64_t *pattern() const { return at<int64_t>(PATTERN); }
    uint8_t *begin() const { return at<uint8_t>(BEGIN); }
};

namespace {

int too_many_tokens() { return fail(ACX_ETOOBIG, "2^32 tokens or more in one call"); }

// The device stage on stream st.  d_m: n records; d_counts: R.n words that sum to n (check_sum: record_offsets); d_ts, d_te:
// T words each; d_pattern: T words; d_begin: T bytes.  No record, no row or no position: the fills and nothing else.  *block:
// the stage's temporaries, one block of the buffer cache -- the caller's to return, behind the stage's kernels.
int tokens_stage(int device, hipStream_t st, const acx::RowCut &R, const acx_match_t *d_m, uint64_t n, const uint64_t *d_counts,
                 bool check_sum, const int64_t *d_ts, const int64_t *d_te, uint64_t T, int64_t *d_pattern, uint8_t *d_begin,
                 void **block) {
    if (!T) return ACX_OK;
    if (T >= acx::TOK_MAX_TOKENS) return too_many_tokens();
    if (!n || !R.n || !R.len) {
        HIPCHK(hipMemsetAsync(d_pattern, 0xFF, T * 8, st)); // -1: no owner
        HIPCHK(hipMemsetAsync(d_begin, 0, T, st));
        return ACX_OK;
    }
    if (acx::tiles_of(n, acx::TOK_TILE) >= (1ull << 31)) return fail(ACX_ETOOBIG, "too many records to be labelled in one call");
    // [rec_off: rows + 1][scan][tiles][owners], every part 256-byte aligned
    Carver C;
    const uint64_t o_rec = C.part(R.n + 1), o_scan = C.part(replace_scan_words(R.n)), o_tiles = C.part(acx::tokens_tile_words(n)),
                   o_own = C.part(acx::tokens_owner_words(T));
    HIPCHK(g_bufs.get(block, C.bytes(), device));
    uint64_t *b = (uint64_t *)*block;
    int64_t *rec_off = (int64_t *)(b + o_rec);
    if (int rc = record_offsets(d_counts, R.n, n, check_sum, rec_off, b + o_scan, st)) return rc;
    HIPCHK(acx::tokens_label(d_m, n, rec_off, R, d_ts, d_te, T, b + o_tiles, b + o_own, d_pattern, d_begin, st));
    return ACX_OK;
}

// The device route: the find pipeline as acx_find_device runs it (batch splits and the expansion of copies included, byte
// offsets) on d_search, then the stage on the same stream.  Returns with the stage in flight (out->done).  d_search, the
// token arrays and G.offsets must stay valid until then.
int run_tokens(acx_automaton *a, Ctx *x, const uint8_t *d_search, uint64_t len, const Segments &G, int overlapping,
               const int64_t *d_ts, const int64_t *d_te, uint64_t T, acx_token_labels_t **out) {
    const uint64_t rows = rows_of(G).n;
    // (no token, an empty batch, or empty rows only: nothing to search)
    return find_stage(a, x, d_search, len, G, overlapping, 0, T && rows && len, out, [&](FindStage<acx_token_labels> &F) -> int {
        acx_token_labels *R = F.R;
        acx_result *r = F.r;
        R->n = T;
        int rc;
        if ((rc = R->alloc()) != ACX_OK) return rc;
        const uint64_t *d_counts = nullptr;
        if (r && r->n && (rc = F.counts(&d_counts)) != ACX_OK) return rc;
        return tokens_stage(a->device, F.st, row_cut(G, len), r ? r->d_matches : nullptr, r ? r->n : 0, d_counts, false, d_ts, d_te, T,
                            R->pattern(), R->begin(), &F.temp);
    });
}

// ts[t] <= te[t] <= ts[t + 1], the last end inside the data (a negative word is a large one)
int tokens_rise(const int64_t *ts, const int64_t *te, uint64_t T, uint64_t len) {
    if (T && (!ts || !te)) return fail(ACX_EINVAL, "null argument");
    uint64_t at = 0;
    for (uint64_t t = 0; t < T; t++) {
        const uint64_t s = (uint64_t)ts[t], e = (uint64_t)te[t];
        if (s < at || e < s || e > len) return fail(ACX_EINVAL, "token boundaries must rise and lie inside the data");
        at = e;
    }
    return ACX_OK;
}

} // namespace

extern "C" {

int acx_tokens_host(const acx_match_t *m, uint64_t n_m, const uint64_t *counts, uint64_t n_hay, const uint64_t *offsets, uint64_t len,
                    const int64_t *ts, const int64_t *te, uint64_t n_tokens, int64_t *pattern, uint8_t *begin) {
    const uint64_t T = n_tokens;
    if ((n_m && !m) || (T && (!pattern || !begin))) return fail(ACX_EINVAL, "null argument");
    int rc;
    if (!offsets) {
        if (n_hay > 1) return fail(ACX_EINVAL, "several haystacks need offsets");
        n_hay = 1;
    } else if ((rc = offsets_span(offsets, n_hay, len)) != ACX_OK) {
        return rc;
    }
    if (!counts && n_hay > 1) return fail(ACX_EINVAL, "several haystacks need counts");
    if ((rc = counts_sum_to(counts, n_hay, n_m)) != ACX_OK) return rc;
    if ((rc = tokens_rise(ts, te, T, len)) != ACX_OK) return rc;
    constexpr uint64_t NONE = ~0ull;
    std::vector<uint64_t> owner;
    try {
        owner.assign((size_t)T, NONE);
    } catch (...) { return fail(ACX_ENOMEM, "out of memory"); }
    uint64_t at = 0;
    for (uint64_t h = 0; h < n_hay && T; h++) {
        const uint64_t b = offsets ? offsets[h] : 0, rowlen = (offsets ? offsets[h + 1] : len) - b;
        for (const uint64_t end = counts ? at + counts[h] : n_m; at < end; at++) {
            const uint64_t e = std::min<uint64_t>(m[at].end, rowlen), s = std::min<uint64_t>(m[at].start, e); // clipped to the row
            if (e <= s) continue;
            const uint64_t g_s = b + s, g_e = b + e;
            // the tokens that end at or before g_s come before the first touched one; those that begin before g_e hold the last
            const uint64_t first = (uint64_t)(std::upper_bound(te, te + T, g_s, [](uint64_t x, int64_t v) { return x < (uint64_t)v; }) - te);
            const uint64_t stop = (uint64_t)(std::lower_bound(ts, ts + T, g_e, [](int64_t v, uint64_t x) { return (uint64_t)v < x; }) - ts);
            for (uint64_t t = first; t < stop; t++)
                if (owner[(size_t)t] == NONE) owner[(size_t)t] = at; // (the records come in ascending index: the first one stays)
        }
    }
    for (uint64_t t = 0; t < T; t++) {
        const uint64_t o = owner[(size_t)t];
        pattern[t] = o == NONE ? -1 : (int64_t)m[o].pattern;
        begin[t] = o != NONE && (t == 0 || owner[(size_t)t - 1] != o);
    }
    return ACX_OK;
}

int acx_tokens(acx_automaton_t *a, const uint8_t *hay, uint64_t len, const uint64_t *offsets, uint64_t n_hay, int overlapping,
               int codepoints, const int64_t *ts, const int64_t *te, uint64_t n_tokens, acx_token_labels_t **out) {
    if (!a || !out) return fail(ACX_EINVAL, "null argument");
    *out = nullptr;
    int rc = overlapping ? check_overlapping(a) : ACX_OK; // (the error, no device state)
    if (rc != ACX_OK) return rc;
    if (n_tokens && (!ts || !te)) return fail(ACX_EINVAL, "null argument");
    HostBatch B;
    if ((rc = host_batch(hay, &len, offsets, &n_hay, &B)) != ACX_OK) return rc;
    // the rows in the unit of the tokens: bytes, or (codepoints) characters -- a byte that continues none begins one
    std::vector<uint64_t> chars;
    uint64_t units = len;
    if (codepoints) {
        try {
            chars.assign((size_t)n_hay + 1, 0);
        } catch (...) { return fail(ACX_ENOMEM, "out of memory"); }
        for (uint64_t h = 0; h < n_hay; h++) {
            uint64_t k = 0;
            for (uint64_t i = B.rel[h]; i < B.rel[h + 1]; i++) k += (B.hay[i] & 0xC0) != 0x80;
            chars[(size_t)h + 1] = chars[(size_t)h] + k;
        }
        units = chars[(size_t)n_hay];
    }
    const uint64_t *unit_off = codepoints ? chars.data() : B.rel.data();
    if ((rc = tokens_rise(ts, te, n_tokens, units)) != ACX_OK) return rc; // (before any device work)
    // the find as it is (the small-call kernel, its resident form, the in-place read, the staged pipeline all still apply):
    // the records cross the bus and are labelled here
    HostFind f;
    const bool search = n_tokens && n_hay && len;
    if ((rc = f.find(a, B.hay, len, offsets ? B.rel.data() : nullptr, n_hay, overlapping, codepoints, search)) != ACX_OK) return rc;
    acx_token_labels_t *R = new_result<acx_token_labels_t>(a->device, false);
    if (!R) return ACX_ENOMEM;
    R->n = n_tokens;
    if ((rc = R->alloc()) == ACX_OK)
        rc = acx_tokens_host(f.m, f.nm, f.counts.data(), n_hay, unit_off, units, ts, te, n_tokens, R->pattern(), R->begin());
    if (rc != ACX_OK) { free_result(R); return rc; }
    *out = R;
    return ACX_OK;
}

int acx_tokens_device(acx_automaton_t *a, const void *d_hay, uint64_t len, const uint64_t *d_offsets, uint64_t n_hay,
                      uint64_t uniform_len, int overlapping, const int64_t *d_ts, const int64_t *d_te, uint64_t n_tokens,
                      acx_token_labels_t **out) {
    if (!a || !out) return fail(ACX_EINVAL, "null argument");
    *out = nullptr;
    if (n_tokens && (!d_ts || !d_te)) return fail(ACX_EINVAL, "null argument");
    if (((uintptr_t)d_ts | (uintptr_t)d_te) & 7) return fail(ACX_EINVAL, "token arrays must be 8-byte aligned");
    if (n_tokens >= acx::TOK_MAX_TOKENS) return too_many_tokens();
    // (a case-insensitive handle: the folded copy is searched; no byte is output)
    return device_call(a, d_hay, len, d_offsets, n_hay, uniform_len, overlapping, [&](Ctx *c, const uint8_t *d_search, const Segments &G) {
        return run_tokens(a, c, d_search, len, G, overlapping, d_ts, d_te, n_tokens, out);
    });
}

int acx_tokens_rows_device(uint64_t len, const uint64_t *d_offsets, uint64_t n_hay, uint64_t uniform_len, const acx_match_t *d_records,
                           uint64_t n, const uint64_t *d_counts, const int64_t *d_ts, const int64_t *d_te, uint64_t n_tokens,
                           int64_t *d_pattern, uint8_t *d_begin) {
    int rc;
    if ((rc = device_rows_args(d_offsets, &n_hay, uniform_len, len)) != ACX_OK) return rc;
    if ((n_tokens && (!d_ts || !d_te || !d_pattern || !d_begin)) || (n && (!d_records || !d_counts)))
        return fail(ACX_EINVAL, "null argument");
    if (!n_hay && n) return fail(ACX_EINVAL, "the counts do not sum to the number of records");
    if (((uintptr_t)d_offsets | (uintptr_t)d_records | (uintptr_t)d_counts | (uintptr_t)d_ts | (uintptr_t)d_te | (uintptr_t)d_pattern) & 7)
        return fail(ACX_EINVAL, "offsets, records, counts, token arrays and the pattern column must be 8-byte aligned");
    if (n_tokens >= acx::TOK_MAX_TOKENS) return too_many_tokens();
    if (!n_tokens) return ACX_OK; // (no entry to write)
    return rows_call(d_pattern, [&](int device, void **block, void **) {
        const int span = device_offsets_span(d_offsets, n_hay, len);
        if (span != ACX_OK) return span;
        const acx::RowCut R{d_offsets, uniform_len, n_hay, len};
        return tokens_stage(device, nullptr, R, d_records, n, d_counts, true, d_ts, d_te, n_tokens, d_pattern, d_begin, block);
    });
}

uint64_t acx_token_labels_count(const acx_token_labels_t *l) { return l ? l->n : 0; }
int acx_token_labels_on_device(const acx_token_labels_t *l) { return l ? l->on_device : 0; }

const int64_t *acx_token_labels_pattern(const acx_token_labels_t *l) {
    return (const int64_t *)part_ptr(l, acx_token_labels::PATTERN, acx_token_labels::N_PARTS);
}
const uint8_t *acx_token_labels_begin(const acx_token_labels_t *l) {
    return (const uint8_t *)part_ptr(l, acx_token_labels::BEGIN, acx_token_labels::N_PARTS);
}
int acx_token_labels_copy_pattern(const acx_token_labels_t *l, int64_t *host_dst) {
    return part_copy(l, acx_token_labels::PATTERN, acx_token_labels::N_PARTS, host_dst, "null argument");
}
int acx_token_labels_copy_begin(const acx_token_labels_t *l, uint8_t *host_dst) {
    return part_copy(l, acx_token_labels::BEGIN, acx_token_labels::N_PARTS, host_dst, "null argument");
}

void acx_free_token_labels(acx_token_labels_t *l) { free_result(l); }

} // extern "C"
