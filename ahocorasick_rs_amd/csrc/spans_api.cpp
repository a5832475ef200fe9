// spans_api.cpp -- the merged spans of a search's matches (spans.hpp): the host form, the device stage behind the find
// pipeline, the acx_spans* entry points and the accessors of their result.
#include "spans.hpp"
#include "replace.hpp"
#include "result_block.hpp"

using namespace acxh;

// acx_spans / acx_spans_device: two columns of `n` words and, for a batch, rows + 1 row offsets, in ONE block
// (result_block.hpp).  Device route: the find's records and the stage's temporaries have gone back to the cache behind the
// stage's kernels.
struct ACX_HIDDEN acx_spans : ResultBlock {
    bool batch = false;
    uint64_t n = 0, rows = 0;

    // the block (by on_device) and its parts, ACX_SPAN_*; the single form has no row offsets
    int alloc() { return batch ? alloc_parts({n * 8, n * 8, (rows + 1) * 8}) : alloc_parts({n * 8, n * 8}); }
    int64_t *col(int which) const { return at<int64_t>(which); }
};

namespace {

constexpr int N_PARTS = ACX_SPAN_ROW_OFFSETS + 1;

constexpr uint64_t GAP_LIMIT = 1ull << 63;

int check_gap(uint64_t gap) { return gap >= GAP_LIMIT ? fail(ACX_EINVAL, "gap must be below 2^63") : ACX_OK; }

// The definition on the host, by the stage's own formulas (spans.hpp): one row's records m[0 .. k) -- sufmin from the back,
// then the closers and openers from the front.  sm: room for k words.  Appends at start[at ..] / end[at ..]; returns the new at.
uint64_t host_row(const acx_match_t *m, uint64_t k, uint64_t gap, uint64_t *sm, int64_t *start, int64_t *end, uint64_t at) {
    constexpr uint64_t INF = ~0ull;
    uint64_t behind = INF;
    for (uint64_t i = k; i-- > 0;) {
        if (m[i].start < m[i].end) behind = std::min<uint64_t>(behind, m[i].start);
        sm[i] = behind;
    }
    bool open = false; // a span has its start and waits for its end
    for (uint64_t i = 0; i < k; i++) {
        if (!open && sm[i] != INF) {
            start[at] = (int64_t)sm[i];
            open = true;
        }
        if (m[i].start >= m[i].end) continue;
        const uint64_t next = i + 1 < k ? sm[i + 1] : INF;
        if (next == INF || (next > m[i].end && next - m[i].end > gap)) {
            end[at++] = (int64_t)m[i].end;
            open = false;
        }
    }
    return at;
}

// The temporaries of one run of the device stage: one block of the buffer cache.
struct Stage {
    void *block = nullptr;
    const int64_t *rec_off = nullptr; // rows + 1
    const uint64_t *temp = nullptr;   // the tiles' rows, heads and carries
    const int64_t *base = nullptr;    // the scan of the tiles' closers, its last entry the total
    uint64_t S = 0;
};

// The stage up to the point where the result's size is known (n > 0, rows > 0): where the rows' records begin, the tiles'
// closers, their scan, and the 8 bytes that cross the bus.  d_counts: rows words that sum to n (check_sum: record_offsets).
int stage_sizes(int device, hipStream_t st, const acx_match_t *d_m, uint64_t n, const uint64_t *d_counts, uint64_t rows,
                bool check_sum, uint64_t gap, Stage *G) {
    const uint64_t T = acx::spans_tiles(n);
    if (T >= (1ull << 31)) return fail(ACX_ETOOBIG, "too many records to be merged in one call");
    // [rec_off: rows + 1][scan of the rows][tiles][closers: T][base: T + 1][scan of the tiles], every part 256-byte aligned
    Carver C;
    const uint64_t o_rec = C.part(rows + 1), o_scan = C.part(replace_scan_words(rows)), o_temp = C.part(acx::spans_temp_words(n)),
                   o_cnt = C.part(T), o_base = C.part(T + 1), o_scan2 = C.part(replace_scan_words(T));
    HIPCHK(g_bufs.get(&G->block, C.bytes(), device));
    uint64_t *b = (uint64_t *)G->block;
    int64_t *rec_off = (int64_t *)(b + o_rec);
    G->rec_off = rec_off;
    G->temp = b + o_temp;
    G->base = (const int64_t *)(b + o_base);
    if (int rc = record_offsets(d_counts, rows, n, check_sum, rec_off, b + o_scan, st)) return rc;
    HIPCHK(acx::spans_count(d_m, n, rec_off, rows, gap, b + o_temp, b + o_cnt, st));
    HIPCHK(acx::replace_scan(nullptr, nullptr, b + o_cnt, T, (int64_t *)(b + o_base), b + o_scan2, st));
    uint64_t total = 0; // all that crosses the bus
    HIPCHK(hipMemcpyAsync(&total, b + o_base + T, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (total > n) return fail(ACX_EDEVICE, "more spans than records");
    G->S = total;
    return ACX_OK;
}

// The device route: the find pipeline as acx_find_device runs it (byte ranges, batch splits and the expansion of copies
// included), then the stage on the same stream.  Returns when the number of spans is known; the emit kernel may still run
// (out->done).  d_hay, and G.offsets, must stay valid until then.
int run_spans(acx_automaton *a, Ctx *x, const uint8_t *d_hay, uint64_t len, const Segments &G, int overlapping, int codepoints,
              uint64_t gap, acx_spans_t **out) {
    const bool segmented = rows_of(G).segmented;
    // (an empty batch: nothing to search, one row offset)
    return find_stage(a, x, d_hay, len, G, overlapping, codepoints, !(segmented && G.n_hay == 0), out, [&](FindStage<acx_spans_t> &F) -> int {
        acx_spans_t *R = F.R;
        hipStream_t st = F.st;
        R->batch = segmented;
        R->rows = segmented ? G.n_hay : 0;
        int rc;
        const uint64_t n = F.r ? F.r->n : 0;
        if (!n) { // no record: no span, and the rows' offsets are zeros
            if ((rc = R->alloc()) != ACX_OK) return rc;
            if (R->batch) HIPCHK(hipMemsetAsync(R->col(ACX_SPAN_ROW_OFFSETS), 0, (R->rows + 1) * 8, st));
            return ACX_OK;
        }
        const uint64_t *d_counts = nullptr;
        if ((rc = F.counts(&d_counts)) != ACX_OK) return rc;
        const uint64_t rows = rows_of(G).n;
        Stage S;
        rc = stage_sizes(a->device, st, F.r->d_matches, n, d_counts, rows, false, gap, &S);
        F.temp = S.block;
        if (rc != ACX_OK) return rc;
        R->n = S.S;
        if ((rc = R->alloc()) != ACX_OK) return rc; // (at most 16 bytes per record: a failure is the call's)
        HIPCHK(acx::spans_emit(F.r->d_matches, n, S.rec_off, rows, gap, S.temp, S.base, S.S, R->col(ACX_SPAN_ROW_OFFSETS),
                               R->col(ACX_SPAN_START), R->col(ACX_SPAN_END), st));
        return ACX_OK;
    });
}

} // namespace

extern "C" {

int acx_spans_host(const acx_match_t *m, uint64_t n_m, const uint64_t *counts, uint64_t n_hay, uint64_t gap, int64_t *row_offsets,
                   int64_t *start, int64_t *end, uint64_t *n_spans) {
    if (!n_spans || (n_m && (!m || !start || !end))) return fail(ACX_EINVAL, "null argument");
    *n_spans = 0;
    int rc = check_gap(gap);
    if (rc != ACX_OK) return rc;
    if (!counts) {
        if (n_hay > 1) return fail(ACX_EINVAL, "several haystacks need counts");
        n_hay = 1;
    }
    if ((rc = counts_sum_to(counts, n_hay, n_m)) != ACX_OK) return rc;
    uint64_t longest = 0;
    for (uint64_t h = 0; h < n_hay; h++) longest = std::max(longest, counts ? counts[h] : n_m);
    std::vector<uint64_t> sm;
    try {
        sm.resize((size_t)longest);
    } catch (...) { return fail(ACX_ENOMEM, "out of memory"); }
    uint64_t first = 0, at = 0;
    for (uint64_t h = 0; h < n_hay; h++) {
        const uint64_t k = counts ? counts[h] : n_m;
        if (row_offsets) row_offsets[h] = (int64_t)at;
        at = host_row(m + first, k, gap, sm.data(), start, end, at);
        first += k;
    }
    if (row_offsets) row_offsets[n_hay] = (int64_t)at;
    *n_spans = at;
    return ACX_OK;
}

int acx_spans(acx_automaton_t *a, const uint8_t *hay, uint64_t len, const uint64_t *offsets, uint64_t n_hay, int overlapping,
              int codepoints, uint64_t gap, acx_spans_t **out) {
    if (!a || !out) return fail(ACX_EINVAL, "null argument");
    *out = nullptr;
    int rc = check_gap(gap);
    if (rc == ACX_OK && overlapping) rc = check_overlapping(a); // (the error, no device state)
    if (rc != ACX_OK) return rc;
    // the find entry points as they are (K0, the resident K0, the in-place read, the staged pipeline), each under its lease:
    // the records cross the bus, the spans are made of them here
    HostFind f;
    if ((rc = f.find(a, hay, len, offsets, n_hay, overlapping, codepoints)) != ACX_OK) return rc;
    const uint64_t rows = offsets ? n_hay : 1, nm = f.nm;
    std::vector<int64_t> tmp;
    uint64_t S = 0;
    try {
        tmp.resize((size_t)(2 * nm + rows + 1));
    } catch (...) { return fail(ACX_ENOMEM, "out of memory"); }
    int64_t *ro = tmp.data() + 2 * nm;
    if ((rc = acx_spans_host(f.m, nm, f.counts.data(), rows, gap, ro, tmp.data(), tmp.data() + nm, &S)) != ACX_OK) return rc;
    acx_spans_t *R = new_result<acx_spans_t>(a->device, false);
    if (!R) return ACX_ENOMEM;
    R->batch = offsets != nullptr;
    R->rows = R->batch ? n_hay : 0;
    R->n = S;
    if ((rc = R->alloc()) != ACX_OK) { free_result(R); return rc; }
    for (int k = 0; k < 2; k++) R->col(k)[0] = 0; // (the one word of an empty column)
    std::memcpy(R->col(ACX_SPAN_START), tmp.data(), (size_t)S * 8);
    std::memcpy(R->col(ACX_SPAN_END), tmp.data() + nm, (size_t)S * 8);
    if (R->batch) std::memcpy(R->col(ACX_SPAN_ROW_OFFSETS), ro, (size_t)(rows + 1) * 8);
    *out = R;
    return ACX_OK;
}

int acx_spans_device(acx_automaton_t *a, const void *d_hay, uint64_t len, const uint64_t *d_offsets, uint64_t n_hay,
                     uint64_t uniform_len, int overlapping, int codepoints, uint64_t gap, acx_spans_t **out) {
    if (!a || !out) return fail(ACX_EINVAL, "null argument");
    *out = nullptr;
    int rc = check_gap(gap);
    if (rc != ACX_OK) return rc;
    return device_call(a, d_hay, len, d_offsets, n_hay, uniform_len, overlapping, [&](Ctx *c, const uint8_t *d_search, const Segments &G) {
        return run_spans(a, c, d_search, len, G, overlapping, codepoints, gap, out);
    });
}

int acx_spans_rows_device(const acx_match_t *d_records, uint64_t n, const uint64_t *d_counts, uint64_t n_hay, uint64_t gap,
                          int64_t *d_row_offsets, int64_t *d_start, int64_t *d_end, uint64_t *n_spans) {
    if (!n_spans || !d_row_offsets || (n && (!d_records || !d_counts || !d_start || !d_end))) return fail(ACX_EINVAL, "null argument");
    *n_spans = 0;
    int rc = check_gap(gap);
    if (rc != ACX_OK) return rc;
    if (!n_hay && n) return fail(ACX_EINVAL, "the counts do not sum to the number of records");
    if (((uintptr_t)d_records | (uintptr_t)d_counts | (uintptr_t)d_row_offsets | (uintptr_t)d_start | (uintptr_t)d_end) & 7)
        return fail(ACX_EINVAL, "records, counts and columns must be 8-byte aligned");
    return rows_call(d_row_offsets, [&](int device, void **block, void **) -> int {
        if (!n) { // no record: no span, and the rows' offsets are zeros
            HIPCHK(hipMemsetAsync(d_row_offsets, 0, (n_hay + 1) * 8, nullptr));
            return ACX_OK;
        }
        Stage S;
        const int sized = stage_sizes(device, nullptr, d_records, n, d_counts, n_hay, true, gap, &S);
        *block = S.block;
        if (sized != ACX_OK) return sized;
        HIPCHK(acx::spans_emit(d_records, n, S.rec_off, n_hay, gap, S.temp, S.base, S.S, d_row_offsets, d_start, d_end, nullptr));
        *n_spans = S.S;
        return ACX_OK;
    });
}

uint64_t acx_spans_count(const acx_spans_t *s) { return s ? s->n : 0; }
uint64_t acx_spans_rows(const acx_spans_t *s) { return s ? s->rows : 0; }
int acx_spans_on_device(const acx_spans_t *s) { return s ? s->on_device : 0; }

const int64_t *acx_spans_data(const acx_spans_t *s, int which) { return (const int64_t *)part_ptr(s, which, N_PARTS); }
int acx_spans_copy(const acx_spans_t *s, int which, int64_t *host_dst) {
    return part_copy(s, which, N_PARTS, host_dst, "no such column", "the single form has no row offsets");
}

void acx_free_spans(acx_spans_t *s) { free_result(s); }

} // extern "C"
