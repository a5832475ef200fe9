// columns_api.cpp -- a find's matches as columns (columns.hpp): the host split, the device route behind the find pipeline,
// the acx_find_columns* entry points, acx_find_words* (the whole-word stage, words.hpp, in front of the columns) and the
// accessors of their result.
#include "columns.hpp"
#include "replace.hpp"
#include "result_block.hpp"

using namespace acxh;

// acx_find_columns / acx_find_columns_device: three columns of `n` words and, for a batch, rows + 1 row offsets, in ONE
// block (result_block.hpp).  Device route: the find's records have gone back to the cache behind the split, only the
// columns and the scan's scratch are kept until acx_free_columns.
struct ACX_HIDDEN acx_columns : ResultBlock {
    bool batch = false;
    uint64_t n = 0, rows = 0;

    // the block (by on_device) and its parts, ACX_COL_*; the single form has no row offsets
    int alloc() { return batch ? alloc_parts({n * 8, n * 8, n * 8, (rows + 1) * 8}) : alloc_parts({n * 8, n * 8, n * 8}); }
    int64_t *col(int which) const { return at<int64_t>(which); }
};

namespace {

constexpr int N_PARTS = ACX_COL_ROW_OFFSETS + 1;

// The device route: the find pipeline as acx_find_device runs it (byte ranges, batch splits and the expansion of copies
// included), then the split -- and, for a batch, the scan of the counts -- on the same stream.  Returns when the number of
// matches is known; the kernels may still run (out->done).  d_hay, and G.offsets, must stay valid until then.
int run_columns(acx_automaton *a, Ctx *x, const uint8_t *d_hay, uint64_t len, const Segments &G, int overlapping,
                int codepoints, acx_columns **out) {
    const bool segmented = rows_of(G).segmented;
    // (an empty batch: nothing to search, one row offset)
    return find_stage(a, x, d_hay, len, G, overlapping, codepoints, !(segmented && G.n_hay == 0), out, [&](FindStage<acx_columns> &F) -> int {
        acx_columns *R = F.R;
        R->batch = segmented;
        R->rows = segmented ? G.n_hay : 0;
        R->n = F.r ? F.r->n : 0;
        int rc = R->alloc();
        if (rc != ACX_OK) return rc;
        if (F.r) HIPCHK(acx::col_split(F.r->d_matches, R->n, R->col(0), R->col(1), R->col(2), F.st));
        if (R->batch && R->rows) { // where every haystack's records begin, from the counts
            uint64_t *temp = nullptr;
            HIPCHK(g_bufs.get((void **)&temp, std::max<uint64_t>(replace_scan_words(R->rows) * 8, 16), a->device));
            F.keep(temp);
            HIPCHK(acx::replace_scan(nullptr, nullptr, F.r->d_counts, R->rows, R->col(3), temp, F.st));
        } else if (R->batch) {
            HIPCHK(hipMemsetAsync(R->col(3), 0, 8, F.st));
        }
        return ACX_OK;
    });
}

// acx_find_words_device: an OVERLAPPING find on d_search (a case-insensitive handle: the folded copy), then the whole-word
// stage (words.hpp) on the same stream over d_hay -- the caller's own bytes -- and its survivors straight into the columns.
// Returns when the number of matches is known; the last kernel may still run (out->done).
int run_words(acx_automaton *a, Ctx *x, const uint8_t *d_hay, const uint8_t *d_search, uint64_t len, const Segments &G,
              const WordsArgs &A, acx_columns **out) {
    const bool segmented = rows_of(G).segmented;
    // (an empty batch: nothing to search, one row offset)
    return find_stage(a, x, d_search, len, G, 1, 0, !(segmented && G.n_hay == 0), out, [&](FindStage<acx_columns> &F) -> int {
        acx_columns *R = F.R;
        R->batch = segmented;
        R->rows = segmented ? G.n_hay : 0;
        const uint64_t n = F.r ? F.r->n : 0;
        int rc;
        if (!n) { // no occurrence: no whole word, and the rows' offsets are zeros
            if ((rc = R->alloc()) != ACX_OK) return rc;
            if (R->batch) HIPCHK(hipMemsetAsync(R->col(ACX_COL_ROW_OFFSETS), 0, (R->rows + 1) * 8, F.st));
            return ACX_OK;
        }
        const uint64_t *d_counts = nullptr;
        if ((rc = F.counts(&d_counts)) != ACX_OK) return rc;
        WordsStage S;
        rc = words_sizes(a->device, F.st, F.r->d_matches, n, d_counts, row_cut(G, len), false, d_hay, A, &S);
        F.temp = S.block;
        if (rc != ACX_OK) return rc;
        R->n = S.total;
        if ((rc = R->alloc()) != ACX_OK) return rc;
        return words_finish(S, acx::WordsOut{nullptr, R->col(ACX_COL_PATTERN), R->col(ACX_COL_START), R->col(ACX_COL_END)},
                            R->batch ? R->col(ACX_COL_ROW_OFFSETS) : nullptr, nullptr, F.st);
    });
}

// a host result for n matches (rows: of a batch), its columns' first words zeroed; null: the error is set
acx_columns *host_columns(int device, bool batch, uint64_t rows, uint64_t n) {
    acx_columns *R = new_result<acx_columns>(device, false);
    if (!R) return nullptr;
    R->batch = batch;
    R->rows = batch ? rows : 0;
    R->n = n;
    if (R->alloc() != ACX_OK) { free_result(R); return nullptr; }
    for (int k = 0; k < 3; k++) R->col(k)[0] = 0; // (the one word of an empty column)
    return R;
}

} // namespace

extern "C" {

int acx_split_host(const acx_match_t *m, uint64_t n, int64_t *pattern, int64_t *start, int64_t *end) {
    if (n && (!m || !pattern || !start || !end)) return fail(ACX_EINVAL, "null argument");
    for (uint64_t i = 0; i < n; i++) {
        pattern[i] = (int64_t)m[i].pattern;
        start[i] = (int64_t)m[i].start;
        end[i] = (int64_t)m[i].end;
    }
    return ACX_OK;
}

int acx_split_device(const acx_match_t *d_m, uint64_t n, int64_t *d_pattern, int64_t *d_start, int64_t *d_end) {
    if (!n) return ACX_OK;
    if (!d_m || !d_pattern || !d_start || !d_end) return fail(ACX_EINVAL, "null argument");
    if (((uintptr_t)d_m | (uintptr_t)d_pattern | (uintptr_t)d_start | (uintptr_t)d_end) & 7)
        return fail(ACX_EINVAL, "records and columns must be 8-byte aligned");
    return rows_call(d_m, [&](int, void **, void **) -> int {
        HIPCHK(acx::col_split(d_m, n, d_pattern, d_start, d_end, nullptr));
        return ACX_OK;
    });
}

int acx_find_columns(acx_automaton_t *a, const uint8_t *hay, uint64_t len, const uint64_t *offsets, uint64_t n_hay,
                     int overlapping, int codepoints, acx_columns_t **out) {
    if (!a || !out) return fail(ACX_EINVAL, "null argument");
    *out = nullptr;
    // the find entry points as they are (K0, the resident K0, the in-place read, the staged pipeline), each under its lease
    HostFind f;
    int rc = f.find(a, hay, len, offsets, n_hay, overlapping, codepoints);
    if (rc != ACX_OK) return rc;
    acx_columns *R = new_result<acx_columns>(a->device, false);
    if (!R) return ACX_ENOMEM;
    R->batch = offsets != nullptr;
    R->rows = R->batch ? n_hay : 0;
    R->n = f.nm;
    if ((rc = R->alloc()) != ACX_OK) { free_result(R); return rc; }
    for (int k = 0; k < 3; k++) R->col(k)[0] = 0; // (the one word of an empty column)
    rc = acx_split_host(f.m, f.nm, R->col(0), R->col(1), R->col(2));
    if (R->batch) {
        int64_t at = 0;
        for (uint64_t h = 0; h < n_hay; h++) { R->col(3)[h] = at; at += (int64_t)f.counts[h]; }
        R->col(3)[n_hay] = at;
    }
    if (rc != ACX_OK) { free_result(R); return rc; }
    *out = R;
    return ACX_OK;
}

int acx_find_columns_device(acx_automaton_t *a, const void *d_hay, uint64_t len, const uint64_t *d_offsets, uint64_t n_hay,
                            uint64_t uniform_len, int overlapping, int codepoints, acx_columns_t **out) {
    if (!a || !out) return fail(ACX_EINVAL, "null argument");
    *out = nullptr;
    return device_call(a, d_hay, len, d_offsets, n_hay, uniform_len, overlapping, [&](Ctx *c, const uint8_t *d_search, const Segments &G) {
        return run_columns(a, c, d_search, len, G, overlapping, codepoints, out);
    });
}

int acx_find_words(acx_automaton_t *a, const uint8_t *hay, uint64_t len, const uint64_t *offsets, uint64_t n_hay, int overlapping,
                   int match_kind, const uint8_t *word_set, acx_columns_t **out) {
    if (!a || !out) return fail(ACX_EINVAL, "null argument");
    *out = nullptr;
    WordsArgs A;
    int rc = words_args(overlapping, match_kind, word_set, &A);
    if (rc == ACX_OK) rc = check_overlapping(a); // (the stage's find is an overlapping one: the error, no device state)
    if (rc != ACX_OK) return rc;
    HostBatch B;
    if ((rc = host_batch(hay, &len, offsets, &n_hay, &B)) != ACX_OK) return rc;
    const bool batch = offsets != nullptr;
    if (len <= words_host_max() || !n_hay) {
        std::vector<acx_match_t> m;
        std::vector<uint64_t> counts;
        if ((rc = words_host_find(a, B, len, n_hay, batch, A, word_set, &m, &counts)) != ACX_OK) return rc;
        acx_columns *R = host_columns(a->device, batch, n_hay, m.size());
        if (!R) return ACX_ENOMEM;
        (void)acx_split_host(m.data(), m.size(), R->col(0), R->col(1), R->col(2));
        if (batch) {
            int64_t at = 0;
            for (uint64_t h = 0; h < n_hay; h++) { R->col(3)[h] = at; at += (int64_t)counts[h]; }
            R->col(3)[n_hay] = at;
        }
        *out = R;
        return ACX_OK;
    }
    // device route: staged, searched and resolved under one lease; the columns come home in one copy
    acx_columns *D = nullptr;
    rc = staged_call(a, B, len, n_hay, batch, [&](Ctx *c, const uint8_t *d_search, const Segments &G) {
        const int run = run_words(a, c, c->ws.hay, d_search, len, G, A, &D);
        return run == ACX_OK ? D->wait() : run; // (the staging buffers are the context's: the lease ends behind the kernels)
    });
    return copy_down(rc, D, rc == ACX_OK ? host_columns(a->device, batch, n_hay, D->n) : nullptr, D ? D->block_bytes : 0,
                     "copying the columns to the host", out);
}

int acx_find_words_device(acx_automaton_t *a, const void *d_hay, uint64_t len, const uint64_t *d_offsets, uint64_t n_hay,
                          uint64_t uniform_len, int overlapping, int match_kind, const uint8_t *word_set, acx_columns_t **out) {
    if (!a || !out) return fail(ACX_EINVAL, "null argument");
    *out = nullptr;
    WordsArgs A;
    const int rc = words_args(overlapping, match_kind, word_set, &A);
    if (rc != ACX_OK) return rc;
    // (a case-insensitive handle: the folded copy is searched, the caller's bytes are tested)
    return device_call(a, d_hay, len, d_offsets, n_hay, uniform_len, 1, [&](Ctx *c, const uint8_t *d_search, const Segments &G) {
        return run_words(a, c, (const uint8_t *)d_hay, d_search, len, G, A, out);
    });
}

uint64_t acx_columns_count(const acx_columns_t *c) { return c ? c->n : 0; }
uint64_t acx_columns_rows(const acx_columns_t *c) { return c ? c->rows : 0; }
int acx_columns_on_device(const acx_columns_t *c) { return c ? c->on_device : 0; }

const int64_t *acx_columns_data(const acx_columns_t *c, int which) { return (const int64_t *)part_ptr(c, which, N_PARTS); }
int acx_columns_copy(const acx_columns_t *c, int which, int64_t *host_dst) {
    return part_copy(c, which, N_PARTS, host_dst, "no such column", "the single form has no row offsets");
}

void acx_free_columns(acx_columns_t *c) { free_result(c); }

} // extern "C"
