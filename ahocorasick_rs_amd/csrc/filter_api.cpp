// filter_api.cpp -- keep or drop the rows of a batch by match (filter.hpp): the host form, the device stage behind the find
// pipeline, the acx_filter* entry points and the accessors of their result.
#include "filter.hpp"
#include "replace.hpp"
#include "result_block.hpp"
#include "score.hpp"

using namespace acxh;

// acx_filter / acx_filter_device: the kept rows' source indexes (k words), their offsets (k + 1 words) and their bytes in ONE
// block (result_block.hpp), the data part rounded up to 16 bytes for the tile's stores.  Device route: the find's records
// and counts and the stage's temporaries have gone back to the cache behind the stage's kernels.
struct ACX_HIDDEN acx_filtered : ResultBlock {
    uint64_t n_src = 0, rows = 0, bytes = 0;

    // the block (by on_device) and its parts, ACX_FILT_*; the tail of 16 gives the data round_up(bytes, 16), at least 16
    int alloc() { return alloc_parts({rows * 8, (rows + 1) * 8, bytes}, 16); }
};

namespace {

constexpr int N_PARTS = ACX_FILT_DATA + 1;

// The temporaries of one run of the device stage: one block of the buffer cache.
struct Stage {
    void *block = nullptr;
    uint64_t *klen = nullptr, *kflag = nullptr, *scan_tmp = nullptr, *src = nullptr, *tiles = nullptr;
    int64_t *A = nullptr, *B = nullptr;
    acx::RowCut R{nullptr, 0, 0, 0};
};

// The stage up to the point where the result's size is known: the flags and the two scans (n > 0).  d_counts: n words.
int stage_sizes(int device, hipStream_t st, const acx::RowCut &R, const uint64_t *d_counts, uint64_t min_matches,
                bool keep_matched, Stage *S, uint64_t *k, uint64_t *total) {
    S->R = R;
    const uint64_t n = R.n;
    // [klen: n][kflag: n][A: n + 1][B: n + 1][scan][src: n][tiles], every part 256-byte aligned
    Carver C;
    const uint64_t o_len = C.part(n), o_flag = C.part(n), o_a = C.part(n + 1), o_b = C.part(n + 1),
                   o_scan = C.part(replace_scan_words(n)), o_src = C.part(n), o_tiles = C.part(acx::filter_tile_words(R.len));
    HIPCHK(g_bufs.get(&S->block, C.bytes(), device));
    uint64_t *b = (uint64_t *)S->block;
    S->klen = b + o_len;
    S->kflag = b + o_flag;
    S->A = (int64_t *)(b + o_a);
    S->B = (int64_t *)(b + o_b);
    S->scan_tmp = b + o_scan;
    S->src = b + o_src;
    S->tiles = b + o_tiles;
    HIPCHK(acx::filter_flags(R, d_counts, min_matches, keep_matched, S->klen, S->kflag, st));
    HIPCHK(acx::replace_scan(nullptr, nullptr, S->klen, n, S->A, S->scan_tmp, st));
    HIPCHK(acx::replace_scan(nullptr, nullptr, S->kflag, n, S->B, S->scan_tmp, st));
    uint64_t back[2] = {0, 0}; // the output's bytes, the kept rows: all that crosses the bus
    HIPCHK(hipMemcpyAsync(&back[0], S->A + n, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&back[1], S->B + n, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (back[1] > n || back[0] > R.len) return fail(ACX_EINVAL, "the rows' lengths do not sum to the batch's length");
    *total = back[0];
    *k = back[1];
    return ACX_OK;
}

// ... and from there: the three parts into their places (device memory; rows and offsets 8-byte aligned, data 16-byte aligned
// with room for round_up(total, 16)).  k == 0: one offset, 0.  k == n: the data is a copy of the input.
int stage_finish(const Stage *S, const uint8_t *d_hay, uint64_t k, uint64_t total, int64_t *rows, int64_t *offsets, uint8_t *data,
                 hipStream_t st) {
    if (!k) {
        HIPCHK(hipMemsetAsync(offsets, 0, 8, st));
        return ACX_OK;
    }
    HIPCHK(acx::filter_index(S->R, S->A, S->B, rows, offsets, S->src, st));
    if (!total) return ACX_OK;
    if (k == S->R.n) {
        HIPCHK(hipMemcpyAsync(data, d_hay, total, hipMemcpyDeviceToDevice, st));
        return ACX_OK;
    }
    HIPCHK(acx::filter_gather(d_hay, S->R.len, offsets, S->src, k, S->tiles, data, total, st));
    return ACX_OK;
}

// acx_filter_scored*: the verdict on a row is its score (score.hpp) against min_score, not its number of matches
struct ScoreBy {
    const int32_t *weights; // host memory, n_weights of them
    uint64_t n_weights;
    int64_t min_score;
};

int check_scored(const acx_automaton *a, const ScoreBy &sc, uint32_t flags) {
    if (flags & ~(uint32_t)ACX_FILTER_KEEP_MATCHED) return fail(ACX_EINVAL, "unknown filter flags");
    if (sc.n_weights != a->host.n_patterns) return fail(ACX_EINVAL, "one weight per pattern is needed");
    if (sc.n_weights && !sc.weights) return fail(ACX_EINVAL, "null argument");
    return ACX_OK;
}

int check_args(uint64_t min_matches, uint32_t flags) {
    if (flags & ~(uint32_t)ACX_FILTER_KEEP_MATCHED) return fail(ACX_EINVAL, "unknown filter flags");
    if (!min_matches) return fail(ACX_EINVAL, "min_matches must be at least 1");
    return ACX_OK;
}

// The device route: the find pipeline as acx_find_device runs it (batch splits and the expansion of copies included, byte
// offsets: no offset is reported) on d_search, then the stage on the same stream over d_hay -- the caller's own bytes.
// Returns when the result's size is known; the gather may still run (out->done).  d_hay, d_search and G.offsets must stay
// valid until then.  by != null: the rows' scores and their 0 / 1 verdicts are made between the find and the stage, on the
// same stream, and the stage runs on the verdicts as its counts with min_matches = 1.  words != null (the find is an
// overlapping one): the whole-word stage (words.hpp) runs between the find and the stage, on the same stream, and the stage
// runs on the new counts -- no record is written.
int run_filter(acx_automaton *a, Ctx *x, const uint8_t *d_hay, const uint8_t *d_search, uint64_t len, const Segments &G,
               int overlapping, uint64_t min_matches, uint32_t flags, acx_filtered_t **out, const ScoreBy *by = nullptr,
               const WordsArgs *words = nullptr) {
    const uint64_t n = rows_of(G).n;
    // (an empty batch: nothing to search, one offset)
    return find_stage(a, x, d_search, len, G, overlapping, 0, n != 0, out, [&](FindStage<acx_filtered> &F) -> int {
        acx_filtered *R = F.R;
        hipStream_t st = F.st;
        R->n_src = n;
        int rc;
        Stage S;
        if (n) {
            const uint64_t *d_counts = nullptr;
            if ((rc = F.counts(&d_counts)) != ACX_OK) return rc;
            if (by) { // (stage_sizes waits for the stream: the caller's weights are uploaded when it returns)
                ScoreTemps T;
                rc = score_stage(a->device, st, F.r->d_matches, F.r->n, d_counts, n, by->weights, nullptr, by->n_weights, false, nullptr,
                                 &by->min_score, &T);
                F.keep(T.block); // (the scored form: kept until acx_free_filtered)
                if (rc != ACX_OK) return rc;
                d_counts = T.flags;
                min_matches = 1;
            }
            void *wblock = nullptr;
            if (words && F.r->n) { // (no occurrence: the find's zeros are the counts)
                WordsStage W;
                rc = words_sizes(a->device, st, F.r->d_matches, F.r->n, d_counts, row_cut(G, len), false, d_hay, *words, &W);
                wblock = W.block;
                if (rc == ACX_OK) rc = words_finish(W, acx::WordsOut{nullptr, nullptr, nullptr, nullptr}, nullptr, W.new_counts, st);
                if (rc != ACX_OK) { F.keep(wblock); return rc; } // (it goes back with the result, behind the stream)
                d_counts = W.new_counts;
            }
            const acx::RowCut rows = row_cut(G, len);
            rc = stage_sizes(a->device, st, rows, d_counts, min_matches, (flags & ACX_FILTER_KEEP_MATCHED) != 0, &S, &R->rows, &R->bytes);
            F.temp = S.block;
            if (rc == ACX_OK) g_bufs.put(wblock, a->device); // (stage_sizes has waited for the stream: the new counts are spent)
            else F.keep(wblock);
            if (rc != ACX_OK) return rc;
        }
        if ((rc = R->alloc()) != ACX_OK) return rc;
        return stage_finish(&S, d_hay, R->rows, R->bytes, R->at<int64_t>(0), R->at<int64_t>(1), R->at<uint8_t>(2), st);
    });
}

// The host route's end: the rows kept by counts[h] >= min_matches, copied from the caller's memory (the output never crosses
// the bus)
int host_filtered(const acx_automaton *a, const HostBatch &B, uint64_t len, uint64_t n_hay, const uint64_t *counts,
                  uint64_t min_matches, uint32_t flags, acx_filtered_t **out) {
    uint64_t k = 0, total = 0;
    int rc = acx_filter_host(B.hay, len, B.rel.data(), n_hay, counts, min_matches, flags, nullptr, nullptr, nullptr, &k, &total);
    if (rc != ACX_OK) return rc;
    acx_filtered_t *R = new_result<acx_filtered_t>(a->device, false);
    if (!R) return ACX_ENOMEM;
    R->n_src = n_hay;
    R->rows = k;
    R->bytes = total;
    if ((rc = R->alloc()) != ACX_OK) { free_result(R); return rc; }
    rc = acx_filter_host(B.hay, len, B.rel.data(), n_hay, counts, min_matches, flags, R->at<int64_t>(0), R->at<int64_t>(1),
                         R->at<uint8_t>(2), &R->rows, &R->bytes);
    if (rc != ACX_OK) { free_result(R); return rc; }
    *out = R;
    return ACX_OK;
}

} // namespace

extern "C" {

int acx_filter_host(const uint8_t *hay, uint64_t len, const uint64_t *offsets, uint64_t n_hay, const uint64_t *counts,
                    uint64_t min_matches, uint32_t flags, int64_t *rows, int64_t *out_offsets, uint8_t *dst, uint64_t *n_rows,
                    uint64_t *n_bytes) {
    int rc = check_args(min_matches, flags);
    if (rc != ACX_OK) return rc;
    if (!n_rows || !n_bytes || (n_hay && !counts) || (len && dst && !hay)) return fail(ACX_EINVAL, "null argument");
    if (!offsets && n_hay > 1) return fail(ACX_EINVAL, "several haystacks need offsets");
    if (offsets && (rc = offsets_span(offsets, n_hay, len)) != ACX_OK) return rc;
    const bool keep_matched = (flags & ACX_FILTER_KEEP_MATCHED) != 0;
    uint64_t k = 0, at = 0;
    for (uint64_t h = 0; h < n_hay; h++) {
        if ((counts[h] >= min_matches) != keep_matched) continue;
        const uint64_t b = offsets ? offsets[h] : 0, e = offsets ? offsets[h + 1] : len;
        if (rows) rows[k] = (int64_t)h;
        if (out_offsets) out_offsets[k] = (int64_t)at;
        if (dst && e > b) std::memcpy(dst + at, hay + b, e - b);
        at += e - b;
        k++;
    }
    if (out_offsets) out_offsets[k] = (int64_t)at;
    *n_rows = k;
    *n_bytes = at;
    return ACX_OK;
}

int acx_filter(acx_automaton_t *a, const uint8_t *hay, uint64_t len, const uint64_t *offsets, uint64_t n_hay, int overlapping,
               uint64_t min_matches, uint32_t flags, acx_filtered_t **out) {
    if (!a || !out) return fail(ACX_EINVAL, "null argument");
    *out = nullptr;
    int rc = check_args(min_matches, flags);
    if (rc == ACX_OK && overlapping) rc = check_overlapping(a); // (the error, no device state)
    if (rc != ACX_OK) return rc;
    HostBatch B;
    if ((rc = host_batch(hay, &len, offsets, &n_hay, &B)) != ACX_OK) return rc;
    std::vector<uint64_t> counts;
    try {
        counts.assign(n_hay + 1, 0);
    } catch (...) { return fail(ACX_ENOMEM, "out of memory"); }
    if (n_hay) { // the counts: the summary chooses its own route, 8 bytes per row come back
        acx_summary_t *s = nullptr;
        rc = acx_summarize(a, B.hay, len, offsets ? B.rel.data() : nullptr, n_hay, overlapping, 0, 0, &s);
        if (rc == ACX_OK) rc = acx_summary_counts(s, counts.data());
        acx_free_summary(s);
        if (rc != ACX_OK) return rc;
    }
    return host_filtered(a, B, len, n_hay, counts.data(), min_matches, flags, out);
}

int acx_filter_scored(acx_automaton_t *a, const uint8_t *hay, uint64_t len, const uint64_t *offsets, uint64_t n_hay, int overlapping,
                      const int32_t *weights, uint64_t n_weights, int64_t min_score, uint32_t flags, acx_filtered_t **out) {
    if (!a || !out) return fail(ACX_EINVAL, "null argument");
    *out = nullptr;
    int rc = check_scored(a, ScoreBy{weights, n_weights, min_score}, flags);
    if (rc == ACX_OK && overlapping) rc = check_overlapping(a); // (the error, no device state)
    if (rc != ACX_OK) return rc;
    HostBatch B;
    if ((rc = host_batch(hay, &len, offsets, &n_hay, &B)) != ACX_OK) return rc;
    std::vector<uint64_t> verdict;
    std::vector<int64_t> score;
    try {
        verdict.assign(n_hay + 1, 0);
        score.assign(n_hay + 1, 0);
    } catch (...) { return fail(ACX_ENOMEM, "out of memory"); }
    if (n_hay) { // the scores: acx_score chooses its own route, 8 bytes per row come back
        acx_scores_t *s = nullptr;
        rc = acx_score(a, B.hay, len, B.rel.data(), n_hay, overlapping, weights, n_weights, &s);
        if (rc == ACX_OK) rc = acx_scores_copy(s, score.data());
        acx_free_scores(s);
        if (rc != ACX_OK) return rc;
    }
    for (uint64_t h = 0; h < n_hay; h++) verdict[h] = score[h] >= min_score ? 1 : 0;
    return host_filtered(a, B, len, n_hay, verdict.data(), 1, flags, out);
}

int acx_filter_device(acx_automaton_t *a, const void *d_hay, uint64_t len, const uint64_t *d_offsets, uint64_t n_hay,
                      uint64_t uniform_len, int overlapping, uint64_t min_matches, uint32_t flags, acx_filtered_t **out) {
    if (!a || !out) return fail(ACX_EINVAL, "null argument");
    *out = nullptr;
    int rc = check_args(min_matches, flags);
    if (rc != ACX_OK) return rc;
    // (a case-insensitive handle: the folded copy is searched, the caller's bytes are copied)
    return device_call(a, d_hay, len, d_offsets, n_hay, uniform_len, overlapping, [&](Ctx *c, const uint8_t *d_search, const Segments &G) {
        return run_filter(a, c, (const uint8_t *)d_hay, d_search, len, G, overlapping, min_matches, flags, out);
    });
}

int acx_filter_scored_device(acx_automaton_t *a, const void *d_hay, uint64_t len, const uint64_t *d_offsets, uint64_t n_hay,
                             uint64_t uniform_len, int overlapping, const int32_t *weights, uint64_t n_weights, int64_t min_score,
                             uint32_t flags, acx_filtered_t **out) {
    if (!a || !out) return fail(ACX_EINVAL, "null argument");
    *out = nullptr;
    const ScoreBy by{weights, n_weights, min_score};
    int rc = check_scored(a, by, flags);
    if (rc != ACX_OK) return rc;
    return device_call(a, d_hay, len, d_offsets, n_hay, uniform_len, overlapping, [&](Ctx *c, const uint8_t *d_search, const Segments &G) {
        return run_filter(a, c, (const uint8_t *)d_hay, d_search, len, G, overlapping, 1, flags, out, &by);
    });
}

int acx_filter_words(acx_automaton_t *a, const uint8_t *hay, uint64_t len, const uint64_t *offsets, uint64_t n_hay, int overlapping,
                     int match_kind, const uint8_t *word_set, uint64_t min_matches, uint32_t flags, acx_filtered_t **out) {
    if (!a || !out) return fail(ACX_EINVAL, "null argument");
    *out = nullptr;
    WordsArgs A;
    int rc = check_args(min_matches, flags);
    if (rc == ACX_OK) rc = words_args(overlapping, match_kind, word_set, &A);
    if (rc == ACX_OK) rc = check_overlapping(a); // (the stage's find is an overlapping one: the error, no device state)
    if (rc != ACX_OK) return rc;
    HostBatch B;
    const bool batch = offsets != nullptr;
    if ((rc = host_batch(hay, &len, offsets, &n_hay, &B)) != ACX_OK) return rc;
    if (len <= words_host_max() || !n_hay) {
        std::vector<acx_match_t> m;
        std::vector<uint64_t> counts;
        if ((rc = words_host_find(a, B, len, n_hay, batch, A, word_set, &m, &counts)) != ACX_OK) return rc;
        return host_filtered(a, B, len, n_hay, counts.data(), min_matches, flags, out);
    }
    // device route: staged, searched, resolved and compacted under one lease; the kept rows come home in one copy
    acx_filtered_t *D = nullptr, *R = nullptr;
    rc = staged_call(a, B, len, n_hay, batch, [&](Ctx *c, const uint8_t *d_search, const Segments &G) {
        const int run = run_filter(a, c, c->ws.hay, d_search, len, G, 1, min_matches, flags, &D, nullptr, &A);
        return run == ACX_OK ? D->wait() : run; // (the staging buffers are the context's: the lease ends behind the kernels)
    });
    if (rc == ACX_OK && (R = new_result<acx_filtered_t>(a->device, false))) {
        R->n_src = D->n_src;
        R->rows = D->rows;
        R->bytes = D->bytes;
        if (R->alloc() != ACX_OK) { free_result(R); R = nullptr; }
    }
    return copy_down(rc, D, R, D ? D->block_bytes : 0, "copying the kept rows to the host", out);
}

int acx_filter_words_device(acx_automaton_t *a, const void *d_hay, uint64_t len, const uint64_t *d_offsets, uint64_t n_hay,
                            uint64_t uniform_len, int overlapping, int match_kind, const uint8_t *word_set, uint64_t min_matches,
                            uint32_t flags, acx_filtered_t **out) {
    if (!a || !out) return fail(ACX_EINVAL, "null argument");
    *out = nullptr;
    WordsArgs A;
    int rc = check_args(min_matches, flags);
    if (rc == ACX_OK) rc = words_args(overlapping, match_kind, word_set, &A);
    if (rc != ACX_OK) return rc;
    return device_call(a, d_hay, len, d_offsets, n_hay, uniform_len, 1, [&](Ctx *c, const uint8_t *d_search, const Segments &G) {
        return run_filter(a, c, (const uint8_t *)d_hay, d_search, len, G, 1, min_matches, flags, out, nullptr, &A);
    });
}

int acx_filter_rows_device(const void *d_hay, uint64_t len, const uint64_t *d_offsets, uint64_t n_hay, uint64_t uniform_len,
                           const uint64_t *d_counts, uint64_t min_matches, uint32_t flags, int64_t *d_rows,
                           int64_t *d_out_offsets, uint8_t *d_data, uint64_t *n_rows, uint64_t *n_bytes) {
    int rc = check_args(min_matches, flags);
    if (rc != ACX_OK) return rc;
    if (!d_out_offsets || !n_rows || !n_bytes) return fail(ACX_EINVAL, "null argument");
    *n_rows = *n_bytes = 0;
    if ((rc = device_rows_args(d_offsets, &n_hay, uniform_len, len)) != ACX_OK) return rc;
    if ((n_hay && (!d_counts || !d_rows)) || (len && (!d_hay || !d_data))) return fail(ACX_EINVAL, "null argument");
    if (((uintptr_t)d_offsets | (uintptr_t)d_counts | (uintptr_t)d_rows | (uintptr_t)d_out_offsets) & 7)
        return fail(ACX_EINVAL, "offsets, counts and the word outputs must be 8-byte aligned");
    if ((uintptr_t)d_data & 15) return fail(ACX_EINVAL, "the data output must be 16-byte aligned");
    uint64_t k = 0, total = 0;
    rc = rows_call(d_out_offsets, [&](int device, void **block, void **) -> int {
        if (!n_hay) { // (no row: the one offset)
            HIPCHK(hipMemsetAsync(d_out_offsets, 0, 8, nullptr));
            return ACX_OK;
        }
        int rs = device_offsets_span(d_offsets, n_hay, len);
        if (rs != ACX_OK) return rs;
        Stage S;
        const acx::RowCut rows{d_offsets, uniform_len, n_hay, len};
        rs = stage_sizes(device, nullptr, rows, d_counts, min_matches, (flags & ACX_FILTER_KEEP_MATCHED) != 0, &S, &k, &total);
        *block = S.block;
        return rs == ACX_OK ? stage_finish(&S, (const uint8_t *)d_hay, k, total, d_rows, d_out_offsets, d_data, nullptr) : rs;
    });
    if (rc == ACX_OK) { *n_rows = k; *n_bytes = total; }
    return rc;
}

uint64_t acx_filtered_rows(const acx_filtered_t *f) { return f ? f->rows : 0; }
uint64_t acx_filtered_bytes(const acx_filtered_t *f) { return f ? f->bytes : 0; }
int acx_filtered_on_device(const acx_filtered_t *f) { return f ? f->on_device : 0; }

const void *acx_filtered_data(const acx_filtered_t *f, int which) { return part_ptr(f, which, N_PARTS); }
int acx_filtered_copy(const acx_filtered_t *f, int which, void *host_dst) { return part_copy(f, which, N_PARTS, host_dst, "no such part"); }

void acx_free_filtered(acx_filtered_t *f) { free_result(f); }

} // extern "C"
