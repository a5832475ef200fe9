// score_api.cpp -- per-row scores from per-pattern weights (score.hpp): the host form, the device stage behind the find
// pipeline, the acx_score* entry points and the accessors of their result.  acx_filter_scored* are filter_api.cpp's: they
// return its result.
#include "replace.hpp"
#include "result_block.hpp"
#include "score.hpp"

using namespace acxh;

// acx_score / acx_score_device: rows int64 words in ONE block (result_block.hpp).  Device route: the find's records and the
// stage's temporaries have gone back to the cache behind the stage's kernels; `weights` is the call's copy of the caller's
// weights, which the upload reads until `done`.
struct ACX_HIDDEN acx_scores : ResultBlock {
    uint64_t rows = 0;
    std::vector<int32_t> weights;

    int alloc() { return alloc_parts({rows * 8}); } // the block (by on_device): its one part
    int64_t *score() const { return at<int64_t>(0); }
};

namespace acxh ACX_HIDDEN {

int score_stage(int device, hipStream_t st, const acx_match_t *d_m, uint64_t n, const uint64_t *d_counts, uint64_t rows,
                const int32_t *h_weights, const int32_t *d_weights, uint64_t n_patterns, bool check_sum, int64_t *d_score,
                const int64_t *min_score, ScoreTemps *T) {
    // [rec_off: rows + 1][scan][tiles][weights: n_patterns int32][score: rows][flags: rows], every part 256-byte aligned
    Carver C;
    const uint64_t o_rec = C.part(rows + 1), o_scan = C.part(replace_scan_words(rows)), o_tiles = C.part(acx::score_tile_words(n)),
                   o_w = C.part(h_weights ? (n_patterns + 1) / 2 : 0), o_score = C.part(d_score ? 0 : rows),
                   o_flags = C.part(min_score ? rows : 0);
    HIPCHK(g_bufs.get(&T->block, C.bytes(), device));
    uint64_t *b = (uint64_t *)T->block;
    int64_t *rec_off = (int64_t *)(b + o_rec);
    T->score = d_score ? d_score : (int64_t *)(b + o_score);
    if (h_weights) {
        if (n_patterns) HIPCHK(hipMemcpyAsync(b + o_w, h_weights, n_patterns * 4, hipMemcpyHostToDevice, st));
        d_weights = (const int32_t *)(b + o_w);
    }
    int rc = record_offsets(d_counts, rows, n, check_sum, rec_off, b + o_scan, st);
    if (rc != ACX_OK) return rc;
    HIPCHK(acx::score_rows(d_m, n, rec_off, rows, d_weights, n_patterns, b + o_tiles, T->score, st));
    if (min_score) {
        T->flags = b + o_flags;
        HIPCHK(acx::score_flags(T->score, rows, *min_score, T->flags, st));
    }
    return ACX_OK;
}

} // namespace acxh

namespace {

// ACX_SCORE_HOST_MAX (bytes, read per call): batches up to this size are scored on the host, behind acx_find_batch.  The
// default is ACX_SUMMARY_HOST_MAX's, which is itself not a measured crossover.
uint64_t score_host_max() {
    const char *e = std::getenv("ACX_SCORE_HOST_MAX");
    return e ? std::strtoull(e, nullptr, 10) : (1ull << 20);
}

int check_weights(const acx_automaton *a, const int32_t *weights, uint64_t n_weights) {
    if (n_weights != a->host.n_patterns) return fail(ACX_EINVAL, "one weight per pattern is needed");
    if (n_weights && !weights) return fail(ACX_EINVAL, "null argument");
    return ACX_OK;
}

// The device route: the find pipeline as acx_find_device runs it (batch splits and the expansion of copies included, byte
// offsets: no offset is reported), then the stage on the same stream.  Returns with the stage in flight (out->done).
// d_hay, and G.offsets, must stay valid until then; the weights are copied here.
int run_score(acx_automaton *a, Ctx *x, const uint8_t *d_hay, uint64_t len, const Segments &G, int overlapping,
              const int32_t *weights, uint64_t n_weights, acx_scores_t **out) {
    const uint64_t rows = rows_of(G).n;
    // (an empty batch: nothing to search, no score)
    return find_stage(a, x, d_hay, len, G, overlapping, 0, rows != 0, out, [&](FindStage<acx_scores> &F) -> int {
        acx_scores *R = F.R;
        R->rows = rows;
        try {
            R->weights.assign(weights, weights + n_weights);
        } catch (...) { return fail(ACX_ENOMEM, "out of memory"); }
        int rc;
        if ((rc = R->alloc()) != ACX_OK || !rows) return rc;
        const uint64_t *d_counts = nullptr;
        if ((rc = F.counts(&d_counts)) != ACX_OK) return rc;
        ScoreTemps T;
        rc = score_stage(a->device, F.st, F.r->d_matches, F.r->n, d_counts, rows, R->weights.data(), nullptr, n_weights, false,
                         R->score(), nullptr, &T);
        F.temp = T.block;
        return rc;
    });
}

acx_scores_t *host_scores(int device, uint64_t rows) {
    acx_scores_t *R = new_result<acx_scores_t>(device, false);
    if (!R) return nullptr;
    R->rows = rows;
    if (R->alloc() != ACX_OK) { free_result(R); return nullptr; }
    R->score()[0] = 0;
    return R;
}

} // namespace

extern "C" {

int acx_score_host(const acx_match_t *m, uint64_t n_m, const uint64_t *counts, uint64_t n_hay, const int32_t *weights,
                   uint64_t n_weights, int64_t *scores) {
    if ((n_m && !m) || (n_weights && !weights) || (n_hay && !scores)) return fail(ACX_EINVAL, "null argument");
    if (!counts && n_hay > 1) return fail(ACX_EINVAL, "several haystacks need counts");
    if (int rc = counts_sum_to(counts, n_hay, n_m)) return rc;
    uint64_t at = 0;
    for (uint64_t h = 0; h < n_hay; h++) {
        const uint64_t end = counts ? at + counts[h] : n_m;
        uint64_t s = 0; // (unsigned: the sum wraps modulo 2^64)
        for (; at < end; at++)
            if (m[at].pattern < n_weights) s += (uint64_t)(int64_t)weights[m[at].pattern];
        scores[h] = (int64_t)s;
    }
    return ACX_OK;
}

int acx_score(acx_automaton_t *a, const uint8_t *hay, uint64_t len, const uint64_t *offsets, uint64_t n_hay, int overlapping,
              const int32_t *weights, uint64_t n_weights, acx_scores_t **out) {
    if (!a || !out) return fail(ACX_EINVAL, "null argument");
    *out = nullptr;
    int rc = check_weights(a, weights, n_weights);
    if (rc == ACX_OK && overlapping) rc = check_overlapping(a); // (the error, no device state)
    if (rc != ACX_OK) return rc;
    HostBatch B;
    if ((rc = host_batch(hay, &len, offsets, &n_hay, &B)) != ACX_OK) return rc;
    if (len <= score_host_max() || !n_hay) {
        // host route: acx_find_batch as it is (the small-call kernel, the in-place read, the staged pipeline), then the sums here
        HostFind f;
        if ((rc = f.find(a, B.hay, len, B.rel.data(), n_hay, overlapping, 0, n_hay != 0)) != ACX_OK) return rc;
        acx_scores_t *R = host_scores(a->device, n_hay);
        if (!R) return fail(ACX_ENOMEM, "out of memory");
        if (n_hay) rc = acx_score_host(f.m, f.nm, f.counts.data(), n_hay, weights, n_weights, R->score());
        if (rc != ACX_OK) { free_result(R); return rc; }
        *out = R;
        return ACX_OK;
    }
    // device route: staged, searched and scored under one lease; 8 bytes per row come back
    acx_scores_t *D = nullptr;
    rc = staged_call(a, B, len, n_hay, true, [&](Ctx *c, const uint8_t *d_search, const Segments &G) {
        const int run = run_score(a, c, d_search, len, G, overlapping, weights, n_weights, &D);
        return run == ACX_OK ? D->wait() : run; // (the staging buffers are the context's: the lease ends behind the kernels)
    });
    return copy_down(rc, D, rc == ACX_OK ? host_scores(a->device, D->rows) : nullptr, D ? D->rows * 8 : 0,
                     "copying the scores to the host", out);
}

int acx_score_device(acx_automaton_t *a, const void *d_hay, uint64_t len, const uint64_t *d_offsets, uint64_t n_hay,
                     uint64_t uniform_len, int overlapping, const int32_t *weights, uint64_t n_weights, acx_scores_t **out) {
    if (!a || !out) return fail(ACX_EINVAL, "null argument");
    *out = nullptr;
    int rc = check_weights(a, weights, n_weights);
    if (rc != ACX_OK) return rc;
    return device_call(a, d_hay, len, d_offsets, n_hay, uniform_len, overlapping, [&](Ctx *c, const uint8_t *d_search, const Segments &G) {
        return run_score(a, c, d_search, len, G, overlapping, weights, n_weights, out);
    });
}

int acx_score_rows_device(const acx_match_t *d_records, uint64_t n, const uint64_t *d_counts, uint64_t n_hay,
                          const int32_t *d_weights, uint64_t n_weights, int64_t *d_scores) {
    if (!n_hay) return n ? fail(ACX_EINVAL, "the counts do not sum to the number of records") : ACX_OK;
    if (!d_scores || !d_counts || (n && !d_records) || (n_weights && !d_weights)) return fail(ACX_EINVAL, "null argument");
    if (((uintptr_t)d_records | (uintptr_t)d_counts | (uintptr_t)d_scores) & 7)
        return fail(ACX_EINVAL, "records, counts and scores must be 8-byte aligned");
    if ((uintptr_t)d_weights & 3) return fail(ACX_EINVAL, "the weights must be 4-byte aligned");
    return rows_call(d_scores, [&](int device, void **t1, void **) {
        ScoreTemps T;
        const int rc = score_stage(device, nullptr, d_records, n, d_counts, n_hay, nullptr, d_weights, n_weights, true, d_scores, nullptr, &T);
        *t1 = T.block;
        return rc;
    });
}

uint64_t acx_scores_rows(const acx_scores_t *s) { return s ? s->rows : 0; }
int acx_scores_on_device(const acx_scores_t *s) { return s ? s->on_device : 0; }

const int64_t *acx_scores_data(const acx_scores_t *s) { return (const int64_t *)part_ptr(s, 0, 1); }
int acx_scores_copy(const acx_scores_t *s, int64_t *host_dst) { return part_copy(s, 0, 1, host_dst, "null argument"); }

void acx_free_scores(acx_scores_t *s) { free_result(s); }

} // extern "C"
