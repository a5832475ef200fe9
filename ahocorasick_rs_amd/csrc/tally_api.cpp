// tally_api.cpp -- per-haystack pattern counts as a CSR matrix (tally.hpp): the host reduction, the device stage behind the
// find pipeline, the acx_tally* entry points and the accessors of their result.
#include "replace.hpp"
#include "result_block.hpp"
#include "tally.hpp"

using namespace acxh;

// acx_tally / acx_tally_device: row offsets (rows + 1 words), patterns and counts (nnz words each) in ONE block
// (result_block.hpp).  Device route: the find's records and the stage's temporaries have gone back to the cache behind the
// stage's kernels.
struct ACX_HIDDEN acx_tally : ResultBlock {
    uint64_t rows = 0, nnz = 0;

    // the block (by on_device) and its parts, ACX_TALLY_*, with room for nnz_room entries
    int alloc(uint64_t nnz_room) { return alloc_parts({(rows + 1) * 8, nnz_room * 8, nnz_room * 8}); }
    // ... of which nnz count, known only now (the host route gives every record room)
    void set_nnz(uint64_t k) {
        nnz = k;
        resize_part(ACX_TALLY_PATTERN, k * 8);
        resize_part(ACX_TALLY_COUNT, k * 8);
    }
    int64_t *words(int which) const { return at<int64_t>(which); }
};

namespace {

constexpr int N_PARTS = ACX_TALLY_COUNT + 1;

// ACX_TALLY_HOST_MAX (bytes, read per call): batches up to this size reduce on the host, behind acx_find_batch.  The
// default is ACX_SUMMARY_HOST_MAX's, which is itself not a measured crossover.
uint64_t tally_host_max() {
    const char *e = std::getenv("ACX_TALLY_HOST_MAX");
    return e ? std::strtoull(e, nullptr, 10) : (1ull << 20);
}

// ACX_TALLY_ROW_MAX (records, read per call): rows longer than this take the radix-sort form.  It only ever lowers
// acx::TALLY_ROW_MAX; 0 sends every row that way (the tests' seam for that form at small sizes, and the baseline the tile
// kernel is measured against).
uint32_t tally_row_max() {
    const char *e = std::getenv("ACX_TALLY_ROW_MAX");
    if (!e || !*e) return acx::TALLY_ROW_MAX;
    return (uint32_t)std::min<uint64_t>(std::strtoull(e, nullptr, 10), acx::TALLY_ROW_MAX);
}

// The temporaries of one run of the device stage: one block of the buffer cache (and a second one when there are long rows).
struct Stage {
    int device = 0;
    void *block = nullptr, *long_block = nullptr;
    int64_t *rec_off = nullptr, *roff = nullptr, *tmp_pattern = nullptr, *tmp_count = nullptr;
    uint64_t *nnz_row = nullptr, *scan_tmp = nullptr;
    uint64_t n = 0, rows = 0;
};

// The stage up to the point where nnz is known: the scans, the tile kernel, the long rows' form when there are any.
// S->roff then holds the row offsets (rows + 1 words); d_m: n records, d_counts: rows words (rows > 0; check_sum:
// record_offsets).
int stage_count(int device, hipStream_t st, const acx_match_t *d_m, uint64_t n, const uint64_t *d_counts, uint64_t rows,
                uint64_t n_patterns, bool check_sum, Stage *S, uint64_t *nnz) {
    S->device = device;
    S->n = n;
    S->rows = rows;
    *nnz = 0;
    const uint32_t row_max = tally_row_max();
    // [rec_off: rows + 1][roff: rows + 1, then the long rows' records: 1][nnz_row: rows][scan][tmp_pattern: n][tmp_count: n]
    Carver C;
    const uint64_t o_rec = C.part(rows + 1), o_roff = C.part(rows + 2), o_nnz = C.part(rows),
                   o_scan = C.part(replace_scan_words(rows)), o_tp = C.part(n), o_tc = C.part(n);
    HIPCHK(g_bufs.get(&S->block, C.bytes(), device));
    uint64_t *b = (uint64_t *)S->block;
    S->rec_off = (int64_t *)(b + o_rec);
    S->roff = (int64_t *)(b + o_roff);
    S->nnz_row = b + o_nnz;
    S->scan_tmp = b + o_scan;
    S->tmp_pattern = (int64_t *)(b + o_tp);
    S->tmp_count = (int64_t *)(b + o_tc);
    uint64_t *n_long = (uint64_t *)S->roff + rows + 1; // (behind the scan's last entry: one readback brings both)
    if (int rc = record_offsets(d_counts, rows, n, check_sum, S->rec_off, S->scan_tmp, st)) return rc;
    if (!n) { // every row is empty
        HIPCHK(hipMemsetAsync(S->roff, 0, (rows + 1) * 8, st));
        return ACX_OK;
    }
    HIPCHK(hipMemsetAsync(S->nnz_row, 0, rows * 8, st));
    HIPCHK(hipMemsetAsync(n_long, 0, 8, st));
    HIPCHK(acx::tally_tiles(d_m, n, S->rec_off, rows, n_patterns, row_max, S->tmp_pattern, S->tmp_count, S->nnz_row, n_long, st));
    HIPCHK(acx::replace_scan(nullptr, nullptr, S->nnz_row, rows, S->roff, S->scan_tmp, st));
    uint64_t back[2] = {0, 0}; // nnz (of the short rows, until the long ones are in), the long rows' records
    HIPCHK(hipMemcpyAsync(back, S->roff + rows, 16, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (back[1]) {
        if (back[1] > n) return fail(ACX_EDEVICE, "the tile kernel counted more long-row records than there are records");
        HIPCHK(g_bufs.get(&S->long_block, acx::tally_long_words(rows, back[1], row_max) * 8, device));
        HIPCHK(acx::tally_long(d_m, S->rec_off, rows, row_max, back[1], (uint64_t *)S->long_block, S->tmp_pattern, S->tmp_count,
                               S->nnz_row, st));
        HIPCHK(acx::replace_scan(nullptr, nullptr, S->nnz_row, rows, S->roff, S->scan_tmp, st));
        HIPCHK(hipMemcpyAsync(back, S->roff + rows, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    if (back[0] > n) return fail(ACX_EDEVICE, "more runs than records");
    *nnz = back[0];
    return ACX_OK;
}

// ... and from there: the row offsets and the compact columns into their places (device memory, 8-byte aligned)
int stage_finish(const Stage *S, uint64_t nnz, int64_t *row_offsets, int64_t *pattern, int64_t *count, hipStream_t st) {
    HIPCHK(hipMemcpyAsync(row_offsets, S->roff, (S->rows + 1) * 8, hipMemcpyDeviceToDevice, st));
    HIPCHK(acx::tally_compact(S->roff, S->rows, S->rec_off, nnz, S->tmp_pattern, S->tmp_count, pattern, count, st));
    return ACX_OK;
}

// The device route: the find pipeline as acx_find_device runs it (batch splits and the expansion of copies included, byte
// offsets: no offset is reported), then the stage on the same stream.  Returns when nnz is known; tally_compact may still
// run (out->done).  d_hay, and G.offsets, must stay valid until then.
int run_tally(acx_automaton *a, Ctx *x, const uint8_t *d_hay, uint64_t len, const Segments &G, int overlapping, acx_tally_t **out) {
    const uint64_t rows = rows_of(G).n;
    // (an empty batch: nothing to search, one row offset)
    return find_stage(a, x, d_hay, len, G, overlapping, 0, rows != 0, out, [&](FindStage<acx_tally_t> &F) -> int {
        acx_tally_t *R = F.R;
        R->rows = rows;
        int rc;
        Stage S;
        if (rows) {
            const uint64_t *d_counts = nullptr;
            if ((rc = F.counts(&d_counts)) != ACX_OK) return rc;
            rc = stage_count(a->device, F.st, F.r->d_matches, F.r->n, d_counts, rows, a->host.n_patterns, false, &S, &R->nnz);
            F.temp = S.block;
            F.keep(S.long_block); // (the rare form: kept until acx_free_tally)
            if (rc != ACX_OK) return rc;
        }
        if ((rc = R->alloc(R->nnz)) != ACX_OK) return rc;
        if (rows) return stage_finish(&S, R->nnz, R->words(0), R->words(1), R->words(2), F.st);
        HIPCHK(hipMemsetAsync(R->words(0), 0, 8, F.st));
        return ACX_OK;
    });
}

acx_tally_t *host_tally(int device, uint64_t rows, uint64_t nnz_room) {
    acx_tally_t *R = new_result<acx_tally_t>(device, false);
    if (!R) return nullptr;
    R->rows = rows;
    if (R->alloc(nnz_room) != ACX_OK) { free_result(R); return nullptr; }
    for (int k = 0; k < 3; k++) R->words(k)[0] = 0;
    return R;
}

} // namespace

extern "C" {

int acx_tally_host(const acx_match_t *m, uint64_t n_m, const uint64_t *counts, uint64_t n_hay, int64_t *row_offsets,
                   int64_t *pattern, int64_t *count, uint64_t *nnz) {
    if (!row_offsets || !nnz || (n_m && (!m || !pattern || !count)) || (n_hay && !counts)) return fail(ACX_EINVAL, "null argument");
    if (int rc = counts_sum_to(counts, n_hay, n_m)) return rc;
    std::vector<uint64_t> row;
    uint64_t at = 0, w = 0;
    try {
        for (uint64_t h = 0; h < n_hay; h++) {
            row_offsets[h] = (int64_t)w;
            row.resize(counts[h]);
            for (uint64_t i = 0; i < counts[h]; i++) row[i] = m[at + i].pattern;
            at += counts[h];
            std::sort(row.begin(), row.end());
            for (uint64_t i = 0; i < row.size();) {
                uint64_t j = i + 1;
                while (j < row.size() && row[j] == row[i]) j++;
                pattern[w] = (int64_t)row[i];
                count[w] = (int64_t)(j - i);
                w++;
                i = j;
            }
        }
    } catch (...) { return fail(ACX_ENOMEM, "out of memory"); }
    row_offsets[n_hay] = (int64_t)w;
    *nnz = w;
    return ACX_OK;
}

int acx_tally(acx_automaton_t *a, const uint8_t *hay, uint64_t len, const uint64_t *offsets, uint64_t n_hay, int overlapping,
              acx_tally_t **out) {
    if (!a || !out) return fail(ACX_EINVAL, "null argument");
    *out = nullptr;
    int rc = overlapping ? check_overlapping(a) : ACX_OK; // (the error, no device state)
    if (rc != ACX_OK) return rc;
    HostBatch B;
    if ((rc = host_batch(hay, &len, offsets, &n_hay, &B)) != ACX_OK) return rc;
    if (len <= tally_host_max() || !n_hay) {
        // host route: acx_find_batch as it is (the small-call kernel, the in-place read, the staged pipeline), then the
        // reduction here
        HostFind f;
        if ((rc = f.find(a, B.hay, len, B.rel.data(), n_hay, overlapping, 0, n_hay != 0)) != ACX_OK) return rc;
        acx_tally_t *R = host_tally(a->device, n_hay, f.nm);
        if (!R) return fail(ACX_ENOMEM, "out of memory");
        uint64_t nnz = 0;
        rc = acx_tally_host(f.m, f.nm, f.counts.data(), n_hay, R->words(0), R->words(1), R->words(2), &nnz);
        if (rc != ACX_OK) { free_result(R); return rc; }
        R->set_nnz(nnz);
        *out = R;
        return ACX_OK;
    }
    // device route: staged, searched and reduced under one lease; the compact block comes back in one copy
    acx_tally_t *D = nullptr;
    rc = staged_call(a, B, len, n_hay, true, [&](Ctx *c, const uint8_t *d_search, const Segments &G) {
        const int run = run_tally(a, c, d_search, len, G, overlapping, &D);
        return run == ACX_OK ? D->wait() : run; // (the staging buffers are the context's: the lease ends behind the kernels)
    });
    acx_tally_t *R = rc == ACX_OK ? host_tally(a->device, D->rows, D->nnz) : nullptr;
    if (R) R->nnz = D->nnz;
    return copy_down(rc, D, R, D ? D->block_bytes : 0, "copying the tally to the host", out); // (the twins' blocks are one size)
}

int acx_tally_device(acx_automaton_t *a, const void *d_hay, uint64_t len, const uint64_t *d_offsets, uint64_t n_hay,
                     uint64_t uniform_len, int overlapping, acx_tally_t **out) {
    if (!a || !out) return fail(ACX_EINVAL, "null argument");
    *out = nullptr;
    return device_call(a, d_hay, len, d_offsets, n_hay, uniform_len, overlapping, [&](Ctx *c, const uint8_t *d_search, const Segments &G) {
        return run_tally(a, c, d_search, len, G, overlapping, out);
    });
}

int acx_tally_rows_device(const acx_match_t *d_records, uint64_t n, const uint64_t *d_counts, uint64_t n_hay, uint64_t n_patterns,
                          int64_t *d_row_offsets, int64_t *d_pattern, int64_t *d_count, uint64_t *nnz) {
    if (!d_row_offsets || !nnz) return fail(ACX_EINVAL, "null argument");
    *nnz = 0;
    if ((n && (!d_records || !d_pattern || !d_count)) || (n_hay && !d_counts)) return fail(ACX_EINVAL, "null argument");
    if (((uintptr_t)d_records | (uintptr_t)d_counts | (uintptr_t)d_row_offsets | (uintptr_t)d_pattern | (uintptr_t)d_count) & 7)
        return fail(ACX_EINVAL, "records, counts and outputs must be 8-byte aligned");
    if (n_patterns > (1ull << acx::TALLY_PATTERN_BITS)) return fail(ACX_EINVAL, "more than 2^24 patterns");
    if (n && !n_hay) return fail(ACX_EINVAL, "the counts do not sum to the number of records");
    return rows_call(d_row_offsets, [&](int device, void **t1, void **t2) -> int {
        if (!n_hay) { // (no row: the one offset)
            HIPCHK(hipMemsetAsync(d_row_offsets, 0, 8, nullptr));
            return ACX_OK;
        }
        Stage S;
        int rc = stage_count(device, nullptr, d_records, n, d_counts, n_hay, n_patterns, true, &S, nnz);
        if (rc == ACX_OK) rc = stage_finish(&S, *nnz, d_row_offsets, d_pattern, d_count, nullptr);
        *t1 = S.block;
        *t2 = S.long_block;
        return rc;
    });
}

uint64_t acx_tally_nnz(const acx_tally_t *t) { return t ? t->nnz : 0; }
uint64_t acx_tally_rows(const acx_tally_t *t) { return t ? t->rows : 0; }
int acx_tally_on_device(const acx_tally_t *t) { return t ? t->on_device : 0; }

const int64_t *acx_tally_data(const acx_tally_t *t, int which) { return (const int64_t *)part_ptr(t, which, N_PARTS); }
int acx_tally_copy(const acx_tally_t *t, int which, int64_t *host_dst) { return part_copy(t, which, N_PARTS, host_dst, "no such part"); }

void acx_free_tally(acx_tally_t *t) { free_result(t); }

} // extern "C"
