// columns_api.cpp -- a find's matches as columns (columns.hpp): the host split, the device route behind the find pipeline,
// the acx_find_columns* entry points and the accessors of their result.
#include "columns.hpp"
#include "find_pipeline.hpp"
#include "replace.hpp"

using namespace acxh;

// acx_find_columns / acx_find_columns_device: three columns of `n` words and, for a batch, rows + 1 row offsets, in ONE
// block.  Device route: a block of the buffer cache (g_bufs, workspace.cpp), written by kernels that may still run when the
// call returns (done); the find's records have gone back to the cache behind the same kernels, only the columns and the
// scan's scratch are kept until acx_free_columns.  Host route: a block of host memory.
struct ACX_HIDDEN acx_columns {
    int device = 0;
    int on_device = 0;
    bool batch = false;
    uint64_t n = 0, rows = 0;
    int64_t *col[4] = {nullptr, nullptr, nullptr, nullptr}; // ACX_COL_*; [3]: null in the single form
    int64_t *h_block = nullptr;
    void *d_block = nullptr;
    hipEvent_t done = nullptr;
    std::vector<void *> scratch;
};

namespace {

// where the parts of a block begin, in words: every part at least one word long (a column of no matches still has an
// address that DLPack consumers accept) and a multiple of 32 words (256 bytes) behind the previous one
struct Layout {
    uint64_t at[4], words;
    Layout(uint64_t n, uint64_t rows, bool batch) {
        const uint64_t c = (std::max<uint64_t>(n, 1) + 31) / 32 * 32;
        for (int k = 0; k < 4; k++) at[k] = (uint64_t)k * c;
        words = 3 * c + (batch ? (rows + 1 + 31) / 32 * 32 : 0);
    }
};

// The device route: the find pipeline as acx_find_device runs it (byte ranges, batch splits and the expansion of copies
// included), then the split -- and, for a batch, the scan of the counts -- on the same stream.  Returns when the number of
// matches is known; the kernels may still run (out->done).  d_hay, and G.offsets, must stay valid until then.
int run_columns(acx_automaton *a, Ctx *x, const uint8_t *d_hay, uint64_t len, const Segments &G, int overlapping,
                int codepoints, acx_columns **out) {
    *out = nullptr;
    const bool segmented = G.uniform_len != 0 || G.offsets != nullptr;
    acx_result *r = nullptr;
    if (!(segmented && G.n_hay == 0)) { // (an empty batch: nothing to search, one row offset)
        int rc = run_find(a, x, d_hay, len, G, overlapping, codepoints, &r);
        if (rc != ACX_OK) return rc;
    }
    acx_columns *R = new (std::nothrow) acx_columns();
    if (!R) { acx_free_result(r); return fail(ACX_ENOMEM, "out of memory"); }
    hipStream_t st = x->stream;
    R->device = a->device;
    R->on_device = 1;
    R->batch = segmented;
    R->rows = segmented ? G.n_hay : 0;
    R->n = r ? r->n : 0;
    const Layout L(R->n, R->rows, R->batch);
    auto body = [&]() -> int {
        HIPCHK(g_bufs.get(&R->d_block, L.words * 8, a->device));
        for (int k = 0; k < 3 + (R->batch ? 1 : 0); k++) R->col[k] = (int64_t *)R->d_block + L.at[k];
        if (r) HIPCHK(acx::col_split(r->d_matches, R->n, R->col[0], R->col[1], R->col[2], st));
        if (R->batch && R->rows) { // where every haystack's records begin, from the counts
            uint64_t *temp = nullptr;
            HIPCHK(g_bufs.get((void **)&temp, std::max<uint64_t>(replace_scan_words(R->rows) * 8, 16), a->device));
            R->scratch.push_back(temp);
            HIPCHK(acx::replace_scan(nullptr, nullptr, r->d_counts, R->rows, R->col[3], temp, st));
        } else if (R->batch) {
            HIPCHK(hipMemsetAsync(R->col[3], 0, 8, st));
        }
        // The find's records and counts are not needed beyond this point of the stream: they go back to the buffer cache,
        // which holds them until an event recorded HERE has fired (the result's own event lies in front of the split).
        hipEvent_t freed = g_events.get(a->device);
        R->done = g_events.get(a->device);
        if (!freed || !R->done) {
            HIPCHK(hipStreamSynchronize(st));
            g_events.put(a->device, freed);
            g_events.put(a->device, R->done);
            freed = R->done = nullptr;
        } else {
            HIPCHK(hipEventRecord(freed, st));
            HIPCHK(hipEventRecord(R->done, st));
        }
        if (r) {
            g_events.put(a->device, r->done);
            r->done = nullptr;
            g_bufs.put(r->borrowed ? nullptr : r->d_matches, a->device, freed, r->d_counts);
            r->d_matches = nullptr;
            r->d_counts = nullptr;
        } else {
            g_events.put(a->device, freed);
        }
        return ACX_OK;
    };
    int rc = body();
    if (rc != ACX_OK) (void)hipStreamSynchronize(st);
    acx_free_result(r); // (emptied above when all went well)
    if (rc != ACX_OK) { acx_free_columns(R); return rc; }
    *out = R;
    return ACX_OK;
}

// every accessor's wait for the split (and the scan)
int columns_wait(const acx_columns *c) {
    if (!c->on_device || !c->done) return ACX_OK;
    DeviceScope ds(c->device);
    HIPCHK(hipEventSynchronize(c->done));
    return ACX_OK;
}

uint64_t part_words(const acx_columns *c, int which) { return which == ACX_COL_ROW_OFFSETS ? c->rows + 1 : c->n; }

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
    hipPointerAttribute_t at;
    HIPCHK(hipPointerGetAttributes(&at, d_m));
    DeviceScope ds(at.device);
    HIPCHK(acx::col_split(d_m, n, d_pattern, d_start, d_end, nullptr));
    HIPCHK(hipStreamSynchronize(nullptr));
    return ACX_OK;
}

int acx_find_columns(acx_automaton_t *a, const uint8_t *hay, uint64_t len, const uint64_t *offsets, uint64_t n_hay,
                     int overlapping, int codepoints, acx_columns_t **out) {
    if (!a || !out) return fail(ACX_EINVAL, "null argument");
    *out = nullptr;
    // the find entry points as they are (K0, the resident K0, the in-place read, the staged pipeline), each under its lease
    acx_match_t *m = nullptr;
    uint64_t nm = 0;
    std::vector<uint64_t> counts;
    int rc;
    if (offsets) {
        try { counts.assign(n_hay, 0); } catch (...) { return fail(ACX_ENOMEM, "out of memory"); }
        rc = acx_find_batch(a, hay, offsets, n_hay, overlapping, codepoints, &m, &nm, counts.data());
    } else {
        rc = acx_find(a, hay, len, overlapping, codepoints, &m, &nm);
    }
    if (rc != ACX_OK) return rc;
    acx_columns *R = new (std::nothrow) acx_columns();
    const Layout L(nm, offsets ? n_hay : 0, offsets != nullptr);
    if (R) R->h_block = new (std::nothrow) int64_t[L.words];
    if (!R || !R->h_block) { acx_free_matches(m); delete R; return fail(ACX_ENOMEM, "out of memory"); }
    R->device = a->device;
    R->batch = offsets != nullptr;
    R->rows = R->batch ? n_hay : 0;
    R->n = nm;
    for (int k = 0; k < 3 + (R->batch ? 1 : 0); k++) R->col[k] = R->h_block + L.at[k];
    for (int k = 0; k < 3; k++) R->col[k][0] = 0; // (the one word of an empty column)
    rc = acx_split_host(m, nm, R->col[0], R->col[1], R->col[2]);
    acx_free_matches(m);
    if (R->batch) {
        int64_t at = 0;
        for (uint64_t h = 0; h < n_hay; h++) { R->col[3][h] = at; at += (int64_t)counts[h]; }
        R->col[3][n_hay] = at;
    }
    if (rc != ACX_OK) { acx_free_columns(R); return rc; }
    *out = R;
    return ACX_OK;
}

int acx_find_columns_device(acx_automaton_t *a, const void *d_hay, uint64_t len, const uint64_t *d_offsets, uint64_t n_hay,
                            uint64_t uniform_len, int overlapping, int codepoints, acx_columns_t **out) {
    if (!a || !out) return fail(ACX_EINVAL, "null argument");
    *out = nullptr;
    if (len && !d_hay) return fail(ACX_EINVAL, "null haystack");
    Segments G;
    int rc = make_segments(d_offsets, n_hay, uniform_len, len, &G);
    if (rc == ACX_OK && overlapping) rc = check_overlapping(a); // (the error, no device state)
    if (rc != ACX_OK) return rc;
    Lease lease(a);
    if (!lease.c) return fail(ACX_EDEVICE, "could not create a stream for the call");
    const uint8_t *d_search = nullptr;
    rc = fold_copy(a, lease.c, (const uint8_t *)d_hay, len, &d_search);
    if (rc != ACX_OK) return rc;
    return run_columns(a, lease.c, d_search, len, G, overlapping, codepoints, out);
}

uint64_t acx_columns_count(const acx_columns_t *c) { return c ? c->n : 0; }
uint64_t acx_columns_rows(const acx_columns_t *c) { return c ? c->rows : 0; }
int acx_columns_on_device(const acx_columns_t *c) { return c ? c->on_device : 0; }

const int64_t *acx_columns_data(const acx_columns_t *c, int which) {
    if (!c || which < 0 || which > ACX_COL_ROW_OFFSETS || !c->col[which]) return nullptr;
    if (columns_wait(c) != ACX_OK) return nullptr;
    return c->col[which];
}

int acx_columns_copy(const acx_columns_t *c, int which, int64_t *host_dst) {
    if (!c || which < 0 || which > ACX_COL_ROW_OFFSETS) return fail(ACX_EINVAL, "no such column");
    if (!c->col[which]) return fail(ACX_EINVAL, "the single form has no row offsets");
    const uint64_t words = part_words(c, which);
    if (!words) return ACX_OK;
    if (!host_dst) return fail(ACX_EINVAL, "null argument");
    if (!c->on_device) { std::memcpy(host_dst, c->col[which], words * 8); return ACX_OK; }
    int rc = columns_wait(c);
    if (rc != ACX_OK) return rc;
    DeviceScope ds(c->device);
    HIPCHK(hipMemcpy(host_dst, c->col[which], words * 8, hipMemcpyDeviceToHost));
    return ACX_OK;
}

void acx_free_columns(acx_columns_t *c) {
    if (!c) return;
    if (c->on_device) {
        DeviceScope ds(c->device);
        // (the kernels write the columns and read the scratch: nothing goes back to the pool before they are done)
        if (c->done) (void)hipEventSynchronize(c->done);
        for (void *p : c->scratch) g_bufs.put(p, c->device);
        g_bufs.put(c->d_block, c->device);
        g_events.put(c->device, c->done);
    }
    delete[] c->h_block;
    delete c;
}

} // extern "C"
