// filter_api.cpp -- keep or drop the rows of a batch by match (filter.hpp): the host form, the device stage behind the find
// pipeline, the acx_filter* entry points and the accessors of their result.
#include "filter.hpp"
#include "find_pipeline.hpp"
#include "replace.hpp"

using namespace acxh;

// acx_filter / acx_filter_device: the kept rows' source indexes (k words), their offsets (k + 1 words) and their bytes in ONE
// block.  Device route: a block of the buffer cache (g_bufs, workspace.cpp), written by kernels that may still run when the
// call returns (done); the find's records and counts and the stage's temporaries have gone back to the cache behind the
// same kernels.  Host route: a block of host memory.
struct ACX_HIDDEN acx_filtered {
    int device = 0;
    int on_device = 0;
    uint64_t n_src = 0, rows = 0, bytes = 0;
    uint8_t *part[3] = {nullptr, nullptr, nullptr}; // ACX_FILT_*
    uint8_t *h_block = nullptr;
    void *d_block = nullptr;
    hipEvent_t done = nullptr;
};

namespace {

// where the parts of a block begin, in bytes: every part at least one word long (an empty part still has an address that
// DLPack consumers accept) and a multiple of 256 bytes behind the previous one (the rules of the columns' block,
// columns_api.cpp); the data part rounded up to 16 bytes for the tile's stores
struct Layout {
    uint64_t at[3], bytes;
    Layout(uint64_t k, uint64_t total) {
        const uint64_t r = (std::max<uint64_t>(k, 1) * 8 + 255) / 256 * 256, o = ((k + 1) * 8 + 255) / 256 * 256;
        at[ACX_FILT_ROWS] = 0;
        at[ACX_FILT_OFFSETS] = r;
        at[ACX_FILT_DATA] = r + o;
        bytes = r + o + std::max<uint64_t>((total + 15) / 16 * 16, 16);
    }
};

uint64_t part_bytes(const acx_filtered_t *f, int which) {
    return which == ACX_FILT_ROWS ? f->rows * 8 : which == ACX_FILT_OFFSETS ? (f->rows + 1) * 8 : f->bytes;
}

// The temporaries of one run of the device stage: one block of the buffer cache.
struct Stage {
    void *block = nullptr;
    uint64_t *klen = nullptr, *kflag = nullptr, *scan_tmp = nullptr, *src = nullptr, *tiles = nullptr;
    int64_t *A = nullptr, *B = nullptr;
    acx::FilterRows R{nullptr, 0, 0, 0};
};

// The stage up to the point where the result's size is known: the flags and the two scans (n > 0).  d_counts: n words.
int stage_sizes(int device, hipStream_t st, const acx::FilterRows &R, const uint64_t *d_counts, uint64_t min_matches,
                bool keep_matched, Stage *S, uint64_t *k, uint64_t *total) {
    S->R = R;
    const uint64_t n = R.n;
    // [klen: n][kflag: n][A: n + 1][B: n + 1][scan][src: n][tiles], every part 256-byte aligned
    uint64_t at = 0;
    auto part = [&](uint64_t w) { const uint64_t here = at; at += (w + 31) / 32 * 32; return here; };
    const uint64_t o_len = part(n), o_flag = part(n), o_a = part(n + 1), o_b = part(n + 1), o_scan = part(replace_scan_words(n)),
                   o_src = part(n), o_tiles = part(acx::filter_tile_words(R.len));
    HIPCHK(g_bufs.get(&S->block, std::max<uint64_t>(at, 32) * 8, device));
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

int check_args(uint64_t min_matches, uint32_t flags) {
    if (flags & ~(uint32_t)ACX_FILTER_KEEP_MATCHED) return fail(ACX_EINVAL, "unknown filter flags");
    if (!min_matches) return fail(ACX_EINVAL, "min_matches must be at least 1");
    return ACX_OK;
}

// The device route: the find pipeline as acx_find_device runs it (batch splits and the expansion of copies included, byte
// offsets: no offset is reported) on d_search, then the stage on the same stream over d_hay -- the caller's own bytes.
// Returns when the result's size is known; the gather may still run (out->done).  d_hay, d_search and G.offsets must stay
// valid until then.
int run_filter(acx_automaton *a, Ctx *x, const uint8_t *d_hay, const uint8_t *d_search, uint64_t len, const Segments &G,
               int overlapping, uint64_t min_matches, uint32_t flags, acx_filtered_t **out) {
    *out = nullptr;
    const bool segmented = G.uniform_len != 0 || G.offsets != nullptr;
    const uint64_t n = segmented ? G.n_hay : 1;
    acx_result *r = nullptr;
    if (n) { // (an empty batch: nothing to search, one offset)
        int rc = run_find(a, x, d_search, len, G, overlapping, 0, &r);
        if (rc != ACX_OK) return rc;
    }
    acx_filtered_t *R = new (std::nothrow) acx_filtered_t();
    if (!R) { acx_free_result(r); return fail(ACX_ENOMEM, "out of memory"); }
    hipStream_t st = x->stream;
    R->device = a->device;
    R->on_device = 1;
    R->n_src = n;
    Stage S;
    uint64_t *one_count = nullptr; // (one haystack that is no batch: the find kept no counts)
    auto body = [&]() -> int {
        uint64_t k = 0, total = 0;
        if (n) {
            const uint64_t *d_counts = r->d_counts;
            if (!d_counts) {
                HIPCHK(g_bufs.get((void **)&one_count, 16, a->device));
                HIPCHK(hipMemcpyAsync(one_count, &r->n, 8, hipMemcpyHostToDevice, st));
                d_counts = one_count;
            }
            const acx::FilterRows rows{G.offsets, G.uniform_len, n, len};
            int rc = stage_sizes(a->device, st, rows, d_counts, min_matches, (flags & ACX_FILTER_KEEP_MATCHED) != 0, &S, &k, &total);
            if (rc != ACX_OK) return rc;
        }
        R->rows = k;
        R->bytes = total;
        const Layout L(k, total);
        HIPCHK(g_bufs.get(&R->d_block, L.bytes, a->device));
        for (int p = 0; p < 3; p++) R->part[p] = (uint8_t *)R->d_block + L.at[p];
        int rc = stage_finish(&S, d_hay, k, total, (int64_t *)R->part[0], (int64_t *)R->part[1], R->part[2], st);
        if (rc != ACX_OK) return rc;
        // The find's records and counts and the stage's temporaries are not needed beyond this point of the stream: they go
        // back to the buffer cache, which holds them until an event recorded HERE has fired.
        hipEvent_t freed = g_events.get(a->device), freed2 = g_events.get(a->device);
        R->done = g_events.get(a->device);
        if (!freed || !freed2 || !R->done) {
            HIPCHK(hipStreamSynchronize(st));
            g_events.put(a->device, freed);
            g_events.put(a->device, freed2);
            g_events.put(a->device, R->done);
            freed = freed2 = R->done = nullptr;
        } else {
            HIPCHK(hipEventRecord(freed, st));
            HIPCHK(hipEventRecord(freed2, st));
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
        g_bufs.put(S.block, a->device, freed2, one_count);
        S.block = nullptr;
        one_count = nullptr;
        return ACX_OK;
    };
    int rc = body();
    if (rc != ACX_OK) {
        (void)hipStreamSynchronize(st);
        g_bufs.put(S.block, a->device);
        g_bufs.put(one_count, a->device);
    }
    acx_free_result(r); // (emptied above when all went well)
    if (rc != ACX_OK) { acx_free_filtered(R); return rc; }
    *out = R;
    return ACX_OK;
}

// every accessor's wait for the stage's last kernel
int filtered_wait(const acx_filtered_t *f) {
    if (!f->on_device || !f->done) return ACX_OK;
    DeviceScope ds(f->device);
    HIPCHK(hipEventSynchronize(f->done));
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
    if (!offsets) {
        if (n_hay > 1) return fail(ACX_EINVAL, "several haystacks need offsets");
    } else {
        if (offsets[0] != 0 || offsets[n_hay] != len) return fail(ACX_EINVAL, "offsets must rise from 0 to the batch's length");
        for (uint64_t h = 0; h < n_hay; h++)
            if (offsets[h + 1] < offsets[h]) return fail(ACX_EINVAL, "offsets must rise from 0 to the batch's length");
    }
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
    uint64_t base = 0;
    if (offsets) {
        for (uint64_t i = 0; i < n_hay; i++)
            if (offsets[i + 1] < offsets[i]) return fail(ACX_EINVAL, "offsets not monotone");
        base = offsets[0];
        len = offsets[n_hay] - base;
    } else {
        n_hay = 1;
    }
    if (len && !hay) return fail(ACX_EINVAL, "null haystack");
    const uint8_t *h = len ? hay + base : nullptr;
    std::vector<uint64_t> rel, counts;
    try {
        rel.resize(n_hay + 1);
        counts.assign(n_hay + 1, 0);
    } catch (...) { return fail(ACX_ENOMEM, "out of memory"); }
    for (uint64_t i = 0; i <= n_hay; i++) rel[i] = offsets ? offsets[i] - base : (i ? len : 0);
    if (n_hay) { // the counts: the summary chooses its own route, 8 bytes per row come back
        acx_summary_t *s = nullptr;
        rc = acx_summarize(a, h, len, offsets ? rel.data() : nullptr, n_hay, overlapping, 0, 0, &s);
        if (rc == ACX_OK) rc = acx_summary_counts(s, counts.data());
        acx_free_summary(s);
        if (rc != ACX_OK) return rc;
    }
    // the gather: a memcpy per kept row from the caller's memory (the output never crosses the bus)
    uint64_t k = 0, total = 0;
    rc = acx_filter_host(h, len, rel.data(), n_hay, counts.data(), min_matches, flags, nullptr, nullptr, nullptr, &k, &total);
    if (rc != ACX_OK) return rc;
    acx_filtered_t *R = new (std::nothrow) acx_filtered_t();
    const Layout L(k, total);
    if (R) R->h_block = new (std::nothrow) uint8_t[L.bytes];
    if (!R || !R->h_block) { delete R; return fail(ACX_ENOMEM, "out of memory"); }
    R->device = a->device;
    R->n_src = n_hay;
    for (int p = 0; p < 3; p++) R->part[p] = R->h_block + L.at[p];
    rc = acx_filter_host(h, len, rel.data(), n_hay, counts.data(), min_matches, flags, (int64_t *)R->part[0], (int64_t *)R->part[1],
                         R->part[2], &R->rows, &R->bytes);
    if (rc != ACX_OK) { acx_free_filtered(R); return rc; }
    *out = R;
    return ACX_OK;
}

int acx_filter_device(acx_automaton_t *a, const void *d_hay, uint64_t len, const uint64_t *d_offsets, uint64_t n_hay,
                      uint64_t uniform_len, int overlapping, uint64_t min_matches, uint32_t flags, acx_filtered_t **out) {
    if (!a || !out) return fail(ACX_EINVAL, "null argument");
    *out = nullptr;
    int rc = check_args(min_matches, flags);
    if (rc != ACX_OK) return rc;
    if (len && !d_hay) return fail(ACX_EINVAL, "null haystack");
    Segments G;
    rc = make_segments(d_offsets, n_hay, uniform_len, len, &G);
    if (rc == ACX_OK && overlapping) rc = check_overlapping(a); // (the error, no device state)
    if (rc != ACX_OK) return rc;
    Lease lease(a);
    if (!lease.c) return fail(ACX_EDEVICE, "could not create a stream for the call");
    const uint8_t *d_search = nullptr; // (a case-insensitive handle: the folded copy is searched, the caller's bytes are copied)
    rc = fold_copy(a, lease.c, (const uint8_t *)d_hay, len, &d_search);
    if (rc != ACX_OK) return rc;
    return run_filter(a, lease.c, (const uint8_t *)d_hay, d_search, len, G, overlapping, min_matches, flags, out);
}

int acx_filter_rows_device(const void *d_hay, uint64_t len, const uint64_t *d_offsets, uint64_t n_hay, uint64_t uniform_len,
                           const uint64_t *d_counts, uint64_t min_matches, uint32_t flags, int64_t *d_rows,
                           int64_t *d_out_offsets, uint8_t *d_data, uint64_t *n_rows, uint64_t *n_bytes) {
    int rc = check_args(min_matches, flags);
    if (rc != ACX_OK) return rc;
    if (!d_out_offsets || !n_rows || !n_bytes) return fail(ACX_EINVAL, "null argument");
    *n_rows = *n_bytes = 0;
    if (d_offsets && uniform_len) return fail(ACX_EINVAL, "offsets and uniform_len exclude one another");
    if (!d_offsets && !uniform_len) n_hay = 1;
    if (uniform_len && n_hay * uniform_len != len) return fail(ACX_EINVAL, "n_hay * uniform_len is not the batch's length");
    if ((n_hay && (!d_counts || !d_rows)) || (len && (!d_hay || !d_data))) return fail(ACX_EINVAL, "null argument");
    if (((uintptr_t)d_offsets | (uintptr_t)d_counts | (uintptr_t)d_rows | (uintptr_t)d_out_offsets) & 7)
        return fail(ACX_EINVAL, "offsets, counts and the word outputs must be 8-byte aligned");
    if ((uintptr_t)d_data & 15) return fail(ACX_EINVAL, "the data output must be 16-byte aligned");
    hipPointerAttribute_t at;
    HIPCHK(hipPointerGetAttributes(&at, d_out_offsets));
    DeviceScope ds(at.device);
    if (!n_hay) {
        HIPCHK(hipMemsetAsync(d_out_offsets, 0, 8, nullptr));
        HIPCHK(hipStreamSynchronize(nullptr));
        return ACX_OK;
    }
    if (d_offsets) { // where the offsets begin and end; between the two they are the caller's word
        uint64_t ends[2] = {1, 0};
        HIPCHK(hipMemcpy(&ends[0], d_offsets, 8, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(&ends[1], d_offsets + n_hay, 8, hipMemcpyDeviceToHost));
        if (ends[0] != 0 || ends[1] != len) return fail(ACX_EINVAL, "offsets must rise from 0 to the batch's length");
    }
    Stage S;
    uint64_t k = 0, total = 0;
    const acx::FilterRows rows{d_offsets, uniform_len, n_hay, len};
    rc = stage_sizes(at.device, nullptr, rows, d_counts, min_matches, (flags & ACX_FILTER_KEEP_MATCHED) != 0, &S, &k, &total);
    if (rc == ACX_OK) rc = stage_finish(&S, (const uint8_t *)d_hay, k, total, d_rows, d_out_offsets, d_data, nullptr);
    const hipError_t e = hipStreamSynchronize(nullptr);
    g_bufs.put(S.block, at.device);
    if (rc == ACX_OK && e != hipSuccess) rc = hipfail(e, "hipStreamSynchronize");
    if (rc == ACX_OK) { *n_rows = k; *n_bytes = total; }
    return rc;
}

uint64_t acx_filtered_rows(const acx_filtered_t *f) { return f ? f->rows : 0; }
uint64_t acx_filtered_bytes(const acx_filtered_t *f) { return f ? f->bytes : 0; }
int acx_filtered_on_device(const acx_filtered_t *f) { return f ? f->on_device : 0; }

const void *acx_filtered_data(const acx_filtered_t *f, int which) {
    if (!f || which < 0 || which > ACX_FILT_DATA) return nullptr;
    if (filtered_wait(f) != ACX_OK) return nullptr;
    return f->part[which];
}

int acx_filtered_copy(const acx_filtered_t *f, int which, void *host_dst) {
    if (!f || which < 0 || which > ACX_FILT_DATA) return fail(ACX_EINVAL, "no such part");
    const uint64_t bytes = part_bytes(f, which);
    if (!bytes) return ACX_OK;
    if (!host_dst) return fail(ACX_EINVAL, "null argument");
    if (!f->on_device) { std::memcpy(host_dst, f->part[which], bytes); return ACX_OK; }
    int rc = filtered_wait(f);
    if (rc != ACX_OK) return rc;
    DeviceScope ds(f->device);
    HIPCHK(hipMemcpy(host_dst, f->part[which], bytes, hipMemcpyDeviceToHost));
    return ACX_OK;
}

void acx_free_filtered(acx_filtered_t *f) {
    if (!f) return;
    if (f->on_device) {
        DeviceScope ds(f->device);
        // (the kernels write the block: it does not go back to the pool before they are done)
        if (f->done) (void)hipEventSynchronize(f->done);
        g_bufs.put(f->d_block, f->device);
        g_events.put(f->device, f->done);
    }
    delete[] f->h_block;
    delete f;
}

} // extern "C"
