// summary_api.cpp -- the summaries of a find (summary.hpp): the host reduction, the device route behind the find pipeline,
// the acx_summarize* entry points and the accessors of their result.
#include "find_pipeline.hpp"
#include "replace.hpp"
#include "summary.hpp"

using namespace acxh;

// acx_summarize / acx_summarize_device: what is left of a find.  Device route: the reductions in HBM, written by kernels
// that may still run when the call returns (done); the find's records have gone back to the buffer cache behind the same
// kernels, only the summaries and the scan's scratch are kept until acx_free_summary.  Host route: the vectors.
struct ACX_HIDDEN acx_summary {
    int device = 0;
    int on_device = 0;
    uint32_t what = 0;
    uint64_t n_hay = 0, n_patterns = 0, total = 0;
    std::vector<uint64_t> counts, any, hist;
    std::vector<acx_match_t> first;
    uint64_t *d_counts = nullptr, *d_any = nullptr, *d_hist = nullptr;
    acx_match_t *d_first = nullptr;
    hipEvent_t done = nullptr;
    std::vector<void *> scratch;
};

namespace {

constexpr uint32_t SUM_ALL = ACX_SUM_FIRST | ACX_SUM_BY_PATTERN;

// The device route of a summary: the find pipeline as acx_find_device runs it (byte ranges and batch splits included), then
// the reductions on the same stream -- the kernels follow the find's write kernel in stream order.  Returns when the number
// of matches is known; the reductions may still run (out->done).  d_hay, and G.offsets, must stay valid until then.
int run_summary(acx_automaton *a, Ctx *x, const uint8_t *d_hay, uint64_t len, const Segments &G, int overlapping,
                int codepoints, uint32_t what, acx_summary **out) {
    *out = nullptr;
    acx_result *r = nullptr;
    int rc = run_find(a, x, d_hay, len, G, overlapping, codepoints, &r);
    if (rc != ACX_OK) return rc;
    acx_summary *R = new (std::nothrow) acx_summary();
    if (!R) { acx_free_result(r); return fail(ACX_ENOMEM, "out of memory"); }
    hipStream_t st = x->stream;
    const bool segmented = G.uniform_len != 0 || G.offsets != nullptr;
    R->device = a->device;
    R->on_device = 1;
    R->what = what;
    R->n_hay = segmented ? G.n_hay : 1;
    R->n_patterns = a->host.n_patterns;
    R->total = r->n;
    const uint64_t n_hay = R->n_hay, n = r->n;
    auto get = [&](void **p, uint64_t bytes) -> hipError_t { return g_bufs.get(p, std::max<uint64_t>(bytes, 16), a->device); };
    auto body = [&]() -> int {
        if (segmented) { // the per-haystack counts are the summary's from here on
            R->d_counts = r->d_counts;
            r->d_counts = nullptr;
        } else {
            HIPCHK(get((void **)&R->d_counts, 8));
            HIPCHK(hipMemcpyAsync(R->d_counts, &R->total, 8, hipMemcpyHostToDevice, st));
        }
        if (what & ACX_SUM_FIRST) {
            int64_t *prefix = nullptr;
            if (segmented) { // where every haystack's records begin, from the counts
                uint64_t *temp = nullptr;
                HIPCHK(get((void **)&temp, replace_scan_words(n_hay) * 8));
                R->scratch.push_back(temp);
                HIPCHK(get((void **)&prefix, (n_hay + 1) * 8));
                R->scratch.push_back(prefix);
                HIPCHK(acx::replace_scan(nullptr, nullptr, R->d_counts, n_hay, prefix, temp, st));
            }
            HIPCHK(get((void **)&R->d_first, n_hay * sizeof(acx_match_t)));
            HIPCHK(get((void **)&R->d_any, (n_hay + 63) / 64 * 8));
            HIPCHK(acx::summary_gather(r->d_matches, n, prefix, n_hay, R->d_first, R->d_any, st));
        }
        if (what & ACX_SUM_BY_PATTERN) {
            HIPCHK(get((void **)&R->d_hist, R->n_patterns * 8));
            HIPCHK(acx::summary_hist(r->d_matches, n, R->n_patterns, R->d_hist, st));
        }
        // The find's records are not needed beyond this point of the stream: they go back to the buffer cache, which holds
        // them until an event recorded HERE has fired (the result's own event lies in front of the reductions).
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
        g_events.put(a->device, r->done);
        r->done = nullptr;
        g_bufs.put(r->borrowed ? nullptr : r->d_matches, a->device, freed);
        r->d_matches = nullptr;
        return ACX_OK;
    };
    rc = body();
    if (rc != ACX_OK) (void)hipStreamSynchronize(st);
    acx_free_result(r); // (emptied above when all went well)
    if (rc != ACX_OK) { acx_free_summary(R); return rc; }
    *out = R;
    return ACX_OK;
}

// ACX_SUMMARY_HOST_MAX (bytes, read per call): calls up to this size reduce on the host, behind acx_find / acx_find_batch
uint64_t summary_host_max() {
    const char *e = std::getenv("ACX_SUMMARY_HOST_MAX");
    return e ? std::strtoull(e, nullptr, 10) : (1ull << 20);
}

// device words -> the caller's, behind the reductions
int copy_back(const acx_summary *r, void *dst, const void *d_src, uint64_t bytes) {
    if (!bytes) return ACX_OK;
    DeviceScope ds(r->device);
    if (r->done) HIPCHK(hipEventSynchronize(r->done));
    HIPCHK(hipMemcpy(dst, d_src, bytes, hipMemcpyDeviceToHost));
    return ACX_OK;
}

const void *device_part(const acx_summary *r, const void *p) {
    if (!r || !r->on_device || !p) return nullptr;
    if (r->done) {
        DeviceScope ds(r->device);
        if (hipEventSynchronize(r->done) != hipSuccess) return nullptr;
    }
    return p;
}

} // namespace

extern "C" {

int acx_summarize_host(const acx_match_t *m, uint64_t n_m, const uint64_t *counts, uint64_t n_hay, uint64_t n_patterns,
                       uint32_t what, uint64_t *any_bits, acx_match_t *first, uint64_t *by_pattern) {
    if (what & ~SUM_ALL) return fail(ACX_EINVAL, "unknown summary bits");
    if (n_m && !m) return fail(ACX_EINVAL, "null matches");
    if (!counts) n_hay = 1;
    if ((what & ACX_SUM_FIRST) && n_hay && (!any_bits || !first)) return fail(ACX_EINVAL, "null argument");
    if ((what & ACX_SUM_BY_PATTERN) && n_patterns && !by_pattern) return fail(ACX_EINVAL, "null argument");
    uint64_t sum = 0;
    for (uint64_t h = 0; counts && h < n_hay; h++) {
        if (counts[h] > n_m - sum) return fail(ACX_EINVAL, "the counts do not sum to the number of matches");
        sum += counts[h];
    }
    if (counts && sum != n_m) return fail(ACX_EINVAL, "the counts do not sum to the number of matches");
    for (uint64_t i = 0; i < n_m; i++)
        if (m[i].pattern >= n_patterns)
            return fail(ACX_EINVAL, "match " + std::to_string(i) + " names pattern " + std::to_string(m[i].pattern) + " of " +
                                        std::to_string(n_patterns));
    if (what & ACX_SUM_FIRST) {
        for (uint64_t w = 0; w < (n_hay + 63) / 64; w++) any_bits[w] = 0;
        uint64_t at = 0;
        for (uint64_t h = 0; h < n_hay; h++) {
            const uint64_t c = counts ? counts[h] : n_m;
            if (c) { first[h] = m[at]; any_bits[h >> 6] |= 1ull << (h & 63); }
            else first[h] = acx_match_t{UINT64_MAX, 0, 0};
            at += c;
        }
    }
    if (what & ACX_SUM_BY_PATTERN) {
        for (uint64_t p = 0; p < n_patterns; p++) by_pattern[p] = 0;
        for (uint64_t i = 0; i < n_m; i++) by_pattern[m[i].pattern]++;
    }
    return ACX_OK;
}

int acx_summarize(acx_automaton_t *a, const uint8_t *hay, uint64_t len, const uint64_t *offsets, uint64_t n_hay,
                  int overlapping, int codepoints, uint32_t what, acx_summary_t **out) {
    if (!a || !out) return fail(ACX_EINVAL, "null argument");
    *out = nullptr;
    if (what & ~SUM_ALL) return fail(ACX_EINVAL, "unknown summary bits");
    int rc = overlapping ? check_overlapping(a) : ACX_OK; // (the error, no device state)
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
    std::vector<uint64_t> rel(n_hay + 1);
    for (uint64_t i = 0; i <= n_hay; i++) rel[i] = offsets ? offsets[i] - base : (i ? len : 0);
    if (len <= summary_host_max()) {
        // host route: the find entry points as they are (K0, the resident K0, the in-place read), then the reduction here
        acx_match_t *m = nullptr;
        uint64_t nm = 0;
        std::vector<uint64_t> counts(n_hay, 0);
        if (!offsets) {
            rc = acx_find(a, h, len, overlapping, codepoints, &m, &nm);
            counts[0] = nm;
        } else if (n_hay) {
            rc = acx_find_batch(a, h, rel.data(), n_hay, overlapping, codepoints, &m, &nm, counts.data());
        }
        if (rc != ACX_OK) return rc;
        acx_summary *R = new (std::nothrow) acx_summary();
        if (!R) { acx_free_matches(m); return fail(ACX_ENOMEM, "out of memory"); }
        R->device = a->device;
        R->what = what;
        R->n_hay = n_hay;
        R->n_patterns = a->host.n_patterns;
        R->total = nm;
        try {
            if (what & ACX_SUM_FIRST) { R->any.assign((n_hay + 63) / 64, 0); R->first.resize(n_hay); }
            if (what & ACX_SUM_BY_PATTERN) R->hist.assign(R->n_patterns, 0);
        } catch (...) { rc = fail(ACX_ENOMEM, "out of memory"); }
        const uint64_t none = 0; // (an empty batch: the counts' vector has no storage to point at)
        if (rc == ACX_OK)
            rc = acx_summarize_host(m, nm, n_hay ? counts.data() : &none, n_hay, R->n_patterns, what, R->any.data(), R->first.data(),
                                    R->hist.data());
        R->counts = std::move(counts);
        acx_free_matches(m);
        if (rc != ACX_OK) { acx_free_summary(R); return rc; }
        *out = R;
        return ACX_OK;
    }
    // device route: staged, searched and reduced under one lease
    Lease lease(a);
    Ctx *c = lease.c;
    if (!c) return fail(ACX_EDEVICE, "could not create a stream for the call");
    rc = stage_host(a, c, h, len, offsets ? rel.data() : nullptr, offsets ? n_hay + 1 : 0, false);
    if (rc != ACX_OK) return rc;
    const uint8_t *d_search = nullptr;
    if ((rc = fold_copy(a, c, c->ws.hay, len, &d_search)) != ACX_OK) return rc;
    const Segments G = offsets ? Segments{c->ws.offsets, n_hay, 0} : Segments{nullptr, 1, 0};
    return run_summary(a, c, d_search, len, G, overlapping, codepoints, what, out);
}

int acx_summarize_device(acx_automaton_t *a, const void *d_hay, uint64_t len, const uint64_t *d_offsets, uint64_t n_hay,
                         uint64_t uniform_len, int overlapping, int codepoints, uint32_t what, acx_summary_t **out) {
    if (!a || !out) return fail(ACX_EINVAL, "null argument");
    *out = nullptr;
    if (what & ~SUM_ALL) return fail(ACX_EINVAL, "unknown summary bits");
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
    return run_summary(a, lease.c, d_search, len, G, overlapping, codepoints, what, out);
}

uint64_t acx_summary_total(const acx_summary_t *r) { return r ? r->total : 0; }
int acx_summary_on_device(const acx_summary_t *r) { return r ? r->on_device : 0; }

int acx_summary_counts(const acx_summary_t *r, uint64_t *host_counts) {
    if (!r || (!host_counts && r->n_hay)) return fail(ACX_EINVAL, "null argument");
    if (r->on_device) return copy_back(r, host_counts, r->d_counts, r->n_hay * 8);
    if (r->n_hay) std::memcpy(host_counts, r->counts.data(), r->n_hay * 8);
    return ACX_OK;
}

int acx_summary_any(const acx_summary_t *r, uint64_t *host_bits) {
    if (!r || (!host_bits && r->n_hay)) return fail(ACX_EINVAL, "null argument");
    if (!(r->what & ACX_SUM_FIRST)) return fail(ACX_EINVAL, "the summary was made without ACX_SUM_FIRST");
    const uint64_t bytes = (r->n_hay + 63) / 64 * 8;
    if (r->on_device) return copy_back(r, host_bits, r->d_any, bytes);
    if (bytes) std::memcpy(host_bits, r->any.data(), bytes);
    return ACX_OK;
}

int acx_summary_first(const acx_summary_t *r, acx_match_t *host_first) {
    if (!r || (!host_first && r->n_hay)) return fail(ACX_EINVAL, "null argument");
    if (!(r->what & ACX_SUM_FIRST)) return fail(ACX_EINVAL, "the summary was made without ACX_SUM_FIRST");
    const uint64_t bytes = r->n_hay * sizeof(acx_match_t);
    if (r->on_device) return copy_back(r, host_first, r->d_first, bytes);
    if (bytes) std::memcpy(host_first, r->first.data(), bytes);
    return ACX_OK;
}

int acx_summary_by_pattern(const acx_summary_t *r, uint64_t *host_hist) {
    if (!r || (!host_hist && r->n_patterns)) return fail(ACX_EINVAL, "null argument");
    if (!(r->what & ACX_SUM_BY_PATTERN)) return fail(ACX_EINVAL, "the summary was made without ACX_SUM_BY_PATTERN");
    if (r->on_device) return copy_back(r, host_hist, r->d_hist, r->n_patterns * 8);
    if (r->n_patterns) std::memcpy(host_hist, r->hist.data(), r->n_patterns * 8);
    return ACX_OK;
}

const uint64_t *acx_summary_device_counts(const acx_summary_t *r) { return (const uint64_t *)device_part(r, r ? r->d_counts : nullptr); }
const uint64_t *acx_summary_device_any(const acx_summary_t *r) { return (const uint64_t *)device_part(r, r ? r->d_any : nullptr); }
const acx_match_t *acx_summary_device_first(const acx_summary_t *r) {
    return (const acx_match_t *)device_part(r, r ? r->d_first : nullptr);
}
const uint64_t *acx_summary_device_by_pattern(const acx_summary_t *r) {
    return (const uint64_t *)device_part(r, r ? r->d_hist : nullptr);
}

void acx_free_summary(acx_summary_t *r) {
    if (!r) return;
    if (r->on_device) {
        DeviceScope ds(r->device);
        // (the reductions write the summaries and read the scratch: nothing goes back to the pool before they are done)
        if (r->done) (void)hipEventSynchronize(r->done);
        for (void *p : r->scratch) g_bufs.put(p, r->device);
        g_bufs.put(r->d_counts, r->device);
        g_bufs.put(r->d_any, r->device);
        g_bufs.put(r->d_first, r->device);
        g_bufs.put(r->d_hist, r->device);
        g_events.put(r->device, r->done);
    }
    delete r;
}

} // extern "C"
