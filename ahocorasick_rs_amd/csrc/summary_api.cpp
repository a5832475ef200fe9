// summary_api.cpp -- the summaries of a find (summary.hpp): the host reduction, the device route behind the find pipeline,
// the acx_summarize* entry points and the accessors of their result.
#include "replace.hpp"
#include "result_block.hpp"
#include "summary.hpp"

using namespace acxh;

// acx_summarize / acx_summarize_device: what is left of a find.  Device route: the reductions in HBM, each in a buffer of its
// own -- all of them the owner's scratch (result_block.hpp), d_* are views; the find's records have gone back to the buffer
// cache behind the reductions.  Host route: the vectors.
struct ACX_HIDDEN acx_summary : ResultBlock {
    uint32_t what = 0;
    uint64_t n_hay = 0, n_patterns = 0, total = 0;
    std::vector<uint64_t> counts, any, hist;
    std::vector<acx_match_t> first;
    uint64_t *d_counts = nullptr, *d_any = nullptr, *d_hist = nullptr;
    acx_match_t *d_first = nullptr;
};

namespace {

constexpr uint32_t SUM_ALL = ACX_SUM_FIRST | ACX_SUM_BY_PATTERN;

// The device route of a summary: the find pipeline as acx_find_device runs it (byte ranges and batch splits included), then
// the reductions on the same stream -- the kernels follow the find's write kernel in stream order.  Returns when the number
// of matches is known; the reductions may still run (out->done).  d_hay, and G.offsets, must stay valid until then.
int run_summary(acx_automaton *a, Ctx *x, const uint8_t *d_hay, uint64_t len, const Segments &G, int overlapping,
                int codepoints, uint32_t what, acx_summary **out) {
    // (the summary always searches: an empty batch's find is its counts)
    return find_stage(a, x, d_hay, len, G, overlapping, codepoints, true, out, [&](FindStage<acx_summary> &F) -> int {
        acx_summary *R = F.R;
        acx_result *r = F.r;
        hipStream_t st = F.st;
        const bool segmented = rows_of(G).segmented;
        R->what = what;
        R->n_hay = rows_of(G).n;
        R->n_patterns = a->host.n_patterns;
        R->total = r->n;
        const uint64_t n_hay = R->n_hay, n = r->n;
        auto get = [&](void **p, uint64_t bytes) -> hipError_t { // (kept until acx_free_summary)
            const hipError_t e = g_bufs.get(p, std::max<uint64_t>(bytes, 16), a->device);
            if (e == hipSuccess) F.keep(*p);
            return e;
        };
        if (segmented) { // the per-haystack counts are the summary's from here on
            F.keep(r->d_counts);
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
                HIPCHK(get((void **)&prefix, (n_hay + 1) * 8));
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
        return ACX_OK;
    });
}

// ACX_SUMMARY_HOST_MAX (bytes, read per call): calls up to this size reduce on the host, behind acx_find / acx_find_batch
uint64_t summary_host_max() {
    const char *e = std::getenv("ACX_SUMMARY_HOST_MAX");
    return e ? std::strtoull(e, nullptr, 10) : (1ull << 20);
}

const void *device_part(const acx_summary *r, const void *p) { return r && r->on_device ? r->ptr_after_wait(p) : nullptr; }

} // namespace

extern "C" {

int acx_summarize_host(const acx_match_t *m, uint64_t n_m, const uint64_t *counts, uint64_t n_hay, uint64_t n_patterns,
                       uint32_t what, uint64_t *any_bits, acx_match_t *first, uint64_t *by_pattern) {
    if (what & ~SUM_ALL) return fail(ACX_EINVAL, "unknown summary bits");
    if (n_m && !m) return fail(ACX_EINVAL, "null matches");
    if (!counts) n_hay = 1;
    if ((what & ACX_SUM_FIRST) && n_hay && (!any_bits || !first)) return fail(ACX_EINVAL, "null argument");
    if ((what & ACX_SUM_BY_PATTERN) && n_patterns && !by_pattern) return fail(ACX_EINVAL, "null argument");
    if (int rc = counts_sum_to(counts, n_hay, n_m)) return rc;
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
    HostBatch B;
    if ((rc = host_batch(hay, &len, offsets, &n_hay, &B)) != ACX_OK) return rc;
    if (len <= summary_host_max()) {
        // host route: the find entry points as they are (K0, the resident K0, the in-place read), then the reduction here
        HostFind f;
        if ((rc = f.find(a, B.hay, len, offsets ? B.rel.data() : nullptr, n_hay, overlapping, codepoints)) != ACX_OK) return rc;
        acx_summary *R = new_result<acx_summary>(a->device, false);
        if (!R) return ACX_ENOMEM;
        R->what = what;
        R->n_hay = n_hay;
        R->n_patterns = a->host.n_patterns;
        R->total = f.nm;
        try {
            if (what & ACX_SUM_FIRST) { R->any.assign((n_hay + 63) / 64, 0); R->first.resize(n_hay); }
            if (what & ACX_SUM_BY_PATTERN) R->hist.assign(R->n_patterns, 0);
        } catch (...) { rc = fail(ACX_ENOMEM, "out of memory"); }
        if (rc == ACX_OK)
            rc = acx_summarize_host(f.m, f.nm, f.counts.data(), n_hay, R->n_patterns, what, R->any.data(), R->first.data(), R->hist.data());
        R->counts = std::move(f.counts);
        if (rc != ACX_OK) { free_result(R); return rc; }
        *out = R;
        return ACX_OK;
    }
    // device route: staged, searched and reduced under one lease
    return staged_call(a, B, len, n_hay, offsets != nullptr, [&](Ctx *c, const uint8_t *d_search, const Segments &G) {
        return run_summary(a, c, d_search, len, G, overlapping, codepoints, what, out);
    });
}

int acx_summarize_device(acx_automaton_t *a, const void *d_hay, uint64_t len, const uint64_t *d_offsets, uint64_t n_hay,
                         uint64_t uniform_len, int overlapping, int codepoints, uint32_t what, acx_summary_t **out) {
    if (!a || !out) return fail(ACX_EINVAL, "null argument");
    *out = nullptr;
    if (what & ~SUM_ALL) return fail(ACX_EINVAL, "unknown summary bits");
    return device_call(a, d_hay, len, d_offsets, n_hay, uniform_len, overlapping, [&](Ctx *c, const uint8_t *d_search, const Segments &G) {
        return run_summary(a, c, d_search, len, G, overlapping, codepoints, what, out);
    });
}

uint64_t acx_summary_total(const acx_summary_t *r) { return r ? r->total : 0; }
int acx_summary_on_device(const acx_summary_t *r) { return r ? r->on_device : 0; }

int acx_summary_counts(const acx_summary_t *r, uint64_t *host_counts) {
    if (!r || (!host_counts && r->n_hay)) return fail(ACX_EINVAL, "null argument");
    return r->copy_out(host_counts, r->on_device ? (const void *)r->d_counts : r->counts.data(), r->n_hay * 8);
}

int acx_summary_any(const acx_summary_t *r, uint64_t *host_bits) {
    if (!r || (!host_bits && r->n_hay)) return fail(ACX_EINVAL, "null argument");
    if (!(r->what & ACX_SUM_FIRST)) return fail(ACX_EINVAL, "the summary was made without ACX_SUM_FIRST");
    const uint64_t bytes = (r->n_hay + 63) / 64 * 8;
    return r->copy_out(host_bits, r->on_device ? (const void *)r->d_any : r->any.data(), bytes);
}

int acx_summary_first(const acx_summary_t *r, acx_match_t *host_first) {
    if (!r || (!host_first && r->n_hay)) return fail(ACX_EINVAL, "null argument");
    if (!(r->what & ACX_SUM_FIRST)) return fail(ACX_EINVAL, "the summary was made without ACX_SUM_FIRST");
    const uint64_t bytes = r->n_hay * sizeof(acx_match_t);
    return r->copy_out(host_first, r->on_device ? (const void *)r->d_first : r->first.data(), bytes);
}

int acx_summary_by_pattern(const acx_summary_t *r, uint64_t *host_hist) {
    if (!r || (!host_hist && r->n_patterns)) return fail(ACX_EINVAL, "null argument");
    if (!(r->what & ACX_SUM_BY_PATTERN)) return fail(ACX_EINVAL, "the summary was made without ACX_SUM_BY_PATTERN");
    return r->copy_out(host_hist, r->on_device ? (const void *)r->d_hist : r->hist.data(), r->n_patterns * 8);
}

const uint64_t *acx_summary_device_counts(const acx_summary_t *r) { return (const uint64_t *)device_part(r, r ? r->d_counts : nullptr); }
const uint64_t *acx_summary_device_any(const acx_summary_t *r) { return (const uint64_t *)device_part(r, r ? r->d_any : nullptr); }
const acx_match_t *acx_summary_device_first(const acx_summary_t *r) {
    return (const acx_match_t *)device_part(r, r ? r->d_first : nullptr);
}
const uint64_t *acx_summary_device_by_pattern(const acx_summary_t *r) {
    return (const uint64_t *)device_part(r, r ? r->d_hist : nullptr);
}

void acx_free_summary(acx_summary_t *r) { free_result(r); }

} // extern "C"
