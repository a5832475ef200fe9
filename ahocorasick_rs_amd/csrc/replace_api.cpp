// replace_api.cpp -- replace_all (replace.hpp): the host splice, the device route behind the find pipeline, the acx_replace*
// entry points and the accessors of their result.
#include "replace.hpp"
#include "result_block.hpp"

using namespace acxh;

// acx_replace / acx_replace_device: the spliced output.  Device route: the owner's block in HBM (round_up(len, 16) bytes),
// written by kernels that may still run when the call returns (done); the find result and the scratch they read are kept
// until acx_free_replaced.  Host route: h_out.
struct ACX_HIDDEN acx_replaced : ResultBlock {
    uint64_t len = 0;
    std::vector<uint64_t> offsets; // n_hay + 1: every haystack's output bounds
    std::vector<uint8_t> h_out;
    acx_result *find = nullptr;
    const uint8_t *bytes() const { return on_device ? (const uint8_t *)d_block : h_out.data(); }
};

namespace {

// The device route of a replacement (replace.hpp): the find pipeline as acx_find_device runs it (byte ranges and batch
// splits included), then the splice on the same stream -- the kernels follow the find's write kernel in stream order.
// Returns when the output's length is known; the gather may still run (out->done).  d_hay: the bytes the find reads (a
// case-insensitive handle's folded copy), d_orig: the caller's bytes the splice takes; they, and G.offsets, must stay
// valid until then.
int run_replace(acx_automaton *a, Ctx *x, const uint8_t *d_hay, const uint8_t *d_orig, uint64_t len, const Segments &G,
                const uint8_t *repl_blob, const uint64_t *repl_offsets, uint64_t n_repl, acx_replaced **out) {
    *out = nullptr;
    acx_result *r = nullptr;
    int rc = run_find(a, x, d_hay, len, G, 0, 0, &r);
    if (rc != ACX_OK) return rc;
    acx_replaced *R = new_result<acx_replaced>(a->device, true);
    if (!R) { acx_free_result(r); return ACX_ENOMEM; }
    R->find = r;
    hipStream_t st = x->stream;
    const bool segmented = rows_of(G).segmented;
    const uint64_t n_hay = rows_of(G).n, n = r->n;
    const uint64_t r0 = n_repl ? repl_offsets[0] : 0, blob_len = n_repl ? repl_offsets[n_repl] - r0 : 0;
    std::vector<uint64_t> roff(n_repl + 1);
    for (uint64_t i = 0; i <= n_repl; i++) roff[i] = n_repl ? repl_offsets[i] - r0 : 0;
    uint8_t *d_blob = nullptr;
    uint64_t *d_roff = nullptr, *temp = nullptr, *first = nullptr, *o = nullptr, *out_off = nullptr, *tiles = nullptr;
    int64_t *P = nullptr;
    auto get = [&](void **p, uint64_t bytes) -> hipError_t {
        hipError_t e = g_bufs.get(p, std::max<uint64_t>(bytes, 16), a->device);
        if (e == hipSuccess) R->scratch.push_back(*p);
        return e;
    };
    auto body = [&]() -> int {
        const uint64_t scan_words = replace_scan_words(std::max(n, n_hay));
        HIPCHK(get((void **)&d_blob, blob_len + 32));
        HIPCHK(get((void **)&d_roff, (n_repl + 1) * 8));
        HIPCHK(get((void **)&temp, scan_words * 8));
        HIPCHK(get((void **)&P, (n + 1) * 8));
        HIPCHK(get((void **)&o, n * 8));
        HIPCHK(get((void **)&out_off, (n_hay + 1) * 8));
        if (blob_len) HIPCHK(hipMemcpyAsync(d_blob, repl_blob + r0, blob_len, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_roff, roff.data(), (n_repl + 1) * 8, hipMemcpyHostToDevice, st));
        if (segmented) { // the first match of every haystack, from the result's per-haystack counts
            HIPCHK(get((void **)&first, (n_hay + 1) * 8));
            HIPCHK(replace_scan(nullptr, nullptr, r->d_counts, n_hay, (int64_t *)first, temp, st));
        }
        HIPCHK(replace_scan(r->d_matches, d_roff, nullptr, n, P, temp, st));
        const RepSegs S{row_cut(G, len), first};
        HIPCHK(replace_positions(r->d_matches, n, P, S, o, out_off, st));
        R->offsets.resize(n_hay + 1);
        HIPCHK(hipMemcpyAsync(R->offsets.data(), out_off, (n_hay + 1) * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st)); // (the output's length sizes its buffer; roff is read by then)
        R->len = R->offsets[n_hay];
        int rc = R->alloc(std::max<uint64_t>((R->len + 15) / 16 * 16, 16));
        if (rc != ACX_OK) return rc;
        uint8_t *d_out = (uint8_t *)R->d_block;
        if (!n) { // nothing matched: the output is the input
            if (len) HIPCHK(hipMemcpyAsync(d_out, d_orig, len, hipMemcpyDeviceToDevice, st));
        } else {
            HIPCHK(get((void **)&tiles, replace_tile_words(R->len) * 8));
            HIPCHK(replace_gather(d_orig, len, r->d_matches, n, o, P, d_blob, blob_len + 32, d_roff, tiles, d_out, R->len, st));
        }
        return ACX_OK;
    };
    rc = retire_find(body(), st, nullptr, R); // (the find result stays whole: the gather reads it)
    if (rc != ACX_OK) { acx_free_replaced(R); return rc; }
    a->path[12]++;
    *out = R;
    return ACX_OK;
}

int check_repl(const acx_automaton_t *a, const uint64_t *repl_offsets, uint64_t n_repl) {
    if (n_repl != a->host.n_patterns)
        return fail(ACX_EINVAL, "replace_with has " + std::to_string(n_repl) + " entries, the automaton " +
                                    std::to_string(a->host.n_patterns) + " patterns");
    if (n_repl && !repl_offsets) return fail(ACX_EINVAL, "null replacement offsets");
    for (uint64_t i = 0; i < n_repl; i++)
        if (repl_offsets[i + 1] < repl_offsets[i]) return fail(ACX_EINVAL, "replacement offsets not monotone");
    return ACX_OK;
}
// ACX_REPLACE_HOST_MAX (bytes, read per call): calls up to this size splice on the host, behind acx_find / acx_find_batch
uint64_t replace_host_max() {
    const char *e = std::getenv("ACX_REPLACE_HOST_MAX");
    return e ? std::strtoull(e, nullptr, 10) : (1ull << 20);
}

} // namespace

extern "C" {

// ---- replacement (replace.hpp) ----
int acx_splice_host(const uint8_t *hay, uint64_t len, const acx_match_t *m, uint64_t n_m, const uint8_t *repl_blob,
                    const uint64_t *repl_offsets, uint64_t n_repl, uint8_t *dst, uint64_t *dst_len) {
    if (!dst_len || (n_m && !m) || (n_repl && !repl_offsets) || (len && !hay && dst)) return fail(ACX_EINVAL, "null argument");
    for (uint64_t i = 0; i < n_repl; i++)
        if (repl_offsets[i + 1] < repl_offsets[i]) return fail(ACX_EINVAL, "replacement offsets not monotone");
    if (n_repl && repl_offsets[n_repl] > repl_offsets[0] && !repl_blob) return fail(ACX_EINVAL, "null replacement blob");
    uint64_t total = len, at = 0;
    for (uint64_t i = 0; i < n_m; i++) {
        const acx_match_t &x = m[i];
        if (x.start < at || x.end < x.start || x.end > len)
            return fail(ACX_EINVAL, "match " + std::to_string(i) + " is out of order, overlaps the one before or lies beyond the haystack");
        if (x.pattern >= n_repl)
            return fail(ACX_EINVAL, "match " + std::to_string(i) + " names pattern " + std::to_string(x.pattern) + " of " +
                                        std::to_string(n_repl) + " replacements");
        total = total - (x.end - x.start) + (repl_offsets[x.pattern + 1] - repl_offsets[x.pattern]);
        at = x.end;
    }
    *dst_len = total;
    if (!dst) return ACX_OK;
    uint8_t *d = dst;
    at = 0;
    for (uint64_t i = 0; i < n_m; i++) {
        const acx_match_t &x = m[i];
        const uint64_t rl = repl_offsets[x.pattern + 1] - repl_offsets[x.pattern];
        if (x.start > at) { std::memcpy(d, hay + at, x.start - at); d += x.start - at; }
        if (rl) { std::memcpy(d, repl_blob + repl_offsets[x.pattern], rl); d += rl; }
        at = x.end;
    }
    if (len > at) std::memcpy(d, hay + at, len - at);
    return ACX_OK;
}

int acx_replace(acx_automaton_t *a, const uint8_t *hay, uint64_t len, const uint64_t *offsets, uint64_t n_hay,
                const uint8_t *repl_blob, const uint64_t *repl_offsets, uint64_t n_repl, acx_replaced_t **out) {
    if (!a || !out) return fail(ACX_EINVAL, "null argument");
    *out = nullptr;
    int rc = check_repl(a, repl_offsets, n_repl);
    if (rc != ACX_OK) return rc;
    HostBatch B;
    if ((rc = host_batch(hay, &len, offsets, &n_hay, &B)) != ACX_OK) return rc;
    const uint8_t *h = B.hay;
    const std::vector<uint64_t> &rel = B.rel;
    if (len <= replace_host_max()) {
        // host route: the find entry points as they are (K0, the resident K0, the in-place read), then the splice here
        HostFind f;
        if ((rc = f.find(a, h, len, offsets ? rel.data() : nullptr, n_hay, 0, 0)) != ACX_OK) return rc;
        const acx_match_t *m = f.m;
        const std::vector<uint64_t> &counts = f.counts;
        acx_replaced *R = new_result<acx_replaced>(a->device, false);
        if (!R) return ACX_ENOMEM;
        R->offsets.assign(n_hay + 1, 0);
        uint64_t at = 0;
        for (uint64_t i = 0; i < n_hay && rc == ACX_OK; i++) { // (sizes first: one allocation)
            uint64_t sz = 0;
            rc = acx_splice_host(h ? h + rel[i] : nullptr, rel[i + 1] - rel[i], m + at, counts[i], repl_blob, repl_offsets,
                                 n_repl, nullptr, &sz);
            R->offsets[i + 1] = R->offsets[i] + sz;
            at += counts[i];
        }
        if (rc == ACX_OK) {
            R->len = R->offsets[n_hay];
            try { R->h_out.resize(R->len); } catch (...) { rc = fail(ACX_ENOMEM, "out of memory"); }
        }
        at = 0;
        for (uint64_t i = 0; i < n_hay && rc == ACX_OK; i++) {
            uint64_t sz = 0;
            rc = acx_splice_host(h ? h + rel[i] : nullptr, rel[i + 1] - rel[i], m + at, counts[i], repl_blob, repl_offsets,
                                 n_repl, R->h_out.data() + R->offsets[i], &sz);
            at += counts[i];
        }
        if (rc != ACX_OK) { acx_free_replaced(R); return rc; }
        *out = R;
        return ACX_OK;
    }
    // device route: staged, searched and spliced under one lease
    return staged_call(a, B, len, n_hay, offsets != nullptr, [&](Ctx *c, const uint8_t *d_search, const Segments &G) {
        return run_replace(a, c, d_search, c->ws.hay, len, G, repl_blob, repl_offsets, n_repl, out);
    });
}

int acx_replace_device(acx_automaton_t *a, const void *d_hay, uint64_t len, const uint64_t *d_offsets, uint64_t n_hay,
                       uint64_t uniform_len, const uint8_t *repl_blob, const uint64_t *repl_offsets, uint64_t n_repl,
                       acx_replaced_t **out) {
    if (!a || !out) return fail(ACX_EINVAL, "null argument");
    *out = nullptr;
    if (len && !d_hay) return fail(ACX_EINVAL, "null haystack");
    int rc = check_repl(a, repl_offsets, n_repl);
    if (rc != ACX_OK) return rc;
    Segments G;
    if ((rc = make_segments(d_offsets, n_hay, uniform_len, len, &G)) != ACX_OK) return rc;
    Lease lease(a);
    if (!lease.c) return fail(ACX_EDEVICE, "could not create a stream for the call");
    const uint8_t *d_search = nullptr;
    rc = fold_copy(a, lease.c, (const uint8_t *)d_hay, len, &d_search);
    if (rc != ACX_OK) return rc;
    return run_replace(a, lease.c, d_search, (const uint8_t *)d_hay, len, G, repl_blob, repl_offsets, n_repl, out);
}

uint64_t acx_replaced_len(const acx_replaced_t *r) { return r ? r->len : 0; }

int acx_replaced_offsets(const acx_replaced_t *r, uint64_t *host_offsets) {
    if (!r || !host_offsets) return fail(ACX_EINVAL, "null argument");
    std::memcpy(host_offsets, r->offsets.data(), r->offsets.size() * 8);
    return ACX_OK;
}

int acx_replaced_copy(const acx_replaced_t *r, void *host_dst) {
    if (!r || (!host_dst && r->len)) return fail(ACX_EINVAL, "null argument");
    return r->copy_out(host_dst, r->bytes(), r->len);
}

const void *acx_replaced_device_bytes(const acx_replaced_t *r) { return r && r->on_device ? r->ptr_after_wait(r->d_block) : nullptr; }

void acx_free_replaced(acx_replaced_t *r) {
    acx_result *find = r ? r->find : nullptr;
    free_result(r); // (the gather reads the find result as well: it goes after the wait)
    acx_free_result(find);
}

} // extern "C"
