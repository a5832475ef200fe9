// acx_api.cpp -- the find / result / profile / device entry points of the C ABI declared in include/acx.h: each validates,
// leases a context, calls one function of the host layer and converts its result.  The layer's other units: build_upload.cpp
// (acx_build*), replace_api.cpp (acx_replace*), find_pipeline.cpp + find_attempts.cpp (the device pipeline, kernels.hip),
// small_calls.cpp (K0), workspace.cpp (contexts, buffers).  There is no CPU
// matching path here: without a HIP device every find call fails (ACX_EDEVICE).
//
// Concurrency (reference: methods take a shared PyRef and release the GIL, the module is
// gil_used = false -- /root/reference/src/lib.rs:238, 261, 433, 438): a handle owns a small pool of
// *contexts* (stream + workspace + pinned scratch); every call leases one, so calls from different
// threads on ONE automaton run side by side on different streams instead of queueing on a lock.
#include <thread>

#include "find_pipeline.hpp"
#include "small_calls.hpp"

using namespace acxh;

namespace {

// device result -> host array the caller owns (acx_free_matches).  Large results land in a pinned
// buffer that is handed out as it is.
int download_matches(const acx_result *r, acx_match_t **out, uint64_t *n_out) {
    *out = nullptr;
    const uint64_t n = r->n;
    *n_out = n;
    if (!n) return result_wait(r);
    const size_t bytes = n * sizeof(acx_match_t);
    acx_match_t *m = nullptr;
    if (bytes >= (1u << 20)) m = (acx_match_t *)g_pinned_results.get(bytes);
    const bool pinned = m != nullptr;
    if (!m) m = (acx_match_t *)std::malloc(bytes);
    if (!m) return fail(ACX_ENOMEM, "out of memory");
    int rc = acx_result_copy(r, m);
    if (rc != ACX_OK) {
        if (pinned) g_pinned_results.put(m); else std::free(m);
        return rc;
    }
    *out = m;
    return ACX_OK;
}

// The result of a mid-size host call whose records the write kernel put into the context's pinned buffer (r->borrowed): wait
// for the kernel (a few microseconds behind the totals: polled, a blocking wait's wake-up costs more than the kernel), copy
// them out -- no device-to-host copy call.  Under the call's lease.
int copy_borrowed(Ctx *c, const acx_result *r, acx_match_t **out, uint64_t *n_out) {
    if (r->done) {
        hipError_t e = hipSuccess, sync_e = hipSuccess;
        (void)poll_until([&] { return (e = hipEventQuery(r->done)) != hipErrorNotReady; }, 255, std::chrono::milliseconds(2),
                         [&] { sync_e = hipEventSynchronize(r->done); });
        if (sync_e != hipSuccess) e = sync_e;
        if (e != hipSuccess) return hipfail(e, "the write kernel");
    } else {
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    *n_out = r->n;
    if (!r->n) return ACX_OK;
    acx_match_t *m = (acx_match_t *)std::malloc(r->n * sizeof(acx_match_t));
    if (!m) return fail(ACX_ENOMEM, "out of memory");
    std::memcpy(m, r->d_matches, r->n * sizeof(acx_match_t));
    *out = m;
    return ACX_OK;
}

} // namespace

// ---------------------------------------------------------------------------
extern "C" {

// (comm.cpp reports through the same thread-local message)
int acx_internal_fail(int code, const char *msg) { return fail(code, msg ? msg : ""); }

int acx_version(void) { return ACX_VERSION; }
const char *acx_last_error(void) { return g_err.c_str(); }

int acx_device_count(int *n) {
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) { *n = 0; return hipfail(e, "hipGetDeviceCount"); }
    *n = c;
    return ACX_OK;
}

int acx_set_device(int ordinal) {
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) return hipfail(e, "hipGetDeviceCount");
    if (ordinal < 0 || ordinal >= c) return fail(ACX_EINVAL, "device ordinal out of range");
    g_device = ordinal;
    HIPCHK(hipSetDevice(ordinal));
    return ACX_OK;
}


int acx_find_device(acx_automaton_t *a, const void *d_hay, uint64_t len, const uint64_t *d_offsets,
                    uint64_t n_hay, uint64_t uniform_len, int overlapping, int codepoints,
                    acx_result_t **out) {
    if (!a || !out) return fail(ACX_EINVAL, "null argument");
    if (len && !d_hay) return fail(ACX_EINVAL, "null haystack");
    *out = nullptr;
    Segments G;
    int rc = make_segments(d_offsets, n_hay, uniform_len, len, &G);
    if (rc == ACX_OK && overlapping) rc = check_overlapping(a); // (the error, no device state)
    if (rc != ACX_OK) return rc;
    g_trace.mark(0);
    {
        Lease lease(a);
        g_trace.mark(1);
        const uint8_t *d_search = (const uint8_t *)d_hay;
        rc = lease.c ? fold_copy(a, lease.c, (const uint8_t *)d_hay, len, &d_search) : ACX_OK;
        // returns when the totals are known; accessors of the result wait for the rest of its device work
        if (rc == ACX_OK) rc = run_find(a, lease.c, d_search, len, G, overlapping, codepoints, out);
    }
    g_trace.mark(7);
    return rc;
}

uint64_t acx_result_count(const acx_result_t *r) { return r ? r->n : 0; }
const acx_match_t *acx_result_device_matches(const acx_result_t *r) {
    if (!r || result_wait(r) != ACX_OK) return nullptr;
    return r->d_matches;
}
const uint64_t *acx_result_device_counts(const acx_result_t *r) {
    if (!r || result_wait(r) != ACX_OK) return nullptr;
    return r->d_counts;
}

int acx_result_copy(const acx_result_t *r, acx_match_t *host_out) {
    if (!r) return fail(ACX_EINVAL, "null result");
    int rc = result_wait(r);
    if (rc != ACX_OK || !r->n) return rc;
    DeviceScope ds(r->device);
    HIPCHK(hipMemcpy(host_out, r->d_matches, r->n * sizeof(acx_match_t), hipMemcpyDeviceToHost));
    return ACX_OK;
}

int acx_result_copy_counts(const acx_result_t *r, uint64_t *host_counts) {
    if (!r) return fail(ACX_EINVAL, "null result");
    int rc = result_wait(r);
    if (rc != ACX_OK || !r->d_counts || !r->n_hay) return rc;
    DeviceScope ds(r->device);
    HIPCHK(hipMemcpy(host_counts, r->d_counts, r->n_hay * 8, hipMemcpyDeviceToHost));
    return ACX_OK;
}

void acx_free_result(acx_result_t *r) {
    if (!r) return;
    g_trace.mark(8);
    struct AtExit { ~AtExit() { g_trace.mark(9); } } at_exit;
    // the buffers may still be written by the call's last kernels: the cache holds them back until
    // the event has fired (one event guards both buffers; nobody waits here -- a batch caller that
    // frees a result and starts the next call used to sit out the write kernel in this function)
    g_bufs.put(r->borrowed ? nullptr : r->d_matches, r->device, r->done, r->d_counts);
    delete r;
}

int acx_find(acx_automaton_t *a, const uint8_t *hay, uint64_t len, int overlapping, int codepoints,
             acx_match_t **out, uint64_t *n_out) {
    if (!a || !out || !n_out) return fail(ACX_EINVAL, "null argument");
    *out = nullptr; *n_out = 0;
    if (len && !hay) return fail(ACX_EINVAL, "null haystack");
    int rc = overlapping ? check_overlapping(a) : ACX_OK; // (the error, no device state)
    if (rc != ACX_OK) return rc;
    const bool try_small = small_ok(a, len);
    Lease lease(a, try_small);
    Ctx *c = lease.c;
    if (!c) return fail(ACX_EDEVICE, "could not create a stream for the call");
    if (try_small) { // K0: the resident kernel or one launch, on pinned memory -- no H2D / D2H copies at all
        acx_match_t *m = nullptr;
        uint64_t n = 0;
        bool done = false;
        if ((rc = run_small_host(a, c, hay, len, overlapping, codepoints, &m, &n, &done)) != ACX_OK) return rc;
        if (done) {
            // (copies of a string: K0 reported the lowest ids)
            if (n && overlapping && a->expand_ov && (rc = expand_copies_host(a, &m, &n)) != ACX_OK) { std::free(m); return rc; }
            *out = m;
            *n_out = n;
            return ACX_OK;
        }
    }
    stop_resident(c); // (a small call that turned out dense: the pipeline has the context to itself)
    g_trace.begin();
    const uint8_t *d_hay = nullptr;
    rc = place_host_haystack(a, c, hay, len, &d_hay); // (pinned memory the scan reads in place, or the staging buffer)
    g_trace.lap(0);
    if (rc != ACX_OK) return rc;
    acx_result_t *r = nullptr;
    FindOpts opts;
    opts.allow_small = !try_small;
    opts.host_result = true;
    if ((rc = run_find(a, c, d_hay, len, Segments{nullptr, 1, 0}, overlapping, codepoints, &r, opts)) != ACX_OK) return rc;
    g_trace.lap(1);
    // (either way waits for the call's device work: the staging buffer is free again)
    rc = r->borrowed ? copy_borrowed(c, r, out, n_out) : download_matches(r, out, n_out);
    g_trace.lap(2);
    acx_free_result(r);
    g_trace.lap(3);
    return rc;
}

void acx_free_matches(acx_match_t *m) {
    if (!m) return;
    if (!g_pinned_results.put(m)) std::free(m);
}

int acx_find_batch(acx_automaton_t *a, const uint8_t *hay, const uint64_t *offsets, uint64_t n_hay,
                   int overlapping, int codepoints, acx_match_t **out, uint64_t *n_out,
                   uint64_t *counts) {
    if (!a || !out || !n_out || !offsets) return fail(ACX_EINVAL, "null argument");
    *out = nullptr; *n_out = 0;
    for (uint64_t i = 0; i < n_hay; i++) {
        if (offsets[i + 1] < offsets[i]) return fail(ACX_EINVAL, "offsets not monotone");
        if (counts) counts[i] = 0;
    }
    if (overlapping) {
        if (int rc = check_overlapping(a)) return rc; // (the error, no device state)
    }
    if (n_hay == 0) return ACX_OK;
    acx_result_t *r = nullptr;
    uint64_t base = offsets[0], len = offsets[n_hay] - base;
    std::vector<uint64_t> rel(n_hay + 1);
    for (uint64_t i = 0; i <= n_hay; i++) rel[i] = offsets[i] - base;
    Lease lease(a);
    Ctx *c = lease.c;
    if (!c) return fail(ACX_EDEVICE, "could not create a stream for the call");
    int rc = stage_host(a, c, hay ? hay + base : nullptr, len, rel.data(), n_hay + 1);
    if (rc == ACX_OK) {
        Segments G{c->ws.offsets, n_hay, 0};
        rc = run_find(a, c, c->ws.hay, len, G, overlapping, codepoints, &r);
    }
    if (rc != ACX_OK) return rc;
    rc = download_matches(r, out, n_out);
    if (counts && rc == ACX_OK) rc = acx_result_copy_counts(r, counts);
    if (rc != ACX_OK && *out) { acx_free_matches(*out); *out = nullptr; *n_out = 0; }
    acx_free_result(r);
    return rc;
}

void acx_shard_range(uint64_t n_items, int shard, int n_shards, uint64_t *lo, uint64_t *hi) {
    if (n_shards <= 0 || shard < 0 || shard >= n_shards) { // no such shard: the empty range
        if (lo) *lo = 0;
        if (hi) *hi = 0;
        return;
    }
    const uint64_t base = n_items / (uint64_t)n_shards, extra = n_items % (uint64_t)n_shards;
    const uint64_t s = (uint64_t)shard;
    *lo = s * base + std::min<uint64_t>(s, extra);
    *hi = *lo + base + (s < extra ? 1 : 0);
}

int acx_find_batch_multi(acx_automaton_t *const *handles, int n_handles, const uint8_t *hay,
                         const uint64_t *offsets, uint64_t n_hay, int overlapping, int codepoints,
                         acx_match_t **out, uint64_t *n_out, uint64_t *counts) {
    if (!handles || n_handles < 1 || !out || !n_out || !offsets) return fail(ACX_EINVAL, "null argument");
    for (int i = 0; i < n_handles; i++)
        if (!handles[i]) return fail(ACX_EINVAL, "null automaton");
    if (n_handles == 1) return acx_find_batch(handles[0], hay, offsets, n_hay, overlapping, codepoints, out, n_out, counts);
    *out = nullptr; *n_out = 0;
    // one host thread per handle, each on its contiguous range of haystacks (acx_shard_range: the
    // same split as distributed.shard_range, so the concatenation over shards is the batch in
    // order); the only thing combined afterwards are the shards' match counts (their exclusive
    // prefix = where a shard's matches go in the output)
    struct Shard { acx_match_t *m = nullptr; uint64_t n = 0; int rc = ACX_OK; std::string err; uint64_t lo = 0, hi = 0; };
    std::vector<Shard> sh((size_t)n_handles);
    std::vector<std::thread> th;
    for (int i = 0; i < n_handles; i++) {
        acx_shard_range(n_hay, i, n_handles, &sh[i].lo, &sh[i].hi);
        th.emplace_back([&, i] {
            Shard &s = sh[(size_t)i];
            s.rc = acx_find_batch(handles[i], hay, offsets + s.lo, s.hi - s.lo, overlapping, codepoints, &s.m, &s.n,
                                  counts ? counts + s.lo : nullptr);
            if (s.rc != ACX_OK) s.err = acx_last_error(); // (thread-local: carried to the caller's thread)
        });
    }
    for (auto &t : th) t.join();
    int rc = ACX_OK;
    uint64_t total = 0;
    for (auto &s : sh) {
        if (s.rc != ACX_OK && rc == ACX_OK) rc = fail(s.rc, s.err);
        total += s.n;
    }
    acx_match_t *all = nullptr;
    if (rc == ACX_OK && total) {
        all = (acx_match_t *)std::malloc(total * sizeof(acx_match_t));
        if (!all) rc = fail(ACX_ENOMEM, "out of memory");
    }
    uint64_t at = 0;
    for (auto &s : sh) {
        if (rc == ACX_OK && s.n) std::memcpy(all + at, s.m, s.n * sizeof(acx_match_t));
        at += s.n;
        acx_free_matches(s.m);
    }
    if (rc != ACX_OK) return rc;
    *out = all;
    *n_out = total;
    return ACX_OK;
}

int acx_profile_enable(acx_automaton_t *a, int on) {
    if (!a) return fail(ACX_EINVAL, "null automaton");
    a->prof = on != 0;
    a->prof_every = on > 1 ? on : 1;
    return ACX_OK;
}

int acx_profile_read(acx_automaton_t *a, acx_profile_t *out, int reset) {
    if (!a || !out) return fail(ACX_EINVAL, "null argument");
    {
        // settle the post-stage time of every context that is not in use right now
        DeviceScope scope(a->device);
        std::vector<Ctx *> idle;
        {
            std::lock_guard<std::mutex> lk(a->pool_mu);
            idle.swap(a->idle);
        }
        for (Ctx *c : idle) { settle_scan_profile(a, c); settle_post_profile(a, c); }
        {
            std::lock_guard<std::mutex> lk(a->pool_mu);
            a->idle.insert(a->idle.end(), idle.begin(), idle.end());
        }
        a->pool_cv.notify_all();
    }
    std::lock_guard<std::mutex> lk(a->prof_mu);
    *out = a->profile;
    if (reset) a->profile = acx_profile_t{};
    return ACX_OK;
}

int acx_path_stats(acx_automaton_t *a, uint64_t out[ACX_PATH_STATS], int reset) {
    if (!a || !out) return fail(ACX_EINVAL, "null argument");
    for (int i = 0; i < ACX_PATH_STATS; i++) out[i] = reset ? a->path[i].exchange(0) : a->path[i].load();
    return ACX_OK;
}

int acx_device_alloc(void **d_ptr, uint64_t bytes) {
    if (!d_ptr) return fail(ACX_EINVAL, "null argument");
    HIPCHK(hipMalloc(d_ptr, bytes ? bytes : 16));
    return ACX_OK;
}
int acx_device_free(void *d_ptr) { HIPCHK(hipFree(d_ptr)); return ACX_OK; }
int acx_device_upload(void *d_dst, const void *h_src, uint64_t bytes) {
    if (bytes) HIPCHK(hipMemcpy(d_dst, h_src, bytes, hipMemcpyHostToDevice));
    return ACX_OK;
}
int acx_device_download(void *h_dst, const void *d_src, uint64_t bytes) {
    if (bytes) HIPCHK(hipMemcpy(h_dst, d_src, bytes, hipMemcpyDeviceToHost));
    return ACX_OK;
}
int acx_device_synchronize(void) { HIPCHK(hipDeviceSynchronize()); return ACX_OK; }
int acx_device_synchronize_on(int device) {
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(ACX_EINVAL, "device ordinal out of range");
    DeviceScope ds(device);
    HIPCHK(hipDeviceSynchronize());
    return ACX_OK;
}

int acx_generate_haystack(acx_automaton_t *a, void *d_dst, uint64_t len, int kind, uint64_t seed,
                          uint64_t stream_offset) {
    if (!a || (!d_dst && len)) return fail(ACX_EINVAL, "null argument");
    if (kind != 0 && kind != 1) return fail(ACX_EINVAL, "unknown haystack kind");
    if (kind == 1 && (stream_offset % 1024)) return fail(ACX_EINVAL, "stream_offset must be a multiple of 1024");
    Lease lease(a);
    if (!lease.c) return fail(ACX_EDEVICE, "could not create a stream for the call");
    HIPCHK(generate(a->dev, (uint8_t *)d_dst, len, kind, seed, stream_offset, lease.c->stream));
    HIPCHK(hipStreamSynchronize(lease.c->stream));
    return ACX_OK;
}

} // extern "C"
