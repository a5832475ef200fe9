// find_pipeline.cpp -- one find call from a device haystack to its result: K0 or the general pipeline (find_attempts.cpp), the
// expansion of pattern copies, and the calls that one pass cannot index -- a haystack in byte ranges, a batch in two parts.
#include "find_pipeline.hpp"

#include "find_attempts.hpp"
#include "small_calls.hpp"

namespace acxh ACX_HIDDEN {

int check_overlapping(const acx_automaton *a) {
    if (a->host.match_kind == ACX_MATCH_STANDARD) return ACX_OK;
    static const char *names[3] = {"Standard", "LeftmostFirst", "LeftmostLongest"};
    return fail(ACX_EOVERLAP, std::string("match kind ") + names[a->host.match_kind] +
                                  " does not support overlapping searches");
}

int make_segments(const uint64_t *d_offsets, uint64_t n_hay, uint64_t uniform_len, uint64_t len, Segments *G) {
    *G = Segments{nullptr, 1, 0};
    if (uniform_len) {
        if (n_hay * uniform_len != len) return fail(ACX_EINVAL, "n_hay * uniform_len != len");
        G->uniform_len = uniform_len; G->n_hay = n_hay;
    } else if (d_offsets) {
        G->offsets = d_offsets; G->n_hay = n_hay;
    }
    return ACX_OK;
}

// post_ms of the previous profiled call: ev[1] (end of the scan) .. ev[2] (end of the call's device work)
void settle_post_profile(acx_automaton *a, Ctx *c) {
    if (!c->post_pending) return;
    c->post_pending = false;
    float ms = 0;
    hipEvent_t scan_end = c->ev[(c->ev_pair ^ 1) ? 4 : 1]; // the pair the last launch took
    if (hipEventSynchronize(c->ev[2]) == hipSuccess && hipEventElapsedTime(&ms, scan_end, c->ev[2]) == hipSuccess) {
        std::lock_guard<std::mutex> lk(a->prof_mu);
        a->profile.post_ms += ms;
    }
}

// the scan time of the last profiled launch of this context, if it has not been read yet
void settle_scan_profile(acx_automaton *a, Ctx *c) {
    if (!c->scan_pending) return;
    c->scan_pending = false;
    float ms = 0;
    hipEvent_t e0 = c->ev[c->pend_pair ? 3 : 0], e1 = c->ev[c->pend_pair ? 4 : 1];
    if (hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess) return;
    std::lock_guard<std::mutex> lk(a->prof_mu);
    a->profile.scan_ms += ms;
    a->profile.scan_launches++;
    a->profile.scan_bytes += c->pend_len;
}

int result_wait(const acx_result *r) {
    if (r && r->done) {
        DeviceScope ds(r->device);
        HIPCHK(hipEventSynchronize(r->done));
    }
    return ACX_OK;
}

// Overlapping search over a set with copies of a string: the pipeline ran on the view without the later copies (one
// occurrence per string, lowest id); every occurrence becomes the run of its string's copies, ids ascending -- the order
// the reference reports them in (one state's match list, in the order the patterns were added).  In place of r->d_matches;
// batch: the per-haystack counts follow.  One round trip (the number of records).
int expand_copies(acx_automaton *a, Ctx *x, acx_result *r, bool segmented) {
    const uint64_t n = r->n;
    if (!n) return ACX_OK;
    hipStream_t st = x->stream;
    Workspace &w = x->ws;
    int rc = ensure_common(x);
    if (rc) return rc;
    const uint64_t n_hay = segmented ? r->n_hay : 0;
    const size_t tb = scan_temp_bytes(std::max(n, n_hay) + 1) + 256;
    void *temp = nullptr;
    uint64_t *k = nullptr, *offs = nullptr, *incl = nullptr;
    acx_match_t *out = nullptr;
    auto done = [&](int code) -> int {
        (void)hipStreamSynchronize(st); // (the scratch goes back to the pool: nothing may still use it)
        g_bufs.put(temp, a->device); g_bufs.put(k, a->device); g_bufs.put(offs, a->device); g_bufs.put(incl, a->device);
        g_bufs.put(out, a->device);
        return code;
    };
    HIPCHK(g_bufs.get(&temp, tb, a->device));
    if (hipError_t e = g_bufs.get((void **)&k, (n + 1) * 8, a->device); e != hipSuccess) return done(hipfail(e, "expand_copies"));
    if (hipError_t e = g_bufs.get((void **)&offs, (n + 1) * 8, a->device); e != hipSuccess) return done(hipfail(e, "expand_copies"));
    hipError_t e = copy_runs(r->d_matches, n, a->d_xcnt, temp, tb, k, offs, st);
    if (e == hipSuccess) e = hipMemcpyAsync(w.h_pinned + PIN_EXPANDED, offs + n, 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return done(hipfail(e, "expand_copies"));
    const uint64_t total = w.h_pinned[PIN_EXPANDED];
    if (total == n) return done(ACX_OK); // (no occurrence of a string with copies)
    if ((e = g_bufs.get((void **)&out, total * sizeof(acx_match_t), a->device)) != hipSuccess) return done(hipfail(e, "expand_copies"));
    e = expand_copies_write(r->d_matches, n, offs, a->d_xoff, a->d_xids, out, total, st);
    if (e == hipSuccess && n_hay) {
        if ((e = g_bufs.get((void **)&incl, n_hay * 8, a->device)) == hipSuccess)
            e = expand_copies_counts(temp, tb, r->d_counts, n_hay, incl, offs, st);
    }
    if (e != hipSuccess) return done(hipfail(e, "expand_copies"));
    std::swap(out, r->d_matches); // (the unexpanded buffer goes back to the pool with the scratch)
    r->n = total;
    return done(ACX_OK);
}

// (the same on the host, for K0's result of the host entry point: *m is replaced when a string with copies occurs)
int expand_copies_host(const acx_automaton *a, acx_match_t **m, uint64_t *n) {
    const acx_match_t *src = *m;
    uint64_t total = 0;
    for (uint64_t i = 0; i < *n; i++) total += 1 + a->x_cnt[src[i].pattern];
    if (total == *n) return ACX_OK;
    acx_match_t *m2 = (acx_match_t *)std::malloc(total * sizeof(acx_match_t));
    if (!m2) return fail(ACX_ENOMEM, "out of memory");
    uint64_t at = 0;
    for (uint64_t i = 0; i < *n; i++) {
        m2[at++] = src[i];
        const uint32_t *ids = a->x_ids.data() + a->x_off[src[i].pattern];
        for (uint32_t q = 0; q < a->x_cnt[src[i].pattern]; q++) { m2[at] = src[i]; m2[at++].pattern = ids[q]; }
    }
    std::free(*m);
    *m = m2;
    *n = total;
    return ACX_OK;
}

namespace {
int run_chunked(acx_automaton *a, Ctx *x, const uint8_t *d_hay, uint64_t len, int overlapping, int codepoints,
                acx_result **out, uint64_t piece, int depth);
int run_batch_split(acx_automaton *a, Ctx *x, const uint8_t *d_hay, uint64_t len, const Segments &G, int overlapping,
                    int codepoints, acx_result **out, int depth);
} // namespace

int run_find(acx_automaton *a, Ctx *x, const uint8_t *d_hay, uint64_t len, const Segments &G, int overlapping, int codepoints,
             acx_result **out, const FindOpts &o) {
    *out = nullptr;
    const bool allow_small = o.allow_small, wait = o.wait;
    const int depth = o.depth;
    if (overlapping) {
        if (int rc = check_overlapping(a)) return rc;
    }
    if (len >= (1ull << 38)) return fail(ACX_ETOOBIG, "haystack stream of 2^38 bytes or more");
    if (!x) return fail(ACX_EDEVICE, "could not create a stream for the call");
    settle_post_profile(a, x);
    hipStream_t st = x->stream;
    const bool segmented = is_segmented(G);
    acx_result *r = new (std::nothrow) acx_result(a->device);
    if (!r) return fail(ACX_ENOMEM, "out of memory");
    r->n_hay = segmented ? G.n_hay : 0;
    FindCall c{a, x, d_hay, len, G, overlapping != 0, codepoints != 0, segmented, r,
               overlapping ? 0 : a->host.match_kind};
    c.host_result = o.host_result;
    auto body = [&]() -> int {
        if (segmented) {
            HIPCHK(g_bufs.get((void **)&r->d_counts, std::max<uint64_t>(G.n_hay, 1) * 8, a->device));
        }
        if (allow_small && !segmented && small_ok(a, len)) { // small haystack: the whole call in one workgroup (K0)
            HIPCHK(g_bufs.get((void **)&r->d_matches, SMALL_MAX_OCC * sizeof(acx_match_t), a->device));
            bool done = false;
            int rc = run_small(a, x, d_hay, len, overlapping, codepoints, r->d_matches, &r->n, &done);
            if (rc) return rc;
            if (done) return overlapping && a->expand_ov ? expand_copies(a, x, r, false) : ACX_OK;
            g_bufs.put(r->d_matches, a->device); // dense: the general pipeline takes over
            r->d_matches = nullptr;
        }
        if (len > 0 && a->host.n_patterns > 0) {
            int rc = run_pipeline(c);
            if (rc) return rc;
            if (overlapping && a->expand_ov) { // (copies of a string: the view reported the lowest ids)
                if ((rc = expand_copies(a, x, r, segmented)) != ACX_OK) return rc;
                c.queued = false; // (synchronised)
            }
        } else {
            // nothing to scan (a batch of empty haystacks, or no patterns): the per-haystack counts come
            // out of the buffer cache uninitialised -- they are this call's to clear
            int rc = zero_counts(c);
            if (rc) return rc;
        }
        if (c.queued) {
            // the totals are known; what is still running (the write kernel, the fix-ups) is fenced
            // by an event the result's accessors wait for
            if (wait) {
                HIPCHK(hipStreamSynchronize(st));
            } else {
                if (!r->done) r->done = g_events.get(a->device);
                if (!r->done) HIPCHK(hipStreamSynchronize(st));
                else HIPCHK(hipEventRecord(r->done, st)); // (again, if a fix-up was queued behind an early record)
            }
        }
        return ACX_OK;
    };
    c.early_event = !wait;
    c.timed = a->prof && (a->prof_every <= 1 || (x->prof_calls++ % (uint32_t)a->prof_every) == 0);
    // (tests: ACX_CHUNK_BYTES cuts every one-haystack call longer than that, whatever it holds)
    const char *cb = depth == 0 && !segmented ? std::getenv("ACX_CHUNK_BYTES") : nullptr;
    const uint64_t forced = cb ? std::strtoull(cb, nullptr, 10) : 0;
    int rc = forced && len > forced ? TOO_MANY_OCC : body();
    if (rc != ACX_OK) {
        (void)hipStreamSynchronize(st);
        acx_free_result(r);
        if (rc != TOO_MANY_OCC) return rc;
        // more occurrences than one pass can index: the haystack in byte ranges, one after the other -- a batch in two parts,
        // cut at a haystack boundary, where nothing has to be carried over (round 6; until then the error was the caller's)
        const uint64_t m = a->host.max_len ? a->host.max_len - 1 : 0;
        const uint64_t piece = forced && len > forced ? forced : len / 2;
        if (segmented && depth < 40) return run_batch_split(a, x, d_hay, len, G, overlapping, codepoints, out, depth + 1);
        if (segmented || depth >= 40 || piece <= 2 * m + 16)
            return fail(ACX_ETOOBIG, "more than 2^32 occurrences");
        return run_chunked(a, x, d_hay, len, overlapping, codepoints, out, piece, depth + 1);
    }
    *out = r;
    return ACX_OK;
}

namespace {

// A batch whose occurrences one pass cannot index (2^32, the width of the device's indexes): its haystacks in two parts,
// searched one after the other on the same context -- each part again a batch (or, a part of ONE haystack, a call of its
// own, which may go on in byte ranges) -- and the parts' matches (offsets are local to their haystack: nothing to shift)
// and per-haystack counts put behind one another.  The reference's loop has no limit (/root/reference/src/lib.rs:53, 59).
int run_batch_split(acx_automaton *a, Ctx *x, const uint8_t *d_hay, uint64_t len, const Segments &G, int overlapping,
                    int codepoints, acx_result **out, int depth) {
    *out = nullptr;
    hipStream_t st = x->stream;
    Workspace &w = x->ws;
    const uint64_t n = G.n_hay;
    a->path[8]++;
    FindOpts part_opts; // (a part waits for its device work: its buffers are copied from and given back here)
    part_opts.wait = true;
    part_opts.depth = depth;
    auto one_haystack = [&](const uint8_t *h, uint64_t hl, acx_result **r) -> int { // a part of one haystack: its count is its matches
        int rc = run_find(a, x, h, hl, Segments{nullptr, 1, 0}, overlapping, codepoints, r, part_opts);
        if (rc != ACX_OK) return rc;
        hipError_t e = g_bufs.get((void **)&(*r)->d_counts, 8, a->device);
        if (e == hipSuccess) e = hipMemcpyAsync((*r)->d_counts, &(*r)->n, 8, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) { acx_free_result(*r); *r = nullptr; return hipfail(e, "count of a one-haystack part"); }
        (*r)->n_hay = 1;
        return ACX_OK;
    };
    if (n <= 1) return one_haystack(d_hay, len, out);
    const uint64_t half = n / 2;
    uint64_t cut = 0; // the first byte of haystack `half`
    uint64_t *reb = nullptr; // the second part's offsets, from its first byte
    if (G.uniform_len) {
        cut = half * G.uniform_len;
    } else {
        HIPCHK(hipMemcpyAsync(w.h_pinned + PIN_SPLIT_CUT, G.offsets + half, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        cut = w.h_pinned[PIN_SPLIT_CUT];
        HIPCHK(g_bufs.get((void **)&reb, (n - half + 1) * 8, a->device));
        hipError_t e = rebase_offsets(reb, G.offsets + half, n - half + 1, cut, st);
        if (e != hipSuccess) { g_bufs.put(reb, a->device); return hipfail(e, "rebase_offsets"); }
    }
    acx_result *ra = nullptr, *rb = nullptr;
    auto part = [&](const uint8_t *h, uint64_t hl, const uint64_t *offs, uint64_t k, acx_result **r) -> int {
        if (k == 1) return one_haystack(h, hl, r);
        const Segments S{G.uniform_len ? nullptr : offs, k, G.uniform_len};
        return run_find(a, x, h, hl, S, overlapping, codepoints, r, part_opts);
    };
    int rc = part(d_hay, cut, G.offsets, half, &ra);
    if (rc == ACX_OK) rc = part(d_hay + cut, len - cut, reb, n - half, &rb);
    acx_result *r = rc == ACX_OK ? new (std::nothrow) acx_result(a->device) : nullptr;
    if (rc == ACX_OK && !r) rc = fail(ACX_ENOMEM, "out of memory");
    if (rc == ACX_OK) {
        r->n_hay = n;
        r->n = ra->n + rb->n;
        hipError_t e = g_bufs.get((void **)&r->d_counts, n * 8, a->device);
        if (e == hipSuccess && r->n) e = g_bufs.get((void **)&r->d_matches, r->n * sizeof(acx_match_t), a->device);
        if (e == hipSuccess) e = hipMemcpyAsync(r->d_counts, ra->d_counts, half * 8, hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(r->d_counts + half, rb->d_counts, (n - half) * 8, hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess && ra->n) e = hipMemcpyAsync(r->d_matches, ra->d_matches, ra->n * sizeof(acx_match_t), hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess && rb->n) e = hipMemcpyAsync(r->d_matches + ra->n, rb->d_matches, rb->n * sizeof(acx_match_t), hipMemcpyDeviceToDevice, st);
        if (e != hipSuccess) rc = hipfail(e, "result of a batch in two parts");
    }
    hipError_t e2 = hipStreamSynchronize(st); // (the parts' buffers go back to the pool: nothing may still read them)
    if (rc == ACX_OK && e2 != hipSuccess) rc = hipfail(e2, "a batch in two parts");
    if (ra) acx_free_result(ra);
    if (rb) acx_free_result(rb);
    if (reb) g_bufs.put(reb, a->device);
    if (rc != ACX_OK) { if (r) acx_free_result(r); return rc; }
    *out = r;
    return ACX_OK;
}

// One haystack in byte ranges of `piece` bytes, searched one after the other; the pieces' matches, cut where the ranges
// meet, are copied into one result with global offsets.  The reference's loop has no limit on what it reports
// (/root/reference/src/lib.rs:53, 59: an iterator); one pass here has -- 2^32 occurrences, the width of the device's
// indexes.  What couples the ranges is what couples the ranks of a sharded haystack (distributed.py):
//   overlapping      a range reports the occurrences that END in (lo, hi]; it is scanned from max_len - 1 bytes before lo;
//   non-overlapping  a range reports the matches that START in [carry, hi): the iteration resumes at `carry`, the end of
//                    the last match in front (or lo); a match that starts before hi ends at most max_len - 1 bytes behind
//                    it, so the scan stops there, and nothing the truncated window hides beats what it shows.
// Code points (str API): the pieces run on byte offsets, the conversion runs once over the whole result.
int run_chunked(acx_automaton *a, Ctx *x, const uint8_t *d_hay, uint64_t len, int overlapping, int codepoints,
                acx_result **out, uint64_t piece, int depth) {
    *out = nullptr;
    hipStream_t st = x->stream;
    Workspace &w = x->ws;
    const uint64_t m = a->host.max_len ? a->host.max_len - 1 : 0;
    struct Piece { acx_match_t *buf; uint64_t first, n, shift; };
    std::vector<Piece> pieces;
    auto drop = [&]() { for (auto &p : pieces) g_bufs.put(p.buf, a->device); pieces.clear(); };
    uint64_t total = 0, carry = 0;
    if (int rc = ensure_common(x)) return rc; // (the context's scratch: the first call of a context may be this one)
    FindOpts piece_opts; // (a piece waits for its device work: its matches are cut and copied here)
    piece_opts.wait = true;
    piece_opts.depth = depth;
    uint64_t *cut = w.summary + SCR_RANGE_CUT; // (two device words of the context's scratch)
    for (uint64_t lo = 0; lo < len;) {
        const uint64_t hi = std::min(len, lo + piece);
        const bool last = hi == len;
        uint64_t a0, a1;
        if (overlapping) { a0 = lo > m ? lo - m : 0; a1 = hi; }
        else { carry = std::max(carry, lo); a0 = carry; a1 = last ? len : std::min(len, hi + m); }
        if (a0 >= hi) { lo = hi; continue; } // (a match from the ranges in front covers this one)
        acx_result *r = nullptr;
        a->path[8]++;
        int rc = run_find(a, x, d_hay + a0, a1 - a0, Segments{nullptr, 1, 0}, overlapping, 0, &r, piece_opts);
        if (rc != ACX_OK) { drop(); return rc; }
        uint64_t first = 0, n = r->n, last_end = 0;
        if (n && ((overlapping && lo > 0) || (!overlapping && !last))) {
            // overlapping: the occurrences that end at or before lo belong to the range in front (a prefix: ordered by
            // end); non-overlapping: the matches that start at or behind hi to the next one (a suffix: ordered by start)
            hipError_t e = overlapping ? cut_point(r->d_matches, n, true, a0, lo + 1, cut, st)
                                       : cut_point(r->d_matches, n, false, a0, hi, cut, st);
            if (e == hipSuccess) e = hipMemcpyAsync(w.h_pinned + PIN_RANGE_CUT, cut, 16, hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            if (e != hipSuccess) { acx_free_result(r); drop(); return hipfail(e, "cut of a byte range"); }
            if (overlapping) first = w.h_pinned[PIN_RANGE_CUT];
            else { n = w.h_pinned[PIN_RANGE_CUT]; last_end = w.h_pinned[PIN_RANGE_CUT + 1]; }
        } else if (n && !overlapping) {
            last_end = len; // (the last range: nothing follows)
        }
        if (n > first) {
            pieces.push_back(Piece{r->d_matches, first, n - first, a0});
            r->d_matches = nullptr; // (ours now)
            total += n - first;
        }
        acx_free_result(r);
        if (!overlapping) carry = std::max(std::max(carry, hi), last_end);
        lo = hi;
    }
    acx_result *r = new (std::nothrow) acx_result(a->device);
    if (!r) { drop(); return fail(ACX_ENOMEM, "out of memory"); }
    r->n = total;
    auto body = [&]() -> int {
        if (!total) return ACX_OK;
        hipError_t e = g_bufs.get((void **)&r->d_matches, total * sizeof(acx_match_t), a->device);
        if (e != hipSuccess) return hipfail(e, "result of a call in byte ranges");
        uint64_t at = 0;
        for (auto &p : pieces) {
            if ((e = copy_shifted(r->d_matches + at, p.buf + p.first, p.n, p.shift, st)) != hipSuccess) return hipfail(e, "copy_shifted");
            at += p.n;
        }
        if (codepoints) {
            const Segments one{nullptr, 1, 0};
            FindCall c{a, x, d_hay, len, one, overlapping != 0, true, false, r, 0};
            c.n_final = total;
            int rc = finish_matches(c);
            if (rc) return rc;
        }
        return ACX_OK;
    };
    int rc = body();
    hipError_t e = hipStreamSynchronize(st); // (the pieces' buffers go back to the pool: nothing may still read them)
    drop();
    if (rc == ACX_OK && e != hipSuccess) rc = hipfail(e, "a call in byte ranges");
    if (rc != ACX_OK) { acx_free_result(r); return rc; }
    *out = r;
    return ACX_OK;
}

} // namespace

} // namespace acxh
