// find_attempts.cpp -- the device pipeline of one find call on an allocated result: the sparse attempt (hit slots + tile
// kernels, the hot pipeline for the groups they cannot finish), the two dense forms, and what follows the matches
// (code points, per-haystack offsets and counts).  find_attempts.hpp: FindCall, run_pipeline.
#include "find_attempts.hpp"

#include "small_calls.hpp"

namespace acxh ACX_HIDDEN {

// ---------------------------------------------------------------------------
// The device pipeline.  d_hay: device pointer, len bytes.
//
//   small haystack:          K0, the whole call in one workgroup                 one launch
//   sparse output (default): scan (K1b: prefix hits / K1a: occurrences) into per-tile hit slots ->
//                            k_tile_main (verify, order, match kind) -> k_tile_write (output offsets, final records);
//                            the host returns as soon as the scan kernel has published the totals
//   dense output:            scan emits into regions -> (walk) -> compact -> radix sort -> spans ->
//                            resolve -> offsets -> write                         (two round trips)
// ---------------------------------------------------------------------------

namespace {

int bits_for(uint64_t x) { // number of bits needed to represent x
    int b = 0;
    while (x) { b++; x >>= 1; }
    return b;
}

inline hipEvent_t scan_start_ev(Ctx *c) { return c->ev[c->ev_pair ? 3 : 0]; }
inline hipEvent_t scan_stop_ev(Ctx *c) { return c->ev[c->ev_pair ? 4 : 1]; }

// the scan just launched with the current pair of events: its time is read later (the next launch
// of this context takes the other pair)
void add_scan_profile(acx_automaton *a, Ctx *c, uint64_t len, bool timed) {
    if (!timed) return;
    settle_scan_profile(a, c); // (normally settled already, behind this call's own launches)
    c->scan_pending = true;
    c->pend_pair = c->ev_pair;
    c->pend_len = len;
    c->ev_pair ^= 1;
}

enum class Attempt { Done, GoDense, Again };

// ---- sparse output, groups the tile kernels could not finish (a dense stretch of the input: more hits than a tile's
// slots, a full bucket, more matches than a group's stretch, an uncertifiable chain): the HOT pipeline -- the hot
// groups' hits (slots + overflow list) through the tile-ordered dense machinery, their counts credited to the sparse
// path's groups, then the write kernel again.  One dense region costs the groups it lies in, not the call (it used to
// send the whole call to the dense path and keep the handle there for eight more calls).  *lost: the hot pipeline gave
// up too (a bucket of more than DT_SLOTS occurrences, a chain longer than the context) -- the radix-sort form takes the call.
constexpr uint64_t PIN_FINAL_MAX = 32ull << 20; // bytes of pinned result buffer a context keeps for host calls (acx_find up to ~8 MiB)
// hot groups whose capacity the output buffer has room for anyway: 16 to start with, up to 128 for a context that has seen more
// (Ctx::hot_inline; round 6 -- until then 128 for every call: ~100 MB per result from 32 MiB haystacks on, whatever the input);
// beyond a context's figure: hot_totals, then a buffer of the exact size
constexpr uint64_t HOT_INLINE = 16, HOT_INLINE_MAX = 128;
int run_hot(FindCall &c, uint32_t *abort_flag, uint64_t seq, uint32_t n_hot, uint32_t ovf_max, uint64_t *seg_counts,
            const uint64_t *cp_pre, bool counts_clear, bool *lost) {
    acx_automaton *a = c.a;
    Ctx *x = c.c;
    Workspace &w = x->ws;
    hipStream_t st = x->stream;
    TileSpace &T = w.T;
    *lost = false;
    if (ensure_dense_tiles(x, c.tiles) != ACX_OK) { // (no room for the buckets: the radix-sort form needs less)
        (void)hipGetLastError();
        free_dense_tiles(w);
        c.no_dense_tiles = true;
        *lost = true;
        return ACX_OK;
    }
    uint32_t *hot_abort = (uint32_t *)(w.summary + 10);
    // (the bucket counters and the pipeline's abort flag, summary[10]: cleared by the write kernel that announced the hot
    // groups -- unless the buckets are allocated by this very call)
    if (!counts_clear) HIPCHK(hipMemsetAsync(w.dt.counts, 0, ((uint64_t)w.dt.n_tiles + 1) * 4, st));
    HIPCHK(hot_verify_main(view(a, c.overlapping), c.key_mode, c.overlapping, c.G, T, w.hot_list, n_hot, abort_flag, ovf_max,
                              w.dt, w.TD, c.lead, c.d_hay, c.len, hot_abort, seq, 0, st));
    // the output's room: the groups' capacities bound the matches; with many hot groups the buffer is sized exactly
    // instead (one more round trip, next to that much hot work)
    const uint64_t bound = ((uint64_t)T.n_groups - n_hot) * T.gmax + (uint64_t)n_hot * HOT_SUB * DT_GMAX;
    if (bound > c.out_cap && c.out != w.final) { // (the pinned buffer is not regrown: the dense path takes this call)
        *lost = true;
        return ACX_OK;
    }
    if (bound > w.final_cap && c.out == w.final) {
        const uint64_t pub_t = seq | (1ull << 62);
        HIPCHK(hot_totals(T, seq, w.h_pinned + PIN_HOT_TOTALS, pub_t, st));
        uint64_t early[8];
        int rc = wait_line(x, PIN_HOT_TOTALS, pub_t, early, "the hot pipeline did not publish its total");
        if (rc) return rc;
        const uint64_t n = std::min<uint64_t>(early[1], bound); // (meaningless when the pipeline gave up: bounded all the same)
        if (n >= occ_limit()) {
            // (the call goes on in byte ranges on this context: the control blocks and both sets of supergroup words clear again)
            w.flags_dirty = true;
            HIPCHK(hipStreamSynchronize(st));
            HIPCHK(hipMemsetAsync(T.sgw, 0, 4 * (uint64_t)T.sg_cap * 8, st));
            return fail_occ();
        }
        if (n > w.final_cap) {
            HIPCHK(hipStreamSynchronize(st));
            g_bufs.put(w.final, a->device);
            w.final = nullptr; w.final_cap = 0;
            HIPCHK(g_bufs.get((void **)&w.final, n * sizeof(acx_match_t), a->device));
            w.final_cap = n;
            c.out = w.final; c.out_cap = n;
        }
    }
    // an input that is dense (nearly) everywhere: the dense path proper takes the handle's next calls -- its scan writes
    // the hits where its verification reads them, no sparse attempt in front
    if ((uint64_t)n_hot * 4 > T.n_groups && T.n_groups >= 8) { x->dense_hold = 8; x->hold_dense_input = true; }
    const uint64_t pub = seq | (1ull << 63);
    HIPCHK(hot_write(view(a, c.overlapping), c.key_mode, T, w.TD, w.hot_list, n_hot, c.lead, c.d_hay, c.out, w.summary,
                        abort_flag, hot_abort, w.h_pinned + PIN_TOTALS, seq, pub, c.G, seg_counts, cp_pre, w.blocksub, 0, st));
    if (c.early_event && c.r->done) HIPCHK(hipEventRecord(c.r->done, st)); // (again: behind the kernels queued since)
    int rc = wait_line(x, PIN_TOTALS, pub, w.t_line, "the write kernel did not publish its totals");
    if (rc) return rc;
    if ((w.t_line[4] & 0xFF) != 0) {
        c.no_dense_tiles = true;
        *lost = true;
    }
    return ACX_OK;
}

// ---- sparse output: hit slots + tile kernels; returns when the totals are known
int attempt_sparse(FindCall &c, Attempt *what) {
    acx_automaton *a = c.a;
    Ctx *x = c.c;
    Workspace &w = x->ws;
    hipStream_t st = x->stream;
    // (the wide form of the post stage: K1b's hits only -- the hot pipeline behind it is theirs)
    static const bool force_wide = std::getenv("ACX_FORCE_WIDE") != nullptr; // tests: every K1b call in the wide form
    const bool wide = (x->wide || force_wide) && c.pre;
    const uint32_t gmax = wide ? GROUP_MAX_WIDE : GROUP_MAX;
    int rc = ensure_tiles(a, x, c.tiles, gmax);
    if (rc) return rc;
    TileSpace &T = w.T;
    // automata of at most 32 byte classes: the failureless walk (k1a_scan + k1a_walk) instead of the
    // chunked one (ACX_NO_PFAC: always the chunked walk -- measurements)
    static const bool no_pfac = std::getenv("ACX_NO_PFAC") != nullptr;
    const bool pfac = !c.pre && pfac_available(a->dev, a->max_lds) && !no_pfac;
    const uint32_t pgrid = pfac ? pfac_scan_grid(c.d_hay, c.len, a->n_cus) : 0;
    // hit counts: contiguous per wave of the scan (K1b, k1a_scan); the chunked walk: plain per-tile
    // arrival counters
    T.cnt_nw = c.pre ? c.scan_grid * 16 : pfac ? pgrid * 16 : 1;
    T.cnt_iters = T.cnt_nw > 1 ? (uint32_t)((c.tiles + T.cnt_nw - 1) / T.cnt_nw) : (uint32_t)c.tiles;
    // (room for every group's capacity + what a few hot groups can report beyond it: run_hot)
    // (a host call's records go to the CONTEXT's pinned buffer, which is not regrown in the middle of a call: there the room
    // for hot groups is the full figure while the whole fits PIN_FINAL_MAX; a device result's buffer is the caller's to hold:
    // the context's own figure)
    auto cap_for = [&](uint64_t hot_room) {
        return (uint64_t)T.n_groups * gmax + (c.pre ? std::min<uint64_t>(T.n_groups, hot_room) * HOT_SUB * DT_GMAX : 0);
    };
    const bool pin = c.host_result && !c.segmented && cap_for(HOT_INLINE_MAX) * sizeof(acx_match_t) <= PIN_FINAL_MAX &&
                     !(c.overlapping && a->expand_ov);
    const uint64_t out_cap = cap_for(pin ? HOT_INLINE_MAX : x->hot_inline);
    if (pin && w.pin_final.cap < out_cap) {
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(w.pin_final.grow(out_cap, hipHostMallocDefault));
    }
    if (pin) {
        c.out = w.pin_final; c.out_cap = w.pin_final.cap;
    } else {
        if (w.final && w.final_cap < out_cap) { g_bufs.put(w.final, a->device); w.final = nullptr; }
        if (!w.final) {
            HIPCHK(g_bufs.get((void **)&w.final, out_cap * sizeof(acx_match_t), a->device));
            w.final_cap = out_cap;
        }
        c.out = w.final; c.out_cap = w.final_cap;
    }
    if (w.flags_dirty) {
        HIPCHK(hipMemsetAsync(w.ctl, 0, 12, st));
        HIPCHK(hipMemsetAsync(w.ctl + CTL_WORDS, 0, 12, st));
        HIPCHK(hipMemsetAsync(w.ovf_counts, 0, 2 * OVF_LISTS * OVF_COUNT_STRIDE * 4, st));
    }
    w.flags_dirty = true;
    // two control blocks used in turn: this attempt's write kernel clears the other one
    uint32_t *abort_flag = w.ctl + CTL_WORDS * x->flag_idx;
    uint32_t *next_flag = w.ctl + CTL_WORDS * (x->flag_idx ^ 1);
    x->flag_idx ^= 1;
    const Sink K{nullptr, nullptr, 0, c.key_mode, T.hslots, T.hcnt, abort_flag, c.lead, T.cnt_nw, T.cnt_iters};
    // batch with byte offsets: the write kernel localises and counts per haystack itself
    uint64_t *seg_counts = c.segmented && !c.codepoints ? c.r->d_counts : nullptr;
    const bool prof = c.timed;
    hipEvent_t side_after = nullptr;
    if (c.pre) {
        // str API: the scan counts the UTF-8 lead bytes on its way (aligned haystacks: the blocks of
        // the code-point prefix are then the rows of the scan's tiles)
        uint8_t *cp_sub = nullptr;
        if (c.codepoints && c.lead == 0) {
            if ((rc = ensure_blocks(x, 4 * c.tiles + 1)) != ACX_OK) return rc;
            cp_sub = w.blocksub;
        }
        // measurement: the event pair rides on the dispatch
        // (str API, one haystack: the code-point prefix runs on the second stream as soon as the scan
        // is done -- the event it waits for rides on the scan's own dispatch, no packet in between)
        side_after = cp_sub && !c.segmented ? (prof ? scan_stop_ev(x) : x->fork_ev) : nullptr;
        g_trace.mark(2);
        HIPCHK(launch_prefilter(a->dev, K, c.d_hay, c.len, c.scan_grid, st, prof ? scan_start_ev(x) : nullptr,
                                   prof ? scan_stop_ev(x) : side_after, cp_sub));
        g_trace.mark(3);
        c.leads_counted = cp_sub != nullptr;
    } else {
        // the failureless walk: the scan writes the hits it settles itself and every tile's count, the
        // walk appends to them; its survivor records take the place of K1b's dense-path hit sink.  More
        // survivors than their regions hold (1 per 16 haystack bytes): the walk raises the abort flag, the
        // call is redone on the dense path, which walks in chunks.
        if (!pfac) HIPCHK(hipMemsetAsync(T.hcnt, 0, (c.tiles + 1) * 4, st)); // arrival counters of the walk's emission
        uint64_t surv_total = 0;
        if (pfac) {
            surv_total = pfac_workspace_words(c.len, pgrid, false);
            if ((rc = ensure_hits(x, (surv_total + 3) / 4)) != ACX_OK) return rc; // (records of 32 B there, u64 words here)
        }
        if (prof) HIPCHK(hipEventRecord(scan_start_ev(x), st));
        if (pfac)
            HIPCHK(launch_pfac(view(a, c.overlapping), d_view(a, c.overlapping), c.G, K, c.d_hay, c.len, pgrid, (uint64_t *)w.hrecs.p, w.hit_counts,
                                  pgrid * 16, false, st));
        else
            HIPCHK(launch_dfa_walk(view(a, c.overlapping), d_view(a, c.overlapping), c.G, K, c.d_hay, c.len, c.scan_grid, a->max_lds, st));
        if (prof) HIPCHK(hipEventRecord(scan_stop_ev(x), st));
    }
    // str API, one haystack: the prefix of the lead-byte counts is ready before the write kernel
    // needs it (it depends on the scan only), so the write kernel converts on the way out
    // (three small latency-bound kernels, ~30 us: on the context's second stream, beside k_tile_main,
    // which does not need them; the write kernel waits for both)
    const uint64_t *cp_pre = nullptr;
    hipEvent_t before_write = nullptr;
    if (c.leads_counted && !c.segmented) {
        const uint64_t nb1 = (c.len + 1023) / 1024 + 1;
        hipStream_t side = x->copy_stream;
        if (!side_after) { side_after = x->fork_ev; HIPCHK(hipEventRecord(x->fork_ev, st)); }
        HIPCHK(hipStreamWaitEvent(side, side_after, 0));
        HIPCHK(block_prefix(w.blocksub, w.blockcnt, w.blockpre, nb1 - 1, w.temp, w.temp.cap, side));
        HIPCHK(hipEventRecord(x->join_ev, side));
        before_write = x->join_ev;
        cp_pre = w.blockpre;
    }
    const uint64_t seq = ++x->seq;
    // (the hot pipeline's bucket counters, when a call of this context has allocated them: the write kernel clears them
    // when it announces hot groups)
    uint32_t *hot_counts = c.pre && w.dt.counts && c.tiles + 1 <= w.dt_cap ? w.dt.counts : nullptr;
    // The hot pipeline queued ahead of the knowledge that the call needs it (round 6): the context's last call had a few hot
    // groups and the buckets are allocated -- grids for spec_bound hot groups, their number read on the device (kernels.hip:
    // hot_groups_here); more of them, or none: the kernels return at once.  (Not beyond the room the output buffer has for
    // hot groups, nor where a call with that many would rather take the wide form.)
    static const bool no_spec = std::getenv("ACX_NO_SPEC_HOT") != nullptr; // measurements
    uint32_t spec_bound = 0;
    if (hot_counts && x->spec_hot && !no_spec) {
        uint64_t b = std::min<uint64_t>(2ull * x->spec_hot, HOT_INLINE_MAX);
        b = std::min<uint64_t>(b, pin ? HOT_INLINE_MAX : x->hot_inline);
        b = std::min<uint64_t>(b, T.n_groups >= 32 ? T.n_groups / 32 : T.n_groups);
        if (b >= x->spec_hot && ensure_dense_tiles(x, c.tiles) == ACX_OK) spec_bound = (uint32_t)b;
    }
    T.w8 = tile_words_narrow(view(a, c.overlapping), cp_pre != nullptr) ? 1u : 0u; // (what the groups' stretches hold: kernels.hpp)
    HIPCHK(tile_post(view(a, c.overlapping), c.key_mode, c.overlapping, T, c.lead, c.d_hay, c.len, c.out, w.summary, abort_flag,
                        next_flag, w.h_pinned + PIN_TOTALS, seq, c.G, seg_counts, cp_pre, w.blocksub, before_write, c.pre, hot_counts,
                        (uint32_t)(c.tiles + 2), st));
    const uint64_t pub_spec = seq | (1ull << 63);
    if (spec_bound) {
        uint32_t *hot_abort = (uint32_t *)(w.summary + 10);
        HIPCHK(hot_verify_main(view(a, c.overlapping), c.key_mode, c.overlapping, c.G, T, w.hot_list, 0, abort_flag, x->spec_ovf, w.dt,
                                  w.TD, c.lead, c.d_hay, c.len, hot_abort, seq, spec_bound, st));
        HIPCHK(hot_write(view(a, c.overlapping), c.key_mode, T, w.TD, w.hot_list, 0, c.lead, c.d_hay, c.out, w.summary, abort_flag,
                            hot_abort, w.h_pinned + PIN_SPEC_TOTALS, seq, pub_spec, c.G, seg_counts, cp_pre, w.blocksub, spec_bound, st));
    }
    g_trace.mark(4);
    if (seg_counts) c.counts_zeroed = true; // (k_tile_main clears them, k_tile_write adds to them)
    // while the kernels run: the scan time of the previous call, and the event the result's
    // accessors wait for (nothing more is queued behind the write kernel unless a fix-up follows)
    settle_scan_profile(a, x);
    if (c.early_event && !c.r->done) {
        c.r->done = g_events.get(a->device);
        if (c.r->done) HIPCHK(hipEventRecord(c.r->done, st));
        c.event_at_post = c.r->done != nullptr;
    }
    g_trace.mark(5);
    if ((rc = wait_line(x, PIN_TOTALS, seq, w.t_line, "the write kernel did not publish its totals")) != ACX_OK) return rc;
    g_trace.mark(6);
    w.flags_dirty = false; // the write kernel left the next control block clean
    add_scan_profile(a, x, c.len, c.timed);
    // the line (k_tile_write): [1] matches, [2] occurrences, [3] prefix hits, [4] why | hot groups << 8, [5] overflow hits |
    // the fullest overflow list << 32
    uint64_t gave_up = w.t_line[4] & 0xFF;
    const uint64_t n_hot = w.t_line[4] >> 8, n_ovf = w.t_line[5] & 0xFFFFFFFFull, ovf_max = w.t_line[5] >> 32;
    if (gave_up == 2 && !c.ovf_grown && ovf_max * OVF_LISTS <= 3 * c.tiles * HIT_SLOTS + (OVF_LISTS << 12)) {
        // K1b found more hits beyond their tiles' slots than an overflow list holds (nothing else is wrong): with lists
        // of the size this input needs the sparse kernels + the hot pipeline take it -- again, once
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipMemsetAsync(T.sgw, 0, 4 * (uint64_t)T.sg_cap * 8, st));
        if ((rc = set_overflow_room(x, ovf_max + ovf_max / 4 + 64)) == ACX_OK) {
            c.ovf_grown = true;
            c.leads_counted = false;
            c.event_at_post = false;
            *what = Attempt::Again;
            return ACX_OK;
        }
        (void)hipGetLastError(); // (no room for it: the dense path)
    }
    // what the context's next call queues ahead: the hot pipeline, when this one had a few hot groups
    x->spec_hot = (!gave_up && n_hot && n_hot <= HOT_INLINE_MAX) ? (uint32_t)n_hot : 0u;
    x->spec_ovf = (uint32_t)ovf_max;
    bool spec_done = false;
    if (spec_bound && !gave_up && n_hot && n_hot <= spec_bound) {
        // the speculative pipeline is this call's: its pass 1 publishes the totals (a line of its own: pass 0's stays readable)
        if ((rc = wait_line(x, PIN_SPEC_TOTALS, pub_spec, w.t_line, "the speculative hot pipeline did not publish its totals")) != ACX_OK) return rc;
        if ((w.t_line[4] & 0xFF) != 0) { c.no_dense_tiles = true; gave_up = 1; }
        else { a->path[1]++; a->path[2] += n_hot; a->path[3] += n_ovf; }
        spec_done = true;
    }
    if (c.ovf_grown && gave_up != 2) a->path[6]++;
    // many groups gave up on the narrow stage although their tiles' slots held the hits (a match every 100 - 500 bytes: more
    // than 24 occurrences in a 4 KiB bucket, more than GROUP_MAX in a group): the context takes the WIDE form of the post stage
    // -- this call again, its next calls from the start -- instead of handing every group to the hot pipeline and the handle
    // to the dense path (until round 5: 2 437 -> 1 057 GB/s between a match every 512 and every 256 bytes)
    static const bool no_wide = std::getenv("ACX_NO_WIDE") != nullptr; // measurements
    if (!gave_up && c.pre && !wide && !c.wide_tried && !no_wide && T.n_groups >= 32 && n_hot * 32 > T.n_groups &&
        n_ovf * 8 <= w.t_line[3]) {
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipMemsetAsync(T.sgw, 0, 4 * (uint64_t)T.sg_cap * 8, st));
        if (seg_counts) HIPCHK(hipMemsetAsync(c.r->d_counts, 0, std::max<uint64_t>(c.G.n_hay, 1) * 8, st));
        x->wide = true;
        c.wide_tried = true;
        c.leads_counted = false;
        c.event_at_post = false;
        a->path[9]++;
        *what = Attempt::Again;
        return ACX_OK;
    }
    if (!gave_up && n_hot && !spec_done) { // groups the sparse kernels could not finish: the hot pipeline, then the write kernel again
        bool lost = false;
        if ((rc = run_hot(c, abort_flag, seq, (uint32_t)n_hot, (uint32_t)ovf_max, seg_counts, cp_pre, hot_counts != nullptr, &lost)) != ACX_OK) return rc;
        if (lost) gave_up = 1;
        else {
            a->path[1]++; a->path[2] += n_hot; a->path[3] += n_ovf;
            if (n_hot > x->hot_inline) x->hot_inline = std::min<uint64_t>(HOT_INLINE_MAX, 2 * n_hot); // (the context's next calls)
        }
    } else if (!gave_up && !spec_done) {
        a->path[0]++;
    }
    if (gave_up != 0) { // the slots could not hold the output: dense path
        HIPCHK(hipStreamSynchronize(st));
        c.event_at_post = false; // (the dense path queues more: the event is recorded again at the end)
        // (both sets of supergroup words clear again, whatever made the call give up)
        HIPCHK(hipMemsetAsync(T.sgw, 0, 4 * (uint64_t)T.sg_cap * 8, st));
        if (seg_counts) HIPCHK(hipMemsetAsync(c.r->d_counts, 0, std::max<uint64_t>(c.G.n_hay, 1) * 8, st));
        x->dense_hold = 8;
        x->hold_dense_input = false; // (unless the dense path finds the input dense: below)
        c.leads_counted = false;
        c.cp_done = false;
        *what = Attempt::GoDense;
        return ACX_OK;
    }
    c.n_raw = w.t_line[2]; // (the hot pipeline's second publication when it ran)
    c.n_hits = w.t_line[3];
    c.n_final = w.t_line[1];
    // (back to the narrow form -- twice the groups in flight -- when the input no longer needs the wide one)
    if (wide && n_hot == 0 && c.n_raw * 5 < (uint64_t)T.n_groups * GROUP_MAX * 2) x->wide = false;
    if (c.out == w.final) {
        c.r->d_matches = w.final; // hand the buffer over; the next call takes a fresh one
        w.final = nullptr;
    } else {
        c.r->d_matches = c.out;   // the context's pinned buffer: the caller (acx_find) copies out of it under its lease
        c.r->borrowed = true;
    }
    c.localized = seg_counts != nullptr;
    c.cp_done = cp_pre != nullptr;
    c.queued = !c.event_at_post; // k_tile_write is still running (and the event that fences it is in place)
    *what = Attempt::Done;
    return ACX_OK;
}

// ---- dense output, tile-ordered (K1b sets whose patterns fit the context tiles): prefix hits in per-wave regions ->
// occurrence words in the bucket of their key tile -> per group: sort + match kind in LDS -> the sparse path's write
// kernel.  One round trip for the totals (the output buffer is sized exactly), a second pass only when the hit
// regions were too small.  Gives up (Attempt::Again with no_dense_tiles) when a bucket overflows -- more than one
// occurrence per 8 bytes -- or a chain of overlapping occurrences is longer than the context.
int attempt_dense_tiles(FindCall &c, Attempt *what) {
    acx_automaton *a = c.a;
    Ctx *x = c.c;
    Workspace &w = x->ws;
    hipStream_t st = x->stream;
    int rc = ensure_hits(x, std::max<uint64_t>(1u << 16, c.len / 64));
    if (rc) return rc;
    if ((rc = ensure_dense_tiles(x, c.tiles)) != ACX_OK) return rc;
    const uint32_t hit_grid = prefilter_hit_regions(c.scan_grid);
    const uint64_t hit_cap = w.hit_total() / hit_grid;
    const Sink H{w.hrecs, w.hit_counts, hit_cap, c.key_mode, nullptr, nullptr, nullptr, c.lead, 1, 0};
    uint32_t *abort_flag = (uint32_t *)(w.summary + 10), *zero_flag = (uint32_t *)(w.summary + 11);
    HIPCHK(hipMemsetAsync(w.dt.counts, 0, ((uint64_t)w.dt.n_tiles + 1) * 4, st));
    HIPCHK(hipMemsetAsync(w.TD.sgw, 0, 2 * (uint64_t)w.TD.sg_cap * 8, st));
    HIPCHK(hipMemsetAsync(w.summary + 10, 0, 16, st));
    const bool prof = c.timed;
    HIPCHK(launch_prefilter(a->dev, H, c.d_hay, c.len, c.scan_grid, st, prof ? scan_start_ev(x) : nullptr,
                               prof ? scan_stop_ev(x) : nullptr));
    HIPCHK(dense_tiles_verify(view(a, c.overlapping), c.G, H, hit_grid, w.dt, c.key_mode, c.lead, c.d_hay, c.len, abort_flag, st));
    // (the hit regions' fill: summary[2] = hits kept, [3] = the fullest region)
    HIPCHK(sink_summary(w.hit_counts, hit_grid, hit_cap, w.hit_counts, hit_grid, hit_cap, w.summary, w.region_off, st));
    // (k_dense_main in its compact form -- sixteen groups per CU -- unless a call of this context did not fit it lately)
    static const bool no_compact = std::getenv("ACX_NO_DENSE_COMPACT") != nullptr; // measurements
    bool compact = x->dense_full == 0 && !no_compact;
    if (x->dense_full > 0) x->dense_full--;
    HIPCHK(dense_tiles_main(a->dev, c.key_mode, c.overlapping, w.dt, w.TD, c.lead, abort_flag, w.summary, compact, st));
    // ([0..3]: the hit regions' fill; [8] matches, [9] occurrences, [10] the abort flag -- not [7], [11]: the words the
    // sparse path and K0 publish their sequence numbers in)
    HIPCHK(hipMemcpyAsync(w.h_pinned, w.summary, 32, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(w.h_pinned + 8, w.summary + 8, 24, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    add_scan_profile(a, x, c.len, c.timed);
    const uint64_t hit_max = w.h_pinned[3];
    if (hit_max > hit_cap) { // hits were dropped: more room, again (the regions are balanced: a wave's tiles are spread over the stream)
        if ((rc = ensure_hits(x, (uint64_t)hit_grid * (hit_max + hit_max / 8 + 64))) != ACX_OK) return rc;
        *what = Attempt::Again;
        return ACX_OK;
    }
    if (compact && (uint32_t)w.h_pinned[10] == 2) { // a group's occurrences did not fit the compact stage: the kernel again, full
        x->dense_full = 8;
        HIPCHK(hipMemsetAsync(w.TD.sgw, 0, 2 * (uint64_t)w.TD.sg_cap * 8, st));
        HIPCHK(hipMemsetAsync(w.summary + 10, 0, 16, st));
        HIPCHK(dense_tiles_main(a->dev, c.key_mode, c.overlapping, w.dt, w.TD, c.lead, abort_flag, w.summary, false, st));
        HIPCHK(hipMemcpyAsync(w.h_pinned + 8, w.summary + 8, 24, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    if ((uint32_t)w.h_pinned[10] != 0) { // a bucket overflowed / a chain left its context: the radix-sort form
        c.no_dense_tiles = true;
        *what = Attempt::Again;
        return ACX_OK;
    }
    const uint64_t n_final = w.h_pinned[8], n_raw = w.h_pinned[9];
    if (std::max(n_raw, w.h_pinned[2]) >= occ_limit()) return fail_occ(); // (the tiles' counts and their prefixes are 32 bits wide)
    // (round 5: a hold that a dense INPUT set ends with the first input that is not dense -- the dense path on a sparse input
    // costs 2-3x, eight calls of it were the price of one dense call in front: bench.py's 8 GiB run behind its density sweep)
    if (n_raw > 8 * c.tiles) { x->dense_hold = 8; x->hold_dense_input = true; }
    else if (x->dense_hold > 0) x->dense_hold = x->hold_dense_input ? 0 : x->dense_hold - 1;
    c.n_raw = n_raw;
    c.n_hits = w.h_pinned[2];
    c.n_final = n_final;
    *what = Attempt::Done;
    a->path[4]++;
    if (n_final == 0) return ACX_OK;
    HIPCHK(g_bufs.get((void **)&c.r->d_matches, n_final * sizeof(acx_match_t), a->device));
    // batch with byte offsets: the write kernel localises and counts per haystack itself
    uint64_t *seg_counts = c.segmented && !c.codepoints ? c.r->d_counts : nullptr;
    if (seg_counts && (rc = zero_counts(c)) != ACX_OK) return rc;
    HIPCHK(dense_tiles_write(a->dev, c.key_mode, w.TD, c.d_hay, c.r->d_matches, w.summary, zero_flag, w.h_pinned + PIN_TOTALS, c.lead,
                                c.G, seg_counts, nullptr, nullptr, st));
    c.localized = seg_counts != nullptr;
    c.queued = true;
    return ACX_OK;
}

// ---- dense output: region mode -> compact -> radix sort -> resolve (two round trips)
int attempt_dense(FindCall &c, Attempt *what) {
    acx_automaton *a = c.a;
    Ctx *x = c.c;
    Workspace &w = x->ws;
    hipStream_t st = x->stream;
    Workspace::OccBufs &o = w.occ;
    {
        const bool no_tiles_env = std::getenv("ACX_NO_DENSE_TILES") != nullptr; // tests / measurements: the radix-sort form (read per call)
        if (c.pre && a->sparse_ok && !c.no_dense_tiles && !no_tiles_env && c.tiles < (1ull << 26))
            return attempt_dense_tiles(c, what);
    }
    int rc = ensure_occ_capacity(x, std::max<uint64_t>(1u << 16, c.len / 64));
    if (rc) return rc;
    if (c.pre && (rc = ensure_hits(x, std::max<uint64_t>(1u << 16, c.len / 64))) != ACX_OK) return rc;
    const uint32_t hit_grid = c.pre ? prefilter_hit_regions(c.scan_grid) : 0;
    // K1a: the failureless walk here too (one occurrence region per block of k1a_walk); the chunked walk
    // when the automaton has none, or when its items did not fit
    static const bool no_pfac = std::getenv("ACX_NO_PFAC") != nullptr;
    const bool pfac = !c.pre && pfac_available(a->dev, a->max_lds) && !no_pfac && !c.chunked_walk;
    const uint32_t pgrid = pfac ? pfac_scan_grid(c.d_hay, c.len, a->n_cus) : 0;
    if (pfac && (rc = ensure_hits(x, (pfac_workspace_words(c.len, pgrid, true) + 3) / 4)) != ACX_OK) return rc;
    const uint32_t grid = c.pre ? walk_hits_grid(hit_grid) : pfac ? pgrid * 16 : c.scan_grid; // occurrence regions
    const uint64_t hit_cap = c.pre ? w.hit_total() / hit_grid : 0;
    // exact_regions (second pass after an occurrence region overflowed): every region gets the room
    // it asked for in the first pass, at the exclusive prefix of the counts (stored behind the counts)
    const uint64_t region_cap = c.exact_regions ? 0 : w.cap / grid;
    const Sink H{w.hrecs, w.hit_counts, hit_cap, c.key_mode, nullptr, nullptr, nullptr, c.lead, 1, 0};
    uint32_t *items_overflow = (uint32_t *)(w.summary + 4);
    const Sink K{o.recs, w.block_counts, region_cap, c.key_mode, nullptr, nullptr, pfac ? items_overflow : nullptr, c.lead, 1, 0};
    const bool prof = c.timed;
    if (c.pre) {
        HIPCHK(launch_prefilter(a->dev, H, c.d_hay, c.len, c.scan_grid, st, prof ? scan_start_ev(x) : nullptr,
                                   prof ? scan_stop_ev(x) : nullptr));
        HIPCHK(launch_walk_hits(view(a, c.overlapping), c.G, H, hit_grid, K, grid, c.d_hay, c.len, st));
    } else {
        if (pfac) HIPCHK(hipMemsetAsync(w.summary + 4, 0, 8, st));
        if (prof) HIPCHK(hipEventRecord(scan_start_ev(x), st));
        if (pfac)
            HIPCHK(launch_pfac(view(a, c.overlapping), d_view(a, c.overlapping), c.G, K, c.d_hay, c.len, pgrid, (uint64_t *)w.hrecs.p, w.hit_counts,
                                  grid, true, st));
        else
            HIPCHK(launch_dfa_walk(view(a, c.overlapping), d_view(a, c.overlapping), c.G, K, c.d_hay, c.len, c.scan_grid, a->max_lds, st));
        if (prof) HIPCHK(hipEventRecord(scan_stop_ev(x), st));
    }
    HIPCHK(sink_summary(w.block_counts, grid, c.exact_regions ? ~0ull : region_cap, c.pre ? w.hit_counts : nullptr,
                           hit_grid, hit_cap, w.summary, w.region_off, st));
    HIPCHK(hipMemcpyAsync(w.h_pinned, w.summary, 40, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    add_scan_profile(a, x, c.len, c.timed);
    if (pfac && (uint32_t)w.h_pinned[4] != 0) { // more items than 1 per 16 bytes: the chunked walk has no such limit
        c.chunked_walk = true;
        c.exact_regions = false;
        *what = Attempt::Again;
        return ACX_OK;
    }
    const uint64_t n_raw = w.h_pinned[0], region_max = w.h_pinned[1], hit_max = c.pre ? w.h_pinned[3] : 0;
    if (c.exact_regions) {
        if (n_raw != c.exact_total || (c.pre && hit_max > hit_cap))
            return fail(ACX_EDEVICE, "the second pass of the dense path counted differently");
    } else if (region_max > region_cap || hit_max > hit_cap) { // a sink region overflowed: grow, redo
        if (hit_max > hit_cap) {
            // hits that overflowed were dropped, so the occurrence counts are lower bounds: more room for
            // both, uniform regions (the hit regions are balanced: a wave's tiles are spread over the stream)
            if ((rc = ensure_hits(x, (uint64_t)hit_grid * (hit_max + hit_max / 8 + 64))) != ACX_OK) return rc;
            uint64_t want = std::max((uint64_t)grid * (region_max + region_max / 8 + 64), w.cap * 4);
            // (bounded growth: ~72 B of workspace per record; once the hit regions hold everything the
            // counts are exact and the second pass sizes the occurrence buffer exactly)
            want = std::min<uint64_t>(want, std::max<uint64_t>(w.cap * 4, 1ull << 28));
            if ((rc = ensure_occ_capacity(x, want)) != ACX_OK) return rc;
        } else {
            // the regions' counts are exact (a full region keeps counting): the second pass puts every
            // region at the exclusive prefix of the counts -- room for exactly the occurrences there are,
            // however unevenly they are spread (grid * the fullest region can be 100x that)
            uint64_t *bases = w.block_counts + grid;
            HIPCHK(sink_summary(w.block_counts, grid, ~0ull, nullptr, 0, 0, w.summary + 8, bases, st));
            HIPCHK(hipMemcpyAsync(w.h_pinned + 10, bases + grid, 8, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            c.exact_total = w.h_pinned[10];
            if (c.exact_total >= occ_limit()) return fail_occ();
            // (an eighth of headroom: the NEXT call's uniform regions -- capacity / grid each -- then hold an
            // output that is spread as evenly as this one, and it needs no second pass)
            if ((rc = ensure_occ_capacity(x, c.exact_total + c.exact_total / 8 + 64 * (uint64_t)grid)) != ACX_OK) return rc;
            c.exact_regions = true;
        }
        *what = Attempt::Again;
        return ACX_OK;
    }
    if (n_raw >= occ_limit()) return fail_occ();
    // (round 5: a hold that a dense INPUT set ends with the first input that is not dense -- the dense path on a sparse input
    // costs 2-3x, eight calls of it were the price of one dense call in front: bench.py's 8 GiB run behind its density sweep)
    if (n_raw > 8 * c.tiles) { x->dense_hold = 8; x->hold_dense_input = true; }
    else if (x->dense_hold > 0) x->dense_hold = x->hold_dense_input ? 0 : x->dense_hold - 1;
    c.n_raw = n_raw;
    c.n_hits = c.pre ? w.h_pinned[2] : 0;
    *what = Attempt::Done;
    a->path[5]++;
    if (n_raw == 0) return ACX_OK;
    HIPCHK(sink_compact(o.recs, w.region_off, grid, region_cap, o.keys[1], o.pids[1], st));
    const int end_bit = std::min(64, (int)a->dev.rank_bits + bits_for(c.len));
    HIPCHK(sort_occurrences(w.temp, w.temp.cap, o.keys[1], o.keys[0], o.pids[1], o.pids[0], n_raw, end_bit, st));
    HIPCHK(make_spans(a->dev, c.key_mode, o.keys[0], o.pids[0], o.S, o.E, n_raw, st));
    if (c.overlapping) {
        c.n_final = n_raw;
    } else {
        // Standard: sorted by end, so the running max of the ends IS the array of ends
        const uint64_t *M = o.E;
        if (c.key_mode != 0) {
            HIPCHK(prefix_max(w.temp, w.temp.cap, o.E, o.M, n_raw, st));
            M = o.M;
        }
        HIPCHK(hipMemsetAsync(o.flags + n_raw, 0, 4, st));
        HIPCHK(resolve_greedy(o.S, o.E, M, o.flags, n_raw, st));
        HIPCHK(flag_offsets(w.temp, w.temp.cap, o.flags, o.idx, n_raw, st));
        HIPCHK(hipMemcpyAsync(w.h_pinned + 6, o.idx + n_raw, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        c.n_final = *(uint32_t *)(w.h_pinned + 6);
    }
    HIPCHK(g_bufs.get((void **)&c.r->d_matches, std::max<uint64_t>(c.n_final, 1) * sizeof(acx_match_t),
                         a->device));
    HIPCHK(write_matches(o.pids[0], o.S, o.E, c.overlapping ? nullptr : o.flags, c.overlapping ? nullptr : o.idx,
                            c.r->d_matches, n_raw, st));
    c.queued = true;
    return ACX_OK;
}

} // namespace

// batch: the per-haystack counts start at zero.  No memset in front of the scan (it delayed the scan's
// launch by a dispatch and ~15 us of host time on every batch call): the sparse path has k_tile_main
// clear them on its way, every other path clears them here, when it gets to them.
int zero_counts(FindCall &c) {
    if (c.segmented && !c.counts_zeroed) {
        HIPCHK(hipMemsetAsync(c.r->d_counts, 0, std::max<uint64_t>(c.G.n_hay, 1) * 8, c.c->stream));
        c.queued = true;
    }
    c.counts_zeroed = true;
    return ACX_OK;
}

// everything after the matches exist: code points (str API), local offsets + counts (batches)
int finish_matches(FindCall &c) {
    Ctx *x = c.c;
    Workspace &w = x->ws;
    hipStream_t st = x->stream;
    if (!c.n_final || c.cp_done || !(c.codepoints || (c.segmented && !c.localized))) return ACX_OK;
    if (c.codepoints) {
        const uint64_t nb1 = (c.len + 1023) / 1024 + 1;
        int rc = ensure_blocks(x, c.leads_counted ? std::max<uint64_t>(nb1, 4 * c.tiles + 1) : nb1);
        if (rc) return rc;
        if (!c.leads_counted) HIPCHK(count_lead_bytes(c.d_hay, c.len, w.blockcnt, w.blocksub, st));
        HIPCHK(block_prefix(c.leads_counted ? w.blocksub : nullptr, w.blockcnt, w.blockpre, nb1 - 1, w.temp, w.temp.cap, st));
    }
    if (c.segmented) {
        int rc = zero_counts(c);
        if (rc) return rc;
        HIPCHK(localize(c.G, c.d_hay, c.len, w.blockpre, w.blocksub, c.codepoints, c.r->d_matches, c.n_final,
                           c.r->d_counts, st));
    }
    else
        HIPCHK(to_code_points(c.d_hay, c.len, w.blockpre, w.blocksub, c.r->d_matches, c.n_final, st));
    c.queued = true;
    return ACX_OK;
}

// the general pipeline on an allocated result
int run_pipeline(FindCall &c) {
    acx_automaton *a = c.a;
    Ctx *x = c.c;
    int rc = ensure_common(x);
    if (rc) return rc;
    c.pre = a->kernel == ACX_KERNEL_PREFILTER;
    c.scan_grid = c.pre ? prefilter_grid(c.d_hay, c.len, a->n_cus) : dfa_walk_grid(a->dev, c.len, a->n_cus);
    c.lead = (uint32_t)((uintptr_t)c.d_hay & 15);
    c.tiles = prefilter_tiles(c.d_hay, c.len);
    const bool no_sparse_env = std::getenv("ACX_NO_BUCKET") != nullptr; // tests / profiling: force the dense path (read per call)
    bool sparse = a->sparse_ok && x->dense_hold == 0 && !no_sparse_env && c.tiles < (1ull << 26);
    for (int attempt = 0;; attempt++) {
        if (attempt == 6) return fail(ACX_EDEVICE, "occurrence buffer overflow persisted");
        Attempt what = Attempt::Done;
        if ((rc = sparse ? attempt_sparse(c, &what) : attempt_dense(c, &what)) != ACX_OK) return rc;
        if (what == Attempt::GoDense) sparse = false;
        if (what == Attempt::Done) break;
    }
    if (c.timed) {
        std::lock_guard<std::mutex> lk(a->prof_mu);
        a->profile.raw_occurrences += c.n_raw;
        a->profile.prefix_hits += c.n_hits;
    }
    c.r->n = c.n_final;
    if ((rc = finish_matches(c)) != ACX_OK) return rc;
    if ((rc = zero_counts(c)) != ACX_OK) return rc; // (a batch without a match never got to them)
    static const bool prof_post = std::getenv("ACX_PROFILE_POST") != nullptr;
    if (a->prof && prof_post) { // end of the post stage (costs the next call a wait for this one's last kernel)
        HIPCHK(hipEventRecord(x->ev[2], x->stream));
        x->post_pending = true;
    }
    return ACX_OK;
}

} // namespace acxh
