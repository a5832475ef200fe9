// find_attempts.cpp -- the device pipeline of one find call on an allocated result: the sparse attempt (hit slots + tile
// kernels, the hot pipeline for the groups they cannot finish), the two dense forms, and what follows the matches
// (code points, per-haystack offsets and counts).  find_attempts.hpp: FindCall, run_pipeline.  WHICH path a call takes is
// find_policy.hpp's (pure functions of the totals' line and the context's history); here are the steps that launch, clear
// and wait, and what a failed allocation does.
#include "find_attempts.hpp"

#include "find_policy.hpp"
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

namespace pol = acx_policy;

// ---- the environment switches of this file, all read here
//   switch                for            read              what it does
//   ACX_FORCE_WIDE        tests          once per process  every K1b call takes the wide form of the post stage
//   ACX_NO_WIDE           measurements   once per process  no call is redone in the wide form
//   ACX_NO_SPEC_HOT       measurements   once per process  the hot pipeline is never queued ahead
//   ACX_NO_PFAC           measurements   once per process  K1a: always the chunked walk
//   ACX_NO_DENSE_COMPACT  measurements   once per process  k_dense_main always in its full form
//   ACX_PROFILE_POST      profiling      once per process  an event at the end of the post stage (post_ms)
//   ACX_NO_BUCKET         tests          every call        the dense path from the first attempt on
//   ACX_NO_DENSE_TILES    tests          every call        the dense path in its radix-sort form
// (once per process: where a call first asks; tests run those in processes of their own)
bool force_wide_on() { static const bool force_wide = std::getenv("ACX_FORCE_WIDE") != nullptr; return force_wide; }
bool no_wide_on() { static const bool no_wide = std::getenv("ACX_NO_WIDE") != nullptr; return no_wide; }
bool no_spec_on() { static const bool no_spec = std::getenv("ACX_NO_SPEC_HOT") != nullptr; return no_spec; }
bool no_pfac_on() { static const bool no_pfac = std::getenv("ACX_NO_PFAC") != nullptr; return no_pfac; }
bool no_compact_on() { static const bool no_compact = std::getenv("ACX_NO_DENSE_COMPACT") != nullptr; return no_compact; }
bool prof_post_on() { static const bool prof_post = std::getenv("ACX_PROFILE_POST") != nullptr; return prof_post; }
bool no_bucket_now() { const bool no_sparse_env = std::getenv("ACX_NO_BUCKET") != nullptr; return no_sparse_env; }
bool no_dense_tiles_now() { const bool no_tiles_env = std::getenv("ACX_NO_DENSE_TILES") != nullptr; return no_tiles_env; }

constexpr uint64_t PIN_FINAL_MAX = 32ull << 20; // bytes of pinned result buffer a context keeps for host calls (acx_find up to ~8 MiB)
// hot groups whose capacity the output buffer has room for anyway: 16 to start with, up to 128 for a context that has seen more
// (Ctx::hot_inline; round 6 -- until then 128 for every call: ~100 MB per result from 32 MiB haystacks on, whatever the input);
// beyond a context's figure: hot_totals, then a buffer of the exact size
constexpr uint64_t HOT_INLINE = 16, HOT_INLINE_MAX = 128;
constexpr pol::Limits LIM{HIT_SLOTS, OVF_LISTS, GROUP_MAX, GROUP_MAX_WIDE, HOT_SUB, DT_GMAX, sizeof(acx_match_t),
                          HOT_INLINE, HOT_INLINE_MAX, PIN_FINAL_MAX};

int bits_for(uint64_t x) { return x ? 64 - __builtin_clzll(x) : 0; } // number of bits needed to represent x

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

// ---- what every attempt works on -- the call, and its context's parts under the names the launches use -- and what the
// attempts share
struct Frame {
    FindCall &c;
    acx_automaton *a = c.a;
    Ctx *x = c.c;
    Workspace &w = x->ws;
    hipStream_t st = x->stream;
    TileSpace &T = w.T;
    const bool prof = c.timed;
    // batch with byte offsets: the write kernel localises and counts per haystack itself
    uint64_t *const seg_counts = c.segmented && !c.codepoints ? c.r->d_counts : nullptr;
    // the abort flag of the hot pipeline and of the tile-ordered dense form
    uint32_t *const dense_abort = (uint32_t *)(w.summary + SCR_ABORT);
    // automata of at most 32 byte classes: the failureless walk (k1a_scan + k1a_walk) instead of the chunked one -- unless
    // its items did not fit (the dense path's second attempt)
    const bool pfac = !c.pre && pfac_available(a->dev, a->max_lds) && !no_pfac_on() && !c.chunked_walk;
    const uint32_t pgrid = pfac ? pfac_scan_grid(c.d_hay, c.len, a->n_cus) : 0;
    explicit Frame(FindCall &c_) : c(c_) {}

    // the K1a scan, between the pair of profiling events: the failureless walk (pgrid workgroups of k1a_scan, `regions`
    // regions of k1a_walk, dense: into occurrence regions) or the chunked one
    int launch_k1a(const Sink &K, uint32_t regions, bool dense) {
        if (prof) HIPCHK(hipEventRecord(scan_start_ev(x), st));
        if (pfac)
            HIPCHK(launch_pfac(view(a, c.overlapping), d_view(a, c.overlapping), c.G, K, c.d_hay, c.len, pgrid, (uint64_t *)w.hrecs.p, w.hit_counts,
                                  regions, dense, st));
        else
            HIPCHK(launch_dfa_walk(view(a, c.overlapping), d_view(a, c.overlapping), c.G, K, c.d_hay, c.len, c.scan_grid, a->max_lds, st));
        if (prof) HIPCHK(hipEventRecord(scan_stop_ev(x), st));
        return ACX_OK;
    }
    void set_hold(pol::Hold h) { x->dense_hold = h.calls; x->hold_dense_input = h.input; }
};

// ---- sparse output: hit slots + tile kernels; returns when the totals are known
struct SparseAttempt : Frame {
    using Frame::Frame;
    // (the wide form of the post stage: K1b's hits only -- the hot pipeline behind it is theirs)
    const bool force_wide = force_wide_on();
    const bool wide = (x->wide || force_wide) && c.pre;
    const uint32_t gmax = wide ? GROUP_MAX_WIDE : GROUP_MAX;
    bool pin = false;                                     // the records go to the context's pinned buffer
    uint32_t *abort_flag = nullptr, *next_flag = nullptr; // this attempt's control block, and the next one's
    hipEvent_t side_after = nullptr;   // str API: what the code-point prefix on the second stream waits for,
    hipEvent_t before_write = nullptr; //   what the write kernel waits for,
    const uint64_t *cp_pre = nullptr;  //   and the prefix, when the write kernel converts on the way out
    uint32_t *hot_counts = nullptr;    // the hot pipeline's bucket counters, when a call of this context has allocated them
    uint32_t spec_bound = 0;           // > 0: the hot pipeline is queued ahead, for this many hot groups
    uint64_t seq = 0, pub_spec = 0;    // the numbers pass 0's line and the speculative pipeline's carry

    int run(Attempt *what) {
        int rc = ensure_tiles(a, x, c.tiles, gmax);
        if (rc) return rc;
        const pol::HitCounters cnt = pol::hit_counters(c.pre, pfac, c.scan_grid, pgrid, c.tiles);
        T.cnt_nw = cnt.nw; T.cnt_iters = cnt.iters;
        if ((rc = output_room()) != ACX_OK) return rc;
        if ((rc = take_control_block()) != ACX_OK) return rc;
        if ((rc = launch_scan()) != ACX_OK) return rc;
        if ((rc = codepoint_prefix_beside()) != ACX_OK) return rc;
        if ((rc = launch_post_stage()) != ACX_OK) return rc;
        g_trace.mark(4);
        if (seg_counts) c.counts_zeroed = true; // (k_tile_main clears them, k_tile_write adds to them)
        if ((rc = fence_and_wait_for_totals()) != ACX_OK) return rc;
        return act_on_totals(what);
    }

    // room for every group's capacity + what a few hot groups can report beyond it (run_hot): the context's pinned buffer
    // (a host call, while the whole fits: find_policy.hpp, pin_result) or a buffer of the cache
    int output_room() {
        pin = pol::pin_result(LIM, c.host_result, c.segmented, c.overlapping && a->expand_ov, T.n_groups, gmax, c.pre);
        const uint64_t out_cap = pol::cap_for(LIM, T.n_groups, gmax, c.pre, pin ? HOT_INLINE_MAX : x->hot_inline);
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
        return ACX_OK;
    }

    // two control blocks used in turn: this attempt's write kernel clears the other one
    int take_control_block() {
        if (w.flags_dirty) {
            HIPCHK(hipMemsetAsync(w.ctl, 0, 12, st));
            HIPCHK(hipMemsetAsync(w.ctl + CTL_WORDS, 0, 12, st));
            HIPCHK(hipMemsetAsync(w.ovf_counts, 0, 2 * OVF_LISTS * OVF_COUNT_STRIDE * 4, st));
        }
        w.flags_dirty = true;
        abort_flag = w.ctl + CTL_WORDS * x->flag_idx;
        next_flag = w.ctl + CTL_WORDS * (x->flag_idx ^ 1);
        x->flag_idx ^= 1;
        return ACX_OK;
    }

    // the scan into the tiles' hit slots: K1b, or K1a's walk
    int launch_scan() {
        int rc;
        const Sink K{nullptr, nullptr, 0, c.key_mode, T.hslots, T.hcnt, abort_flag, c.lead, T.cnt_nw, T.cnt_iters};
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
            return ACX_OK;
        }
        // the failureless walk: the scan writes the hits it settles itself and every tile's count, the
        // walk appends to them; its survivor records take the place of K1b's dense-path hit sink.  More
        // survivors than their regions hold (1 per 16 haystack bytes): the walk raises the abort flag, the
        // call is redone on the dense path, which walks in chunks.
        if (!pfac) HIPCHK(hipMemsetAsync(T.hcnt, 0, (c.tiles + 1) * 4, st)); // arrival counters of the walk's emission
        // (records of 32 B there, u64 words here)
        if (pfac && (rc = ensure_hits(x, (pfac_workspace_words(c.len, pgrid, false) + 3) / 4)) != ACX_OK) return rc;
        return launch_k1a(K, pgrid * 16, false);
    }

    // str API, one haystack: the prefix of the lead-byte counts is ready before the write kernel
    // needs it (it depends on the scan only), so the write kernel converts on the way out
    // (three small latency-bound kernels, ~30 us: on the context's second stream, beside k_tile_main,
    // which does not need them; the write kernel waits for both)
    int codepoint_prefix_beside() {
        if (!(c.leads_counted && !c.segmented)) return ACX_OK;
        const uint64_t nb1 = (c.len + 1023) / 1024 + 1;
        hipStream_t side = x->copy_stream;
        if (!side_after) { side_after = x->fork_ev; HIPCHK(hipEventRecord(x->fork_ev, st)); }
        HIPCHK(hipStreamWaitEvent(side, side_after, 0));
        HIPCHK(block_prefix(w.blocksub, w.blockcnt, w.blockpre, nb1 - 1, w.temp, w.temp.cap, side));
        HIPCHK(hipEventRecord(x->join_ev, side));
        before_write = x->join_ev;
        cp_pre = w.blockpre;
        return ACX_OK;
    }

    // the hot pipeline's two launches -- run_hot: n_hot groups, the host knows them; queued ahead: n_hot = 0, grids for
    // `bound` groups, their number read on the device (kernels.hip: hot_groups_here)
    int launch_hot_verify(uint32_t n_hot, uint32_t ovf_max, uint32_t bound) {
        HIPCHK(hot_verify_main(view(a, c.overlapping), c.key_mode, c.overlapping, c.G, T, w.hot_list, n_hot, abort_flag, ovf_max, w.dt,
                                  w.TD, c.lead, c.d_hay, c.len, dense_abort, seq, bound, st));
        return ACX_OK;
    }
    int launch_hot_write(uint32_t n_hot, uint32_t bound, uint32_t line_at, uint64_t pub) {
        HIPCHK(hot_write(view(a, c.overlapping), c.key_mode, T, w.TD, w.hot_list, n_hot, c.lead, c.d_hay, c.out, w.summary, abort_flag,
                            dense_abort, w.h_pinned + line_at, seq, pub, c.G, seg_counts, cp_pre, w.blocksub, bound, st));
        return ACX_OK;
    }

    // k_tile_main + k_tile_write -- and, behind them, the hot pipeline queued ahead of the knowledge that the call needs it
    // (round 6): the context's last call had a few hot groups and the buckets are allocated -- grids for spec_bound hot
    // groups; more of them, or none: the kernels return at once
    int launch_post_stage() {
        seq = ++x->seq;
        pub_spec = seq | (1ull << 63);
        // (the hot pipeline's bucket counters, when a call of this context has allocated them: the write kernel clears them
        // when it announces hot groups)
        hot_counts = c.pre && w.dt.counts && c.tiles + 1 <= w.dt_cap ? w.dt.counts : nullptr;
        if (hot_counts && !no_spec_on()) {
            const uint32_t b = pol::spec_bound(LIM, x->spec_hot, pin, x->hot_inline, T.n_groups);
            if (b && ensure_dense_tiles(x, c.tiles) == ACX_OK) spec_bound = b;
        }
        T.w8 = tile_words_narrow(view(a, c.overlapping), cp_pre != nullptr) ? 1u : 0u; // (what the groups' stretches hold: kernels.hpp)
        HIPCHK(tile_post(view(a, c.overlapping), c.key_mode, c.overlapping, T, c.lead, c.d_hay, c.len, c.out, w.summary, abort_flag,
                            next_flag, w.h_pinned + PIN_TOTALS, seq, c.G, seg_counts, cp_pre, w.blocksub, before_write, c.pre, hot_counts,
                            (uint32_t)(c.tiles + 2), st));
        if (!spec_bound) return ACX_OK;
        const int rc = launch_hot_verify(0, x->spec_ovf, spec_bound);
        return rc ? rc : launch_hot_write(0, spec_bound, PIN_SPEC_TOTALS, pub_spec);
    }

    // while the kernels run: the scan time of the previous call, and the event the result's accessors wait for (nothing
    // more is queued behind the write kernel unless a fix-up follows); then pass 0's line
    int fence_and_wait_for_totals() {
        settle_scan_profile(a, x);
        if (c.early_event && !c.r->done) {
            c.r->done = g_events.get(a->device);
            if (c.r->done) HIPCHK(hipEventRecord(c.r->done, st));
            c.event_at_post = c.r->done != nullptr;
        }
        g_trace.mark(5);
        int rc = wait_line(x, PIN_TOTALS, seq, w.t_line, "the write kernel did not publish its totals");
        if (rc) return rc;
        g_trace.mark(6);
        w.flags_dirty = false; // the write kernel left the next control block clean
        add_scan_profile(a, x, c.len, c.timed);
        return ACX_OK;
    }

    // the attempt starts over (or hands the call to the dense path): nothing of it is in flight, both sets of supergroup
    // words clear again -- and a batch's counts, which its kernels were adding to
    int restart(bool counts) {
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipMemsetAsync(T.sgw, 0, 4 * (uint64_t)T.sg_cap * 8, st));
        if (counts && seg_counts) HIPCHK(hipMemsetAsync(c.r->d_counts, 0, std::max<uint64_t>(c.G.n_hay, 1) * 8, st));
        return ACX_OK;
    }
    int again(Attempt *what) { c.leads_counted = c.event_at_post = false; *what = Attempt::Again; return ACX_OK; } // the next sparse attempt
    void count_hot_call(const pol::TotalsLine &t) { a->path[1]++; a->path[2] += t.n_hot; a->path[3] += t.n_ovf; }

    // the verdict on pass 0's line (find_policy.hpp), and what it asks for
    int act_on_totals(Attempt *what) {
        int rc;
        const pol::TotalsLine t = pol::decode_totals(w.t_line);
        if (pol::regrow_overflow(LIM, t, c.ovf_grown, c.tiles)) {
            if ((rc = restart(false)) != ACX_OK) return rc;
            if (set_overflow_room(x, pol::overflow_room(t)) == ACX_OK) { c.ovf_grown = true; return again(what); }
            (void)hipGetLastError(); // (no room for it: the dense path)
        }
        const pol::Speculation next = pol::next_speculation(LIM, t);
        x->spec_hot = next.hot;
        x->spec_ovf = next.ovf;
        const bool spec_done = pol::spec_is_ours(spec_bound, t);
        pol::TotalsLine sp = t;
        if (spec_done) {
            // the speculative pipeline is this call's: its pass 1 publishes the totals (a line of its own: pass 0's stays readable)
            if ((rc = wait_line(x, PIN_SPEC_TOTALS, pub_spec, w.t_line, "the speculative hot pipeline did not publish its totals")) != ACX_OK) return rc;
            sp = pol::decode_totals(w.t_line);
            if (sp.why != 0) c.no_dense_tiles = true;
        }
        const pol::SparseCall me{c.pre, wide, c.wide_tried, no_wide_on(), c.ovf_grown, T.n_groups};
        pol::Verdict v = pol::verdict(me, t, spec_done, sp.why != 0, sp.prefix_hits);
        if (v.count_hot) count_hot_call(t);
        if (v.count_regrown) a->path[6]++;
        if (v.act == pol::Act::RedoWide) {
            // the context takes the WIDE form of the post stage -- T.n_groups >= 32 && n_hot * 32 > T.n_groups, the hits in their
            // tiles' slots -- this call again, its next calls from the start -- instead of handing every group to the hot pipeline and
            // the handle to the dense path (until round 5: 2 437 -> 1 057 GB/s between a match every 512 and every 256 bytes)
            if ((rc = restart(true)) != ACX_OK) return rc;
            x->wide = c.wide_tried = true;
            a->path[9]++;
            return again(what);
        }
        if (v.act == pol::Act::RunHot) {
            bool lost = false;
            if ((rc = run_hot((uint32_t)t.n_hot, (uint32_t)t.ovf_max, &lost)) != ACX_OK) return rc;
            if (lost) v.act = pol::Act::Dense;
            else { count_hot_call(t); x->hot_inline = pol::grown_hot_inline(LIM, t.n_hot, x->hot_inline); } // (the context's next calls)
        } else if (v.act == pol::Act::Sparse) a->path[0]++;
        if (v.act == pol::Act::Dense) { // the slots could not hold the output: dense path
            // (both sets of supergroup words clear again, whatever made the call give up)
            if ((rc = restart(true)) != ACX_OK) return rc;
            c.event_at_post = false; // (the dense path queues more: the event is recorded again at the end)
            set_hold(pol::hold_gave_up()); // (unless the dense path finds the input dense: hold_after_dense)
            c.leads_counted = c.cp_done = false;
            *what = Attempt::GoDense;
            return ACX_OK;
        }
        const pol::TotalsLine fin = pol::decode_totals(w.t_line); // (the hot pipeline's second publication when it ran)
        c.n_raw = fin.occurrences;
        c.n_hits = fin.prefix_hits;
        c.n_final = fin.matches;
        if (pol::leave_wide(LIM, wide, t.n_hot, c.n_raw, T.n_groups)) x->wide = false;
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

    // groups the tile kernels could not finish (a dense stretch of the input: more hits than a tile's slots, a full bucket,
    // more matches than a group's stretch, an uncertifiable chain): the HOT pipeline -- the hot groups' hits (slots +
    // overflow list) through the tile-ordered dense machinery, their counts credited to the sparse path's groups, then the
    // write kernel again.  One dense region costs the groups it lies in, not the call (it used to send the whole call to the
    // dense path and keep the handle there for eight more calls).  *lost: the hot pipeline gave up too (a bucket of more than
    // DT_SLOTS occurrences, a chain longer than the context) -- the radix-sort form takes the call.
    int run_hot(uint32_t n_hot, uint32_t ovf_max, bool *lost) {
        *lost = true;
        if (ensure_dense_tiles(x, c.tiles) != ACX_OK) { // (no room for the buckets: the radix-sort form needs less)
            (void)hipGetLastError();
            free_dense_tiles(w);
            c.no_dense_tiles = true;
            return ACX_OK;
        }
        // (the bucket counters and the pipeline's abort flag, SCR_ABORT: cleared by the write kernel that announced the hot
        // groups -- unless the buckets are allocated by this very call)
        if (!hot_counts) HIPCHK(hipMemsetAsync(w.dt.counts, 0, ((uint64_t)w.dt.n_tiles + 1) * 4, st));
        int rc = launch_hot_verify(n_hot, ovf_max, 0);
        if (rc) return rc;
        // the output's room: the groups' capacities bound the matches; with many hot groups the buffer is sized exactly
        // instead (one more round trip, next to that much hot work)
        const uint64_t bound = pol::hot_bound(LIM, T.n_groups, T.gmax, n_hot);
        if (bound > c.out_cap && c.out != w.final) return ACX_OK; // (the pinned buffer is not regrown: the dense path takes this call)
        if (bound > w.final_cap && c.out == w.final) {
            const uint64_t pub_t = seq | (1ull << 62);
            HIPCHK(hot_totals(T, seq, w.h_pinned + PIN_HOT_TOTALS, pub_t, st));
            uint64_t early[8];
            if ((rc = wait_line(x, PIN_HOT_TOTALS, pub_t, early, "the hot pipeline did not publish its total")) != ACX_OK) return rc;
            const uint64_t n = std::min<uint64_t>(early[1], bound); // (meaningless when the pipeline gave up: bounded all the same)
            if (n >= occ_limit()) {
                // (the call goes on in byte ranges on this context: the control blocks and both sets of supergroup words clear again)
                w.flags_dirty = true;
                return (rc = restart(false)) != ACX_OK ? rc : fail_occ();
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
        // an input that is dense (nearly) everywhere -- n_hot * 4 > T.n_groups && T.n_groups >= 8 --: the dense path proper takes
        // the handle's next calls -- its scan writes the hits where its verification reads them, no sparse attempt in front
        if (pol::dense_everywhere(n_hot, T.n_groups)) set_hold(pol::hold_dense_input());
        const uint64_t pub = seq | (1ull << 63);
        if ((rc = launch_hot_write(n_hot, 0, PIN_TOTALS, pub)) != ACX_OK) return rc;
        if (c.early_event && c.r->done) HIPCHK(hipEventRecord(c.r->done, st)); // (again: behind the kernels queued since)
        if ((rc = wait_line(x, PIN_TOTALS, pub, w.t_line, "the write kernel did not publish its totals")) != ACX_OK) return rc;
        if (pol::decode_totals(w.t_line).why != 0) c.no_dense_tiles = true;
        else *lost = false;
        return ACX_OK;
    }
};

// ---- dense output
struct DenseAttempt : Frame {
    using Frame::Frame;
    int run(Attempt *what) {
        return pol::dense_in_tiles(c.pre, a->sparse_ok, c.no_dense_tiles, no_dense_tiles_now(), c.tiles) ? tile_ordered(what) : radix(what);
    }
    // a call of either form found n_raw occurrences: the density hold
    void hold_after(uint64_t n_raw) { set_hold(pol::hold_after_dense(pol::Hold{x->dense_hold, x->hold_dense_input}, n_raw, c.tiles)); }

    // tile-ordered (K1b sets whose patterns fit the context tiles): prefix hits in per-wave regions -> occurrence words in
    // the bucket of their key tile -> per group: sort + match kind in LDS -> the sparse path's write kernel.  One round trip
    // for the totals (the output buffer is sized exactly), a second pass only when the hit regions were too small.  Gives up
    // (Attempt::Again with no_dense_tiles) when a bucket overflows -- more than one occurrence per 8 bytes -- or a chain of
    // overlapping occurrences is longer than the context.
    int tile_ordered(Attempt *what) {
        int rc = ensure_hits(x, std::max<uint64_t>(1u << 16, c.len / 64));
        if (rc) return rc;
        if ((rc = ensure_dense_tiles(x, c.tiles)) != ACX_OK) return rc;
        const uint32_t hit_grid = prefilter_hit_regions(c.scan_grid);
        const uint64_t hit_cap = w.hit_total() / hit_grid;
        const Sink H{w.hrecs, w.hit_counts, hit_cap, c.key_mode, nullptr, nullptr, nullptr, c.lead, 1, 0};
        uint32_t *abort_flag = dense_abort, *zero_flag = (uint32_t *)(w.summary + SCR_ZERO);
        HIPCHK(hipMemsetAsync(w.dt.counts, 0, ((uint64_t)w.dt.n_tiles + 1) * 4, st));
        HIPCHK(hipMemsetAsync(w.TD.sgw, 0, 2 * (uint64_t)w.TD.sg_cap * 8, st));
        HIPCHK(hipMemsetAsync(w.summary + SCR_ABORT, 0, 16, st)); // (SCR_ZERO with it)
        HIPCHK(launch_prefilter(a->dev, H, c.d_hay, c.len, c.scan_grid, st, prof ? scan_start_ev(x) : nullptr,
                                   prof ? scan_stop_ev(x) : nullptr));
        HIPCHK(dense_tiles_verify(view(a, c.overlapping), c.G, H, hit_grid, w.dt, c.key_mode, c.lead, c.d_hay, c.len, abort_flag, st));
        // (the hit regions' fill: SCR_HITS = hits kept, SCR_HITS_MAX = the fullest region)
        HIPCHK(sink_summary(w.hit_counts, hit_grid, hit_cap, w.hit_counts, hit_grid, hit_cap, w.summary, w.region_off, st));
        const pol::DenseForm form = pol::dense_form(x->dense_full, no_compact_on());
        x->dense_full = form.dense_full;
        HIPCHK(dense_tiles_main(a->dev, c.key_mode, c.overlapping, w.dt, w.TD, c.lead, abort_flag, w.summary, form.compact, st));
        // (the hit regions' fill, SCR_OCC .. SCR_HITS_MAX; then SCR_DENSE_MATCHES, SCR_DENSE_OCC and the abort flag, SCR_ABORT)
        HIPCHK(hipMemcpyAsync(w.h_pinned, w.summary, 32, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(w.h_pinned + PIN_DENSE_MATCHES, w.summary + SCR_DENSE_MATCHES, 24, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        add_scan_profile(a, x, c.len, c.timed);
        const uint64_t hit_max = w.h_pinned[PIN_HITS_MAX];
        if (hit_max > hit_cap) { // hits were dropped: more room, again (the regions are balanced: a wave's tiles are spread over the stream)
            if ((rc = ensure_hits(x, (uint64_t)hit_grid * (hit_max + hit_max / 8 + 64))) != ACX_OK) return rc;
            *what = Attempt::Again;
            return ACX_OK;
        }
        if (form.compact && (uint32_t)w.h_pinned[PIN_DENSE_ABORT] == 2) { // a group's occurrences did not fit the compact stage: the kernel again, full
            x->dense_full = pol::DENSE_FULL_CALLS;
            HIPCHK(hipMemsetAsync(w.TD.sgw, 0, 2 * (uint64_t)w.TD.sg_cap * 8, st));
            HIPCHK(hipMemsetAsync(w.summary + SCR_ABORT, 0, 16, st));
            HIPCHK(dense_tiles_main(a->dev, c.key_mode, c.overlapping, w.dt, w.TD, c.lead, abort_flag, w.summary, false, st));
            HIPCHK(hipMemcpyAsync(w.h_pinned + PIN_DENSE_MATCHES, w.summary + SCR_DENSE_MATCHES, 24, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
        }
        if ((uint32_t)w.h_pinned[PIN_DENSE_ABORT] != 0) { // a bucket overflowed / a chain left its context: the radix-sort form
            c.no_dense_tiles = true;
            *what = Attempt::Again;
            return ACX_OK;
        }
        const uint64_t n_final = w.h_pinned[PIN_DENSE_MATCHES], n_raw = w.h_pinned[PIN_DENSE_OCC];
        if (std::max(n_raw, w.h_pinned[PIN_HITS]) >= occ_limit()) return fail_occ(); // (the tiles' counts and their prefixes are 32 bits wide)
        hold_after(n_raw);
        c.n_raw = n_raw;
        c.n_hits = w.h_pinned[PIN_HITS];
        c.n_final = n_final;
        *what = Attempt::Done;
        a->path[4]++;
        if (n_final == 0) return ACX_OK;
        HIPCHK(g_bufs.get((void **)&c.r->d_matches, n_final * sizeof(acx_match_t), a->device));
        if (seg_counts && (rc = zero_counts(c)) != ACX_OK) return rc;
        HIPCHK(dense_tiles_write(a->dev, c.key_mode, w.TD, c.d_hay, c.r->d_matches, w.summary, zero_flag, w.h_pinned + PIN_TOTALS, c.lead,
                                    c.G, seg_counts, nullptr, nullptr, st));
        c.localized = seg_counts != nullptr;
        c.queued = true;
        return ACX_OK;
    }

    // region mode -> compact -> radix sort -> resolve (two round trips)
    int radix(Attempt *what) {
        Workspace::OccBufs &o = w.occ;
        int rc = ensure_occ_capacity(x, std::max<uint64_t>(1u << 16, c.len / 64));
        if (rc) return rc;
        if (c.pre && (rc = ensure_hits(x, std::max<uint64_t>(1u << 16, c.len / 64))) != ACX_OK) return rc;
        const uint32_t hit_grid = c.pre ? prefilter_hit_regions(c.scan_grid) : 0;
        // K1a: the failureless walk here too (one occurrence region per block of k1a_walk); the chunked walk
        // when the automaton has none, or when its items did not fit
        if (pfac && (rc = ensure_hits(x, (pfac_workspace_words(c.len, pgrid, true) + 3) / 4)) != ACX_OK) return rc;
        const uint32_t grid = c.pre ? walk_hits_grid(hit_grid) : pfac ? pgrid * 16 : c.scan_grid; // occurrence regions
        const uint64_t hit_cap = c.pre ? w.hit_total() / hit_grid : 0;
        // exact_regions (second pass after an occurrence region overflowed): every region gets the room
        // it asked for in the first pass, at the exclusive prefix of the counts (stored behind the counts)
        const uint64_t region_cap = c.exact_regions ? 0 : w.cap / grid;
        const Sink H{w.hrecs, w.hit_counts, hit_cap, c.key_mode, nullptr, nullptr, nullptr, c.lead, 1, 0};
        uint32_t *items_overflow = (uint32_t *)(w.summary + SCR_ITEMS_OVERFLOW);
        const Sink K{o.recs, w.block_counts, region_cap, c.key_mode, nullptr, nullptr, pfac ? items_overflow : nullptr, c.lead, 1, 0};
        if (c.pre) {
            HIPCHK(launch_prefilter(a->dev, H, c.d_hay, c.len, c.scan_grid, st, prof ? scan_start_ev(x) : nullptr,
                                       prof ? scan_stop_ev(x) : nullptr));
            HIPCHK(launch_walk_hits(view(a, c.overlapping), c.G, H, hit_grid, K, grid, c.d_hay, c.len, st));
        } else {
            if (pfac) HIPCHK(hipMemsetAsync(w.summary + SCR_ITEMS_OVERFLOW, 0, 8, st));
            if ((rc = launch_k1a(K, grid, true)) != ACX_OK) return rc;
        }
        HIPCHK(sink_summary(w.block_counts, grid, c.exact_regions ? ~0ull : region_cap, c.pre ? w.hit_counts : nullptr,
                               hit_grid, hit_cap, w.summary, w.region_off, st));
        HIPCHK(hipMemcpyAsync(w.h_pinned, w.summary, 40, hipMemcpyDeviceToHost, st)); // (SCR_OCC .. SCR_ITEMS_OVERFLOW)
        HIPCHK(hipStreamSynchronize(st));
        add_scan_profile(a, x, c.len, c.timed);
        if (pfac && (uint32_t)w.h_pinned[PIN_ITEMS_OVERFLOW] != 0) { // more items than 1 per 16 bytes: the chunked walk has no such limit
            c.chunked_walk = true;
            c.exact_regions = false;
            *what = Attempt::Again;
            return ACX_OK;
        }
        const uint64_t n_raw = w.h_pinned[PIN_OCC], region_max = w.h_pinned[PIN_OCC_MAX], hit_max = c.pre ? w.h_pinned[PIN_HITS_MAX] : 0;
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
                HIPCHK(sink_summary(w.block_counts, grid, ~0ull, nullptr, 0, 0, w.summary + SCR_DENSE_MATCHES, bases, st));
                HIPCHK(hipMemcpyAsync(w.h_pinned + PIN_EXACT_TOTAL, bases + grid, 8, hipMemcpyDeviceToHost, st));
                HIPCHK(hipStreamSynchronize(st));
                c.exact_total = w.h_pinned[PIN_EXACT_TOTAL];
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
        hold_after(n_raw);
        c.n_raw = n_raw;
        c.n_hits = c.pre ? w.h_pinned[PIN_HITS] : 0;
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
            HIPCHK(hipMemcpyAsync(w.h_pinned + PIN_RADIX_FINAL, o.idx + n_raw, 4, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            c.n_final = *(uint32_t *)(w.h_pinned + PIN_RADIX_FINAL);
        }
        HIPCHK(g_bufs.get((void **)&c.r->d_matches, std::max<uint64_t>(c.n_final, 1) * sizeof(acx_match_t),
                             a->device));
        HIPCHK(write_matches(o.pids[0], o.S, o.E, c.overlapping ? nullptr : o.flags, c.overlapping ? nullptr : o.idx,
                                c.r->d_matches, n_raw, st));
        c.queued = true;
        return ACX_OK;
    }
};

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
    bool sparse = pol::start_sparse(a->sparse_ok, x->dense_hold, no_bucket_now(), c.tiles);
    for (int attempt = 0;; attempt++) {
        if (attempt == pol::MAX_ATTEMPTS) return fail(ACX_EDEVICE, "occurrence buffer overflow persisted");
        Attempt what = Attempt::Done;
        if ((rc = sparse ? SparseAttempt(c).run(&what) : DenseAttempt(c).run(&what)) != ACX_OK) return rc;
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
    if (a->prof && prof_post_on()) { // end of the post stage (costs the next call a wait for this one's last kernel)
        HIPCHK(hipEventRecord(x->ev[2], x->stream));
        x->post_pending = true;
    }
    return ACX_OK;
}

} // namespace acxh
