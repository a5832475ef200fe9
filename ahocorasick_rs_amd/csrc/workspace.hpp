// workspace.hpp -- what a call runs on: the process-wide pools (events, result buffers, pinned results), the owners of
// device and pinned memory, a context (stream + workspace + resident K0) and its lease, the automaton handle that owns
// the contexts.  workspace.cpp: the pools, create / destroy, every ensure_* of the workspace, the staging of host haystacks.
#pragma once
#include <condition_variable>
#include <unordered_map>

#include "fold.hpp"
#include "host_common.hpp"

namespace acxh ACX_HIDDEN {

// ---------------------------------------------------------------------------
// process-wide pools
// ---------------------------------------------------------------------------
// events that mark "this result's device work is done"
struct EventPool {
    std::mutex mu;
    std::vector<std::pair<int, hipEvent_t>> free_list;
    hipEvent_t get(int dev);
    void put(int dev, hipEvent_t e);
};
extern EventPool g_events;

// Small cache of device buffers for results, so that a find call does not pay
// hipMalloc/hipFree (each tens of microseconds and a device sync).  A buffer may come back
// while the kernel that fills it is still running (the call returned as soon as the totals
// were known): it waits in `deferred` until its event has fired.
struct BufCache {
    struct Ent { void *p; size_t bytes; int dev; };
    struct Deferred { void *p; void *p2; int dev; hipEvent_t ev; }; // (p2: a second buffer behind the same event, or null)
    std::mutex mu;
    std::vector<Ent> free_list;
    std::vector<Deferred> deferred;
    std::unordered_map<void *, Ent> live; // every buffer handed out by get()
    size_t cached = 0;
    static constexpr size_t MAX_CACHED = (size_t)4 << 30;

    void release_locked(void *p, int dev);
    void sweep_locked();
    hipError_t get(void **out, size_t bytes, int dev);
    // ev != null: work that writes the buffer may still be running; ev fires when it is done
    // (ownership of the event passes to the cache)
    void put(void *p, int dev, hipEvent_t ev = nullptr, void *p2 = nullptr);
};
extern BufCache g_bufs;

// Pinned host buffers handed to callers as acx_find results (the D2H copy lands in them and
// the caller reads them in place: no second copy).  acx_free_matches() gives them back.
struct PinnedResults {
    struct Ent { void *p; size_t bytes; bool used; };
    std::mutex mu;
    std::vector<Ent> all;
    size_t total = 0;
    static constexpr size_t MAX_TOTAL = (size_t)2 << 30;
    void *get(size_t bytes);
    bool put(void *p); // false: not one of ours
};
extern PinnedResults g_pinned_results;

// ---------------------------------------------------------------------------
// The owner of one block of device memory: a pointer and its capacity in elements.  Move-only; reads like the pointer.
// grow(n) takes the new block BEFORE it gives the old one back: a failed allocation leaves the buffer -- and whatever
// points into it -- as it was.  Nothing is copied over: the contents are the next call's to write.
template <typename T>
struct DevBuf {
    T *p = nullptr;
    uint64_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) { reset(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    ~DevBuf() { reset(); }
    operator T *() const { return p; }
    hipError_t grow(uint64_t n) {
        T *fresh = nullptr;
        const hipError_t e = hipMalloc((void **)&fresh, n * sizeof(T));
        if (e != hipSuccess) return e;
        (void)hipFree(p);
        p = fresh;
        cap = n;
        return hipSuccess;
    }
    void reset() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};
// ... and of one block of pinned host memory (hipHostMalloc with the flags the buffer needs: hipHostMallocCoherent for
// what the host polls while a kernel writes it)
template <typename T>
struct PinBuf {
    T *p = nullptr;
    uint64_t cap = 0;
    PinBuf() = default;
    PinBuf(const PinBuf &) = delete;
    PinBuf &operator=(const PinBuf &) = delete;
    PinBuf &operator=(PinBuf &&o) noexcept {
        if (this != &o) { reset(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    ~PinBuf() { reset(); }
    operator T *() const { return p; }
    hipError_t grow(uint64_t n, unsigned flags) {
        T *fresh = nullptr;
        const hipError_t e = hipHostMalloc((void **)&fresh, n * sizeof(T), flags);
        if (e != hipSuccess) return e;
        if (p) (void)hipHostFree(p);
        p = fresh;
        cap = n;
        return hipSuccess;
    }
    void reset() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
    }
};

// pinned host scratch of a context, in 64-bit words (Workspace::h_pinned): the POLLED lines, each written by one store and
// accepted on its check word (kernels.hpp) ...
constexpr uint32_t PIN_TOTALS = 24, PIN_HOT_TOTALS = 32, PIN_SPEC_TOTALS = 40, PIN_RESIDENT = 48, PIN_K0 = 64, PINNED_WORDS = 96;
// ... and words [0 .. 15]: what a copy or a kernel on the context's stream leaves and the host reads BEHIND a synchronisation
// of that stream.  Host-side names (the kernels keep their literals).  Users that share a word cannot meet: one call holds the
// context at a time, and each of them queues its write, synchronises and reads before it lets anything else onto the stream.
enum PinWord : uint32_t {
    PIN_OCC = 0, PIN_OCC_MAX = 1,   // radix form: occurrences kept / the fullest region (copies of SCR_OCC ..)
    PIN_HITS = 2, PIN_HITS_MAX = 3, // both dense forms: prefix hits kept / the fullest hit region
    PIN_ITEMS_OVERFLOW = 4,         // radix form, K1a: the failureless walk ran out of item room (u32)
    PIN_RADIX_FINAL = 6,            // radix form: the matches the greedy resolution kept (u32)
    PIN_DENSE_MATCHES = 8, PIN_DENSE_OCC = 9, PIN_DENSE_ABORT = 10, // tile-ordered form: its totals and abort flag (u32)
    PIN_EXACT_TOTAL = 10,           // radix form: the exact total of the regions' counts (an attempt of that form never reads
                                    // the tile-ordered form's flag: each reads right behind its own synchronisation)
    // words 8, 9 between pipeline runs -- none of these has an attempt in flight:
    PIN_K0_COUNT = 8, PIN_K0_DENSE = 9, // an unpolled K0: matches / too dense (the pipeline starts after they are read)
    PIN_EXPANDED = 8,                   // expand_copies: the records behind the expansion (the pipeline is over)
    PIN_SPLIT_CUT = 8,                  // run_batch_split: the first byte of the second part (before the parts run)
    PIN_RANGE_CUT = 8,                  // run_chunked: the two words of SCR_RANGE_CUT (between two pieces)
};
// device scratch of a context, in 64-bit words (Workspace::summary, 16 of them)
enum ScratchWord : uint32_t {
    SCR_OCC = 0, SCR_OCC_MAX = 1, SCR_HITS = 2, SCR_HITS_MAX = 3, // sink_summary: the fill of the occurrence / hit regions
                                    // (k_tile_write leaves its occurrences and hits in [0], [2] as well; nobody reads them)
    SCR_ITEMS_OVERFLOW = 4,         // radix form, K1a: the walk's item-overflow flag (u32), cleared in front of the walk -- and
                                    // where k_tile_write leaves its matches, which no host code reads
    SCR_DENSE_MATCHES = 8, SCR_DENSE_OCC = 9, // tile-ordered form: its totals; the radix form's second summary (exact
                                    // regions) scribbles here, in an attempt of its own
    SCR_ABORT = 10, SCR_ZERO = 11,  // (u32 each) the abort flag of the hot pipeline and of the tile-ordered form, and a flag
                                    // that stays zero for its write kernel: the dense form clears both in front of its kernels,
                                    // the sparse write kernel when it announces hot groups -- one stream, one after the other
    SCR_RANGE_CUT = 12,             // run_chunked: the two words cut_point leaves (13 as well)
};
// The structs the kernels take by value (DenseTiles, TileSpace: device_types.hpp) stay plain views; the memory behind a view's
// pointers is owned by the group of buffers next to it, and the view is filled from the group once all of it is allocated.
struct Workspace {
    // dense path (region mode + radix sort): `cap` occurrences, allocated and given back as one group (ensure_occ_capacity)
    uint64_t cap = 0;
    struct OccBufs {
        DevBuf<uint64_t> keys[2];
        DevBuf<uint32_t> pids[2];
        DevBuf<uint64_t> S, E, M;
        DevBuf<uint32_t> flags, idx;
        DevBuf<uint4> recs;           // occurrence sink: cap records of 16 B in per-workgroup regions
    } occ;
    DevBuf<uint8_t> temp;             // sort / scan temp storage, in bytes (the dense group's; grown by ensure_blocks too)
    DevBuf<uint4> hrecs;              // dense path, K1b prefix-hit sink: hit_total() records of 32 B (two elements each)
    uint64_t hit_total() const { return hrecs.cap / 2; }
    DevBuf<uint64_t> hit_counts;      // device: one per K1b wave
    DevBuf<uint64_t> summary;         // device: 16 words of scratch for totals and flags (ScratchWord above: sink fill, the walk's
                                      // overflow flag, the dense totals, the abort and zero flags, the cut of a byte range)
    DevBuf<uint64_t> block_counts;    // device: one per scan workgroup
    DevBuf<uint64_t> region_off;      // device: exclusive prefix of the kept counts
    PinBuf<uint64_t> h_pinned;        // pinned host scratch (PINNED_WORDS x u64, 64-byte lines): [0 .. 15] words read behind a stream
                                      // synchronisation (PinWord above: the dense paths' totals, an unpolled K0's result, the
                                      // borrowers between pipeline runs), then the POLLED lines (PIN_TOTALS ..):
                                      // [64 .. 95] K0's result (up to four lines), [24 .. 31] the sparse path's totals, [32 .. 39] the hot pipeline's
                                      // early total (hot_totals), [40 .. 47] the speculative hot pipeline's, [48] the epoch of
                                      // the last resident K0 that has left (Resident)
    uint64_t t_line[8] = {};          // the sparse path's totals: the verified copy of the line (PIN_TOTALS / PIN_HOT_TOTALS)
    uint64_t h_lines[K0_RESULT_LINES][8] = {}; // K0, polled: the verified copies of the call's result lines (words 1 .. 6 of each)
    PinBuf<acx_match_t> pin_final;    // host entry point, mid-size calls: pinned host memory the write kernel's records go to
    PinBuf<uint8_t> pin_mid;          // mid-size calls: pinned copy of a host haystack the scan reads in place
    PinBuf<uint64_t> mailbox;         // small calls: coherent pinned memory -- the resident K0's command word (kernels.hpp), then
    uint8_t *pin_hay = nullptr;       //   (K0_MAILBOX_HAY bytes behind it, in the same block) the copy of a host haystack K0 reads in place
    PinBuf<acx_match_t> pin_out;      // small calls: pinned output of K0 (host entry point)
    DevBuf<uint64_t> blockcnt, blockpre; // lead bytes per 1 KiB block / their prefix
    DevBuf<uint8_t> blocksub;            // lead bytes per 64 bytes of a block
    uint64_t block_cap = 0;              // blocks (+ 1) the three are allocated for
    // dense path, tile-ordered: occurrence buckets by key tile; its groups' reported occurrences (64-bit words), counts,
    // supergroup words
    struct DenseBufs {
        DevBuf<uint64_t> words, sgw;
        DevBuf<uint32_t> counts, btot;
        DevBuf<uint4> trecs;
    } dense_bufs;
    DenseTiles dt{};                  // (views of dense_bufs)
    TileSpace TD{};
    uint64_t dt_cap = 0;              //   tiles both are allocated for
    // sparse path (hit slots + tile kernels)
    struct TileBufs {
        DevBuf<uint4> hslots, trecs;
        DevBuf<uint32_t> hcnt, btot;
        DevBuf<uint64_t> sgw;
    } tile_bufs;
    TileSpace T{};                    // (view of tile_bufs)
    uint64_t tile_cap = 0;            // tiles T is allocated for
    uint64_t group_cap = 0;           // groups T.gstate is allocated for
    uint32_t trecs_gmax = 0;          // records per group T.trecs is allocated for (GROUP_MAX; GROUP_MAX_WIDE once a call needed it)
    bool flags_dirty = true;          // the control blocks' counters are not known to be zero
    DevBuf<uint32_t> ctl;             // device: the sparse path's two control blocks (device_types.hpp), used by the calls in turn
    DevBuf<uint4> ovf_recs;           // K1b's hits beyond a tile's slots: OVF_LISTS lists of ovf_cap() records of 32 B
    uint64_t ovf_cap() const { return ovf_recs.cap / (2 * OVF_LISTS); } // records per list
    DevBuf<uint32_t> ovf_counts;      //   the lists' fill counters, two sets (one per control block), a cache line each
    DevBuf<uint32_t> hot_list;        // groups left to the hot pipeline (group_cap ids)
    acx_match_t *final = nullptr;     // sparse path: output buffer the next call writes into.  The BUFFER CACHE's (g_bufs),
    uint64_t final_cap = 0;           //   taken from it and given back to it: handed over to the call's result when it is written
    DevBuf<uint8_t> hay;              // device staging buffer of the host-memory entry points
    DevBuf<uint8_t> fold;             // case-insensitive handles: the folded copy of a device haystack (grow-only: as large as
                                      //   the largest device haystack of the context)
    DevBuf<uint64_t> offsets;
};

// The resident K0 of a context (kernels.hip, k0_resident): one workgroup that stays on the device between the calls of a
// loop over short haystacks and is fed through the workspace's mailbox, so that a call costs a poll on either side instead
// of a launch.  At most one of them per context, and nothing else of the context runs beside it (streams may share a
// hardware queue: whatever else the context launches first tells the kernel to leave -- stop_resident).  It leaves by
// itself after idle_us without a call and life_us after its launch (ACX_RESIDENT_IDLE_US, ACX_RESIDENT_LIFE_US;
// ACX_NO_RESIDENT=1: every small call is a launch, as until round 5).
struct Resident {
    hipStream_t stream = nullptr; // its own: created with the first launch
    uint64_t epoch = 0;           // the number of the last launch; h_pinned[PIN_RESIDENT] == epoch: that kernel has left
    bool live = false;            // a kernel has been launched and has not been seen to have left
    int mode = -1, overlapping = 0; // what it was launched for (small_mode; the tables' view and the key follow from overlapping)
    uint32_t delay = 0;           // ticks the kernel waits behind a result before it polls (k0_resident: what the last kernel
                                  // ended with -- h_pinned[PIN_RESIDENT + 5])
    uint64_t secret = 0;          // keys the check of the haystack bytes that travel with the poll (kernels.hpp, k0_hay_check)
    uint32_t switches = 0, calls = 0; // launches for another mode within the last calls: a loop that alternates between two
    uint32_t off = 0;                 //   kinds of call pays a launch per call either way -- small calls left as plain launches
};

// everything one in-flight call needs
struct Ctx {
    hipStream_t stream = nullptr, copy_stream = nullptr; // copy_stream: the second stream (the str API's code-point prefix)
    Resident res;
    // profiling: [0], [1] and [3], [4]: scan start / stop, two pairs used by the calls in turn (the time
    // of a call's scan is read while the NEXT call's kernels run, off the path between two calls);
    // [2]: end of the call
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    uint32_t prof_calls = 0;   // calls of this context while profiling was on (sampling)
    int ev_pair = 0;           // the pair the next scan launch takes
    bool scan_pending = false; // a scan's time has not been read yet
    int pend_pair = 0;
    uint64_t pend_len = 0;
    hipEvent_t fork_ev = nullptr, join_ev = nullptr; // str API: the code-point prefix runs beside k_tile_main
    Workspace ws;
    bool post_pending = false; // profiling: ev[2] of the last call has not been read yet
    int dense_hold = 0;        // > 0: the output was too dense for the sparse path; calls left in region mode
    bool hold_dense_input = false; // why: the INPUT was dense (the hold ends with the first call that is not) -- or the sparse
                                   // kernels gave up on it for another reason (counted down: one failed attempt in nine calls)
    uint32_t spec_hot = 0;     // > 0: the last call had this many hot groups (few): the next one queues the hot pipeline ahead of
                               // knowing that it needs it (kernels.hip: hot_groups_here), spec_ovf: that call's fullest overflow list
    uint32_t spec_ovf = 0;
    uint64_t hot_inline = 16;  // hot groups the output buffer of a sparse attempt has room for (HOT_INLINE .. HOT_INLINE_MAX)
    int dense_full = 0;        // > 0: calls left for which the tile-ordered dense path runs k_dense_main in its full form (a group
                               // did not fit the compact stage)
    bool wide = false;         // the sparse path's post stage runs in its WIDE form (device_types.hpp: GROUP_MAX_WIDE): the last
                               // call's groups mostly gave up on the narrow one (a match every 100 - 500 bytes)
    int flag_idx = 0;          // which of the two abort flags the next sparse attempt uses
    uint64_t seq = 0;          // sequence number the write kernel publishes in the totals' line (h_pinned + PIN_TOTALS)
    uint64_t small_seq = 0;    // K0 (host entry point): the number its result line carries (h_pinned + PIN_K0)
};

} // namespace acxh

// the host compiler's output alone (acx_compile_host_ex): no device is involved
struct ACX_HIDDEN acx_host_automaton {
    acx::Automaton host;
    uint32_t flags = 0; // ACX_BUILD_*: a case-insensitive one was compiled from the folded patterns
};

struct ACX_HIDDEN acx_automaton {
    acx::Automaton host;
    int device = 0;
    acx::DevAutomaton dev{};
    const acx::DevAutomaton *d_dev = nullptr; // the same struct, resident in HBM
    // Copies of a pattern (Standard automata keep them: an overlapping search reports every copy).  A NON-overlapping
    // search can only ever report the lowest id of a string, and the device enumerates every occurrence it is given --
    // hundreds of copies of every pattern on text where every position matches were hundreds of times the work
    // (tools/gpu_fuzz.py, seed 40404).  dev_nov = dev with two tables replaced: own1 holds the lowest id of every
    // state's string (all patterns that end in a trie state ARE one string: never OWN1_MANY), and blist has every
    // candidate list's first-of-their-string ids in front and counts only those (same list indexes: the prefix table
    // and the short patterns' codes are shared).  The DFA walk reports through the own lists (own_off / own_pid: one
    // entry per state in the view) and through its trie records (grec: own1 in their third word).  Taken by the
    // kernels that read those tables (K0, k_tile_main, k_walk_hits, k_dense_verify; k1a_walk, the walks' emit
    // paths through the device-resident copy d_dev_nov) when the call is not overlapping; has_nov = false: no copies.
    // Round 5: an OVERLAPPING search takes the view too -- one occurrence per string under its lowest id -- and the result
    // is expanded where it is complete (expand_copies: every occurrence becomes the run of its string's copies, ids
    // ascending, as the reference reports them): the copies cost their records, not a verification, a sort slot and a
    // 2^32-limited index each.  x_cnt[pid] = the later copies of a lowest id (0 otherwise), x_off[pid] = where their ids
    // begin in x_ids (host: K0's pinned result is expanded on the host; d_x*: the same in HBM).
    acx::DevAutomaton dev_nov{};
    const acx::DevAutomaton *d_dev_nov = nullptr;
    bool has_nov = false;
    // expand_ov: overlapping searches do that -- when at least a quarter of the ids are later copies (ACX_EXPAND_COPIES=1 / 0:
    // whenever there is one / never).  The expansion is a pass over the complete result and a round trip for its size
    // (cfg4's 100 000 random patterns hold half a dozen accidental duplicates: 0.79 -> 0.87 ms when it was taken for them);
    // a set with a few copies enumerates them on the device as before, at the cost of those few.
    bool expand_ov = false;
    std::vector<uint32_t> x_cnt, x_off, x_ids;
    const uint32_t *d_xcnt = nullptr, *d_xoff = nullptr, *d_xids = nullptr;
    std::vector<void *> allocs;
    int kernel = ACX_KERNEL_DFA_WALK;
    int implementation = ACX_IMPL_AUTO; // the caller's hint (replicas are built with the same one)
    uint32_t flags = 0;                 // ACX_BUILD_* (acx_build_ex; replicas are built with the same ones)
    int n_cus = 1;
    size_t max_lds = 65536;
    uint64_t table_bytes = 0;
    bool kernel_forced = false; // the scan kernel was chosen explicitly: K0 never takes a call
    bool sparse_ok = true;      // tile_lookback(max_len) <= MAX_LOOKBACK
    // contexts
    std::mutex pool_mu;
    std::condition_variable pool_cv;
    std::vector<acxh::Ctx *> ctxs, idle;
    int max_ctx = 4;
    // profiling (accumulated over the contexts)
    std::mutex prof_mu;
    std::atomic<bool> prof{false};
    std::atomic<int> prof_every{1}; // profiling events on every N-th call of a context
    acx_profile_t profile{};
    std::atomic<uint64_t> path[ACX_PATH_STATS] = {}; // acx_path_stats
};

namespace acxh ACX_HIDDEN {

// A case-insensitive handle (acx_build_ex): compiled from the folded patterns, it searches folded haystacks (fold.hpp).
inline bool folds(const acx_automaton *a) { return (a->flags & ACX_BUILD_ASCII_CASE_INSENSITIVE) != 0; }
// the calling thread's copy of a host haystack into pinned memory the device reads: a folding copy for such a handle
inline void copy_in(const acx_automaton *a, uint8_t *dst, const uint8_t *src, uint64_t len) {
    if (folds(a)) fold_host(dst, src, len);
    else std::memcpy(dst, src, len);
}
// the device tables a call takes: a non-overlapping search never needs the later copies of a string (acx_automaton::dev_nov)
// (an overlapping search as well since round 5: its result is expanded to the copies afterwards -- expand_copies)
inline const DevAutomaton &view(const acx_automaton *a, bool overlapping) {
    return (overlapping ? a->expand_ov : a->has_nov) ? a->dev_nov : a->dev;
}
inline const DevAutomaton *d_view(const acx_automaton *a, bool overlapping) { // (the same, resident in HBM)
    return (overlapping ? a->expand_ov : a->has_nov) ? a->d_dev_nov : a->d_dev;
}

Ctx *create_ctx(); // the automaton's device is current
void destroy_ctx(Ctx *c, int device);

// a context of the automaton for the duration of one call (and the automaton's device as the
// calling thread's current device)
struct Lease {
    acx_automaton *a;
    Ctx *c = nullptr;
    DeviceScope dev;
    // keep_resident: the call may go to the context's resident K0 (acx_find); every other call has the context to itself
    explicit Lease(acx_automaton *a_, bool keep_resident = false);
    ~Lease();
};

int ensure_common(Ctx *c);
int ensure_hits(Ctx *c, uint64_t want);          // dense path: prefix-hit sink of K1b
int ensure_occ_capacity(Ctx *c, uint64_t want);  // dense path: occurrence regions + the radix sort / resolve pipeline
int set_overflow_room(Ctx *c, uint64_t want);    // sparse path: want records per overflow list; the stream is idle
int ensure_tiles(acx_automaton *a, Ctx *c, uint64_t tiles, uint32_t gmax);
int ensure_dense_tiles(Ctx *c, uint64_t tiles);
void free_dense_tiles(Workspace &w);
int ensure_blocks(Ctx *c, uint64_t nblocks_plus1);
int ensure_mailbox(Ctx *c);                      // small calls of the host entry point: mailbox + pinned haystack, pinned output

int stage_host(acx_automaton *a, Ctx *c, const uint8_t *hay, uint64_t len, const uint64_t *offsets, uint64_t n_off,
               bool fold_in_place = true);
int place_host_haystack(acx_automaton *a, Ctx *c, const uint8_t *hay, uint64_t len, const uint8_t **d_hay);
int fold_copy(acx_automaton *a, Ctx *c, const uint8_t *d_hay, uint64_t len, const uint8_t **d_search);

} // namespace acxh
