// result_block.hpp -- what the stages behind the find pipeline (summaries, splice, columns, tally, row filter, scores) share: the
// owner of a result's memory and the table of its parts, the layout of its block, the frame from a find to a stage's result
// (find_stage) and its end (retire_find), the owner of the host route's records (HostFind), the checks of a stage's
// arguments and the frames of its entry points -- and, at the end, the frames of the stages that run no find (the walkers:
// at_api.cpp, seg_api.cpp, wp_api.cpp).
// The stages' middles are their own (summary_api.cpp .. filter_api.cpp); no kernel includes this.
#pragma once
#include <initializer_list>

#include "find_pipeline.hpp"
#include "stage_device.hpp"
#include "words.hpp"

namespace acxh ACX_HIDDEN {

// Where the parts of a block begin, in bytes, and the block's size: every part at least one word long (an empty part still
// has an address that DLPack consumers accept) and a multiple of 256 bytes behind the previous one.  The last part is
// rounded up to `tail` bytes.
struct Layout {
    uint64_t at[5] = {0, 0, 0, 0, 0}, bytes = 0;
};
constexpr Layout block_layout(std::initializer_list<uint64_t> part_bytes, uint64_t tail = 256) {
    Layout L;
    int k = 0;
    for (const uint64_t b : part_bytes) {
        const uint64_t step = k + 1 < (int)part_bytes.size() ? 256 : tail;
        L.at[k++] = L.bytes;
        L.bytes += ((b > 8 ? b : 8) + step - 1) / step * step;
    }
    return L;
}

// The owner of a result's memory.  Device route: blocks of the buffer cache (g_bufs, workspace.cpp), written by kernels that
// may still run when the call returns -- `done` fires behind the last of them; `scratch` is what those kernels still read.
// Host route: a block of host memory, nothing to wait for.
// `part`: where every part of the block lies and how many bytes of it count -- written once, by alloc_parts, and read by the
// stages (at<T>) and by the accessors (part_ptr, part_copy).  A part the form at hand lacks has no address.
struct ResultBlock {
    struct Part {
        uint8_t *at = nullptr;
        uint64_t bytes = 0;
    };
    Part part[5];
    uint64_t block_bytes = 0;
    int device = 0;
    int on_device = 0;
    uint8_t *h_block = nullptr;
    void *d_block = nullptr;
    hipEvent_t done = nullptr;
    std::vector<void *> scratch;

    int alloc(uint64_t bytes); // the block: of the cache (on_device) or of host memory
    uint8_t *base() const { return on_device ? (uint8_t *)d_block : h_block; }
    // the block as block_layout cuts it for parts of these sizes, and the table of them
    int alloc_parts(std::initializer_list<uint64_t> part_bytes, uint64_t tail = 256);
    // a part that was given room before its size was known (the host tally: room for a run per record): what of it counts
    void resize_part(int k, uint64_t bytes) { part[k].bytes = bytes; }
    template <class T>
    T *at(int k) const { return (T *)part[k].at; }
    // every accessor's wait for the stage's last kernel
    int wait() const;
    // `bytes` at `src` (a part of this result) to host memory, behind the kernels; zero bytes: nothing
    int copy_out(void *dst, const void *src, uint64_t bytes) const;
    // p once the kernels are done; null when the wait fails
    const void *ptr_after_wait(const void *p) const { return p && wait() == ACX_OK ? p : nullptr; }
    // waits, then gives scratch, block and event back to their pools and frees the host block (the kernels write the block
    // and read the scratch: nothing goes back to a pool before they are done)
    void release();
};

// A stage's result (a ResultBlock with the stage's own fields), empty; null: out of memory, the error is set.
template <class T>
T *new_result(int device, bool on_device) {
    T *R = new (std::nothrow) T();
    if (!R) { (void)fail(ACX_ENOMEM, "out of memory"); return nullptr; }
    R->device = device;
    R->on_device = on_device;
    return R;
}
// ... and its end (acx_free_*): behind the kernels that write it; null: nothing
template <class T>
void free_result(T *r) {
    if (!r) return;
    r->release();
    delete r;
}

// The bodies of the accessors by part (acx_*_data, acx_*_copy and the named ones; which: 0 .. n - 1, R may be null).
// The part's address once the kernels are done; null: no result, no such part, a part this form lacks, a failed wait.
const void *part_ptr(const ResultBlock *R, int which, int n);
// ... and the part in host memory.  The refusals, all ACX_EINVAL, in this order: no result or no such part (no_such), a part
// this form lacks (missing), bytes to copy and nowhere to ("null argument").  The texts are the result type's own.
int part_copy(const ResultBlock *R, int which, int n, void *host_dst, const char *no_such, const char *missing = nullptr);

using acx::Carver; // (stage_device.hpp: the walkers' plans carve with it too)

// The end of a stage behind a find, whatever its outcome `rc`.  st: the stream the find and the stage ran on; r: the find's
// result (null: an empty batch; a stage that keeps the counts has taken them out of r); R: the stage's result; t1, t2: the
// stage's temporaries (or null).
// rc == ACX_OK: events are recorded HERE, behind the stage's last launch, and every buffer is returned WITH such an event:
// the records and counts of r behind one, the temporaries behind another -- the cache holds them until it has fired -- and
// R->done is a third.  A dry event pool costs a stream synchronisation instead.
// Otherwise, and when recording fails: the stream is synchronised first, then the temporaries and r's buffers go back.
// Either way r is freed, every event taken from g_events is R's, the cache's or back in the pool, and R stays the caller's.
int retire_find(int rc, hipStream_t st, acx_result *r, ResultBlock *R, void *t1 = nullptr, void *t2 = nullptr);

// The per-haystack counts of a find, on the device: the result's own or, for one haystack that is no batch (the find kept
// none), its total uploaded to *one -- a temporary for retire_find.
int counts_of(const acx_result *r, hipStream_t st, uint64_t **one, const uint64_t **d_counts);

// What find_stage hands a stage's body.
template <class T>
struct FindStage {
    T *R;                    // the stage's result, empty
    hipStream_t st;          // the stream the find ran on, and the stage's
    acx_result *r;           // the find's result; null: there was nothing to search
    void *temp = nullptr;    // the body's: its temporaries, one block of the cache (or null), named as soon as it exists
    uint64_t *one = nullptr; // the frame's: the single count that counts() uploaded

    // the find's per-haystack counts on the device (r != null)
    int counts(const uint64_t **d_counts) { return counts_of(r, st, &one, d_counts); }
    // a buffer of the cache that the result's kernels read after the call: the result's from here on (null: nothing).  The
    // body hands it over straight behind the call that made it, BEFORE it looks at that call's outcome.
    void keep(void *p) {
        if (p) R->scratch.push_back(p);
    }
};

// The frame from a find to a stage's result, for the run_* functions of the stages whose find is spent by them (columns,
// spans, snippets, tally, filter, mask, score, summary).  `search`: the stage's own word on whether there is anything to
// search -- false: no find, the body gets r == null.
// The find first, then the result (a result that cannot be made frees the find's), then body(F) queues the stage on F.st
// and returns its outcome; whatever that is, retire_find ends the stage with F.temp and F.one as its temporaries, and what
// the body kept is R's: free_result gives it back when the body failed halfway.  *out: the result, or null on failure.
template <class T, class Body>
int find_stage(acx_automaton *a, Ctx *x, const uint8_t *d_search, uint64_t len, const Segments &G, int overlapping, int codepoints,
               bool search, T **out, Body &&body) {
    *out = nullptr;
    acx_result *r = nullptr;
    if (search) {
        const int found = run_find(a, x, d_search, len, G, overlapping, codepoints, &r);
        if (found != ACX_OK) return found;
    }
    T *R = new_result<T>(a->device, true);
    if (!R) { acx_free_result(r); return ACX_ENOMEM; }
    FindStage<T> F{R, x->stream, r};
    const int queued = body(F); // (in a statement of its own: F.temp and F.one are read behind it)
    const int rc = retire_find(queued, F.st, r, R, F.temp, F.one);
    if (rc != ACX_OK) { free_result(R); return rc; }
    *out = R;
    return ACX_OK;
}

// The rows a stage makes of a find's segments: G.n_hay of them, or -- neither offsets nor a row length: no batch -- one.
struct Rows {
    bool segmented;
    uint64_t n;
};
inline Rows rows_of(const Segments &G) {
    const bool segmented = is_segmented(G);
    return Rows{segmented, segmented ? G.n_hay : 1};
}
// ... and how they cut the `len` bytes of the find (stage_device.hpp)
inline acx::RowCut row_cut(const Segments &G, uint64_t len) {
    const Rows r = rows_of(G);
    return acx::RowCut{r.segmented ? G.offsets : nullptr, r.segmented ? G.uniform_len : 0, r.n, len};
}

// Where every row's records begin: the scan of d_counts (rows words, rows > 0) into rec_off (rows + 1 words) on st;
// scan_tmp: replace_scan_words(rows) words.  check_sum: the counts are a caller's -- their sum is read back (st is waited
// for) and must be n before a kernel reads a record by them.
int record_offsets(const uint64_t *d_counts, uint64_t rows, uint64_t n, bool check_sum, int64_t *rec_off, uint64_t *scan_tmp,
                   hipStream_t st);

// The *_host forms' check that n_hay counts sum to n_m, whatever the counts are (no sum wraps).  Null counts: one haystack
// holds every match -- there must be one, or no match.
int counts_sum_to(const uint64_t *counts, uint64_t n_hay, uint64_t n_m);
// ... and that n_hay + 1 offsets rise from 0 to len
int offsets_span(const uint64_t *offsets, uint64_t n_hay, uint64_t len);

// How a *_rows_device entry's bytes are cut, in front of its other checks: offsets and a row length exclude one another,
// neither is one row (*n_hay becomes 1), and rows of one length fill the batch.
int device_rows_args(const uint64_t *d_offsets, uint64_t *n_hay, uint64_t uniform_len, uint64_t len);
// ... and, on the data's device: device offsets (null: nothing) begin at 0 and end at len -- two words are read back; between
// the two they are the caller's word
int device_offsets_span(const uint64_t *d_offsets, uint64_t n_hay, uint64_t len);

// The frame of a *_rows_device entry behind its argument checks: on the device that holds `where`, body(device, &t1, &t2)
// queues the stage on the null stream and names its temporaries (blocks of the buffer cache, or null); the stream is waited
// for whatever the body returned, then the temporaries go back to the cache.  The body's error comes first.
template <typename Body>
int rows_call(const void *where, Body &&body) {
    hipPointerAttribute_t at;
    HIPCHK(hipPointerGetAttributes(&at, where));
    DeviceScope ds(at.device);
    void *t1 = nullptr, *t2 = nullptr;
    int rc = body(at.device, &t1, &t2);
    const hipError_t e = hipStreamSynchronize(nullptr);
    g_bufs.put(t1, at.device);
    g_bufs.put(t2, at.device);
    if (rc == ACX_OK && e != hipSuccess) rc = hipfail(e, "hipStreamSynchronize");
    return rc;
}

// The score stage (score.hpp; score_api.cpp) behind a find's records and counts, for acx_score_device, acx_score_rows_device
// and the hook of acx_filter_scored_device.  Its temporaries are one block of the buffer cache -- the caller's to return,
// behind the stage's kernels.
struct ScoreTemps {
    void *block = nullptr;
    int64_t *score = nullptr;  // the scores: d_score, or a part of the block
    uint64_t *flags = nullptr; // score >= *min_score as 0 / 1 words (min_score != null): the row filter's counts
};
// d_m: n records; d_counts: rows words (rows > 0) that sum to n (check_sum: record_offsets below).  The weights, n_patterns
// of them: h_weights (host memory that stays valid until the stream has passed the copy) or d_weights (device memory).
// d_score: rows words, or null: in the block.
int score_stage(int device, hipStream_t st, const acx_match_t *d_m, uint64_t n, const uint64_t *d_counts, uint64_t rows,
                const int32_t *h_weights, const int32_t *d_weights, uint64_t n_patterns, bool check_sum, int64_t *d_score,
                const int64_t *min_score, ScoreTemps *T);

struct HostBatch;

// The whole-word stage (words.hpp; words_api.cpp) behind an OVERLAPPING find's records and counts, for acx_words_rows_device,
// acx_find_words_device (columns_api.cpp) and the hook of acx_filter_words_device (filter_api.cpp).
struct WordsArgs {
    int overlapping = 0; // 1: every whole-word occurrence; 0: those `kind` picks
    int kind = ACX_MATCH_STANDARD;
    acx::WordSet W{};
};
// match_kind is one of the three (ACX_EINVAL); word_set: 32 bytes, or null: ASCII [0-9A-Za-z_]
int words_args(int overlapping, int match_kind, const uint8_t *word_set, WordsArgs *A);
// What words_sizes leaves for words_finish: the items, their flags and ranks, the rows.  `block`: the stage's temporaries,
// one block of the buffer cache -- the caller's to return, behind the stage's kernels.
struct WordsStage {
    void *block = nullptr;
    const uint8_t *flag = nullptr;
    const acx_match_t *items = nullptr;
    const uint32_t *src = nullptr;
    const int64_t *base = nullptr, *rows_off = nullptr;
    int64_t *new_off = nullptr;    // rows + 1 words of the block, for a caller that wants the counts alone
    uint64_t *new_counts = nullptr; // rows words of the block, for a caller that has nowhere else to put them
    uint64_t n_items = 0, rows = 0, total = 0;
};
// The stage up to the point where the result's size is known (n > 0, R.n > 0).  d_m: n records; d_counts: R.n words that sum
// to n (check_sum: record_offsets above); d_hay: the caller's own R.len bytes.  The stream is waited for: G->total is valid.
int words_sizes(int device, hipStream_t st, const acx_match_t *d_m, uint64_t n, const uint64_t *d_counts, const acx::RowCut &R,
                bool check_sum, const uint8_t *d_hay, const WordsArgs &A, WordsStage *G);
// ... and from there: the G.total records to `out`, their rows' offsets (G.rows + 1 words, or null) and counts (G.rows words,
// or null) -- device memory, 8-byte aligned
int words_finish(const WordsStage &G, const acx::WordsOut &out, int64_t *row_offsets, uint64_t *counts, hipStream_t st);
// ACX_WORDS_HOST_MAX (bytes, read per call): host haystacks up to this size take the host route of acx_find_words /
// acx_filter_words.  The default is ACX_SUMMARY_HOST_MAX's, which is itself not a measured crossover.
uint64_t words_host_max();
// The host route's middle: an overlapping find of B's rows as it is (each route under its own lease), then acx_words_host.
// out: the surviving records; counts: n_hay + 1 words, the rows' new counts.
int words_host_find(acx_automaton *a, const HostBatch &B, uint64_t len, uint64_t n_hay, bool batch, const WordsArgs &A,
                    const uint8_t *word_set, std::vector<acx_match_t> *out, std::vector<uint64_t> *counts);

// A host entry point's haystacks as the stages take them: offsets (n_hay + 1 of them, monotone; null: ONE haystack of *len
// bytes, *n_hay becomes 1) cut `hay`; afterwards *len bytes at B->hay (null when there are none) are the haystacks, cut by
// B->rel: *n_hay + 1 offsets from 0.
struct HostBatch {
    const uint8_t *hay = nullptr;
    std::vector<uint64_t> rel;
};
int host_batch(const uint8_t *hay, uint64_t *len, const uint64_t *offsets, uint64_t *n_hay, HostBatch *B);

// The frame of a *_device entry point behind its own argument checks: the haystack's and the segments' checks, the
// overlapping check (the error, no device state), the lease and the folded copy of a case-insensitive handle; then
// run(ctx, d_search, segments) under the lease.
template <typename Run>
int device_call(acx_automaton *a, const void *d_hay, uint64_t len, const uint64_t *d_offsets, uint64_t n_hay,
                uint64_t uniform_len, int overlapping, Run &&run) {
    if (len && !d_hay) return fail(ACX_EINVAL, "null haystack");
    Segments G;
    int rc = make_segments(d_offsets, n_hay, uniform_len, len, &G);
    if (rc == ACX_OK && overlapping) rc = check_overlapping(a);
    if (rc != ACX_OK) return rc;
    Lease lease(a);
    if (!lease.c) return fail(ACX_EDEVICE, "could not create a stream for the call");
    const uint8_t *d_search = nullptr;
    rc = fold_copy(a, lease.c, (const uint8_t *)d_hay, len, &d_search);
    if (rc != ACX_OK) return rc;
    return run(lease.c, d_search, G);
}

// The host route's find and the owner of its records: m goes back (acx_free_matches) when this goes, on every exit.
struct HostFind {
    acx_match_t *m = nullptr;
    uint64_t nm = 0;
    std::vector<uint64_t> counts; // a word per haystack and one more (an empty batch still has a pointer to give)

    HostFind() = default;
    HostFind(const HostFind &) = delete;
    HostFind &operator=(const HostFind &) = delete;
    ~HostFind() { acx_free_matches(m); }
    // acx_find (offsets == null: one haystack of len bytes, counts[0] becomes its matches) or acx_find_batch as they are --
    // the small-call kernel, its resident form, the in-place read, the staged pipeline, each under its own lease.
    // search == false: the entry's word that there is nothing to search (no row, or no byte) -- no record, zero counts.
    int find(acx_automaton *a, const uint8_t *hay, uint64_t len, const uint64_t *offsets, uint64_t n_hay, int overlapping,
             int codepoints, bool search = true);
};

// The staged device route of a host entry point, the mirror of device_call: the lease, the haystacks (and, for a batch,
// B's offsets) staged, the folded copy of a case-insensitive handle; then run(ctx, d_search, segments) under the lease --
// the staged bytes are ctx->ws.hay.  A run whose result goes home (copy_down) waits for it there: the staging buffers are
// the context's.  No batch: ONE haystack, no offsets.
template <typename Run>
int staged_call(acx_automaton *a, const HostBatch &B, uint64_t len, uint64_t n_hay, bool batch, Run &&run) {
    Lease lease(a);
    Ctx *c = lease.c;
    if (!c) return fail(ACX_EDEVICE, "could not create a stream for the call");
    int rc = stage_host(a, c, B.hay, len, batch ? B.rel.data() : nullptr, batch ? n_hay + 1 : 0, false);
    if (rc != ACX_OK) return rc;
    const uint8_t *d_search = nullptr;
    if ((rc = fold_copy(a, c, c->ws.hay, len, &d_search)) != ACX_OK) return rc;
    return run(c, d_search, batch ? Segments{c->ws.offsets, n_hay, 0} : Segments{nullptr, 1, 0});
}

// The end of a staged call whose result goes home: `bytes` of D's block (the device result, waited for under the lease;
// null when rc says the call failed) come down into R's (its host twin; null: out of memory) in one copy.  D is freed
// either way; *out becomes R, which is freed on failure.
template <class T>
int copy_down(int rc, T *D, T *R, uint64_t bytes, const char *what, T **out) {
    if (rc == ACX_OK && !R) rc = fail(ACX_ENOMEM, "out of memory");
    if (rc == ACX_OK) {
        DeviceScope ds(D->device);
        const hipError_t e = hipMemcpy(R->h_block, D->d_block, bytes, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = hipfail(e, what);
    }
    free_result(D);
    if (rc != ACX_OK) { free_result(R); return rc; }
    *out = R;
    return ACX_OK;
}

// ---- The stages that run NO find: the walkers (at_api.cpp, seg_api.cpp, wp_api.cpp).  They fold in
// their loads, so none of these frames makes a folded copy: device_call and staged_call above are not theirs. ----

// A host entry's haystack and offsets: bytes need an address (the refusal's text is the entry's), no offsets is ONE haystack
// (*n_hay becomes 1), offsets rise from 0 to len.
inline int host_rows(const uint8_t *hay, uint64_t len, const uint64_t *offsets, uint64_t *n_hay, const char *null_hay) {
    if (len && !hay) return fail(ACX_EINVAL, null_hay);
    if (offsets) return offsets_span(offsets, *n_hay, len);
    if (*n_hay > 1) return fail(ACX_EINVAL, "several haystacks need offsets");
    *n_hay = 1;
    return ACX_OK;
}

// What a *_host form refuses first, in this order: a null handle (`handles`: every pointer the form cannot do without),
// flags() -- the form's own flags and values --, the match kind, kind() -- what the form asks of the kind --, host_rows.
inline int any_kind() { return ACX_OK; }
template <class Flags, class Kind>
int host_form_args(bool handles, Flags &&flags, int match_kind, Kind &&kind, const uint8_t *hay, uint64_t len, const uint64_t *offsets,
                   uint64_t *n_hay) {
    if (!handles) return fail(ACX_EINVAL, "null argument");
    int rc = flags();
    if (rc != ACX_OK) return rc;
    if (match_kind < ACX_MATCH_STANDARD || match_kind > ACX_MATCH_LEFTMOST_LONGEST) return fail(ACX_EINVAL, "unknown match kind");
    if ((rc = kind()) != ACX_OK) return rc;
    return host_rows(hay, len, offsets, n_hay, "null argument");
}

// What a *_device / *_into_device entry refuses behind its own flags and values: a null haystack, offsets beside a row
// length, own() -- the entry's pointers and their alignment, in the entry's order --, then the segments' checks.  What the
// entry refuses by sizes follows the call; then the lease (leased).
template <class Own>
int walk_device_args(const void *d_hay, uint64_t len, const uint64_t *d_offsets, uint64_t n_hay, uint64_t uniform_len, Own &&own,
                     Segments *G) {
    if (len && !d_hay) return fail(ACX_EINVAL, "null haystack");
    if (d_offsets && uniform_len) return fail(ACX_EINVAL, "offsets and uniform_len exclude one another");
    const int rc = own();
    return rc != ACX_OK ? rc : make_segments(d_offsets, n_hay, uniform_len, len, G);
}
template <class Run>
int leased(acx_automaton *a, Run &&run) {
    Lease lease(a);
    if (!lease.c) return fail(ACX_EDEVICE, "could not create a stream for the call");
    return run(lease.c);
}

// The two-pass frame of a stage whose result is sized by a count, behind a lease, on st:
//   count(st, &temp, &total)  queues the counting pass and reads the total back: st has been waited for when it returns;
//                             *temp: the stage's scratch, one block of the buffer cache, named as soon as it exists;
//   Z->alloc()                Z: the stage's result, its shaping fields set but for the one `total` points to;
//   emit(st, temp, total)     queues the emitting pass into Z's parts;
// and retire_find ends the stage whatever the outcome, with temp and t2 (a temporary of the caller's that the kernels read,
// or null).  Returns with the emitting pass in flight (Z->done).  *out: Z, which is freed on failure.
template <class T, class Count, class Emit>
int two_pass(hipStream_t st, T *Z, uint64_t *total, void *t2, T **out, Count &&count, Emit &&emit) {
    *out = nullptr;
    void *temp = nullptr;
    int queued = count(st, &temp, total);
    if (queued == ACX_OK) queued = Z->alloc();
    if (queued == ACX_OK) queued = emit(st, temp, *total);
    const int rc = retire_find(queued, st, nullptr, Z, temp, t2);
    if (rc != ACX_OK) { free_result(Z); return rc; }
    *out = Z;
    return ACX_OK;
}
// ... and its twin without a result block, for the raw *_into_device entries: the count, the emitting pass into the caller's
// columns if the total fits `cap`, then st is waited for -- complete when it returns, whatever the launches said -- and the
// scratch goes back to the cache.  The passes' error comes first.
template <class Count, class Emit>
int two_pass_raw(int device, hipStream_t st, uint64_t cap, uint64_t *total, Count &&count, Emit &&emit) {
    void *temp = nullptr;
    int rc = count(st, &temp, total);
    if (rc == ACX_OK && *total <= cap) rc = emit(st, temp, *total);
    const hipError_t s = hipStreamSynchronize(st);
    g_bufs.put(temp, device);
    if (rc != ACX_OK) return rc;
    return s == hipSuccess ? ACX_OK : hipfail(s, "hipStreamSynchronize");
}

// The staged device route of a host entry point, staged_call's mirror: the lease, the haystacks (and, for a batch, their
// offsets) staged as they are; then run(ctx, segments, D) makes the device result *D from ctx->ws.hay, and the frame waits for
// it under the lease (the staging buffers are the context's).  No batch: ONE haystack, no offsets.
template <class T, class Run>
int staged_walk(acx_automaton *a, const uint8_t *hay, uint64_t len, const uint64_t *offsets, uint64_t n_hay, T **D, Run &&run) {
    Lease lease(a);
    Ctx *c = lease.c;
    if (!c) return fail(ACX_EDEVICE, "could not create a stream for the call");
    int rc = stage_host(a, c, hay, len, offsets, offsets ? n_hay + 1 : 0, false);
    if (rc != ACX_OK) return rc;
    rc = run(c, offsets ? Segments{c->ws.offsets, n_hay, 0} : Segments{nullptr, 1, 0}, D);
    if (rc == ACX_OK) return (*D)->wait();
    (void)hipStreamSynchronize(c->stream);
    return rc;
}
// ... and its end, whatever staged_walk returned (rc; D: the device result, null on failure): the host twin of D -- a new
// result, shaped like D (T::shaped_like), allocated -- filled by copy_down.
template <class T>
int host_twin(int rc, T *D, const char *what, T **out) {
    T *Z = rc == ACX_OK ? new_result<T>(D->device, false) : nullptr;
    if (Z) {
        Z->shaped_like(*D);
        if ((rc = Z->alloc()) != ACX_OK) { free_result(Z); free_result(D); return rc; }
    }
    return copy_down(rc, D, Z, D ? D->block_bytes : 0, what, out);
}

} // namespace acxh
