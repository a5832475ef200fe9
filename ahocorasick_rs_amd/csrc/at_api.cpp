// at_api.cpp -- the anchored search, "does a pattern begin exactly HERE" (at.hpp has the definition): the host form of the
// definition, the device stage, the acx_match_at* entry points and the accessors of their result.  No find runs: the walk
// reads the trie edges and the own lists every handle has, and a few haystack bytes per anchor.  The entries' preambles, the
// two-pass frame, the staged route and the host twin are the walkers' shared ones (result_block.hpp), the match kind's choice
// on the host is HostTrie::pick.
#include "at.hpp"
#include "host_trie.hpp"
#include "replace.hpp"
#include "result_block.hpp"

using namespace acxh;

// acx_match_at / acx_match_at_device: the patterns and the ends (`entries` int64 words each) and, for an overlapping call,
// anchors + 1 row offsets in ONE block (result_block.hpp).  Not overlapping: an entry per anchor.  Device route: the
// stage's temporaries have gone back to the cache behind the stage's kernels.
struct ACX_HIDDEN acx_at : ResultBlock {
    enum { PATTERN, END, ROW_OFFSETS, N_PARTS };
    uint64_t anchors = 0, entries = 0;
    bool overlapping = false;

    int alloc() { // the block (by on_device) and its parts
        return overlapping ? alloc_parts({entries * 8, entries * 8, (anchors + 1) * 8}) : alloc_parts({entries * 8, entries * 8});
    }
    int64_t *pattern() const { return at<int64_t>(PATTERN); }
    int64_t *end() const { return at<int64_t>(END); }
    int64_t *row_offsets() const { return at<int64_t>(ROW_OFFSETS); }
    void shaped_like(const acx_at &D) { anchors = D.anchors; entries = D.entries; overlapping = D.overlapping; }
};

namespace {

constexpr uint32_t AT_KNOWN_FLAGS = ACX_AT_OVERLAPPING | ACX_AT_FULL | ACX_AT_ROW_STARTS;

int too_many_anchors() { return fail(ACX_ETOOBIG, "2^32 anchors or more in one call"); }

// the flags every entry point refuses, in this order
int at_flags(uint32_t flags) {
    if (flags & ~AT_KNOWN_FLAGS) return fail(ACX_EINVAL, "unknown flags");
    if ((flags & ACX_AT_FULL) && !(flags & ACX_AT_ROW_STARTS)) return fail(ACX_EINVAL, "ACX_AT_FULL needs ACX_AT_ROW_STARTS");
    return ACX_OK;
}

uint32_t kernel_flags(const acx_automaton *a, uint32_t flags) {
    return ((flags & ACX_AT_FULL) ? acx::AT_FULL : 0u) | ((flags & ACX_AT_ROW_STARTS) ? acx::AT_ROW_STARTS : 0u) |
           (folds(a) ? acx::AT_FOLD : 0u);
}

// the anchors of a call: the rows, or the positions
int anchors_of(uint32_t flags, const acx::RowCut &R, uint64_t n_pos, uint64_t *A) {
    *A = (flags & ACX_AT_ROW_STARTS) ? R.n : n_pos;
    return *A >= acx::AT_MAX_ANCHORS ? too_many_anchors() : ACX_OK;
}

// The device route under a lease: the stage on the context's stream, a device result.  Returns when the result's size is
// known, with the stage in flight (Z->done).  d_hay, the offsets and d_pos (n_pos words; null with ACX_AT_ROW_STARTS) must
// stay valid until then; t2: a second temporary of the caller's that goes back to the cache behind the kernels (the staged
// positions), or null.
// Not overlapping: an entry per anchor, nothing to count.  Overlapping: two passes (two_pass) -- at_count, the library's scan,
// the total, 8 bytes, crosses the bus; at_emit walks again -- over one block of the cache: [counts: A][base: A + 1][scan].
int run_at(acx_automaton *a, Ctx *c, const uint8_t *d_hay, uint64_t len, const Segments &G, const int64_t *d_pos, uint64_t n_pos,
           uint32_t flags, void *t2, acx_at **out) {
    *out = nullptr;
    const acx::RowCut R = row_cut(G, len);
    uint64_t A = 0;
    const int rc = anchors_of(flags, R, n_pos, &A);
    acx_at *Z = rc == ACX_OK ? new_result<acx_at>(a->device, true) : nullptr;
    if (!Z) {
        if (t2) (void)hipStreamSynchronize(c->stream); // (the copy that fills it)
        g_bufs.put(t2, a->device);
        return rc == ACX_OK ? ACX_ENOMEM : rc;
    }
    Z->anchors = A;
    Z->overlapping = (flags & ACX_AT_OVERLAPPING) != 0;
    const acx::AtTrie T = acx::at_trie(a->dev); // (the whole own lists: an overlapping call reports every copy)
    const uint32_t kf = kernel_flags(a, flags);
    const bool counted = Z->overlapping && A;
    Carver C;
    const uint64_t o_counts = C.part(A), o_base = C.part(A + 1), o_scan = C.part(replace_scan_words(A));
    return two_pass(
        c->stream, Z, &Z->entries, t2, out,
        [&](hipStream_t st, void **temp, uint64_t *total) -> int {
            *total = Z->overlapping ? 0 : A;
            if (!counted) return ACX_OK;
            HIPCHK(g_bufs.get(temp, C.bytes(), a->device));
            uint64_t *b = (uint64_t *)*temp;
            HIPCHK(acx::at_count(T, d_hay, R, d_pos, A, kf, b + o_counts, st));
            HIPCHK(acx::replace_scan(nullptr, nullptr, b + o_counts, A, (int64_t *)(b + o_base), b + o_scan, st));
            HIPCHK(hipMemcpyAsync(total, b + o_base + A, 8, hipMemcpyDeviceToHost, st)); // all that crosses the bus
            HIPCHK(hipStreamSynchronize(st));
            return *total >= (1ull << 60) ? fail(ACX_EDEVICE, "the anchors' counts do not sum to a size") : ACX_OK;
        },
        [&](hipStream_t st, void *temp, uint64_t total) -> int {
            if (!Z->overlapping) {
                if (A) HIPCHK(acx::at_walk(T, d_hay, R, d_pos, A, a->host.match_kind, kf, Z->pattern(), Z->end(), st));
            } else if (!A) {
                HIPCHK(hipMemsetAsync(Z->row_offsets(), 0, 8, st));
            } else {
                const int64_t *base = (const int64_t *)temp + o_base;
                HIPCHK(hipMemcpyAsync(Z->row_offsets(), base, (A + 1) * 8, hipMemcpyDeviceToDevice, st));
                if (total) HIPCHK(acx::at_emit(T, d_hay, R, d_pos, A, kf, base, Z->pattern(), Z->end(), st));
            }
            return ACX_OK;
        });
}

} // namespace

extern "C" {

int acx_match_at_host(const acx_host_automaton_t *h, const uint8_t *hay, uint64_t len, const uint64_t *offsets, uint64_t n_hay,
                      const int64_t *positions, uint64_t n_pos, uint32_t flags, int match_kind, int64_t *pattern, int64_t *end,
                      int64_t *row_offsets) {
    const bool overlapping = (flags & ACX_AT_OVERLAPPING) != 0, full = (flags & ACX_AT_FULL) != 0,
               row_starts = (flags & ACX_AT_ROW_STARTS) != 0;
    const int rc = host_form_args(
        h != nullptr, [&] { return at_flags(flags); }, match_kind,
        [&] {
            return overlapping && (match_kind != ACX_MATCH_STANDARD || h->host.match_kind != ACX_MATCH_STANDARD)
                       ? fail(ACX_EOVERLAP, "an overlapping search needs match kind Standard")
                       : ACX_OK;
        },
        hay, len, offsets, &n_hay);
    if (rc != ACX_OK) return rc;
    const uint64_t A = row_starts ? n_hay : n_pos;
    if (!row_starts && n_pos && !positions) return fail(ACX_EINVAL, "null argument");
    if (overlapping ? !row_offsets || (!pattern != !end) : A && (!pattern || !end)) return fail(ACX_EINVAL, "null argument");
    for (uint64_t i = 0; !row_starts && i < n_pos; i++)
        if (positions[i] < 0 || (uint64_t)positions[i] > len) return fail(ACX_EINVAL, "a position lies outside the data");
    const HostTrie T{h->host, (h->flags & ACX_BUILD_ASCII_CASE_INSENSITIVE) != 0};
    const acx::Automaton &H = h->host;
    uint64_t w = 0; // overlapping: the entries so far
    for (uint64_t i = 0; i < A; i++) {
        uint64_t p, L;
        if (row_starts) {
            p = offsets ? offsets[i] : 0;
            L = offsets ? offsets[i + 1] : len;
        } else {
            p = (uint64_t)positions[i];
            L = len;
            if (offsets && p < len) // the LAST row that begins at or before p
                L = *std::upper_bound(offsets, offsets + n_hay + 1, p);
        }
        const uint64_t origin = row_starts ? p : 0; // `end` is local to the row for row starts
        if (overlapping) {
            row_offsets[i] = (int64_t)w;
            T.walk(hay, p, L, 0, [&](uint32_t s, uint64_t d) {
                if (full && p + d != L) return true;
                for (uint32_t o = H.own_off[s]; o < H.own_off[s + 1]; o++, w++)
                    if (pattern) { pattern[w] = (int64_t)H.own_pid[o]; end[w] = (int64_t)(p + d - origin); }
                return true;
            });
            continue;
        }
        uint64_t e;
        const bool found = T.pick(hay, p, L, 0, match_kind, full, &pattern[i], &e);
        end[i] = found ? (int64_t)(e - origin) : -1;
    }
    if (overlapping) row_offsets[A] = (int64_t)w;
    return ACX_OK;
}

int acx_match_at_device(acx_automaton_t *a, const void *d_hay, uint64_t len, const uint64_t *d_offsets, uint64_t n_hay,
                        uint64_t uniform_len, const int64_t *d_positions, uint64_t n_pos, uint32_t flags, acx_at_t **out) {
    if (!a || !out) return fail(ACX_EINVAL, "null argument");
    *out = nullptr;
    int rc = at_flags(flags);
    if (rc == ACX_OK && (flags & ACX_AT_OVERLAPPING)) rc = check_overlapping(a); // (the error, no device state)
    if (rc != ACX_OK) return rc;
    const bool row_starts = (flags & ACX_AT_ROW_STARTS) != 0;
    Segments G;
    rc = walk_device_args(d_hay, len, d_offsets, n_hay, uniform_len, [&] {
        if (!row_starts && n_pos && !d_positions) return fail(ACX_EINVAL, "null argument");
        if (((uintptr_t)d_positions | (uintptr_t)d_offsets) & 7) return fail(ACX_EINVAL, "positions and offsets must be 8-byte aligned");
        return !row_starts && n_pos >= acx::AT_MAX_ANCHORS ? too_many_anchors() : ACX_OK;
    }, &G);
    if (rc != ACX_OK) return rc;
    return leased(a, [&](Ctx *c) {
        return run_at(a, c, (const uint8_t *)d_hay, len, G, row_starts ? nullptr : d_positions, n_pos, flags, nullptr, out);
    });
}

int acx_match_at_into_device(acx_automaton_t *a, const void *d_hay, uint64_t len, const uint64_t *d_offsets, uint64_t n_hay,
                             uint64_t uniform_len, const int64_t *d_positions, uint64_t n_pos, uint32_t flags, int64_t *d_pattern,
                             int64_t *d_end) {
    if (!a) return fail(ACX_EINVAL, "null argument");
    int rc = at_flags(flags);
    if (rc != ACX_OK) return rc;
    if (flags & ACX_AT_OVERLAPPING) return fail(ACX_EINVAL, "the raw form is not overlapping: its columns have an entry per anchor");
    const bool row_starts = (flags & ACX_AT_ROW_STARTS) != 0;
    Segments G;
    rc = walk_device_args(d_hay, len, d_offsets, n_hay, uniform_len, [&] {
        if (!row_starts && n_pos && !d_positions) return fail(ACX_EINVAL, "null argument");
        return (((uintptr_t)d_positions | (uintptr_t)d_offsets | (uintptr_t)d_pattern | (uintptr_t)d_end) & 7)
                   ? fail(ACX_EINVAL, "positions, offsets and both columns must be 8-byte aligned")
                   : ACX_OK;
    }, &G);
    if (rc != ACX_OK) return rc;
    const acx::RowCut R = row_cut(G, len);
    uint64_t A = 0;
    if ((rc = anchors_of(flags, R, n_pos, &A)) != ACX_OK) return rc;
    if (!A) return ACX_OK; // (no entry to write)
    if (!d_pattern || !d_end) return fail(ACX_EINVAL, "null argument");
    return leased(a, [&](Ctx *c) {
        const hipError_t e = acx::at_walk(acx::at_trie(a->dev), (const uint8_t *)d_hay, R, row_starts ? nullptr : d_positions, A,
                                          a->host.match_kind, kernel_flags(a, flags), d_pattern, d_end, c->stream);
        const hipError_t s = hipStreamSynchronize(c->stream); // (complete when it returns, whatever the launch said)
        if (e != hipSuccess) return hipfail(e, "at_walk");
        return s == hipSuccess ? ACX_OK : hipfail(s, "hipStreamSynchronize");
    });
}

int acx_match_at(acx_automaton_t *a, const uint8_t *hay, uint64_t len, const uint64_t *offsets, uint64_t n_hay,
                 const int64_t *positions, uint64_t n_pos, uint32_t flags, int codepoints, acx_at_t **out) {
    if (!a || !out) return fail(ACX_EINVAL, "null argument");
    *out = nullptr;
    int rc = at_flags(flags);
    if (rc == ACX_OK && (flags & ACX_AT_OVERLAPPING)) rc = check_overlapping(a); // (the error, no device state)
    if (rc != ACX_OK) return rc;
    if ((rc = host_rows(hay, len, offsets, &n_hay, "null haystack")) != ACX_OK) return rc;
    const bool batch = offsets != nullptr, row_starts = (flags & ACX_AT_ROW_STARTS) != 0;
    if (!row_starts && n_pos && !positions) return fail(ACX_EINVAL, "null argument");
    if (!row_starts && n_pos >= acx::AT_MAX_ANCHORS) return too_many_anchors();
    // positions in the caller's unit -> bytes (codepoints: characters, a byte that continues none begins one)
    std::vector<uint64_t> cs;
    if (codepoints && (rc = char_starts(hay, len, &cs)) != ACX_OK) return rc;
    const uint64_t units = codepoints ? (uint64_t)cs.size() - 1 : len;
    std::vector<int64_t> pos;
    if (!row_starts) {
        try {
            pos.resize((size_t)n_pos);
        } catch (...) { return fail(ACX_ENOMEM, "out of memory"); }
        for (uint64_t i = 0; i < n_pos; i++) {
            if (positions[i] < 0 || (uint64_t)positions[i] > units) return fail(ACX_EINVAL, "a position lies outside the data");
            pos[(size_t)i] = codepoints ? (int64_t)cs[(size_t)positions[i]] : positions[i];
        }
    }
    // the data (and, for a batch, its offsets) through the context's staging buffers, the positions through a block of the
    // buffer cache; the same kernels; the block comes home in one copy
    acx_at *D = nullptr;
    rc = staged_walk(a, hay, len, offsets, n_hay, &D, [&](Ctx *c, const Segments &G, acx_at **dev) -> int {
        void *d_pos = nullptr;
        if (!pos.empty()) {
            HIPCHK(g_bufs.get(&d_pos, pos.size() * 8, a->device));
            const hipError_t e = hipMemcpyAsync(d_pos, pos.data(), pos.size() * 8, hipMemcpyHostToDevice, c->stream);
            if (e != hipSuccess) {
                (void)hipStreamSynchronize(c->stream);
                g_bufs.put(d_pos, a->device);
                return hipfail(e, "hipMemcpyAsync");
            }
        }
        return run_at(a, c, c->ws.hay, len, G, (const int64_t *)d_pos, n_pos, flags, d_pos, dev); // (pos is this call's)
    });
    if ((rc = host_twin(rc, D, "the match-at result's copy", out)) != ACX_OK) return rc;
    if (!codepoints) return ACX_OK;
    acx_at *Z = *out;
    // ends in characters: an entry's anchor gives the row start that a local end counts from
    int64_t *pat = Z->pattern(), *end = Z->end();
    const int64_t *ro = Z->overlapping ? Z->row_offsets() : nullptr;
    for (uint64_t i = 0; i < Z->anchors; i++) {
        const uint64_t b = row_starts ? (batch ? offsets[i] : 0) : 0;
        for (uint64_t k = ro ? (uint64_t)ro[i] : i, stop = ro ? (uint64_t)ro[i + 1] : i + 1; k < stop; k++)
            if (pat[k] >= 0) end[k] = (int64_t)(char_of(cs, b + (uint64_t)end[k]) - char_of(cs, b));
    }
    return ACX_OK;
}

uint64_t acx_at_count(const acx_at_t *r) { return r ? r->anchors : 0; }
uint64_t acx_at_entries(const acx_at_t *r) { return r ? r->entries : 0; }
int acx_at_on_device(const acx_at_t *r) { return r ? r->on_device : 0; }

const int64_t *acx_at_pattern(const acx_at_t *r) { return (const int64_t *)part_ptr(r, acx_at::PATTERN, acx_at::N_PARTS); }
const int64_t *acx_at_end(const acx_at_t *r) { return (const int64_t *)part_ptr(r, acx_at::END, acx_at::N_PARTS); }
const int64_t *acx_at_row_offsets(const acx_at_t *r) { return (const int64_t *)part_ptr(r, acx_at::ROW_OFFSETS, acx_at::N_PARTS); }
int acx_at_copy(const acx_at_t *r, int which, void *host_dst) {
    return part_copy(r, which, acx_at::N_PARTS, host_dst, "no such part of a match-at result",
                     "only an overlapping call has row offsets");
}

void acx_free_at(acx_at_t *r) { free_result(r); }

} // extern "C"
