// wp_api.cpp -- WordPiece tokenization by the dictionary (wp.hpp has the definition): the host form of the definition, the
// device stage, the acx_wordpiece* entry points and the accessors of their result.  No find runs: the chains read the trie
// edges and the own lists every handle has.  The entries' preambles, the two-pass frames, the staged route and the host twin
// are the walkers' shared ones (result_block.hpp), the match kind's choice on the host is HostTrie::pick.
#include "wp.hpp"
#include "host_trie.hpp"
#include "result_block.hpp"

using namespace acxh;

// acx_wordpiece / acx_wordpiece_device: the ids, starts and ends (`pieces` int64 words each), the first flags (`pieces`
// bytes) and the rows' offsets (rows + 1) in ONE block (result_block.hpp).  Device route: the stage's temporaries go back to
// the cache behind its kernels.
struct ACX_HIDDEN acx_wp : ResultBlock {
    enum { ID, START, END, FIRST, ROW_OFFSETS, N_PARTS };
    uint64_t pieces = 0, rows = 0;

    int alloc() { return alloc_parts({pieces * 8, pieces * 8, pieces * 8, pieces, (rows + 1) * 8}); }
    int64_t *id() const { return at<int64_t>(ID); }
    int64_t *start() const { return at<int64_t>(START); }
    int64_t *end() const { return at<int64_t>(END); }
    uint8_t *first() const { return at<uint8_t>(FIRST); }
    int64_t *row_offsets() const { return at<int64_t>(ROW_OFFSETS); }
    void shaped_like(const acx_wp &D) { pieces = D.pieces; rows = D.rows; }
};

namespace {

// what every entry point refuses before any device work, in this order (the offsets' checks stand between the two halves)
int wp_values(uint32_t flags, const uint8_t *cls, const uint8_t *prefix, uint64_t prefix_len, uint64_t max_word) {
    if (flags) return fail(ACX_EINVAL, "unknown flags");
    if (!cls || (prefix_len && !prefix)) return fail(ACX_EINVAL, "null argument");
    for (int b = 0; b < 256; b++)
        if (cls[b] > ACX_WP_ALONE) return fail(ACX_EINVAL, "a byte class is none of WORD, SPACE and ALONE");
    if (max_word < 1 || max_word > acx::WP_MAX_WORD) return fail(ACX_EINVAL, "max_word lies outside 1 .. 1024");
    return ACX_OK;
}
int wp_sizes(uint64_t len, uint64_t rows) {
    if (acx::tiles_of(len, acx::WP_TILE) > acx::WP_MAX_TILES) return fail(ACX_ETOOBIG, "more tiles than a 32-bit grid");
    if (rows >= (1ull << 38)) return fail(ACX_ETOOBIG, "2^38 rows or more in one call");
    return ACX_OK;
}

// the trie node of the continuation prefix, walked over the compiled tables (folded for a folding handle); WP_NO_NODE: the
// path is not in the trie -- no continuation ever matches, which is valid
uint32_t prefix_node(const HostTrie &T, const uint8_t *prefix, uint64_t prefix_len) {
    uint32_t s = 0;
    for (uint64_t k = 0; k < prefix_len; k++) {
        s = T.child(s, T.fold ? acx::fold_byte(prefix[k]) : prefix[k]);
        if (!s) return acx::WP_NO_NODE;
    }
    return s;
}

acx::WpArgs kernel_args(const acx_automaton *a, const uint8_t *cls, const uint8_t *prefix, uint64_t prefix_len, uint64_t max_word,
                        int64_t unk_id) {
    const HostTrie T{a->host, folds(a)};
    return acx::WpArgs{acx::wp_classes(cls), prefix_node(T, prefix, prefix_len), (uint32_t)max_word, folds(a) ? acx::WP_FOLD : 0u,
                       a->host.match_kind, unk_id};
}

// The device stage on st as the two passes of two_pass / two_pass_raw.  count: k_wp<COUNT>, the scan, the carry, and T -- 8
// bytes cross the bus, the stream is waited for; *temp: the stage's scratch, one block of the buffer cache.  emit: into
// columns sized by `total`, every entry of the five is written.
struct WpStage {
    acx_automaton *a;
    const uint8_t *d_hay;
    acx::RowCut R;
    acx::WpArgs A;
    acx::WpPlan P{};

    int count(hipStream_t st, void **temp, uint64_t *total) {
        *total = 0;
        if (!R.len) return ACX_OK;
        P = acx::wp_plan(R.len);
        HIPCHK(g_bufs.get(temp, P.words * 8, a->device));
        uint64_t *scratch = (uint64_t *)*temp;
        HIPCHK(acx::wp_count(acx::at_trie(a->dev), d_hay, R, A, P, scratch, st));
        HIPCHK(hipMemcpyAsync(total, acx::wp_total(P, scratch), 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        return *total > R.len ? fail(ACX_EDEVICE, "the tiles' counts do not sum to a number of pieces") : ACX_OK;
    }
    int emit(hipStream_t st, void *temp, uint64_t total, int64_t *id, int64_t *start, int64_t *end, uint8_t *first,
             int64_t *row_offsets) const {
        if (!R.len) { // no piece: every row begins at piece 0
            HIPCHK(hipMemsetAsync(row_offsets, 0, (R.n + 1) * 8, st));
        } else if (!total) { // (no word in the data: the columns are empty and may have no address)
            HIPCHK(acx::piece_rows(R, start, 0, row_offsets, st));
        } else {
            HIPCHK(acx::wp_emit(acx::at_trie(a->dev), d_hay, R, A, P, (const uint64_t *)temp, total, id, start, end, first, row_offsets, st));
        }
        return ACX_OK;
    }
};

// The device route under a lease: the stage on the context's stream, a device result.  Returns when T is known, with the
// emitting half in flight (Z->done).  d_hay and the offsets must stay valid until then.
int run_wp(acx_automaton *a, Ctx *c, const uint8_t *d_hay, uint64_t len, const Segments &G, const acx::WpArgs &A, acx_wp **out) {
    *out = nullptr;
    WpStage S{a, d_hay, row_cut(G, len), A};
    acx_wp *Z = new_result<acx_wp>(a->device, true);
    if (!Z) return ACX_ENOMEM;
    Z->rows = S.R.n;
    return two_pass(
        c->stream, Z, &Z->pieces, nullptr, out, [&](hipStream_t st, void **temp, uint64_t *total) { return S.count(st, temp, total); },
        [&](hipStream_t st, void *temp, uint64_t total) {
            return S.emit(st, temp, total, Z->id(), Z->start(), Z->end(), Z->first(), Z->row_offsets());
        });
}

struct Piece {
    int64_t id;
    uint64_t start, end;
};

} // namespace

extern "C" {

int acx_wordpiece_host(const acx_host_automaton_t *h, const uint8_t *hay, uint64_t len, const uint64_t *offsets, uint64_t n_hay,
                       const uint8_t *cls, const uint8_t *prefix, uint64_t prefix_len, uint64_t max_word, int64_t unk_id,
                       uint32_t flags, int match_kind, uint64_t cap, int64_t *id, int64_t *start, int64_t *end, uint8_t *first,
                       int64_t *row_offsets, uint64_t *n_pieces) {
    if (n_pieces) *n_pieces = 0;
    int rc = host_form_args(h && n_pieces, [&] { return wp_values(flags, cls, prefix, prefix_len, max_word); }, match_kind, any_kind,
                            hay, len, offsets, &n_hay);
    if (rc != ACX_OK) return rc;
    if (cap && (!id || !start || !end || !first || !row_offsets)) return fail(ACX_EINVAL, "null argument");
    if ((rc = wp_sizes(len, n_hay)) != ACX_OK) return rc;
    const HostTrie T{h->host, (h->flags & ACX_BUILD_ASCII_CASE_INSENSITIVE) != 0};
    const uint32_t cnode = prefix_node(T, prefix, prefix_len);
    std::vector<Piece> word; // the pieces of the word at hand: withdrawn when a step finds nothing
    try {
        word.reserve((size_t)max_word);
    } catch (...) { return fail(ACX_ENOMEM, "out of memory"); }
    // two passes of the loop: the count, then -- it fits -- the pieces
    for (int pass = 0; pass < 2; pass++) {
        uint64_t t = 0;
        for (uint64_t r = 0; r < n_hay; r++) {
            const uint64_t b = offsets ? offsets[r] : 0, L = offsets ? offsets[r + 1] : len;
            if (pass) row_offsets[r] = (int64_t)t;
            for (uint64_t p = b; p < L;) {
                const uint8_t c = cls[hay[p]];
                if (c == ACX_WP_SPACE) { p++; continue; }
                const uint64_t ws = p;
                uint64_t we = p + 1;
                while (c == ACX_WP_WORD && we < L && cls[hay[we]] == ACX_WP_WORD) we++;
                word.clear();
                bool known = we - ws <= max_word;
                for (uint64_t q = ws; known && q < we;) {
                    int64_t pid;
                    uint64_t e;
                    // (a continuation goes on from C's node; none, when that is not in the trie)
                    known = (q == ws || cnode != acx::WP_NO_NODE) && T.pick(hay, q, we, q == ws ? 0u : cnode, match_kind, false, &pid, &e);
                    if (known) word.push_back(Piece{pid, q, e}); // (at most max_word pieces: no allocation)
                    q = e;
                }
                if (!known) { word.clear(); word.push_back(Piece{unk_id, ws, we}); }
                if (pass)
                    for (size_t k = 0; k < word.size(); k++) {
                        id[t + k] = word[k].id;
                        start[t + k] = (int64_t)word[k].start;
                        end[t + k] = (int64_t)word[k].end;
                        first[t + k] = k == 0;
                    }
                t += word.size();
                p = we;
            }
        }
        *n_pieces = t;
        if (!cap || t > cap) return ACX_OK; // (nothing is written)
        if (pass) row_offsets[n_hay] = (int64_t)t;
    }
    return ACX_OK;
}

int acx_wordpiece_device(acx_automaton_t *a, const void *d_hay, uint64_t len, const uint64_t *d_offsets, uint64_t n_hay,
                         uint64_t uniform_len, const uint8_t *cls, const uint8_t *prefix, uint64_t prefix_len, uint64_t max_word,
                         int64_t unk_id, uint32_t flags, acx_wp_t **out) {
    if (!a || !out) return fail(ACX_EINVAL, "null argument");
    *out = nullptr;
    int rc = wp_values(flags, cls, prefix, prefix_len, max_word);
    if (rc != ACX_OK) return rc;
    Segments G;
    rc = walk_device_args(d_hay, len, d_offsets, n_hay, uniform_len,
                          [&] { return (uintptr_t)d_offsets & 7 ? fail(ACX_EINVAL, "offsets must be 8-byte aligned") : ACX_OK; }, &G);
    if (rc != ACX_OK || (rc = wp_sizes(len, rows_of(G).n)) != ACX_OK) return rc;
    return leased(a, [&](Ctx *c) {
        return run_wp(a, c, (const uint8_t *)d_hay, len, G, kernel_args(a, cls, prefix, prefix_len, max_word, unk_id), out);
    });
}

int acx_wordpiece_into_device(acx_automaton_t *a, const void *d_hay, uint64_t len, const uint64_t *d_offsets, uint64_t n_hay,
                              uint64_t uniform_len, const uint8_t *cls, const uint8_t *prefix, uint64_t prefix_len,
                              uint64_t max_word, int64_t unk_id, uint32_t flags, uint64_t cap, int64_t *d_id, int64_t *d_start,
                              int64_t *d_end, uint8_t *d_first, int64_t *d_row_offsets, uint64_t *n_pieces) {
    if (!a || !n_pieces) return fail(ACX_EINVAL, "null argument");
    *n_pieces = 0;
    int rc = wp_values(flags, cls, prefix, prefix_len, max_word);
    if (rc != ACX_OK) return rc;
    Segments G;
    rc = walk_device_args(d_hay, len, d_offsets, n_hay, uniform_len, [&] {
        if (((uintptr_t)d_offsets | (uintptr_t)d_id | (uintptr_t)d_start | (uintptr_t)d_end | (uintptr_t)d_row_offsets) & 7)
            return fail(ACX_EINVAL, "offsets and the four int64 columns must be 8-byte aligned");
        return cap && (!d_id || !d_start || !d_end || !d_first || !d_row_offsets) ? fail(ACX_EINVAL, "null argument") : ACX_OK;
    }, &G);
    if (rc != ACX_OK || (rc = wp_sizes(len, rows_of(G).n)) != ACX_OK) return rc;
    return leased(a, [&](Ctx *c) {
        WpStage S{a, (const uint8_t *)d_hay, row_cut(G, len), kernel_args(a, cls, prefix, prefix_len, max_word, unk_id)};
        return two_pass_raw(
            a->device, c->stream, cap, n_pieces, [&](hipStream_t st, void **temp, uint64_t *total) { return S.count(st, temp, total); },
            [&](hipStream_t st, void *temp, uint64_t total) { // (cap == 0: a count alone, the columns may have no address)
                return cap ? S.emit(st, temp, total, d_id, d_start, d_end, d_first, d_row_offsets) : ACX_OK;
            });
    });
}

int acx_wordpiece(acx_automaton_t *a, const uint8_t *hay, uint64_t len, const uint64_t *offsets, uint64_t n_hay, const uint8_t *cls,
                  const uint8_t *prefix, uint64_t prefix_len, uint64_t max_word, int64_t unk_id, uint32_t flags, int codepoints,
                  acx_wp_t **out) {
    if (!a || !out) return fail(ACX_EINVAL, "null argument");
    *out = nullptr;
    int rc = wp_values(flags, cls, prefix, prefix_len, max_word);
    if (rc != ACX_OK) return rc;
    if ((rc = host_rows(hay, len, offsets, &n_hay, "null haystack")) != ACX_OK) return rc;
    if ((rc = wp_sizes(len, n_hay)) != ACX_OK) return rc;
    // the data (and, for a batch, its offsets) through the context's staging buffers; the same kernels; the block comes home
    // in one copy
    acx_wp *D = nullptr;
    rc = staged_walk(a, hay, len, offsets, n_hay, &D, [&](Ctx *c, const Segments &G, acx_wp **dev) {
        return run_wp(a, c, c->ws.hay, len, G, kernel_args(a, cls, prefix, prefix_len, max_word, unk_id), dev);
    });
    if ((rc = host_twin(rc, D, "the word pieces' copy", out)) != ACX_OK) return rc;
    if (!codepoints) return ACX_OK;
    acx_wp *Z = *out;
    // positions in characters: the characters that begin before each
    std::vector<uint64_t> cs;
    if ((rc = char_starts(hay, len, &cs)) != ACX_OK) { free_result(Z); *out = nullptr; return rc; }
    int64_t *s = Z->start(), *e = Z->end();
    for (uint64_t k = 0; k < Z->pieces; k++) {
        s[k] = (int64_t)char_of(cs, (uint64_t)s[k]);
        e[k] = (int64_t)char_of(cs, (uint64_t)e[k]);
    }
    return ACX_OK;
}

uint64_t acx_wp_count(const acx_wp_t *r) { return r ? r->pieces : 0; }
uint64_t acx_wp_rows(const acx_wp_t *r) { return r ? r->rows : 0; }
int acx_wp_on_device(const acx_wp_t *r) { return r ? r->on_device : 0; }

const int64_t *acx_wp_id(const acx_wp_t *r) { return (const int64_t *)part_ptr(r, acx_wp::ID, acx_wp::N_PARTS); }
const int64_t *acx_wp_start(const acx_wp_t *r) { return (const int64_t *)part_ptr(r, acx_wp::START, acx_wp::N_PARTS); }
const int64_t *acx_wp_end(const acx_wp_t *r) { return (const int64_t *)part_ptr(r, acx_wp::END, acx_wp::N_PARTS); }
const uint8_t *acx_wp_first(const acx_wp_t *r) { return (const uint8_t *)part_ptr(r, acx_wp::FIRST, acx_wp::N_PARTS); }
const int64_t *acx_wp_row_offsets(const acx_wp_t *r) { return (const int64_t *)part_ptr(r, acx_wp::ROW_OFFSETS, acx_wp::N_PARTS); }
int acx_wp_copy(const acx_wp_t *r, int which, void *host_dst) {
    return part_copy(r, which, acx_wp::N_PARTS, host_dst, "no such part of a word-piece result");
}

void acx_free_wp(acx_wp_t *r) { free_result(r); }

} // extern "C"
