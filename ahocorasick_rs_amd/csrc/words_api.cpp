// words_api.cpp -- whole-word matching (words.hpp): the definition on the host, the device stage behind
// an overlapping find's records, and the entry points that are the stage alone (acx_words_host, acx_words_rows_device).
// acx_find_words* live with the columns (columns_api.cpp), acx_filter_words* with the row filter (filter_api.cpp).
#include <tuple>

#include "words.hpp"
#include "replace.hpp"
#include "result_block.hpp"

using namespace acxh;

namespace {

// ASCII [0-9A-Za-z_]: \w of a bytes regex
constexpr uint32_t DEFAULT_WORDS[8] = {0, 0x03FF0000u, 0x87FFFFFEu, 0x07FFFFFEu, 0, 0, 0, 0};

bool in_set(const acx::WordSet &W, uint8_t b) { return (W.w[b >> 5] >> (b & 31)) & 1; }

// the stage's first block goes back once the stream has passed what reads it
struct Early {
    void *p = nullptr;
    int device = 0;
    hipStream_t st = nullptr;
    ~Early() {
        if (!p) return;
        (void)hipStreamSynchronize(st);
        g_bufs.put(p, device);
    }
};

} // namespace

namespace acxh {

int words_args(int overlapping, int match_kind, const uint8_t *word_set, WordsArgs *A) {
    if (match_kind != ACX_MATCH_STANDARD && match_kind != ACX_MATCH_LEFTMOST_FIRST && match_kind != ACX_MATCH_LEFTMOST_LONGEST)
        return fail(ACX_EINVAL, "match_kind must be one of ACX_MATCH_*");
    A->overlapping = overlapping ? 1 : 0;
    A->kind = match_kind;
    for (int k = 0; k < 8; k++)
        A->W.w[k] = word_set ? (uint32_t)word_set[4 * k] | (uint32_t)word_set[4 * k + 1] << 8 | (uint32_t)word_set[4 * k + 2] << 16 |
                                   (uint32_t)word_set[4 * k + 3] << 24
                             : DEFAULT_WORDS[k];
    return ACX_OK;
}

uint64_t words_host_max() {
    const char *e = std::getenv("ACX_WORDS_HOST_MAX");
    return e ? std::strtoull(e, nullptr, 10) : (1ull << 20);
}

int words_sizes(int device, hipStream_t st, const acx_match_t *d_m, uint64_t n, const uint64_t *d_counts, const acx::RowCut &R,
                bool check_sum, const uint8_t *d_hay, const WordsArgs &A, WordsStage *G) {
    const uint64_t rows = R.n, T = acx::words_tiles(n);
    if (n >= acx::WORDS_MAX_RECORDS) return fail(ACX_ETOOBIG, "too many records to be tested in one call");
    if (R.len >= acx::WORDS_MAX_LEN) return fail(ACX_ETOOBIG, "too many bytes for the whole-word stage's keys");
    G->rows = rows;
    // [rec_off: rows + 1][scan of the rows][flag: n bytes][survivors of the tiles: T][base: T + 1][scan of the tiles]
    // [new_off: rows + 1][new_counts: rows], every part 256-byte aligned
    Carver C;
    const uint64_t o_rec = C.part(rows + 1), o_scan = C.part(replace_scan_words(rows)), o_flag = C.part((n + 7) / 8), o_cnt = C.part(T),
                   o_base = C.part(T + 1), o_scan2 = C.part(replace_scan_words(T)), o_new = C.part(rows + 1), o_newc = C.part(rows);
    void *first = nullptr;
    HIPCHK(g_bufs.get(&first, C.bytes(), device));
    Early early; // (non-overlapping: the first block is spent before the call returns)
    if (A.overlapping) G->block = first;
    else { early.p = first; early.device = device; early.st = st; }
    uint64_t *b = (uint64_t *)first;
    int64_t *rec_off = (int64_t *)(b + o_rec), *base = (int64_t *)(b + o_base);
    uint8_t *flag = (uint8_t *)(b + o_flag);
    if (int rc = record_offsets(d_counts, rows, n, check_sum, rec_off, b + o_scan, st)) return rc;
    HIPCHK(acx::words_test(d_m, n, rec_off, rows, R, d_hay, A.W, flag, st));
    HIPCHK(acx::words_count(flag, n, b + o_cnt, st));
    HIPCHK(acx::replace_scan(nullptr, nullptr, b + o_cnt, T, base, b + o_scan2, st));
    uint64_t n1 = 0;
    HIPCHK(hipMemcpyAsync(&n1, base + T, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (n1 > n) return fail(ACX_EDEVICE, "more whole words than records");
    if (A.overlapping || !n1) {
        G->flag = flag;
        G->items = d_m;
        G->base = base;
        G->rows_off = rec_off;
        G->new_off = (int64_t *)(b + o_new);
        G->new_counts = b + o_newc;
        G->n_items = n;
        G->total = n1;
        if (!A.overlapping) { G->block = first; early.p = nullptr; } // (nothing survived: nothing else is made)
        return ACX_OK;
    }
    // the survivors, the resolve and the second compaction: [S: 3 n1][off1: rows + 1][acc: n1 bytes][accepted of the tiles]
    // [base][scan of the tiles][err][new_off: rows + 1][new_counts: rows][the resolve's scratch]
    const uint64_t T1 = acx::words_tiles(n1);
    const acx::ResolveLayout Y(n1);
    Carver D;
    const uint64_t p_s = D.part(3 * n1), p_off = D.part(rows + 1), p_acc = D.part((n1 + 7) / 8), p_cnt = D.part(T1), p_base = D.part(T1 + 1),
                   p_scan = D.part(replace_scan_words(T1)), p_err = D.part(1), p_new = D.part(rows + 1), p_newc = D.part(rows), p_res = D.part(Y.words);
    HIPCHK(g_bufs.get(&G->block, D.bytes(), device));
    uint64_t *d = (uint64_t *)G->block;
    acx_match_t *S = (acx_match_t *)(d + p_s);
    int64_t *off1 = (int64_t *)(d + p_off), *base2 = (int64_t *)(d + p_base);
    uint8_t *acc = (uint8_t *)(d + p_acc);
    HIPCHK(acx::words_emit(flag, n, base, n1, nullptr, d_m, acx::WordsOut{S, nullptr, nullptr, nullptr}, rec_off, rows, off1, st));
    HIPCHK(hipMemsetAsync(d + p_err, 0, 8, st));
    const uint32_t *src = nullptr;
    HIPCHK(acx::words_resolve(S, n1, off1, rows, R, A.kind, d + p_res, acc, &src, d + p_err, st));
    HIPCHK(acx::words_count(acc, n1, d + p_cnt, st));
    HIPCHK(acx::replace_scan(nullptr, nullptr, d + p_cnt, T1, base2, d + p_scan, st));
    uint64_t back[2] = {0, 0}; // a pattern beyond the key's field, and the total: all that crosses the bus from here
    HIPCHK(hipMemcpyAsync(&back[0], d + p_err, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&back[1], base2 + T1, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (back[0]) return fail(ACX_ETOOBIG, "a record's pattern is 2^24 or more: the whole-word stage's keys hold 24 bits of it");
    if (back[1] > n1) return fail(ACX_EDEVICE, "more matches than whole words");
    G->flag = acc;
    G->items = S;
    G->src = src;
    G->base = base2;
    G->rows_off = off1;
    G->new_off = (int64_t *)(d + p_new);
    G->new_counts = d + p_newc;
    G->n_items = n1;
    G->total = back[1];
    return ACX_OK;
}

int words_finish(const WordsStage &G, const acx::WordsOut &out, int64_t *row_offsets, uint64_t *counts, hipStream_t st) {
    if (!G.total) { // nothing is reported: every offset and every count is zero
        if (row_offsets) HIPCHK(hipMemsetAsync(row_offsets, 0, (G.rows + 1) * 8, st));
        if (counts) HIPCHK(hipMemsetAsync(counts, 0, G.rows * 8, st));
        return ACX_OK;
    }
    int64_t *new_off = row_offsets ? row_offsets : counts ? G.new_off : nullptr;
    HIPCHK(acx::words_emit(G.flag, G.n_items, G.base, G.total, G.src, G.items, out, G.rows_off, G.rows, new_off, st));
    if (counts) HIPCHK(acx::words_row_counts(new_off, G.rows, counts, st));
    return ACX_OK;
}

int words_host_find(acx_automaton *a, const HostBatch &B, uint64_t len, uint64_t n_hay, bool batch, const WordsArgs &A,
                    const uint8_t *word_set, std::vector<acx_match_t> *out, std::vector<uint64_t> *counts) {
    // the find entry points as they are (K0, the resident K0, the in-place read, the staged pipeline), each under its lease,
    // with byte offsets: every occurrence crosses the bus, the test reads the caller's own bytes here
    HostFind f;
    int rc = f.find(a, B.hay, len, batch ? B.rel.data() : nullptr, n_hay, 1, 0, n_hay && len);
    if (rc != ACX_OK) return rc;
    try {
        out->resize((size_t)f.nm + 1);
        counts->assign((size_t)n_hay + 1, 0);
    } catch (...) { return fail(ACX_ENOMEM, "out of memory"); }
    uint64_t kept = 0;
    rc = acx_words_host(B.hay, len, B.rel.data(), n_hay, f.m, f.nm, f.counts.data(), A.overlapping, A.kind, word_set, out->data(),
                        counts->data(), &kept);
    if (rc == ACX_OK) out->resize((size_t)kept);
    return rc;
}

} // namespace acxh

extern "C" {

int acx_words_host(const uint8_t *hay, uint64_t len, const uint64_t *offsets, uint64_t n_hay, const acx_match_t *m, uint64_t n_m,
                   const uint64_t *counts, int overlapping, int match_kind, const uint8_t *word_set, acx_match_t *out_m,
                   uint64_t *out_counts, uint64_t *n_out) {
    if (!n_out || (n_m && (!m || !out_m)) || (len && !hay)) return fail(ACX_EINVAL, "null argument");
    *n_out = 0;
    WordsArgs A;
    int rc = words_args(overlapping, match_kind, word_set, &A);
    if (rc != ACX_OK) return rc;
    if (!offsets) {
        if (n_hay > 1) return fail(ACX_EINVAL, "several haystacks need offsets");
        n_hay = 1;
    } else if ((rc = offsets_span(offsets, n_hay, len)) != ACX_OK) {
        return rc;
    }
    if (!counts && n_hay > 1) return fail(ACX_EINVAL, "several haystacks need counts");
    if ((rc = counts_sum_to(counts, n_hay, n_m)) != ACX_OK) return rc;
    std::vector<acx_match_t> ww; // one row's whole-word occurrences
    uint64_t first = 0, at = 0;
    for (uint64_t h = 0; h < n_hay; h++) {
        const uint64_t k = counts ? counts[h] : n_m, b = offsets ? offsets[h] : 0, L = (offsets ? offsets[h + 1] : len) - b;
        const uint8_t *row = hay + b;
        const uint64_t begin = at;
        try {
            ww.clear();
            for (uint64_t i = first; i < first + k; i++) {
                const uint64_t s = m[i].start, e = m[i].end;
                if (!(s < e && e <= L)) continue; // (no occurrence of this row)
                if ((s == 0 || !in_set(A.W, row[s - 1])) && (e == L || !in_set(A.W, row[e]))) ww.push_back(m[i]);
            }
            if (!A.overlapping) { // the kind's key; the walk below takes the least record with start >= pos every time
                std::stable_sort(ww.begin(), ww.end(), [&](const acx_match_t &x, const acx_match_t &y) {
                    if (A.kind == ACX_MATCH_STANDARD) return std::make_tuple(x.end, x.start, x.pattern) < std::make_tuple(y.end, y.start, y.pattern);
                    if (A.kind == ACX_MATCH_LEFTMOST_FIRST) return std::make_tuple(x.start, x.pattern) < std::make_tuple(y.start, y.pattern);
                    return std::make_tuple(x.start, ~x.end, x.pattern) < std::make_tuple(y.start, ~y.end, y.pattern);
                });
            }
        } catch (...) { return fail(ACX_ENOMEM, "out of memory"); }
        uint64_t pos = 0;
        for (const acx_match_t &r : ww) {
            if (!A.overlapping && r.start < pos) continue;
            out_m[at++] = r;
            pos = r.end;
        }
        if (out_counts) out_counts[h] = at - begin;
        first += k;
    }
    *n_out = at;
    return ACX_OK;
}

int acx_words_rows_device(const void *d_hay, uint64_t len, const uint64_t *d_offsets, uint64_t n_hay, uint64_t uniform_len,
                          const acx_match_t *d_m, uint64_t n_m, const uint64_t *d_counts, int overlapping, int match_kind,
                          const uint8_t *word_set, acx_match_t *d_out_m, uint64_t *d_out_counts, uint64_t *n_out) {
    if (!n_out) return fail(ACX_EINVAL, "null argument");
    *n_out = 0;
    WordsArgs A;
    int rc = words_args(overlapping, match_kind, word_set, &A);
    if (rc != ACX_OK) return rc;
    if ((rc = device_rows_args(d_offsets, &n_hay, uniform_len, len)) != ACX_OK) return rc;
    if (!n_hay) return n_m ? fail(ACX_EINVAL, "the counts do not sum to the number of records") : ACX_OK;
    if (!d_out_counts || (len && !d_hay) || (n_m && (!d_m || !d_counts || !d_out_m))) return fail(ACX_EINVAL, "null argument");
    if (((uintptr_t)d_m | (uintptr_t)d_counts | (uintptr_t)d_offsets | (uintptr_t)d_out_m | (uintptr_t)d_out_counts) & 7)
        return fail(ACX_EINVAL, "records, counts and offsets must be 8-byte aligned");
    return rows_call(d_out_counts, [&](int device, void **block, void **) -> int {
        if (!n_m) { // no record: no whole word
            HIPCHK(hipMemsetAsync(d_out_counts, 0, n_hay * 8, nullptr));
            return ACX_OK;
        }
        const int span = device_offsets_span(d_offsets, n_hay, len);
        if (span != ACX_OK) return span;
        WordsStage S;
        const acx::RowCut R{d_offsets, uniform_len, n_hay, len};
        const int sized = words_sizes(device, nullptr, d_m, n_m, d_counts, R, true, (const uint8_t *)d_hay, A, &S);
        *block = S.block;
        if (sized != ACX_OK) return sized;
        *n_out = S.total;
        return words_finish(S, acx::WordsOut{d_out_m, nullptr, nullptr, nullptr}, nullptr, d_out_counts, nullptr);
    });
}

} // extern "C"
