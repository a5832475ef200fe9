// build_upload.cpp -- from patterns to a handle: the host compiler's entry points, the upload of the automaton's tables and of
// the view without pattern copies, the choice of the scan kernel, replicas.
#include "workspace.hpp"

using namespace acxh;

namespace {

template <typename T>
int upload(acx_automaton *a, hipStream_t st, const T *src, size_t count, const T **dst) {
    size_t bytes = std::max<size_t>(count * sizeof(T), 16);
    bytes = (bytes + 15) / 16 * 16;
    void *d = nullptr;
    HIPCHK(hipMalloc(&d, bytes));
    a->allocs.push_back(d);
    HIPCHK(hipMemsetAsync(d, 0, bytes, st));
    if (count) HIPCHK(hipMemcpyAsync(d, src, count * sizeof(T), hipMemcpyHostToDevice, st));
    *dst = (const T *)d;
    return ACX_OK;
}

int bits_for(uint64_t x) { // number of bits needed to represent x
    int b = 0;
    while (x) { b++; x >>= 1; }
    return b;
}

// ACX_BUILD_ASCII_CASE_INSENSITIVE: the pattern bytes folded into fb, fo the offsets rebased to it -- what the compiler reads
// instead of the caller's (fold.hpp: the automaton of fold(P) is the crate's case-insensitive automaton of P).  false:
// nothing to fold (no flag, no patterns, or offsets the compiler refuses anyway).
bool fold_patterns(const uint8_t *blob, const uint64_t *offsets, uint64_t n, uint32_t flags, std::vector<uint8_t> &fb,
                   std::vector<uint64_t> &fo) {
    if (!(flags & ACX_BUILD_ASCII_CASE_INSENSITIVE) || !n) return false;
    for (uint64_t i = 0; i < n; i++)
        if (offsets[i + 1] < offsets[i]) return false;
    const uint64_t total = offsets[n] - offsets[0];
    fb.assign(total + 1, 0);
    if (total) fold_host(fb.data(), blob + offsets[0], total);
    fo.resize(n + 1);
    for (uint64_t i = 0; i <= n; i++) fo[i] = offsets[i] - offsets[0];
    return true;
}

// the patterns through the host compiler (folded first for a case-insensitive handle); dense_limit: automaton.hpp
int compile_patterns(const uint8_t *blob, const uint64_t *offsets, uint64_t n_patterns, int match_kind, uint32_t flags,
                     uint64_t dense_limit, Automaton &out) {
    static const uint64_t zero_off[1] = {0};
    int code = ACX_OK;
    std::string err;
    try {
        std::vector<uint8_t> fb;
        std::vector<uint64_t> fo;
        if (fold_patterns(blob, offsets, n_patterns, flags, fb, fo)) { blob = fb.data(); offsets = fo.data(); }
        err = compile(blob, n_patterns ? offsets : zero_off, n_patterns, match_kind, out, code, dense_limit);
    } catch (const std::bad_alloc &) {
        return fail(ACX_ENOMEM, "out of host memory while compiling the automaton");
    }
    return code != ACX_OK ? fail(code, err) : ACX_OK;
}

// the device the handle lives on: the one acx_set_device named, or the thread's current one
int pick_device(int *device) {
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0)
        return fail(ACX_EDEVICE, std::string("no HIP device available: ") +
                                     (e != hipSuccess ? hipGetErrorString(e) : "device count is 0"));
    int dev = g_device;
    if (dev < 0) { if (hipGetDevice(&dev) != hipSuccess) dev = 0; }
    *device = dev;
    return ACX_OK;
}

// what the launches need to know about the device, and the handle's first context (*st: its stream, the uploads' stream)
int open_device(acx_automaton *a, hipStream_t *st) {
    if (const char *envc = std::getenv("ACX_MAX_CONCURRENCY")) a->max_ctx = std::max(1, std::min(16, std::atoi(envc)));
    int v = 0;
    HIPCHK(hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, a->device));
    a->n_cus = std::max(v, 1);
    int l1 = 0, l2 = 0;
    (void)hipDeviceGetAttribute(&l1, hipDeviceAttributeMaxSharedMemoryPerBlock, a->device);
    (void)hipDeviceGetAttribute(&l2, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, a->device);
    a->max_lds = (size_t)std::max(std::max(l1, l2), 65536);
    if (a->max_lds > 160 * 1024) a->max_lds = 160 * 1024;
    Ctx *c0 = create_ctx();
    if (!c0) return fail(ACX_EDEVICE, "could not create a HIP stream");
    a->ctxs.push_back(c0);
    a->idle.push_back(c0);
    *st = c0->stream;
    return ACX_OK;
}

// the automaton's tables into HBM (a->dev, and the same struct resident there: a->d_dev); complete on return
int upload_tables(acx_automaton *a, hipStream_t st) {
    Automaton &H = a->host;
    DevAutomaton &D = a->dev;
    D.n_patterns = H.n_patterns; D.n_states = H.n_states; D.stride2 = H.stride2;
    D.min_len = H.min_len; D.max_len = H.max_len; D.filter_q = H.filter_q;
    D.ptab_log2 = H.ptab_log2; D.filter_q2 = H.filter_q2;
    D.short_min_len = H.n_short ? H.short_min_len : 0; D.k1b_min_len = H.long_min_len;
    D.max_shift = H.max_shift;
    {
        static const char *big_env = std::getenv("ACX_FILTER_BIG"); // measurements: 0 / 1 force the choice
        // 1: the level-1 table is saturated (10^5 patterns): every position put to both tests; 2: it passes nearly every
        // position (10^6 patterns): ... and the survivors' windows captured from the row staged in LDS (kernels.hip: K1bLds)
        D.filter_big = big_env ? (uint32_t)std::atoi(big_env)
                               : (H.filter_q == 5 && H.filter_density > 0.6 ? 2u : H.filter_q == 5 && H.filter_density > 0.2 ? 1u : 0u);
    }
    D.rank_bits = (uint32_t)std::max(1, bits_for(H.n_patterns ? H.n_patterns - 1 : 0));
    // compact u16 copy of the hot (lowest-id) rows for K1a's LDS tile
    uint32_t hot_rows = H.dense ? dfa_walk_hot_rows(H.n_states, H.stride2, 160 * 1024) : 0;
    std::vector<uint16_t> hot16(((size_t)hot_rows << H.stride2) + 8, 0xFFFF);
    for (size_t i = 0; i < ((size_t)hot_rows << H.stride2); i++) {
        uint32_t en = H.table[i], id = en & ID_MASK;
        hot16[i] = id < 0x3FFFu ? (uint16_t)(id | ((en >> 30) << 14)) : (uint16_t)0xFFFF;
    }
    D.hot_rows = hot_rows;
    // K1a's compact table (automata of at most 65 535 states): see DevAutomaton::table16
    std::vector<uint16_t> table16;
    std::vector<uint32_t> walk_bfs;
    D.n_classes = H.n_classes;
    D.walk_plain = 0;
    if (H.dense && H.n_states <= 0xFFFF && H.n_patterns > 0) {
        const uint32_t NS = H.n_states, NC = H.n_classes, S = H.stride;
        std::vector<uint8_t> reports(NS, 0); // FLAG_OUT is a property of the TARGET state
        for (size_t i = 0; i < (size_t)NS * S; i++)
            if (H.table[i] & FLAG_OUT) reports[H.table[i] & ID_MASK] = 1;
        std::vector<uint32_t> walk_of(NS);
        walk_bfs.resize(NS);
        uint32_t k = 0;
        for (int pass = 0; pass < 2; pass++) {
            for (uint32_t s = 0; s < NS; s++)
                if (reports[s] == pass) { walk_of[s] = k; walk_bfs[k] = s; k++; }
            if (pass == 0) D.walk_plain = k;
        }
        table16.assign((size_t)NS * NC + 8, 0);
        for (uint32_t w = 0; w < NS; w++)
            for (uint32_t c = 0; c < NC; c++)
                table16[(size_t)w * NC + c] = (uint16_t)walk_of[H.table[(size_t)walk_bfs[w] * S + c] & ID_MASK];
    }
    // (K1a's failureless form -- walk_t3b / walk_t3r / walk_grec -- is part of the host compiler's output)
    int rc;
#define UP(vec, field)                                                           \
    if ((rc = upload(a, st, (vec).data(), (vec).size(), &D.field)) != ACX_OK) return rc;
    if (H.dense) { UP(H.table, table) } else { D.table = nullptr; }
    UP(H.first_child, first_child)
    UP(H.in_byte, in_byte)
    UP(H.fail, fail)
    UP(H.sflags, sflags)
    UP(H.root_next, root_next)
    UP(hot16, hot16)
    if (!table16.empty()) {
        UP(table16, table16)
        UP(walk_bfs, walk_bfs)
    } else {
        D.table16 = nullptr; D.walk_bfs = nullptr;
    }
    if (!H.walk_t3b.empty()) {
        UP(H.walk_t3b, t3b)
        const uint32_t *p2 = nullptr;
        if ((rc = upload(a, st, H.walk_t3r.data(), H.walk_t3r.size(), &p2)) != ACX_OK) return rc;
        D.t3r = reinterpret_cast<const uint2 *>(p2);
        if ((rc = upload(a, st, H.walk_grec.data(), H.walk_grec.size(), &p2)) != ACX_OK) return rc;
        D.grec = reinterpret_cast<const uint4 *>(p2);
    } else {
        D.t3b = nullptr; D.t3r = nullptr; D.grec = nullptr;
    }
    UP(H.own_off, own_off)
    UP(H.own_pid, own_pid)
    UP(H.own1, own1)
    UP(H.dlink, dlink)
    UP(H.level_start, level_start)
    UP(H.plen, plen)
    std::vector<uint32_t> pchars(H.plen.size() + 1, 0);
    for (size_t i = 0; i < H.plen.size(); i++)
        for (uint64_t k = H.offsets[i]; k < H.offsets[i + 1]; k++) pchars[i] += (H.blob[k] & 0xC0) != 0x80;
    UP(pchars, pchars)
    UP(H.rank, rank)
    std::vector<uint32_t> by_rank(H.rank.size() + 1, 0);
    for (uint32_t i = 0; i < H.rank.size(); i++) by_rank[H.rank[i]] = i;
    UP(by_rank, by_rank)
    UP(H.filterA, filterA)
    UP(H.ptab, ptab)
    UP(H.blist, blist)
    if (H.rbloom.empty()) H.rbloom.assign(REDIRECT_BLOOM_WORDS, 0);
    UP(H.rbloom, rbloom)
    if (H.pbits.empty()) H.pbits.assign(4, 0);
    UP(H.pbits, pbits)
    if (H.short_xy.empty()) { H.short_xy.assign(SHORT_XY_WORDS, 0); H.short_codes.assign(4, SHORT_NONE); }
    UP(H.short_xy, short_xy)
    if (H.max_shift) {
        const uint32_t *ph = nullptr;
        if ((rc = upload(a, st, H.phead.data(), H.phead.size(), &ph)) != ACX_OK) return rc;
        D.phead = reinterpret_cast<const uint4 *>(ph);
    } else {
        D.phead = nullptr;
    }
    UP(H.short_codes, short_codes)
    {
        const uint32_t *pi = nullptr;
        if ((rc = upload(a, st, H.pinfo.data(), H.pinfo.size(), &pi)) != ACX_OK) return rc;
        D.pinfo = reinterpret_cast<const uint4 *>(pi);
    }
    H.blob.resize(H.blob.size() + 16, 0); // the verification compares 8 bytes at a time
    UP(H.blob, pat_blob)
    UP(H.offsets, pat_off)
#undef UP
    if ((rc = upload(a, st, H.classes, (size_t)256, &D.classes)) != ACX_OK) return rc;
    if ((rc = upload(a, st, &a->dev, (size_t)1, &a->d_dev)) != ACX_OK) return rc;
    HIPCHK(hipStreamSynchronize(st)); // (the copies read this function's vectors)
    return ACX_OK;
}

// the view of a non-overlapping search (struct acx_automaton): only when some string is there more than once
int upload_copy_view(acx_automaton *a, hipStream_t st) {
    Automaton &H = a->host;
    int rc;
    static const bool no_nov = std::getenv("ACX_NO_COPY_VIEW") != nullptr; // measurements
    std::vector<uint8_t> later(H.n_patterns, 0); // a copy of a string with a lower id
    uint64_t n_later = 0;
    for (uint32_t s2 = 0; s2 < H.n_states && H.match_kind == ACX_MATCH_STANDARD; s2++)
        for (uint32_t k = H.own_off[s2] + 1; k < H.own_off[s2 + 1]; k++) { later[H.own_pid[k]] = 1; n_later++; }
    if (!n_later || no_nov) return ACX_OK;
    std::vector<uint32_t> own1_nov(H.n_states, OWN1_NONE);
    for (uint32_t s2 = 0; s2 < H.n_states; s2++)
        if (H.own_off[s2 + 1] > H.own_off[s2]) own1_nov[s2] = H.own_pid[H.own_off[s2]]; // (lists are in id order)
    std::vector<uint32_t> blist_nov(H.blist);
    for (size_t i = 0; i < blist_nov.size();) { // [count, codes ...] records, back to back
        const uint32_t cnt = H.blist[i];
        uint32_t kept = 0;
        for (uint32_t k = 0; k < cnt; k++)
            if (!later[H.blist[i + 1 + k] & CODE_PID_MASK]) blist_nov[i + 1 + kept++] = H.blist[i + 1 + k];
        uint32_t rest = kept;
        for (uint32_t k = 0; k < cnt; k++)
            if (later[H.blist[i + 1 + k] & CODE_PID_MASK]) blist_nov[i + 1 + rest++] = H.blist[i + 1 + k];
        blist_nov[i] = kept;
        i += (size_t)cnt + 1;
    }
    std::vector<uint32_t> own_off_nov((size_t)H.n_states + 1, 0), own_pid_nov(H.own_pid.size(), 0);
    for (uint32_t s2 = 0; s2 < H.n_states; s2++) {
        own_off_nov[s2 + 1] = own_off_nov[s2];
        if (own1_nov[s2] != OWN1_NONE) own_pid_nov[own_off_nov[s2 + 1]++] = own1_nov[s2];
    }
    a->dev_nov = a->dev;
    if ((rc = upload(a, st, own1_nov.data(), own1_nov.size(), &a->dev_nov.own1)) != ACX_OK) return rc;
    if ((rc = upload(a, st, blist_nov.data(), blist_nov.size(), &a->dev_nov.blist)) != ACX_OK) return rc;
    if ((rc = upload(a, st, own_off_nov.data(), own_off_nov.size(), &a->dev_nov.own_off)) != ACX_OK) return rc;
    if ((rc = upload(a, st, own_pid_nov.data(), own_pid_nov.size(), &a->dev_nov.own_pid)) != ACX_OK) return rc;
    if (!H.walk_grec.empty()) { // the failureless walk's trie records: {children bitmap, first child | OWN, own1, ..}
        std::vector<uint32_t> grec_nov(H.walk_grec);
        // (only the records that say "several": a tail record's third word is its leaf's pattern, not own1)
        for (uint32_t s2 = 0; s2 < H.n_states; s2++)
            if (grec_nov[4 * (size_t)s2 + 2] == OWN1_MANY) grec_nov[4 * (size_t)s2 + 2] = own1_nov[s2];
        const uint32_t *p2 = nullptr;
        if ((rc = upload(a, st, grec_nov.data(), grec_nov.size(), &p2)) != ACX_OK) return rc;
        a->dev_nov.grec = reinterpret_cast<const uint4 *>(p2);
    }
    if ((rc = upload(a, st, &a->dev_nov, (size_t)1, &a->d_dev_nov)) != ACX_OK) return rc;
    // the copies of every lowest id, for the expansion of an overlapping search's result
    a->x_cnt.assign(H.n_patterns, 0);
    a->x_off.assign(H.n_patterns, 0);
    a->x_ids.reserve(n_later);
    for (uint32_t s2 = 0; s2 < H.n_states; s2++) {
        const uint32_t b = H.own_off[s2], e2 = H.own_off[s2 + 1];
        if (e2 - b < 2) continue;
        a->x_off[H.own_pid[b]] = (uint32_t)a->x_ids.size();
        a->x_cnt[H.own_pid[b]] = e2 - b - 1;
        for (uint32_t k = b + 1; k < e2; k++) a->x_ids.push_back(H.own_pid[k]);
    }
    if ((rc = upload(a, st, a->x_cnt.data(), a->x_cnt.size(), &a->d_xcnt)) != ACX_OK) return rc;
    if ((rc = upload(a, st, a->x_off.data(), a->x_off.size(), &a->d_xoff)) != ACX_OK) return rc;
    if ((rc = upload(a, st, a->x_ids.data(), a->x_ids.size(), &a->d_xids)) != ACX_OK) return rc;
    a->has_nov = true;
    const char *xe = std::getenv("ACX_EXPAND_COPIES");
    a->expand_ov = xe ? std::atoi(xe) != 0 : n_later * 4 >= (uint64_t)H.n_patterns;
    HIPCHK(hipStreamSynchronize(st)); // (the copies read this function's vectors)
    return ACX_OK;
}

// The Implementation hint never selects a slower scan (the reference's README recommends the
// contiguous NFA as the sensible default, README.md:173-177: a caller following that advice must
// not pay for it): it only decides how large a dense table is kept (acx_build_ex).  The plain
// DFA walk stays reachable through acx_set_kernel / ACX_KERNEL=dfa_walk.
void choose_kernel(acx_automaton *a) {
    const bool prefilter_ok = a->host.filter_q >= 3 && a->max_lds >= prefilter_lds_bytes();
    a->kernel = prefilter_ok ? ACX_KERNEL_PREFILTER : ACX_KERNEL_DFA_WALK;
    if (const char *envk = std::getenv("ACX_KERNEL")) {
        if (!std::strcmp(envk, "dfa_walk")) { a->kernel = ACX_KERNEL_DFA_WALK; a->kernel_forced = true; }
        else if (!std::strcmp(envk, "prefilter") && prefilter_ok) {
            a->kernel = ACX_KERNEL_PREFILTER;
            a->kernel_forced = true;
        }
    }
}
} // namespace

extern "C" {

int acx_build(const uint8_t *blob, const uint64_t *offsets, uint64_t n_patterns, int match_kind,
              int implementation, acx_automaton_t **out) {
    return acx_build_ex(blob, offsets, n_patterns, match_kind, implementation, 0, out);
}

int acx_build_ex(const uint8_t *blob, const uint64_t *offsets, uint64_t n_patterns, int match_kind, int implementation,
                 uint32_t flags, acx_automaton_t **out) {
    if (!out) return fail(ACX_EINVAL, "null output pointer");
    *out = nullptr;
    if (flags & ~(uint32_t)ACX_BUILD_ASCII_CASE_INSENSITIVE) return fail(ACX_EINVAL, "unknown build flags");
    if (n_patterns && (!offsets || (!blob && offsets[n_patterns] != offsets[0])))
        return fail(ACX_EINVAL, "null pattern buffer");
    if (implementation < ACX_IMPL_AUTO || implementation > ACX_IMPL_DFA)
        return fail(ACX_EINVAL, "unknown implementation hint");
    acx_automaton *a = new (std::nothrow) acx_automaton();
    if (!a) return fail(ACX_ENOMEM, "out of memory");
    a->flags = flags;
    a->implementation = implementation;
    // implementation=DFA asks for the dense table outright (the reference's DFA, README.md:173-177,
    // has no size limit either): keep it up to 16 GiB of the 288 GB
    int rc = compile_patterns(blob, offsets, n_patterns, match_kind, flags, implementation == ACX_IMPL_DFA ? (16ull << 30) : 0,
                              a->host);
    // ---- device side.  No device => no matcher (there is no CPU fallback).
    if (rc == ACX_OK) rc = pick_device(&a->device);
    if (rc != ACX_OK) { delete a; return rc; }
    DeviceScope scope(a->device);
    hipStream_t st = nullptr;
    rc = open_device(a, &st);
    if (rc == ACX_OK) rc = upload_tables(a, st);
    if (rc == ACX_OK) rc = upload_copy_view(a, st);
    if (rc != ACX_OK) { acx_free_automaton(a); return rc; }
    a->table_bytes = a->host.table.size() * 4;
    // the big host copy of the table is no longer needed
    std::vector<uint32_t>().swap(a->host.table);
    a->sparse_ok = tile_lookback(a->host.max_len) <= MAX_LOOKBACK;
    choose_kernel(a);
    *out = a;
    return ACX_OK;
}

int acx_compile_host(const uint8_t *blob, const uint64_t *offsets, uint64_t n_patterns,
                     int match_kind, acx_host_automaton_t **out) {
    return acx_compile_host_ex(blob, offsets, n_patterns, match_kind, 0, out);
}

int acx_compile_host_ex(const uint8_t *blob, const uint64_t *offsets, uint64_t n_patterns, int match_kind, uint32_t flags,
                        acx_host_automaton_t **out) {
    if (!out) return fail(ACX_EINVAL, "null output pointer");
    *out = nullptr;
    if (flags & ~(uint32_t)ACX_BUILD_ASCII_CASE_INSENSITIVE) return fail(ACX_EINVAL, "unknown build flags");
    if (n_patterns && (!offsets || (!blob && offsets[n_patterns] != offsets[0])))
        return fail(ACX_EINVAL, "null pattern buffer");
    acx_host_automaton *h = new (std::nothrow) acx_host_automaton();
    if (!h) return fail(ACX_ENOMEM, "out of memory");
    const int rc = compile_patterns(blob, offsets, n_patterns, match_kind, flags, 0, h->host);
    if (rc != ACX_OK) { delete h; return rc; }
    h->flags = flags;
    *out = h;
    return ACX_OK;
}

int acx_host_tables(const acx_host_automaton_t *h, acx_host_tables_t *out) {
    if (!h || !out) return fail(ACX_EINVAL, "null argument");
    const Automaton &A = h->host;
    out->n_patterns = A.n_patterns; out->n_states = A.n_states;
    out->n_classes = A.n_classes; out->stride = A.stride;
    out->min_pattern_len = A.min_len; out->max_pattern_len = A.max_len;
    out->classes = A.classes; out->table = A.dense ? A.table.data() : nullptr;
    out->prefix_bitmap = A.pbits.data();
    out->dense = A.dense ? 1 : 0;
    out->first_child = A.first_child.data(); out->in_byte = A.in_byte.data();
    out->fail = A.fail.data(); out->state_flags = A.sflags.data();
    out->walk_t3b = A.walk_t3b.empty() ? nullptr : A.walk_t3b.data();
    out->walk_t3r = A.walk_t3r.empty() ? nullptr : A.walk_t3r.data();
    out->walk_grec = A.walk_grec.empty() ? nullptr : A.walk_grec.data();
    out->own_off = A.own_off.data(); out->own_pid = A.own_pid.data();
    out->dlink = A.dlink.data(); out->level_start = A.level_start.data();
    out->pattern_len = A.plen.data(); out->rank = A.rank.data();
    out->filter_xy = A.filterA.data();
    out->prefix_table = A.ptab.data();
    out->prefix_lists = A.blist.data();
    out->filter_q = A.filter_q; out->filter_q2 = A.filter_q2;
    out->filter_entries_log2 = FILTER_ENTRIES_LOG2; out->prefix_table_log2 = A.ptab_log2;
    out->filter_density = A.filter_density;
    out->n_prefix_keys = A.n_prefix_keys;
    out->n_prefix_lists = (uint32_t)A.blist.size();
    out->max_shift = A.max_shift; out->pattern_shift = A.shift.data();
    out->pattern_head = A.phead.empty() ? nullptr : A.phead.data();
    out->long_min_len = A.long_min_len; out->n_short = A.n_short; out->short_min_len = A.n_short ? A.short_min_len : 0;
    out->short_xy = A.n_short ? A.short_xy.data() : nullptr;
    out->short_codes = A.n_short ? A.short_codes.data() : nullptr;
    return ACX_OK;
}

uint32_t acx_filter_hash(uint32_t gram) { return filter_hash(gram); }
uint32_t acx_prefix_slot(uint64_t gram, uint32_t q2, uint32_t log2) {
    return prefix_slot(prefix_home_hash(q2 >= 8 ? gram : (gram & ((1ull << (8 * q2)) - 1)), q2), log2);
}

void acx_free_host(acx_host_automaton_t *h) { delete h; }

void acx_free_automaton(acx_automaton_t *a) {
    if (!a) return;
    DeviceScope scope(a->device);
    for (Ctx *c : a->ctxs) destroy_ctx(c, a->device);
    for (void *p : a->allocs) (void)hipFree(p);
    delete a;
}

int acx_automaton_info(const acx_automaton_t *a, acx_info_t *out) {
    if (!a || !out) return fail(ACX_EINVAL, "null argument");
    std::memset(out, 0, sizeof(*out));
    out->n_patterns = a->host.n_patterns;
    out->n_states = a->host.n_states;
    out->n_classes = a->host.n_classes;
    out->stride = a->host.stride;
    out->min_pattern_len = a->host.min_len;
    out->max_pattern_len = a->host.max_len;
    out->table_bytes = a->table_bytes;
    out->lds_hot_rows = std::min(a->dev.hot_rows,
                                 dfa_walk_hot_rows(a->host.n_states, a->host.stride2, a->max_lds));
    out->kernel = a->kernel;
    out->match_kind = a->host.match_kind;
    out->device = a->device;
    out->filter_q = a->host.filter_q;
    out->flags = a->flags;
    return ACX_OK;
}

int acx_set_kernel(acx_automaton_t *a, int kernel) {
    if (!a) return fail(ACX_EINVAL, "null automaton");
    if (kernel == ACX_KERNEL_DFA_WALK) { a->kernel = kernel; a->kernel_forced = true; return ACX_OK; }
    if (kernel == ACX_KERNEL_PREFILTER) {
        if (a->host.filter_q == 0 || a->max_lds < prefilter_lds_bytes())
            return fail(ACX_EINVAL, "prefilter kernel unavailable for this automaton/device");
        a->kernel = kernel;
        a->kernel_forced = true;
        return ACX_OK;
    }
    if (kernel == ACX_KERNEL_AUTO) {
        a->kernel_forced = false;
        a->kernel = (a->host.filter_q >= 3 && a->max_lds >= prefilter_lds_bytes())
                        ? ACX_KERNEL_PREFILTER : ACX_KERNEL_DFA_WALK;
        return ACX_OK;
    }
    return fail(ACX_EINVAL, "unknown kernel");
}

int acx_replicate(const acx_automaton_t *a, int device, acx_automaton_t **out) {
    if (!a || !out) return fail(ACX_EINVAL, "null argument");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
        return fail(ACX_EINVAL, "device ordinal out of range");
    const int saved = g_device;
    g_device = device;
    // (the host copy keeps the pattern bytes and offsets -- folded ones for a case-insensitive handle: folding is
    // idempotent -- and the replica is compiled from them)
    const int rc = acx_build_ex(a->host.blob.data(), a->host.offsets.data(), a->host.n_patterns, a->host.match_kind,
                                a->implementation, a->flags, out);
    g_device = saved;
    if (rc == ACX_OK && a->kernel_forced) (void)acx_set_kernel(*out, a->kernel);
    return rc;
}

int acx_automaton_device(const acx_automaton_t *a) { return a ? a->device : -1; }

} // extern "C"
