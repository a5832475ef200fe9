// result_block.cpp -- the owner of a post-find result's memory and the accessors of its parts, the end of a post-find stage
// and the checks and the find that the stages' entry points share (result_block.hpp).
#include "result_block.hpp"

#include "replace.hpp"

namespace acxh ACX_HIDDEN {

// The layout rule against the formulas the block results were written with, at the sizes where (x + 31) / 32 * 32,
// max(x, 1) and the 256-byte rounding of a part of bytes change.
namespace {
constexpr uint64_t r32(uint64_t words) { return (words + 31) / 32 * 32; }
constexpr uint64_t least1(uint64_t x) { return x > 1 ? x : 1; }
constexpr uint64_t r256(uint64_t bytes) { return ((bytes > 8 ? bytes : 8) + 255) / 256 * 256; }
constexpr bool same(const Layout &L, uint64_t a0, uint64_t a1, uint64_t a2, uint64_t a3, uint64_t bytes, uint64_t a4 = 0) {
    return L.at[0] == a0 && L.at[1] == a1 && L.at[2] == a2 && L.at[3] == a3 && L.at[4] == a4 && L.bytes == bytes;
}
// columns: three columns of n words and, for a batch, rows + 1 row offsets
constexpr bool columns_ok(uint64_t n, uint64_t rows) {
    const uint64_t c = r32(least1(n)) * 8;
    return same(block_layout({n * 8, n * 8, n * 8}), 0, c, 2 * c, 0, 3 * c) &&
           same(block_layout({n * 8, n * 8, n * 8, (rows + 1) * 8}), 0, c, 2 * c, 3 * c, 3 * c + r32(rows + 1) * 8);
}
// tally: rows + 1 row offsets, then patterns and counts of nnz words
constexpr bool tally_ok(uint64_t rows, uint64_t nnz) {
    const uint64_t r = r32(rows + 1) * 8, c = r32(least1(nnz)) * 8;
    return same(block_layout({(rows + 1) * 8, nnz * 8, nnz * 8}), 0, r, r + c, 0, r + 2 * c);
}
// filter: k rows, k + 1 offsets, then the data, rounded up to 16 bytes for the tile's stores
constexpr bool filter_ok(uint64_t k, uint64_t total) {
    const uint64_t r = (least1(k) * 8 + 255) / 256 * 256, o = ((k + 1) * 8 + 255) / 256 * 256;
    const uint64_t data = (total + 15) / 16 * 16 > 16 ? (total + 15) / 16 * 16 : 16;
    return same(block_layout({k * 8, (k + 1) * 8, data}, 16), 0, r, r + o, 0, r + o + data) &&
           same(block_layout({k * 8, (k + 1) * 8, total}, 16), 0, r, r + o, 0, r + o + data); // (the tail of 16 rounds it itself)
}
// spans: two columns of n words and, for a batch, rows + 1 row offsets
constexpr bool spans_ok(uint64_t n, uint64_t rows) {
    const uint64_t c = r32(least1(n)) * 8;
    return same(block_layout({n * 8, n * 8}), 0, c, 0, 0, 2 * c) &&
           same(block_layout({n * 8, n * 8, (rows + 1) * 8}), 0, c, 2 * c, 0, 2 * c + r32(rows + 1) * 8);
}
// snippets: the bytes, n + 1 offsets, two columns of n words and, for a batch, rows + 1 row offsets
constexpr bool snippets_ok(uint64_t n, uint64_t rows, uint64_t bytes) {
    const uint64_t d = r256(bytes), o = r32(n + 1) * 8, c = r32(least1(n)) * 8;
    return same(block_layout({bytes, (n + 1) * 8, n * 8, n * 8}), 0, d, d + o, d + o + c, d + o + 2 * c) &&
           same(block_layout({bytes, (n + 1) * 8, n * 8, n * 8, (rows + 1) * 8}), 0, d, d + o, d + o + c,
                d + o + 2 * c + r32(rows + 1) * 8, d + o + 2 * c);
}
// mask: rows + 1 offsets, then the bytes
constexpr bool mask_ok(uint64_t rows, uint64_t bytes) {
    return same(block_layout({(rows + 1) * 8, bytes}), 0, r32(rows + 1) * 8, 0, 0, r32(rows + 1) * 8 + r256(bytes));
}
constexpr bool all_ok() {
    for (const uint64_t x : {0, 1, 32, 33})
        for (const uint64_t y : {0, 1, 32, 33})
            if (!columns_ok(x, y) || !tally_ok(x, y) || !filter_ok(x, y) || !spans_ok(x, y) || !mask_ok(x, y * 8) ||
                !mask_ok(x, y * 8 + 1) || !snippets_ok(x, y, 0) || !snippets_ok(x, y, 8 * x + 1))
                return false;
    return true;
}
static_assert(all_ok(), "block_layout no longer places the parts where the results' blocks had them");
static_assert(filter_ok(33, 15) && filter_ok(33, 16) && filter_ok(33, 17) && filter_ok(0, 257), "the filter's data part");
} // namespace

int ResultBlock::alloc(uint64_t bytes) {
    block_bytes = bytes;
    if (on_device) {
        HIPCHK(g_bufs.get(&d_block, bytes, device));
        return ACX_OK;
    }
    h_block = new (std::nothrow) uint8_t[bytes];
    return h_block ? ACX_OK : fail(ACX_ENOMEM, "out of memory");
}

int ResultBlock::alloc_parts(std::initializer_list<uint64_t> part_bytes, uint64_t tail) {
    const Layout L = block_layout(part_bytes, tail);
    const int rc = alloc(L.bytes);
    if (rc != ACX_OK) return rc;
    int k = 0;
    for (const uint64_t b : part_bytes) {
        part[k] = Part{base() + L.at[k], b};
        k++;
    }
    return ACX_OK;
}

const void *part_ptr(const ResultBlock *R, int which, int n) {
    return R && which >= 0 && which < n ? R->ptr_after_wait(R->part[which].at) : nullptr;
}

int part_copy(const ResultBlock *R, int which, int n, void *host_dst, const char *no_such, const char *missing) {
    if (!R || which < 0 || which >= n) return fail(ACX_EINVAL, no_such);
    const ResultBlock::Part &p = R->part[which];
    if (missing && !p.at) return fail(ACX_EINVAL, missing);
    if (p.bytes && !host_dst) return fail(ACX_EINVAL, "null argument");
    return R->copy_out(host_dst, p.at, p.bytes);
}

int ResultBlock::wait() const {
    if (!on_device || !done) return ACX_OK;
    DeviceScope ds(device);
    HIPCHK(hipEventSynchronize(done));
    return ACX_OK;
}

int ResultBlock::copy_out(void *dst, const void *src, uint64_t bytes) const {
    if (!bytes) return ACX_OK;
    if (!on_device) { std::memcpy(dst, src, bytes); return ACX_OK; }
    int rc = wait();
    if (rc != ACX_OK) return rc;
    DeviceScope ds(device);
    HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return ACX_OK;
}

void ResultBlock::release() {
    if (on_device) {
        DeviceScope ds(device);
        if (done) (void)hipEventSynchronize(done);
        for (void *p : scratch) g_bufs.put(p, device);
        g_bufs.put(d_block, device);
        g_events.put(device, done);
    }
    delete[] h_block;
    scratch.clear();
    d_block = nullptr;
    done = nullptr;
    h_block = nullptr;
}

int retire_find(int rc, hipStream_t st, acx_result *r, ResultBlock *R, void *t1, void *t2) {
    const int dev = R->device;
    const bool temps = t1 || t2;
    if (rc == ACX_OK) {
        hipEvent_t freed = r ? g_events.get(dev) : nullptr, freed2 = temps ? g_events.get(dev) : nullptr;
        R->done = g_events.get(dev);
        hipError_t e = hipSuccess;
        const bool have = R->done && (freed || !r) && (freed2 || !temps);
        if (have) {
            if (freed) e = hipEventRecord(freed, st);
            if (e == hipSuccess && freed2) e = hipEventRecord(freed2, st);
            if (e == hipSuccess) e = hipEventRecord(R->done, st);
        }
        if (!have || e != hipSuccess) { // a dry pool: the wait takes the events' place; a failed record: the failure path
            g_events.put(dev, freed);
            g_events.put(dev, freed2);
            g_events.put(dev, R->done);
            freed = freed2 = R->done = nullptr;
            if (e != hipSuccess) rc = hipfail(e, "hipEventRecord");
            else if ((e = hipStreamSynchronize(st)) != hipSuccess) rc = hipfail(e, "hipStreamSynchronize(st)");
        }
        if (rc == ACX_OK) {
            if (r) {
                g_events.put(dev, r->done);
                r->done = nullptr;
                g_bufs.put(r->borrowed ? nullptr : r->d_matches, dev, freed, r->d_counts);
                r->d_matches = nullptr;
                r->d_counts = nullptr;
            }
            g_bufs.put(t1, dev, freed2, t2);
            acx_free_result(r); // (emptied)
            return ACX_OK;
        }
    }
    (void)hipStreamSynchronize(st);
    g_bufs.put(t1, dev);
    g_bufs.put(t2, dev);
    acx_free_result(r);
    return rc;
}

int counts_of(const acx_result *r, hipStream_t st, uint64_t **one, const uint64_t **d_counts) {
    *d_counts = r->d_counts;
    if (r->d_counts) return ACX_OK;
    HIPCHK(g_bufs.get((void **)one, 16, r->device));
    HIPCHK(hipMemcpyAsync(*one, &r->n, 8, hipMemcpyHostToDevice, st));
    *d_counts = *one;
    return ACX_OK;
}

int record_offsets(const uint64_t *d_counts, uint64_t rows, uint64_t n, bool check_sum, int64_t *rec_off, uint64_t *scan_tmp,
                   hipStream_t st) {
    HIPCHK(acx::replace_scan(nullptr, nullptr, d_counts, rows, rec_off, scan_tmp, st));
    if (!check_sum) return ACX_OK;
    uint64_t sum = 0;
    HIPCHK(hipMemcpyAsync(&sum, rec_off + rows, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return sum == n ? ACX_OK : fail(ACX_EINVAL, "the counts do not sum to the number of records");
}

int counts_sum_to(const uint64_t *counts, uint64_t n_hay, uint64_t n_m) {
    bool ok = counts || n_hay || !n_m;
    uint64_t sum = 0;
    for (uint64_t h = 0; ok && counts && h < n_hay; h++) {
        ok = counts[h] <= n_m - sum;
        sum += ok ? counts[h] : 0;
    }
    if (counts && sum != n_m) ok = false;
    return ok ? ACX_OK : fail(ACX_EINVAL, "the counts do not sum to the number of matches");
}

namespace {
int span_error() { return fail(ACX_EINVAL, "offsets must rise from 0 to the batch's length"); }
} // namespace

int offsets_span(const uint64_t *offsets, uint64_t n_hay, uint64_t len) {
    bool ok = offsets[0] == 0 && offsets[n_hay] == len;
    for (uint64_t h = 0; ok && h < n_hay; h++) ok = offsets[h + 1] >= offsets[h];
    return ok ? ACX_OK : span_error();
}

int device_rows_args(const uint64_t *d_offsets, uint64_t *n_hay, uint64_t uniform_len, uint64_t len) {
    if (d_offsets && uniform_len) return fail(ACX_EINVAL, "offsets and uniform_len exclude one another");
    if (!d_offsets && !uniform_len) *n_hay = 1;
    if (uniform_len && *n_hay * uniform_len != len) return fail(ACX_EINVAL, "n_hay * uniform_len is not the batch's length");
    return ACX_OK;
}

int device_offsets_span(const uint64_t *d_offsets, uint64_t n_hay, uint64_t len) {
    if (!d_offsets) return ACX_OK;
    uint64_t ends[2] = {1, 0};
    HIPCHK(hipMemcpy(&ends[0], d_offsets, 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&ends[1], d_offsets + n_hay, 8, hipMemcpyDeviceToHost));
    return ends[0] == 0 && ends[1] == len ? ACX_OK : span_error();
}

int HostFind::find(acx_automaton *a, const uint8_t *hay, uint64_t len, const uint64_t *offsets, uint64_t n_hay, int overlapping,
                   int codepoints, bool search) {
    try {
        counts.assign((offsets ? n_hay : 1) + 1, 0);
    } catch (...) { return fail(ACX_ENOMEM, "out of memory"); }
    if (!search) return ACX_OK;
    if (offsets) return acx_find_batch(a, hay, offsets, n_hay, overlapping, codepoints, &m, &nm, counts.data());
    const int rc = acx_find(a, hay, len, overlapping, codepoints, &m, &nm);
    counts[0] = nm;
    return rc;
}

int host_batch(const uint8_t *hay, uint64_t *len, const uint64_t *offsets, uint64_t *n_hay, HostBatch *B) {
    uint64_t base = 0;
    if (offsets) {
        for (uint64_t i = 0; i < *n_hay; i++)
            if (offsets[i + 1] < offsets[i]) return fail(ACX_EINVAL, "offsets not monotone");
        base = offsets[0];
        *len = offsets[*n_hay] - base;
    } else {
        *n_hay = 1;
    }
    if (*len && !hay) return fail(ACX_EINVAL, "null haystack");
    B->hay = *len ? hay + base : nullptr;
    try {
        B->rel.resize(*n_hay + 1);
    } catch (...) { return fail(ACX_ENOMEM, "out of memory"); }
    for (uint64_t i = 0; i <= *n_hay; i++) B->rel[i] = offsets ? offsets[i] - base : (i ? *len : 0);
    return ACX_OK;
}

} // namespace acxh
