// rows_api.cpp -- a delimited buffer cut into rows (rows.hpp): the host form, the device stage, the acx_split_rows* entry
// points and the accessors of their result.  No automaton is involved: the result is the `offsets` the batch entry points take.
#include "rows.hpp"
#include "replace.hpp"
#include "result_block.hpp"

using namespace acxh;

// acx_split_rows / acx_split_rows_device: rows + 1 int64 words in ONE block (result_block.hpp).  Device route: the stage's
// temporaries have gone back to the cache behind the stage's kernels.
struct ACX_HIDDEN acx_rows : ResultBlock {
    uint64_t rows = 0, bytes = 0;

    int alloc() { return alloc_parts({(rows + 1) * 8}); } // the block (by on_device): its one part
    int64_t *offsets() const { return at<int64_t>(0); }
};

namespace {

// the definition on the host: the delimiters of hay[0 .. len), and -- out != null -- the offsets (room for them is the caller's)
uint64_t host_cut(const uint8_t *hay, uint64_t len, uint8_t d, int64_t *out) {
    uint64_t n = 0;
    if (out) out[0] = 0;
    for (const uint8_t *p = hay, *e = hay + len; p < e; p++) {
        p = (const uint8_t *)std::memchr(p, d, (size_t)(e - p));
        if (!p) break;
        n++;
        if (out) out[n] = (int64_t)(p - hay) + 1;
    }
    const bool open = len && hay[len - 1] != d;
    if (open && out) out[n + 1] = (int64_t)len;
    return n + (open ? 1 : 0);
}

int too_small(uint64_t rows, uint64_t capacity) {
    return fail(ACX_EINVAL, "the offsets buffer holds " + std::to_string(capacity) + " words, " + std::to_string(rows + 1) + " are needed");
}

// The temporaries of one run of the device stage: one block of the buffer cache.
struct Stage {
    void *block = nullptr;
    const int64_t *base = nullptr; // the scan of the tile counts, and behind its last entry (the total) the last-byte flag
    uint64_t total = 0;
    bool open = false;             // the last row has no delimiter
};

// The stage up to the point where the result's size is known: the tile counts, their scan, and the 16 bytes that cross the
// bus (len > 0).
int stage_sizes(int device, hipStream_t st, const uint8_t *d_hay, uint64_t len, uint8_t d, Stage *S, uint64_t *rows) {
    const uint64_t ntiles = acx::rows_tiles(d_hay, len);
    if (ntiles >= (1ull << 31)) return fail(ACX_ETOOBIG, "the buffer is too long to be cut in one call");
    // [counts: ntiles][base: ntiles + 1, flag][scan], every part 256-byte aligned
    Carver C;
    const uint64_t o_counts = C.part(ntiles), o_base = C.part(ntiles + 2), o_scan = C.part(replace_scan_words(ntiles));
    HIPCHK(g_bufs.get(&S->block, C.bytes(), device));
    uint64_t *b = (uint64_t *)S->block;
    S->base = (const int64_t *)(b + o_base);
    HIPCHK(acx::rows_count(d_hay, len, d, b + o_counts, b + o_base + ntiles + 1, st));
    HIPCHK(acx::replace_scan(nullptr, nullptr, b + o_counts, ntiles, (int64_t *)(b + o_base), b + o_scan, st));
    uint64_t back[2] = {0, 0}; // the delimiters and whether the last byte is one: all that crosses the bus
    HIPCHK(hipMemcpyAsync(back, b + o_base + ntiles, 16, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (back[0] > len || back[1] > 1) return fail(ACX_EDEVICE, "the tile counts do not fit the buffer's length");
    S->total = back[0];
    S->open = back[1] == 0;
    *rows = back[0] + (S->open ? 1 : 0);
    return ACX_OK;
}

// one word, 0, at d_offsets: what an empty buffer is cut into (a copy, no kernel)
int zero_word(int64_t *d_offsets) {
    static const int64_t zero = 0;
    HIPCHK(hipMemcpy(d_offsets, &zero, 8, hipMemcpyHostToDevice));
    return ACX_OK;
}

} // namespace

extern "C" {

int acx_split_rows_host(const uint8_t *hay, uint64_t len, uint8_t delimiter, int64_t *offsets, uint64_t capacity, uint64_t *n_rows) {
    if (!n_rows || (len && !hay)) return fail(ACX_EINVAL, "null argument");
    const uint64_t rows = host_cut(hay, len, delimiter, nullptr);
    *n_rows = rows;
    if (!offsets) return ACX_OK;
    if (rows + 1 > capacity) return too_small(rows, capacity);
    (void)host_cut(hay, len, delimiter, offsets);
    return ACX_OK;
}

int acx_split_rows(const uint8_t *hay, uint64_t len, uint8_t delimiter, acx_rows_t **out) {
    if (!out) return fail(ACX_EINVAL, "null argument");
    *out = nullptr;
    if (len && !hay) return fail(ACX_EINVAL, "null argument");
    acx_rows_t *R = new_result<acx_rows_t>(0, false);
    if (!R) return ACX_ENOMEM;
    R->rows = host_cut(hay, len, delimiter, nullptr);
    R->bytes = len;
    int rc = R->alloc();
    if (rc != ACX_OK) { free_result(R); return rc; }
    (void)host_cut(hay, len, delimiter, R->offsets());
    *out = R;
    return ACX_OK;
}

int acx_split_rows_device(const void *d_hay, uint64_t len, uint8_t delimiter, acx_rows_t **out) {
    if (!out) return fail(ACX_EINVAL, "null argument");
    *out = nullptr;
    if (len && !d_hay) return fail(ACX_EINVAL, "null argument");
    int device = 0;
    if (len) {
        hipPointerAttribute_t at;
        HIPCHK(hipPointerGetAttributes(&at, d_hay));
        device = at.device;
    } else {
        HIPCHK(hipGetDevice(&device)); // (no byte, no pointer to ask: the calling thread's device)
    }
    DeviceScope ds(device);
    acx_rows_t *R = new_result<acx_rows_t>(device, true);
    if (!R) return ACX_ENOMEM;
    R->bytes = len;
    Stage S;
    auto body = [&]() -> int {
        int rc;
        if (!len) return (rc = R->alloc()) != ACX_OK ? rc : zero_word(R->offsets());
        if ((rc = stage_sizes(device, nullptr, (const uint8_t *)d_hay, len, delimiter, &S, &R->rows)) != ACX_OK) return rc;
        if ((rc = R->alloc()) != ACX_OK) return rc; // (at worst 8 bytes per input byte: a failure is the call's, not the process's)
        HIPCHK(acx::rows_write((const uint8_t *)d_hay, len, delimiter, S.base, S.total, S.open, R->offsets(), nullptr));
        return ACX_OK;
    };
    const int rc = retire_find(body(), nullptr, nullptr, R, S.block);
    if (rc != ACX_OK) { acx_free_rows(R); return rc; }
    *out = R;
    return ACX_OK;
}

int acx_split_rows_into_device(const void *d_hay, uint64_t len, uint8_t delimiter, int64_t *d_offsets, uint64_t capacity,
                               uint64_t *n_rows) {
    if (!n_rows || (len && !d_hay)) return fail(ACX_EINVAL, "null argument");
    *n_rows = 0;
    if ((uintptr_t)d_offsets & 7) return fail(ACX_EINVAL, "the offsets must be 8-byte aligned");
    if (!len) {
        if (!d_offsets) return ACX_OK;
        if (!capacity) return too_small(0, capacity);
        hipPointerAttribute_t at;
        HIPCHK(hipPointerGetAttributes(&at, d_offsets));
        DeviceScope ds(at.device);
        return zero_word(d_offsets);
    }
    return rows_call(d_hay, [&](int device, void **block, void **) -> int {
        Stage S;
        uint64_t rows = 0;
        const int rc = stage_sizes(device, nullptr, (const uint8_t *)d_hay, len, delimiter, &S, &rows);
        *block = S.block;
        if (rc != ACX_OK) return rc;
        *n_rows = rows;
        if (!d_offsets) return ACX_OK;
        if (rows + 1 > capacity) return too_small(rows, capacity);
        const hipError_t e = acx::rows_write((const uint8_t *)d_hay, len, delimiter, S.base, S.total, S.open, d_offsets, nullptr);
        return e == hipSuccess ? ACX_OK : hipfail(e, "rows_write");
    });
}

uint64_t acx_rows_count(const acx_rows_t *r) { return r ? r->rows : 0; }
uint64_t acx_rows_bytes(const acx_rows_t *r) { return r ? r->bytes : 0; }
int acx_rows_on_device(const acx_rows_t *r) { return r ? r->on_device : 0; }
int acx_rows_device(const acx_rows_t *r) { return r ? r->device : 0; }

const int64_t *acx_rows_offsets(const acx_rows_t *r) { return (const int64_t *)part_ptr(r, 0, 1); }
int acx_rows_copy(const acx_rows_t *r, int64_t *host_dst) { return part_copy(r, 0, 1, host_dst, "null argument"); } // (never empty)

void acx_free_rows(acx_rows_t *r) { free_result(r); }

} // extern "C"
