// mask_api.cpp -- the cover of a search's matches (mask.hpp): the host form, the device stage behind the find pipeline, the
// acx_mask* entry points and the accessors of their result.
#include "mask.hpp"
#include "replace.hpp"
#include "result_block.hpp"

using namespace acxh;

// acx_mask / acx_mask_device: the rows' offsets (rows + 1 words from 0) and the output's bytes in ONE block
// (result_block.hpp).  Device route: the find's records and the stage's temporaries have gone back to the cache behind the
// stage's kernels.
struct ACX_HIDDEN acx_masked : ResultBlock {
    enum { OFFSETS, DATA, N_PARTS };
    uint64_t rows = 0, bytes = 0;

    int alloc() { return alloc_parts({(rows + 1) * 8, bytes}); } // the block (by on_device) and its two parts
    int64_t *offsets() const { return at<int64_t>(OFFSETS); }
    uint8_t *data() const { return at<uint8_t>(DATA); }
};

namespace {

int check_flags(uint32_t flags) {
    return flags & ~(uint32_t)ACX_MASK_ZERO ? fail(ACX_EINVAL, "unknown mask flags") : ACX_OK;
}

// The device stage on stream st: d_out becomes a copy of d_hay (or zeros: ACX_MASK_ZERO; or stays as it is: d_out == d_hay),
// then the records' bytes are painted.  d_m: n records; d_counts: R.n words that sum to n (check_sum: record_offsets,
// behind the copy or the clear).  No record, no row or no byte: nothing beyond the copy or the clear.  *block: the stage's
// temporaries, one block of the buffer cache -- the caller's to return, behind the stage's kernels.
int mask_stage(int device, hipStream_t st, const uint8_t *d_hay, const acx::RowCut &R, const acx_match_t *d_m, uint64_t n,
               const uint64_t *d_counts, bool check_sum, uint8_t fill, uint32_t flags, uint8_t *d_out, void **block) {
    if (R.len && d_out != d_hay) {
        if (flags & ACX_MASK_ZERO) HIPCHK(hipMemsetAsync(d_out, 0, R.len, st));
        else HIPCHK(hipMemcpyAsync(d_out, d_hay, R.len, hipMemcpyDeviceToDevice, st));
    }
    if (!n || !R.n || !R.len) return ACX_OK;
    // [rec_off: rows + 1][scan][tiles], every part 256-byte aligned
    Carver C;
    const uint64_t o_rec = C.part(R.n + 1), o_scan = C.part(replace_scan_words(R.n)), o_tiles = C.part(acx::mask_tile_words(n));
    HIPCHK(g_bufs.get(block, C.bytes(), device));
    uint64_t *b = (uint64_t *)*block;
    int64_t *rec_off = (int64_t *)(b + o_rec);
    if (int rc = record_offsets(d_counts, R.n, n, check_sum, rec_off, b + o_scan, st)) return rc;
    HIPCHK(acx::mask_paint(d_m, n, rec_off, R, fill, b + o_tiles, d_out, st));
    return ACX_OK;
}

// The device route: the find pipeline as acx_find_device runs it (batch splits and the expansion of copies included, byte
// offsets: no offset is reported) on d_search, then the stage on the same stream over d_hay -- the caller's own bytes.
// Returns with the stage in flight (out->done).  d_hay, d_search and G.offsets must stay valid until then.
int run_mask(acx_automaton *a, Ctx *x, const uint8_t *d_hay, const uint8_t *d_search, uint64_t len, const Segments &G,
             int overlapping, uint8_t fill, uint32_t flags, acx_masked_t **out) {
    const uint64_t rows = rows_of(G).n;
    // (an empty batch, or empty rows only: nothing to search)
    return find_stage(a, x, d_search, len, G, overlapping, 0, rows && len, out, [&](FindStage<acx_masked> &F) -> int {
        acx_masked *R = F.R;
        acx_result *r = F.r;
        hipStream_t st = F.st;
        R->rows = rows;
        R->bytes = len;
        int rc;
        if ((rc = R->alloc()) != ACX_OK) return rc;
        const acx::RowCut MR = row_cut(G, len);
        if (!rows) {
            HIPCHK(hipMemsetAsync(R->offsets(), 0, 8, st));
        } else {
            HIPCHK(acx::mask_offsets(MR, R->offsets(), st));
        }
        const uint64_t *d_counts = nullptr;
        if (r && (rc = F.counts(&d_counts)) != ACX_OK) return rc;
        return mask_stage(a->device, st, d_hay, MR, r ? r->d_matches : nullptr, r ? r->n : 0, d_counts, false, fill, flags, R->data(),
                          &F.temp);
    });
}

} // namespace

extern "C" {

int acx_mask_host(const uint8_t *hay, uint64_t len, const uint64_t *offsets, uint64_t n_hay, const acx_match_t *m, uint64_t n_m,
                  const uint64_t *counts, uint8_t fill, uint32_t flags, uint8_t *dst) {
    int rc = check_flags(flags);
    if (rc != ACX_OK) return rc;
    const bool zero = (flags & ACX_MASK_ZERO) != 0;
    if ((n_m && !m) || (len && (!dst || (!hay && !zero)))) return fail(ACX_EINVAL, "null argument");
    if (zero && len && dst == hay) return fail(ACX_EINVAL, "ACX_MASK_ZERO cannot be made in place");
    if (!offsets) {
        if (n_hay > 1) return fail(ACX_EINVAL, "several haystacks need offsets");
        n_hay = 1;
    } else if ((rc = offsets_span(offsets, n_hay, len)) != ACX_OK) {
        return rc;
    }
    if (!counts && n_hay > 1) return fail(ACX_EINVAL, "several haystacks need counts");
    if ((rc = counts_sum_to(counts, n_hay, n_m)) != ACX_OK) return rc;
    if (len) {
        if (zero) std::memset(dst, 0, len);
        else if (dst != hay) std::memmove(dst, hay, len);
    }
    uint64_t at = 0;
    for (uint64_t h = 0; h < n_hay; h++) {
        const uint64_t b = offsets ? offsets[h] : 0, rowlen = (offsets ? offsets[h + 1] : len) - b;
        for (const uint64_t end = counts ? at + counts[h] : n_m; at < end; at++) {
            const uint64_t e = std::min<uint64_t>(m[at].end, rowlen), s = std::min<uint64_t>(m[at].start, e); // clipped to the row
            if (e > s) std::memset(dst + b + s, fill, e - s);
        }
    }
    return ACX_OK;
}

int acx_mask(acx_automaton_t *a, const uint8_t *hay, uint64_t len, const uint64_t *offsets, uint64_t n_hay, int overlapping,
             uint8_t fill, uint32_t flags, acx_masked_t **out) {
    if (!a || !out) return fail(ACX_EINVAL, "null argument");
    *out = nullptr;
    int rc = check_flags(flags);
    if (rc == ACX_OK && overlapping) rc = check_overlapping(a); // (the error, no device state)
    if (rc != ACX_OK) return rc;
    HostBatch B;
    if ((rc = host_batch(hay, &len, offsets, &n_hay, &B)) != ACX_OK) return rc;
    // the find as it is (the small-call kernel, its resident form, the in-place read, the staged pipeline all still apply):
    // the records cross the bus, the output never does
    HostFind f;
    const bool search = n_hay && len; // (an empty batch, or empty rows only: nothing to search, nothing to paint)
    if ((rc = f.find(a, B.hay, len, offsets ? B.rel.data() : nullptr, n_hay, overlapping, 0, search)) != ACX_OK) return rc;
    acx_masked_t *R = new_result<acx_masked_t>(a->device, false);
    if (!R) return ACX_ENOMEM;
    R->rows = n_hay;
    R->bytes = len;
    if ((rc = R->alloc()) == ACX_OK) {
        for (uint64_t h = 0; h <= n_hay; h++) R->offsets()[h] = (int64_t)B.rel[h];
        if (search) rc = acx_mask_host(B.hay, len, B.rel.data(), n_hay, f.m, f.nm, f.counts.data(), fill, flags, R->data());
    }
    if (rc != ACX_OK) { free_result(R); return rc; }
    *out = R;
    return ACX_OK;
}

int acx_mask_device(acx_automaton_t *a, const void *d_hay, uint64_t len, const uint64_t *d_offsets, uint64_t n_hay,
                    uint64_t uniform_len, int overlapping, uint8_t fill, uint32_t flags, acx_masked_t **out) {
    if (!a || !out) return fail(ACX_EINVAL, "null argument");
    *out = nullptr;
    int rc = check_flags(flags);
    if (rc != ACX_OK) return rc;
    // (a case-insensitive handle: the folded copy is searched, the caller's bytes are copied)
    return device_call(a, d_hay, len, d_offsets, n_hay, uniform_len, overlapping, [&](Ctx *c, const uint8_t *d_search, const Segments &G) {
        return run_mask(a, c, (const uint8_t *)d_hay, d_search, len, G, overlapping, fill, flags, out);
    });
}

int acx_mask_rows_device(const void *d_hay, uint64_t len, const uint64_t *d_offsets, uint64_t n_hay, uint64_t uniform_len,
                         const acx_match_t *d_records, uint64_t n, const uint64_t *d_counts, uint8_t fill, uint32_t flags,
                         void *d_out) {
    int rc = check_flags(flags);
    if (rc != ACX_OK) return rc;
    const bool zero = (flags & ACX_MASK_ZERO) != 0;
    if ((rc = device_rows_args(d_offsets, &n_hay, uniform_len, len)) != ACX_OK) return rc;
    if ((len && (!d_out || (!d_hay && !zero))) || (n && (!d_records || !d_counts))) return fail(ACX_EINVAL, "null argument");
    if (zero && len && d_out == d_hay) return fail(ACX_EINVAL, "ACX_MASK_ZERO cannot be made in place");
    if (!n_hay && n) return fail(ACX_EINVAL, "the counts do not sum to the number of records");
    if (((uintptr_t)d_offsets | (uintptr_t)d_records | (uintptr_t)d_counts) & 7)
        return fail(ACX_EINVAL, "offsets, records and counts must be 8-byte aligned");
    if (!len) return ACX_OK; // (no byte to write)
    return rows_call(d_out, [&](int device, void **block, void **) {
        const int span = device_offsets_span(d_offsets, n_hay, len);
        if (span != ACX_OK) return span;
        const acx::RowCut R{d_offsets, uniform_len, n_hay, len};
        return mask_stage(device, nullptr, (const uint8_t *)d_hay, R, d_records, n, d_counts, true, fill, flags, (uint8_t *)d_out, block);
    });
}

uint64_t acx_masked_rows(const acx_masked_t *m) { return m ? m->rows : 0; }
uint64_t acx_masked_bytes(const acx_masked_t *m) { return m ? m->bytes : 0; }
int acx_masked_on_device(const acx_masked_t *m) { return m ? m->on_device : 0; }

const void *acx_masked_data(const acx_masked_t *m) { return part_ptr(m, acx_masked::DATA, acx_masked::N_PARTS); }
const int64_t *acx_masked_offsets(const acx_masked_t *m) {
    return (const int64_t *)part_ptr(m, acx_masked::OFFSETS, acx_masked::N_PARTS);
}
// (no result and nowhere to copy to are one refusal here; the offsets are never empty)
int acx_masked_copy(const acx_masked_t *m, void *host_dst) {
    return part_copy(m, acx_masked::DATA, acx_masked::N_PARTS, host_dst, "null argument");
}
int acx_masked_copy_offsets(const acx_masked_t *m, int64_t *host_dst) {
    return part_copy(m, acx_masked::OFFSETS, acx_masked::N_PARTS, host_dst, "null argument");
}

void acx_free_masked(acx_masked_t *m) { free_result(m); }

} // extern "C"
