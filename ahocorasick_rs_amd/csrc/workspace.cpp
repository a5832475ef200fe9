// workspace.cpp -- the process-wide pools, the contexts of a handle and their leases, the allocation of a context's
// workspace (every ensure_*), the staging of host haystacks (workspace.hpp).
#include "workspace.hpp"

#include "small_calls.hpp"

namespace acxh ACX_HIDDEN {

EventPool g_events;
BufCache g_bufs;
PinnedResults g_pinned_results;

hipEvent_t EventPool::get(int dev) {
    {
        std::lock_guard<std::mutex> lk(mu);
        for (size_t i = 0; i < free_list.size(); i++)
            if (free_list[i].first == dev) {
                hipEvent_t e = free_list[i].second;
                free_list.erase(free_list.begin() + i);
                return e;
            }
    }
    hipEvent_t e = nullptr;
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return nullptr;
    return e;
}
void EventPool::put(int dev, hipEvent_t e) {
    if (!e) return;
    std::lock_guard<std::mutex> lk(mu);
    if (free_list.size() >= 64) { (void)hipEventDestroy(e); return; }
    free_list.push_back({dev, e});
}

void BufCache::release_locked(void *p, int dev) {
    auto it = live.find(p);
    const size_t bytes = it == live.end() ? 0 : it->second.bytes;
    if (!bytes || cached + bytes > MAX_CACHED || free_list.size() >= 24) {
        if (it != live.end()) live.erase(it);
        DeviceScope ds(dev);
        (void)hipFree(p);
        return;
    }
    free_list.push_back({p, bytes, dev});
    cached += bytes;
}
// Has the event not fired yet?  Every other answer counts as fired.  A query that fails in another way -- the runtime refuses
// an event whose stream has gone with its handle -- must not stay behind as the thread's sticky last error: the check behind
// the next kernel launch would report it as that launch's.
static bool event_pending(hipEvent_t ev) {
    const hipError_t e = hipEventQuery(ev);
    if (e == hipErrorNotReady) return true;
    if (e != hipSuccess) (void)hipGetLastError();
    return false;
}
void BufCache::sweep_locked() {
    for (size_t i = 0; i < deferred.size();) {
        if (event_pending(deferred[i].ev)) { i++; continue; }
        g_events.put(deferred[i].dev, deferred[i].ev);
        release_locked(deferred[i].p, deferred[i].dev);
        if (deferred[i].p2) release_locked(deferred[i].p2, deferred[i].dev);
        deferred.erase(deferred.begin() + i);
    }
}
hipError_t BufCache::get(void **out, size_t bytes, int dev) {
    bytes = std::max<size_t>((bytes + 255) / 256 * 256, 256);
    {
        std::lock_guard<std::mutex> lk(mu);
        if (!deferred.empty()) sweep_locked();
        int best = -1;
        for (int i = 0; i < (int)free_list.size(); i++)
            if (free_list[i].dev == dev && free_list[i].bytes >= bytes &&
                free_list[i].bytes <= bytes * 4 + 65536 &&
                (best < 0 || free_list[i].bytes < free_list[best].bytes))
                best = i;
        if (best >= 0) {
            *out = free_list[best].p;
            cached -= free_list[best].bytes;
            free_list.erase(free_list.begin() + best);
            return hipSuccess;
        }
    }
    // round up so that slightly larger requests can reuse the buffer later
    size_t alloc = bytes + bytes / 4;
    alloc = (alloc + 4095) / 4096 * 4096;
    DeviceScope ds(dev);
    hipError_t e = hipMalloc(out, alloc);
    if (e == hipErrorOutOfMemory) { // give back everything the cache holds idle, then try once more
        (void)hipGetLastError();
        {
            std::lock_guard<std::mutex> lk(mu);
            sweep_locked();
            for (const Ent &f : free_list) {
                live.erase(f.p);
                DeviceScope fs(f.dev);
                (void)hipFree(f.p);
            }
            free_list.clear();
            cached = 0;
        }
        e = hipMalloc(out, alloc);
        if (e != hipSuccess) e = hipMalloc(out, alloc = bytes);
    }
    if (e == hipSuccess) {
        std::lock_guard<std::mutex> lk(mu);
        live[*out] = {*out, alloc, dev};
    }
    return e;
}
void BufCache::put(void *p, int dev, hipEvent_t ev, void *p2) {
    if (!p) { p = p2; p2 = nullptr; }
    if (!p) { g_events.put(dev, ev); return; }
    std::lock_guard<std::mutex> lk(mu);
    if (ev) {
        if (event_pending(ev)) { deferred.push_back({p, p2, dev, ev}); return; }
        g_events.put(dev, ev);
    }
    release_locked(p, dev);
    if (p2) release_locked(p2, dev);
}

void *PinnedResults::get(size_t bytes) {
    std::lock_guard<std::mutex> lk(mu);
    int best = -1;
    for (int i = 0; i < (int)all.size(); i++)
        if (!all[i].used && all[i].bytes >= bytes && (best < 0 || all[i].bytes < all[best].bytes)) best = i;
    if (best >= 0) { all[best].used = true; return all[best].p; }
    size_t alloc = std::max<size_t>(bytes + bytes / 4, 1 << 20);
    if (total + alloc > MAX_TOTAL) { // drop idle buffers, then give up (the caller falls back to malloc)
        for (size_t i = 0; i < all.size();)
            if (!all[i].used) { (void)hipHostFree(all[i].p); total -= all[i].bytes; all.erase(all.begin() + i); }
            else i++;
        if (total + alloc > MAX_TOTAL) return nullptr;
    }
    void *p = nullptr;
    if (hipHostMalloc(&p, alloc, hipHostMallocDefault) != hipSuccess) return nullptr;
    all.push_back({p, alloc, true});
    total += alloc;
    return p;
}
bool PinnedResults::put(void *p) {
    std::lock_guard<std::mutex> lk(mu);
    for (auto &e : all)
        if (e.p == p) { e.used = false; return true; }
    return false;
}

namespace {
// the sparse path's tile arrays, the hot list and the overflow lists: given back as one group, the view and the capacities with them
void free_tiles(Workspace &w) {
    w.tile_bufs = Workspace::TileBufs();
    w.hot_list.reset();
    w.ovf_recs.reset();
    w.T = TileSpace{};
    w.tile_cap = 0;
    w.group_cap = 0;
    w.trecs_gmax = 0;
}
} // namespace

void free_dense_tiles(Workspace &w) {
    w.dense_bufs = Workspace::DenseBufs();
    w.dt = DenseTiles{};
    w.TD = TileSpace{};
    w.dt_cap = 0;
}

void destroy_ctx(Ctx *c, int device) {
    if (!c) return;
    if (c->res.stream) {
        stop_resident(c);
        (void)hipStreamSynchronize(c->res.stream);
        (void)hipStreamDestroy(c->res.stream);
    }
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->copy_stream) (void)hipStreamSynchronize(c->copy_stream);
    g_bufs.put(c->ws.final, device); // (the buffer cache's; every other buffer goes with its owner)
    c->ws = Workspace();
    for (auto &e : c->ev) if (e) (void)hipEventDestroy(e);
    if (c->fork_ev) (void)hipEventDestroy(c->fork_ev);
    if (c->join_ev) (void)hipEventDestroy(c->join_ev);
    if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

Ctx *create_ctx() { // the automaton's device is current
    Ctx *c = new (std::nothrow) Ctx();
    if (!c) return nullptr;
    bool ok = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) == hipSuccess &&
              hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking) == hipSuccess;
    for (auto &e : c->ev) ok = ok && hipEventCreate(&e) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&c->fork_ev, hipEventDisableTiming) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&c->join_ev, hipEventDisableTiming) == hipSuccess;
    if (!ok) { destroy_ctx(c, 0); return nullptr; }
    return c;
}

namespace {
Ctx *take_ctx(acx_automaton *a) {
    std::unique_lock<std::mutex> lk(a->pool_mu);
    for (;;) {
        if (!a->idle.empty()) { Ctx *c = a->idle.back(); a->idle.pop_back(); return c; }
        if ((int)a->ctxs.size() < a->max_ctx) {
            Ctx *c = create_ctx();
            if (c) { a->ctxs.push_back(c); return c; }
            if (a->ctxs.empty()) return nullptr; // nothing to wait for: the caller reports the failure
        }
        a->pool_cv.wait(lk);
    }
}
} // namespace

Lease::Lease(acx_automaton *a_, bool keep_resident) : a(a_), dev(a_->device) {
    c = take_ctx(a);
    if (c && !keep_resident) stop_resident(c);
}
Lease::~Lease() {
    if (!c) return;
    {
        std::lock_guard<std::mutex> lk(a->pool_mu);
        a->idle.push_back(c);
    }
    a->pool_cv.notify_one();
}

int ensure_common(Ctx *c) {
    Workspace &w = c->ws;
    if (!w.summary) {
        HIPCHK(w.summary.grow(16)); // [0..4] totals, [8], [9] scratch, [10], [11] flags of the dense / hot pipeline, [12], [13] the cut of a byte range
        HIPCHK(hipMemsetAsync(w.summary, 0, 128, c->stream)); // (its flags are cleared by the kernels that use them; recycled memory is not zero)
        HIPCHK(w.ctl.grow(2 * CTL_WORDS));
        // (every clearing of the workspace is queued on the CONTEXT'S stream: the stream does not wait for the null stream
        // (hipStreamNonBlocking), and a hipMemset there has been seen to run behind this context's first scan when another
        // thread kept the device busy -- round 6, tools/stress: a fresh handle's first batch lost its overflow hits)
        HIPCHK(hipMemsetAsync(w.ctl, 0, 2 * CTL_WORDS * 4, c->stream));
        HIPCHK(w.ovf_counts.grow(2 * OVF_LISTS * OVF_COUNT_STRIDE));
        HIPCHK(hipMemsetAsync(w.ovf_counts, 0, 2 * OVF_LISTS * OVF_COUNT_STRIDE * 4, c->stream));
        HIPCHK(w.block_counts.grow(16400)); // counts of <= 8192 regions + their exact bases
        HIPCHK(w.region_off.grow(8193));
        HIPCHK(w.hit_counts.grow(16 * 1024));
        // polled by the host while kernels still run: system-coherent
        HIPCHK(w.h_pinned.grow(PINNED_WORDS, hipHostMallocCoherent));
        std::memset(w.h_pinned, 0, PINNED_WORDS * 8);
        w.flags_dirty = true;
    }
    return ACX_OK;
}

// dense path: prefix-hit sink of K1b
int ensure_hits(Ctx *c, uint64_t want) {
    Workspace &w = c->ws;
    if (want <= w.hit_total()) return ACX_OK;
    HIPCHK(w.hrecs.grow(want * 2)); // (records of 32 B: two elements each)
    return ACX_OK;
}

// dense path: occurrence regions + everything the radix sort / resolve pipeline needs
int ensure_occ_capacity(Ctx *c, uint64_t want) {
    Workspace &w = c->ws;
    if (want <= w.cap) return ACX_OK;
    uint64_t cap = std::max<uint64_t>(want, 1u << 16);
    // (the group is given back first -- its arrays are ~72 B per occurrence --, and w.cap says so until all of it is there again)
    Workspace::OccBufs &o = w.occ;
    w.cap = 0;
    o = Workspace::OccBufs();
    w.temp.reset();
    for (int i = 0; i < 2; i++) {
        HIPCHK(o.keys[i].grow(cap));
        HIPCHK(o.pids[i].grow(cap));
    }
    HIPCHK(o.recs.grow(cap));
    HIPCHK(o.S.grow(cap));
    HIPCHK(o.E.grow(cap));
    HIPCHK(o.M.grow(cap));
    HIPCHK(o.flags.grow(cap + 1));
    HIPCHK(o.idx.grow(cap + 1));
    HIPCHK(w.temp.grow(std::max(sort_temp_bytes(cap), scan_temp_bytes(cap)) + 256));
    w.cap = cap;
    return ACX_OK;
}

// sparse path: the list of K1b's hits beyond their tiles' slots (dense stretches of the input; device_types.hpp: control
// block) -- room for `want` records; both control blocks learn where it is (and where the hot list is).  The stream is idle.
constexpr uint64_t OVF_PER_TILE = 16; // records per tile to start with (a quarter of the slots; grown when an input needs more)
int set_overflow_room(Ctx *c, uint64_t want) { // want: records per list
    Workspace &w = c->ws;
    want = std::min<uint64_t>(std::max<uint64_t>(want, 64), 0xFFFFFFF0ull / OVF_LISTS);
    if (want > w.ovf_cap()) {
        // (grow: the new lists first -- a failed allocation leaves the old ones, and the control blocks that point at them, as they are)
        HIPCHK(hipStreamSynchronize(c->stream));
        HIPCHK(w.ovf_recs.grow(want * OVF_LISTS * 2)); // (records of 32 B: two elements each)
    }
    uint32_t h[2 * CTL_WORDS] = {};
    for (int b = 0; b < 2; b++) {
        uint32_t *blk = h + b * CTL_WORDS;
        blk[CTL_OVF_CAP] = (uint32_t)w.ovf_cap();
        const uint64_t recs = (uint64_t)(uintptr_t)w.ovf_recs.p, list = (uint64_t)(uintptr_t)w.hot_list.p;
        const uint64_t counts = (uint64_t)(uintptr_t)(w.ovf_counts.p + (size_t)b * OVF_LISTS * OVF_COUNT_STRIDE);
        std::memcpy(blk + CTL_OVF_RECS, &recs, 8);
        std::memcpy(blk + CTL_HOT_LIST, &list, 8);
        std::memcpy(blk + CTL_OVF_COUNTS, &counts, 8);
    }
    HIPCHK(hipMemcpyAsync(w.ctl, h, sizeof h, hipMemcpyHostToDevice, c->stream)); // (the counters with them: clear)
    HIPCHK(hipMemsetAsync(w.ovf_counts, 0, 2 * OVF_LISTS * OVF_COUNT_STRIDE * 4, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream)); // (h is this function's; and on the context's stream: see ensure_common)
    w.flags_dirty = false;
    return ACX_OK;
}

// sparse path: hit slots for `tiles` tiles of index space, group arrays.  One bucket beyond the
// last tile exists (an occurrence may END exactly at the end of the last tile).
// Nothing is marked as allocated before every allocation has succeeded -- the view T is filled from its owners then --: a
// failure leaves the workspace without its tile arrays (free_tiles), never with control blocks that point at freed memory.
int ensure_tiles(acx_automaton *a, Ctx *c, uint64_t tiles, uint32_t gmax) {
    Workspace &w = c->ws;
    TileSpace &T = w.T;
    const uint64_t groups = (tiles + 1 + GROUP_TILES - 1) / GROUP_TILES;
    if (tiles > w.tile_cap || gmax > w.trecs_gmax) {
        HIPCHK(hipStreamSynchronize(c->stream));
        // (grown, never shrunk: what the larger of the two demands -- tiles, records per group -- had is kept)
        const uint64_t cap_tiles = tiles > w.tile_cap ? tiles + tiles / 8 + GROUP_TILES : w.tile_cap;
        const uint32_t cap_gmax = std::max(gmax, w.trecs_gmax);
        free_tiles(w);
        if (w.final) { g_bufs.put(w.final, a->device); w.final = nullptr; }
        const uint64_t cap_groups = (cap_tiles + 1 + GROUP_TILES - 1) / GROUP_TILES;
        const uint64_t cap_super = (cap_groups + 63) / 64;
        Workspace::TileBufs &B = w.tile_bufs;
        int rc = ACX_OK;
        auto grab = [&](auto &buf, uint64_t n) {
            if (rc != ACX_OK) return;
            if (const hipError_t e = buf.grow(n); e != hipSuccess) rc = hipfail(e, "hipMalloc (tile workspace)");
        };
        grab(B.hslots, cap_tiles * HIT_SLOTS * 2);    // (records of 32 B: two elements each)
        grab(B.hcnt, cap_tiles + 16 * 1024 + 16);     // + one slot per K1b wave (layout slack)
        grab(B.trecs, cap_groups * cap_gmax);
        grab(B.btot, cap_groups);
        grab(B.sgw, 4 * cap_super);
        grab(w.hot_list, cap_groups);
        if (rc == ACX_OK && hipMemsetAsync(B.sgw, 0, 4 * cap_super * 8, c->stream) != hipSuccess) rc = hipfail(hipGetLastError(), "hipMemset"); // both sets start clear
        if (rc == ACX_OK) rc = set_overflow_room(c, (cap_tiles * OVF_PER_TILE + OVF_LISTS - 1) / OVF_LISTS);
        if (rc != ACX_OK) { free_tiles(w); return rc; }
        T.hslots = B.hslots; T.hcnt = B.hcnt; T.trecs = B.trecs; T.btot = B.btot; T.sgw = B.sgw;
        T.sg_cap = (uint32_t)cap_super;
        w.group_cap = cap_groups;
        w.tile_cap = cap_tiles;
        w.trecs_gmax = cap_gmax;
    }
    T.n_tiles = (uint32_t)tiles;
    T.n_groups = (uint32_t)groups;
    T.gmax = gmax;
    return ACX_OK;
}

// dense path, tile-ordered: buckets of DT_SLOTS words per key tile (tiles + 1 of them), DT_GMAX words per group
int ensure_dense_tiles(Ctx *c, uint64_t tiles) {
    Workspace &w = c->ws;
    const uint64_t key_tiles = tiles + 1;
    if (key_tiles > w.dt_cap) {
        free_dense_tiles(w);
        const uint64_t cap = key_tiles + key_tiles / 8 + DT_GROUP;
        const uint64_t cap_groups = (cap + DT_GROUP - 1) / DT_GROUP, cap_super = (cap_groups + 63) / 64;
        Workspace::DenseBufs &B = w.dense_bufs;
        HIPCHK(B.words.grow(cap * DT_SLOTS));
        HIPCHK(B.counts.grow(cap + 16));
        HIPCHK(B.trecs.grow(cap_groups * DT_GMAX / 2)); // (64-bit words: two per element)
        HIPCHK(B.btot.grow(cap_groups));
        HIPCHK(B.sgw.grow(4 * cap_super));
        HIPCHK(hipMemsetAsync(B.sgw, 0, 4 * cap_super * 8, c->stream));
        w.dt.words = B.words; w.dt.counts = B.counts;
        w.TD.trecs = B.trecs; w.TD.btot = B.btot; w.TD.sgw = B.sgw;
        w.TD.sg_cap = (uint32_t)cap_super;
        w.dt_cap = cap;
    }
    w.dt.n_tiles = (uint32_t)key_tiles;
    w.TD.n_tiles = (uint32_t)key_tiles;
    w.TD.n_groups = (uint32_t)((key_tiles + DT_GROUP - 1) / DT_GROUP);
    return ACX_OK;
}

int ensure_blocks(Ctx *c, uint64_t nblocks_plus1) {
    Workspace &w = c->ws;
    if (nblocks_plus1 > w.block_cap) {
        w.block_cap = 0;
        HIPCHK(w.blockcnt.grow(nblocks_plus1));
        HIPCHK(w.blockpre.grow(nblocks_plus1));
        HIPCHK(w.blocksub.grow(nblocks_plus1 * 64)); // one lead-byte count per 16 bytes
        w.block_cap = nblocks_plus1;
    }
    size_t need = std::max<size_t>(scan_temp_bytes(nblocks_plus1), 32768) + 256; // the scan temp storage must cover this size too (block_prefix: 32 KiB of partial sums)
    if (need > w.temp.cap) HIPCHK(w.temp.grow(need));
    return ACX_OK;
}

// small calls of the host entry point: the resident K0's mailbox with the pinned copy of the haystack behind it, K0's pinned output
int ensure_mailbox(Ctx *c) {
    Workspace &w = c->ws;
    if (w.mailbox) return ACX_OK;
    // (both read by the other side while a kernel runs: system-coherent)
    HIPCHK(w.mailbox.grow((K0_MAILBOX_HAY + SMALL_PF_MAX_LEN + 32) / 8, hipHostMallocCoherent));
    w.mailbox[0] = 0;
    w.pin_hay = (uint8_t *)w.mailbox.p + K0_MAILBOX_HAY;
    HIPCHK(w.pin_out.grow(SMALL_MAX_OCC, hipHostMallocCoherent));
    return ACX_OK;
}

// ---------------------------------------------------------------------------
// host memory -> device staging buffer
// ---------------------------------------------------------------------------
// One hipMemcpyAsync from the caller's (pageable) memory, queued ahead of the scan.  The runtime's own pageable copy
// moves 54 GB/s on the MI355X, the link's rate: pinning the caller's pages for the call (55 GB/s, synchronised) and a
// ring of pinned chunks filled by host threads (51 GB/s) were measured and retired (DESIGN_HISTORY.md section 5).
// A case-insensitive handle's haystack is folded in place behind the copy, on the same stream -- unless the caller keeps
// the original bytes there (fold_in_place = false: acx_replace's splice reads them) and folds a copy of its own.
int stage_host(acx_automaton *a, Ctx *c, const uint8_t *hay, uint64_t len, const uint64_t *offsets,
               uint64_t n_off, bool fold_in_place) {
    Workspace &w = c->ws;
    hipStream_t st = c->stream;
    if (len > w.hay.cap) {
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(w.hay.grow(std::max<uint64_t>(len + len / 8, 4096)));
    }
    if (n_off) {
        if (n_off > w.offsets.cap) {
            HIPCHK(hipStreamSynchronize(st));
            HIPCHK(w.offsets.grow(n_off));
        }
        HIPCHK(hipMemcpyAsync(w.offsets, offsets, n_off * 8, hipMemcpyHostToDevice, st));
    }
    if (len) HIPCHK(hipMemcpyAsync(w.hay, hay, len, hipMemcpyHostToDevice, st));
    if (len && fold_in_place && folds(a)) {
        HIPCHK(fold_device(w.hay, w.hay, len, a->n_cus, st));
        a->path[13]++;
    }
    return ACX_OK;
}

// Where the scan of a host call beyond K0's sizes reads its haystack (*d_hay): pinned host memory, or the staging buffer.
// Mid-size haystacks IN PLACE (round 6): copied into pinned host memory by this thread and read from there by the scan
// itself -- the runtime's copy of pageable memory is a staging copy of the same size PLUS a DMA the scan's launch waits
// for (1 MiB: 26 us in the copy call, 21 us in the launch behind it, the DMA's own time before the scan starts).
// Up to 1 MiB (same-box pairs, profiles/r06/exp_inplace_midsize_pairs.txt: 70 KB 45.2 -> 36.6 us, 128 KiB 49.9 -> 41.5,
// 512 KiB 69.8 -> 60.5, 1 MiB 103.1 -> 93.0; 2 MiB 112 -> 134: beyond, this thread's copy is what the call waits for).
// Only while the context's calls stay on the sparse path (a dense input is read several times: from HBM, then).
int place_host_haystack(acx_automaton *a, Ctx *c, const uint8_t *hay, uint64_t len, const uint8_t **d_hay) {
    static const uint64_t inplace_max = std::getenv("ACX_INPLACE_MAX") ? std::strtoull(std::getenv("ACX_INPLACE_MAX"), nullptr, 10) : (1ull << 20);
    Workspace &w = c->ws;
    if (len <= inplace_max && a->kernel == ACX_KERNEL_PREFILTER && a->sparse_ok && c->dense_hold == 0 && !c->wide && c->spec_hot == 0) {
        if (w.pin_mid.cap < len + 4096)
            HIPCHK(w.pin_mid.grow(std::max<uint64_t>(len + len / 4 + 4096, 1ull << 20), hipHostMallocDefault));
        copy_in(a, w.pin_mid, hay, len);
        std::memset(w.pin_mid + len, 0, 64);
        *d_hay = w.pin_mid;
        a->path[11]++;
        return ACX_OK;
    }
    const int rc = stage_host(a, c, hay, len, nullptr, 0);
    *d_hay = w.hay;
    return rc;
}

// A case-insensitive handle's device haystack: folded into the context's grow-only buffer on its stream, at the same address
// modulo 16 (the caller's memory is never written); *d_search = what the find reads.  Other handles search d_hay itself.
int fold_copy(acx_automaton *a, Ctx *c, const uint8_t *d_hay, uint64_t len, const uint8_t **d_search) {
    *d_search = d_hay;
    if (!folds(a) || !len) return ACX_OK;
    Workspace &w = c->ws;
    const uint64_t shift = (uintptr_t)d_hay & 15;
    if (shift + len > w.fold.cap) {
        HIPCHK(hipStreamSynchronize(c->stream)); // (the kernels of an earlier call may still read the old buffer)
        HIPCHK(w.fold.grow((shift + len + 4095) & ~4095ull));
    }
    HIPCHK(fold_device(d_hay, w.fold + shift, len, a->n_cus, c->stream));
    a->path[13]++;
    *d_search = w.fold + shift;
    return ACX_OK;
}

} // namespace acxh
