// small_calls.cpp -- K0: a whole call in one workgroup, as one launch (run_small) or through the context's resident kernel
// and its mailbox (run_resident), and the polled result lines both answer with (small_calls.hpp; kernels.hpp: the protocol).
#include "small_calls.hpp"

#include <random>

namespace acxh ACX_HIDDEN {

namespace {
void trace_resident(Ctx *c) { // (ACX_RESIDENT_TRACE=1: what the kernel that has just left did -- kernels.hip, k0_resident)
    static const bool on = std::getenv("ACX_RESIDENT_TRACE") != nullptr;
    if (!on) return;
    const uint64_t *s = c->ws.h_pinned + PIN_RESIDENT;
    std::fprintf(stderr, "acx resident K0 epoch %llu: %llu calls, %llu with their bytes in the poll, %.2f us busy per call, %llu polls, delay %llu ticks\n",
                 (unsigned long long)s[0], (unsigned long long)s[1], (unsigned long long)s[2],
                 s[1] ? (double)s[3] / 100.0 / (double)s[1] : 0.0, (unsigned long long)s[4], (unsigned long long)s[5]);
}

void resident_left(Ctx *c) {
    trace_resident(c);
    const uint64_t d = c->ws.h_pinned[PIN_RESIDENT + 5];
    c->res.delay = d < 1000 ? (uint32_t)d : 0;
}
} // namespace

// the context's resident K0 is told to leave, and has left when this returns
void stop_resident(Ctx *c) {
    Resident &R = c->res;
    if (!R.live) return;
    R.live = false;
    volatile uint64_t *status = c->ws.h_pinned + PIN_RESIDENT;
    struct AtExit { Ctx *c; ~AtExit() { resident_left(c); } } at_exit{c};
    if (*status == R.epoch) return;
    // (the word's call number is one the kernel is not waiting for: the quit flag is all it reads)
    __atomic_store_n(c->ws.mailbox.p, k0_mailbox_word(0, 0, false, true), __ATOMIC_RELEASE);
    (void)poll_until([&] { return *status == R.epoch; }, 1023, std::chrono::milliseconds(4),
                     [&] { (void)hipStreamSynchronize(R.stream); });
}

// K0 takes the call when the haystack is small and nobody asked for a particular scan kernel
bool small_ok(const acx_automaton *a, uint64_t len) {
    static const bool off = std::getenv("ACX_NO_SMALL") != nullptr;
    return !off && !a->kernel_forced && len > 0 && a->host.n_patterns > 0 &&
           (len <= SMALL_MAX_LEN || (len <= SMALL_PF_MAX_LEN && small_prefilter_ok(a->dev)));
}

namespace {
// One reading of the polled line at p (kernels.hpp, k0_line_check: one 64-byte line, one store instruction, [0] seq, [1 .. 6]
// payload, [7] seq ^ check(payload)) into a COPY: the line is complete when its first word carries the number and its last
// word agrees with the six in between AS READ HERE -- nothing is read twice, and nothing beside the line is read at all
// (separate device writes to host memory arrive in no particular order).
inline bool read_line(volatile const uint64_t *p, uint64_t seq, uint64_t line[8]) {
    if (p[0] != seq) return false;
    std::atomic_thread_fence(std::memory_order_acquire);
    for (uint32_t i = 1; i < 8; i++) line[i] = p[i];
    return line[7] == (seq ^ k0_line_check(line + 1));
}
} // namespace

// Wait until a kernel has published the line that carries `seq` at pinned word `at` and take a verified copy of it
// (read_line).  The wake-up of a blocking stream synchronisation costs 10-20 us; polling costs one PCIe round trip.
// Falls back to the stream after a few milliseconds.
int wait_line(Ctx *c, uint32_t at, uint64_t seq, uint64_t line[8], const char *what) {
    volatile uint64_t *p = c->ws.h_pinned + at;
    // (the fallback synchronises the context's own stream whoever writes the line -- the resident K0 writes it from its own
    // stream, Resident::stream: which stream to wait for is decided here, and here only)
    hipError_t e = hipSuccess;
    const bool arrived = poll_until([&] { return read_line(p, seq, line); }, 1023, std::chrono::milliseconds(8),
                                    [&] { e = hipStreamSynchronize(c->stream); });
    if (e != hipSuccess) return hipfail(e, "hipStreamSynchronize(c->stream)");
    if (!arrived) return fail(ACX_EDEVICE, what);
    line[0] = seq;
    return ACX_OK;
}

// the result lines behind the first that a polled K0 call with `n` matches wrote (kernels.hpp, K0_RESULT_LINES: the same
// store instruction as the first): verified copies into the workspace
int take_more_lines(Ctx *c, uint64_t seq, uint64_t n) {
    for (uint32_t L = 1; L < k0_result_lines(n); L++) {
        uint64_t line[K0_LINE_WORDS];
        int rc = wait_line(c, PIN_K0 + 8 * L, seq, line, "K0's matches did not arrive");
        if (rc) return rc;
        for (uint32_t i = 1; i < K0_LINE_WORDS - 1; i++) c->ws.h_lines[L][i] = line[i];
    }
    return ACX_OK;
}

namespace {
// a small call was answered by K0, with n matches
void small_call_answered(acx_automaton *a, uint64_t n, uint64_t *n_out, bool *done) {
    *n_out = n;
    *done = true;
    std::lock_guard<std::mutex> lk(a->prof_mu);
    a->profile.small_calls++;
    a->path[7]++;
}
// The first result line of a polled K0 call has been taken (a verified copy): kept for take_small_matches, and -- unless
// the call was too dense for K0 (*done stays false) -- the lines behind it are taken too.
int first_line_taken(acx_automaton *a, Ctx *c, uint64_t seq, const uint64_t line[K0_LINE_WORDS], uint64_t *n_out, bool *done) {
    for (uint32_t i = 1; i < K0_LINE_WORDS - 1; i++) c->ws.h_lines[0][i] = line[i]; // (what the caller unpacks the matches from)
    const uint64_t w1 = line[1]; // matches | too dense << 32 | hash of pin_out << 33
    if (((w1 >> 32) & 1u) != 0) return ACX_OK;
    int rc = take_more_lines(c, seq, w1 & 0xFFFFFFFFull);
    if (rc) return rc;
    small_call_answered(a, w1 & 0xFFFFFFFFull, n_out, done);
    return ACX_OK;
}
} // namespace

// One K0 launch + one sync.  hay / out: anything the device can address (HBM or pinned host);
// out holds SMALL_MAX_OCC records.  *done = false: too many occurrences, use the general path.
// poll: hay and out are host memory the kernel reads / writes in place: wait for the number the kernel publishes
// behind its last store instead of synchronising the stream (tools/ubench_roundtrip.hip: 6 us against 11)
int run_small(acx_automaton *a, Ctx *c, const uint8_t *hay, uint64_t len, int overlapping, int codepoints,
              acx_match_t *out, uint64_t *n_out, bool *done, bool poll) {
    *done = false;
    int rc = ensure_common(c);
    if (rc) return rc;
    Workspace &w = c->ws;
    const int key_mode = overlapping ? 0 : a->host.match_kind;
    const uint64_t seq = poll ? ++c->small_seq : 0;
    HIPCHK(launch_small(view(a, overlapping != 0), hay, (uint32_t)len, key_mode, overlapping != 0, codepoints != 0, out,
                        seq ? w.h_pinned + PIN_K0 : w.h_pinned + PIN_K0_COUNT, seq, c->stream, !(overlapping && a->expand_ov)));
    if (seq) {
        // the result line (kernels.hpp): complete when its first word carries this call's number and its last word
        // agrees with the six in between as read (wait_line: a copy is checked and used)
        uint64_t line[K0_LINE_WORDS];
        int rc = wait_line(c, PIN_K0, seq, line, "K0 did not publish its result");
        if (rc) return rc;
        return first_line_taken(a, c, seq, line, n_out, done);
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    if (w.h_pinned[PIN_K0_DENSE] == 0) small_call_answered(a, w.h_pinned[PIN_K0_COUNT], n_out, done);
    return ACX_OK;
}

namespace {
bool resident_on() {
    static const bool off = std::getenv("ACX_NO_RESIDENT") != nullptr;
    return !off;
}
uint64_t env_ticks(const char *e, uint64_t dflt_us) { // microseconds (an environment value) -> ticks of the device's 100 MHz clock
    const uint64_t us = e && *e ? std::strtoull(e, nullptr, 10) : dflt_us;
    return us * 100;
}
} // namespace

// A small call of the host-memory entry point through the context's RESIDENT K0 (Resident above; kernels.hip k0_resident).
// *taken = false: this call is a plain launch (run_small) -- residency is
// switched off, or the loop alternates between kinds of call.  Otherwise as run_small with poll = true.
int run_resident(acx_automaton *a, Ctx *c, const uint8_t *hay, uint64_t len, int overlapping, int codepoints, uint64_t *n_out,
                 bool *done, bool *taken) {
    *done = false;
    *taken = false;
    Resident &R = c->res;
    if (!resident_on()) return ACX_OK;
    if (R.off) { R.off--; stop_resident(c); return ACX_OK; }
    int rc = ensure_common(c);
    if (rc) return rc;
    Workspace &w = c->ws;
    const DevAutomaton &A = view(a, overlapping != 0);
    const int mode = small_mode(A, (uint32_t)len, !(overlapping && a->expand_ov));
    // (beyond 16 KiB a launch is as good or better -- 60 000 bytes: 28 us launched, 39 through the mailbox, measured; 16 000: 30 and 17)
    if (mode < 0 || len > SMALL_MAX_LEN) { stop_resident(c); return ACX_OK; }
    static const uint64_t idle_ticks = env_ticks(std::getenv("ACX_RESIDENT_IDLE_US"), 200),
                          life_ticks = env_ticks(std::getenv("ACX_RESIDENT_LIFE_US"), 1000);
    volatile uint64_t *status = w.h_pinned + PIN_RESIDENT;
    const int ov = overlapping ? 1 : 0;
    if (R.live && (R.mode != mode || R.overlapping != ov)) {
        // another kind of call than the kernel was launched for: that one leaves, the next one is launched below
        stop_resident(c);
        if (++R.switches >= 4) { R.switches = 0; R.calls = 0; R.off = 256; return ACX_OK; }
    }
    if (++R.calls >= 64) { R.calls = 0; R.switches = 0; }
    const uint64_t seq = ++c->small_seq;
    const int key_mode = overlapping ? 0 : a->host.match_kind;
    auto launch = [&]() -> int { // (the mailbox holds the call: the kernel takes it as its first)
        if (!R.stream) {
            HIPCHK(hipStreamCreateWithFlags(&R.stream, hipStreamNonBlocking));
            std::random_device rd;
            R.secret = ((uint64_t)rd() << 32) ^ rd() ^ (uint64_t)(uintptr_t)c;
        }
        R.epoch++;
        R.mode = mode; R.overlapping = ov;
        HIPCHK(launch_resident(d_view(a, overlapping != 0), mode, w.mailbox, key_mode, ov != 0, w.pin_out, w.h_pinned + PIN_K0,
                               w.h_pinned + PIN_RESIDENT, R.epoch, seq - 1, idle_ticks, life_ticks, R.secret, R.delay, R.stream));
        R.live = true;
        std::lock_guard<std::mutex> lk(a->prof_mu);
        a->path[10]++;
        return ACX_OK;
    };
    // the haystack first (acx_find), its check, the word behind them (one aligned store: the kernel takes the bytes that came
    // with the word when the check agrees, and reads the haystack after it has seen the word otherwise)
    if (!R.live || *status == R.epoch) {
        if (R.live) resident_left(c);
        w.mailbox[0] = 0; // (a word of the past -- a quit -- is not for the kernel launched now)
        rc = launch();
        if (rc) return rc;
    }
    // (nothing between the three writes: a poll that reads the mailbox while they are under way fails its check and reads again;
    // the check is of the bytes the kernel reads -- for a case-insensitive handle the folded copy, hashed behind the copy)
    const uint64_t word = k0_mailbox_word(seq, (uint32_t)len, codepoints != 0, false);
    uint64_t check = folds(a) ? 0 : k0_hay_check(hay, (uint32_t)len, seq, R.secret);
    copy_in(a, w.pin_hay, hay, len);
    std::memset(w.pin_hay + len, 0, (16 - (len & 15)) & 15); // (the check covers whole 16-byte pieces)
    if (folds(a)) check = k0_hay_check(w.pin_hay, (uint32_t)len, seq, R.secret);
    w.mailbox[1] = check;
    __atomic_store_n(w.mailbox.p, word, __ATOMIC_RELEASE);
    // the result line, as run_small waits for it -- and the kernel's epoch: a kernel that has left (idle, end of its life)
    // has published everything it took before it said so (one release store behind its last line): the line is read once
    // more, and a call the kernel did not take is the first call of the next launch
    volatile uint64_t *p = w.h_pinned + PIN_K0;
    uint64_t line[K0_LINE_WORDS];
    auto complete = [&]() -> bool { return read_line(p, seq, line); };
    // every 16 polls: has the kernel left?  Then the line is read once more, and the call is the first of the next launch
    // (a launch that fails ends the wait).  Not after the deadline below: the kernel has been told to leave by then.
    uint32_t polls = 0;
    bool timed_out = false;
    auto answered = [&]() -> bool {
        if (complete()) return true;
        if (timed_out || (polls++ & 15) != 15 || *status != R.epoch) return false;
        std::atomic_thread_fence(std::memory_order_acquire);
        if (complete()) return true;
        resident_left(c);
        return (rc = launch()) != ACX_OK;
    };
    hipError_t sync_e = hipSuccess;
    const bool got = poll_until(answered, 1023, std::chrono::milliseconds(8), [&] {
        // no answer for 8 ms (a kernel that has not started yet -- its hardware queue may be another context's for a
        // while --, a thread of the host that lost its core): the kernel is told to leave, and when the call is not
        // among what it did, a plain launch answers it
        timed_out = true;
        const uint64_t st0 = *status, word0 = w.mailbox[0], l0 = p[0];
        stop_resident(c);
        if ((sync_e = hipStreamSynchronize(R.stream)) != hipSuccess) return;
        static const bool trace = std::getenv("ACX_RESIDENT_TRACE") != nullptr;
        if (trace)
            std::fprintf(stderr, "acx resident K0: call %llu unanswered for 8 ms (epoch %llu, status %llu, word %llx, line %llu): %s\n",
                         (unsigned long long)seq, (unsigned long long)R.epoch, (unsigned long long)st0, (unsigned long long)word0,
                         (unsigned long long)l0, complete() ? "answered by now" : "a launch takes it");
    });
    if (rc) return rc;
    if (sync_e != hipSuccess) return hipfail(sync_e, "hipStreamSynchronize(R.stream)");
    if (!got) { R.off = 64; return ACX_OK; }
    *taken = true;
    return first_line_taken(a, c, seq, line, n_out, done);
}

namespace {
// The matches of a polled K0 call, unpacked into m[0 .. n): the first ride in the result lines (the verified copies
// run_small / run_resident took, not the pinned words themselves), the others are in pin_out; all packed.
int take_small_matches(Ctx *c, uint64_t n, acx_match_t *m) {
    Workspace &w = c->ws;
    auto carried = [&](uint64_t i) -> uint64_t { // (i < K0_LINES_MATCHES: from the lines' verified copies)
        return i < ACX_K0_LINE_MATCHES ? w.h_lines[0][2 + i]
                                       : w.h_lines[1 + (i - ACX_K0_LINE_MATCHES) / K0_MORE_MATCHES][1 + (i - ACX_K0_LINE_MATCHES) % K0_MORE_MATCHES];
    };
    volatile const uint64_t *rest = (volatile const uint64_t *)w.pin_out.p;
    // pin_out and the line are separate writes of the device to host memory: the line carries a hash of what
    // pin_out must hold (k0_rest_mix); what is read here is taken when it agrees, read again when not
    const uint32_t want = (uint32_t)(w.h_lines[0][1] >> K0_REST_HASH_SHIFT);
    const uint64_t sq = c->small_seq;
    auto read_all = [&]() -> bool {
        uint32_t hx = 0;
        for (uint64_t i = 0; i < n; i++) {
            const uint64_t v = i < K0_LINES_MATCHES ? carried(i) : rest[i - K0_LINES_MATCHES];
            if (i >= K0_LINES_MATCHES) hx ^= k0_rest_mix(v, (uint32_t)(i - K0_LINES_MATCHES), sq);
            m[i].pattern = v & 0xFFFFFFFFull; m[i].start = (v >> 32) & 0xFFFF; m[i].end = (v >> 48) + 1;
        }
        return n <= K0_LINES_MATCHES || hx == want;
    };
    // (once the kernel is known to be over its writes have arrived: ONE more reading decides -- a hash that
    // still disagrees is an error, not a reason to synchronise the stream a million times)
    hipError_t e = hipSuccess;
    const bool agreed = poll_until(read_all, 0, std::chrono::milliseconds(8), [&] { e = hipStreamSynchronize(c->stream); });
    if (e != hipSuccess || !agreed) return fail(ACX_EDEVICE, "K0's matches did not arrive");
    return ACX_OK;
}
} // namespace

// small haystack: copied into pinned memory; the context's resident K0 takes it from there (a poll on either
// side), or ONE launch does (K0 reads and writes pinned host memory in place) -- no H2D / D2H copies at all
int run_small_host(acx_automaton *a, Ctx *c, const uint8_t *hay, uint64_t len, int overlapping, int codepoints,
                   acx_match_t **out, uint64_t *n_out, bool *done) {
    *out = nullptr;
    *done = false;
    int rc = ensure_mailbox(c);
    if (rc != ACX_OK) return rc;
    Workspace &w = c->ws;
    uint64_t n = 0;
    bool taken = false;
    if ((rc = run_resident(a, c, hay, len, overlapping, codepoints, &n, done, &taken)) != ACX_OK) return rc;
    if (!taken) {
        copy_in(a, w.pin_hay, hay, len);
        if ((rc = run_small(a, c, w.pin_hay, len, overlapping, codepoints, w.pin_out, &n, done, true)) != ACX_OK) return rc;
    }
    *n_out = n;
    if (!*done || !n) return ACX_OK;
    acx_match_t *m = (acx_match_t *)std::malloc(n * sizeof(acx_match_t));
    if (!m) return fail(ACX_ENOMEM, "out of memory");
    if ((rc = take_small_matches(c, n, m)) != ACX_OK) { std::free(m); return rc; }
    *out = m;
    return ACX_OK;
}

} // namespace acxh
