// small_calls.hpp -- K0, the whole call in one workgroup: one launch, or the context's resident kernel (small_calls.cpp).
#pragma once
#include "workspace.hpp"

namespace acxh ACX_HIDDEN {

// K0 takes the call when the haystack is small and nobody asked for a particular scan kernel
bool small_ok(const acx_automaton *a, uint64_t len);
// One K0 launch on a haystack and an output of SMALL_MAX_OCC records the device can address.  *done = false: too many
// occurrences, the general pipeline takes the call.  poll: both are pinned host memory, the result comes in polled lines.
int run_small(acx_automaton *a, Ctx *c, const uint8_t *hay, uint64_t len, int overlapping, int codepoints, acx_match_t *out,
              uint64_t *n_out, bool *done, bool poll = false);
// A small call of the host-memory entry point: the resident K0 or one polled launch; *done: *out holds the *n_out matches
// (malloc; null when there is none), copies of a pattern not yet expanded
int run_small_host(acx_automaton *a, Ctx *c, const uint8_t *hay, uint64_t len, int overlapping, int codepoints,
                   acx_match_t **out, uint64_t *n_out, bool *done);
// the context's resident K0 is told to leave, and has left when this returns
void stop_resident(Ctx *c);
// waits for the line that carries `seq` at word `at` of the context's pinned scratch and takes a verified copy of it
int wait_line(Ctx *c, uint32_t at, uint64_t seq, uint64_t line[8], const char *what);

} // namespace acxh
