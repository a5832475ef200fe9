"""GPU: the seams of K1b's level 1 -- the lane, row and tile borders of its index space, the ends of the
stream and the lead bytes in front of a misaligned device pointer -- element-wise against the oracle.

The kernel works on the 16-byte aligned address below the haystack pointer: index = lead + stream
position, a lane owns 16 indexes, a row 1 KiB, a tile 4 KiB.  Interior tiles skip the boundary mask; the
first tile (lead > 0) and the tiles the stream ends in apply it (k1b_bounds.hpp).  Every haystack here is
device-resident at a chosen residue of its pointer, the prefilter kernel is forced (K0 never takes a
call: acx_path_stats says so), and patterns are planted where a lane needs its neighbour's bytes, where
lane 63 needs the next row's, across the tile border, flush with the end of the stream, one byte too
late to fit, and in the lead bytes.
"""
import numpy as np
import pytest

import gen
from oracle_lib import KIND_DFA, Oracle

pytestmark = pytest.mark.gpu
capi = pytest.importorskip("ahocorasick_rs_amd.capi")

LENGTHS = [1, 4, 5, 16, 1023, 1024, 1025, 4095, 4096, 4097, 8192 + 21]
RESIDUES = [0, 1, 15]
ALPHABET = np.frombuffer(gen.AZ + b"      ", dtype=np.uint8)  # a-z, a space at one position in six


def pattern_sets():
    q5 = list(dict.fromkeys(gen.gen_patterns(300, 5, 12, gen.AZ, 71)))
    q4 = list(dict.fromkeys(gen.gen_patterns(300, 4, 9, gen.AZ, 72)))
    q3 = list(dict.fromkeys(gen.gen_patterns(300, 3, 8, gen.AZ, 73)))
    sh = list(dict.fromkeys(gen.gen_patterns(250, 5, 10, gen.AZ, 74) + [b"q", b"zx", b"jq", b"kz"]))
    return {"q5": (q5, 5, False), "q4": (q4, 4, False), "q3": (q3, 3, False), "sh": (sh, 5, False),
            "cp": (q5, 5, True)}


SETS = pattern_sets()


def cols(a):
    return np.stack([a["pattern"], a["start"], a["end"]], 1) if len(a) else np.zeros((0, 3), np.uint64)


def build_case(pats, n, lead, seed, tail_fits, multibyte):
    """(bytes in front of the pointer, the stream): `lead` bytes + n bytes of filler with patterns planted at
    the seams of the index space (index = lead + stream position)."""
    rng = np.random.default_rng(seed)
    buf = ALPHABET[rng.integers(0, len(ALPHABET), lead + n)].copy()
    used = np.zeros(lead + n, dtype=bool)
    by_len = sorted(pats, key=len)
    shortest, longest = by_len[0], by_len[-1]
    pick = lambda k: pats[(seed + 7 * k) % len(pats)]

    def plant(idx, p):  # at an index of the kernel's index space; only where it lies wholly inside the stream
        if idx >= lead and idx + len(p) <= lead + n:
            buf[idx:idx + len(p)] = np.frombuffer(p, dtype=np.uint8)
            used[idx:idx + len(p)] = True

    plant(16 * 3 + 15, pick(1))                 # starts at byte 15 of a lane
    plant(16 * 6, pick(2))                      # ... at byte 0 of the next kind of lane (16 of the one before)
    plant(1024 - len(longest), longest)         # bytes .. 1023 of a row: ends flush with the row
    plant(2048 - 3, pick(3))                    # lane 63 reads its look-ahead from the next row
    plant(2048 + 1008, shortest)                # the first byte of lane 63
    plant(4096 - 12, by_len[len(by_len) // 2][:12])  # inside the last 12 bytes of a tile (a prefix may match too)
    plant(4096 - 2, pick(4))                    # across the tile border
    plant(8192 - 1, pick(5))                    # ... and the next one
    # the end of the stream: a pattern flush with the last byte, or the shortest pattern one byte too late to fit
    tail = pick(6) if tail_fits else shortest[:-1]
    if len(tail) and len(tail) <= n:
        buf[lead + n - len(tail):] = np.frombuffer(tail, dtype=np.uint8)
        used[lead + n - len(tail):] = True
    # the lead bytes: a pattern that begins in front of the pointer and runs into the stream -- no match there
    if lead:
        p = pick(8)
        at = max(0, lead + 2 - len(p))
        m = min(len(p), lead + n - at)
        buf[at:at + m] = np.frombuffer(p[:m], dtype=np.uint8)
        used[at:at + m] = True
    if multibyte:  # str API: two-byte characters in the filler, so that code points and bytes part ways
        for at in range(lead + 3, lead + n - 1, 37):
            if not used[at] and not used[at + 1]:
                buf[at], buf[at + 1] = 0xC3, 0xA9
                used[at:at + 2] = True
    return buf[:lead].tobytes(), buf[lead:].tobytes()


def byte_to_code_point(hay: bytes) -> np.ndarray:
    a = np.frombuffer(hay, dtype=np.uint8)
    out = np.zeros(len(a) + 1, dtype=np.uint64)
    np.cumsum((a & 0xC0) != 0x80, out=out[1:])
    return out


def pipeline_calls(st) -> int:
    """calls that the scan kernel's pipeline answered: by the hit slots alone, with the hot pipeline, or densely"""
    return st["sparse"] + st["hot_calls"] + st["dense_tiles"] + st["dense_radix"]


def run(a, o, front, hay, codepoints):
    """the stream at device pointer residue len(front), both match semantics, against the oracle"""
    lead = len(front)
    dev = capi.DeviceBuffer(lead + len(hay) + 16)
    dev.upload(np.frombuffer(front + hay, dtype=np.uint8))
    assert dev.ptr % 16 == 0
    b2c = byte_to_code_point(hay) if codepoints else None
    for ov in (False, True):
        want = o.find_raw(hay, overlapping=ov)
        if codepoints:
            want = np.stack([want[:, 0], b2c[want[:, 1]], b2c[want[:, 2]]], 1) if len(want) else want
        r = a.find_device(dev.ptr + lead, len(hay), overlapping=ov, codepoints=codepoints)
        got = cols(r.matches())
        r.free()
        assert np.array_equal(got, want), (lead, len(hay), ov, len(got), len(want))
    dev.free()


@pytest.mark.parametrize("name", list(SETS))
def test_level1_seams_at_every_length_and_residue(name):
    pats, q, codepoints = SETS[name]
    a = capi.Automaton(pats, 0, kernel=capi.KERNEL_PREFILTER)
    assert a.info.kernel == capi.KERNEL_PREFILTER and a.info.filter_q == q
    o = Oracle(pats, 0, KIND_DFA)
    a.path_stats(reset=True)
    calls = 0
    for n in LENGTHS:
        for lead in RESIDUES:
            for tail_fits in (True, False):
                front, hay = build_case(pats, n, lead, 1000 * n + 10 * lead + tail_fits, tail_fits, codepoints)
                if codepoints:
                    hay.decode("utf-8")
                run(a, o, front, hay, codepoints)
                calls += 2
    st = a.path_stats()
    assert st["k0"] == 0 and pipeline_calls(st) >= calls, st
    a.close()


def test_every_wave_scans_an_interior_tile():
    # 16 MiB + 4 KiB + 7 bytes: 4096 whole tiles for the 4096 waves of a full grid, one more whole tile and a
    # partial one for a second turn; a pattern in every KiB and one across every 4 KiB multiple (the 16 MiB one
    # among them)
    pats, q, _ = SETS["q5"]
    n = (16 << 20) + 4096 + 7
    rng = np.random.default_rng(16)
    buf = ALPHABET[rng.integers(0, len(ALPHABET), n)].copy()
    for k, at in enumerate(range(100, n - 16, 1024)):
        p = pats[k % len(pats)]
        buf[at:at + len(p)] = np.frombuffer(p, dtype=np.uint8)
    for k, at in enumerate(range(4096, n, 4096)):
        p = pats[(5 * k + 1) % len(pats)]
        s = at - 1 - k % (len(p) - 1)  # 1 .. len - 1 bytes in front of the border
        if s + len(p) <= n:
            buf[s:s + len(p)] = np.frombuffer(p, dtype=np.uint8)
    hay = buf.tobytes()
    a = capi.Automaton(pats, 0, kernel=capi.KERNEL_PREFILTER)
    assert a.info.kernel == capi.KERNEL_PREFILTER and a.info.filter_q == q
    o = Oracle(pats, 0, KIND_DFA)
    a.path_stats(reset=True)
    run(a, o, b"", hay, False)
    st = a.path_stats()
    assert st["k0"] == 0 and pipeline_calls(st) >= 2, st
    want = o.find_raw(hay)
    assert len(want) >= (n // 1024) and np.any((want[:, 1] < (16 << 20)) & (want[:, 2] > (16 << 20)))
    a.close()
