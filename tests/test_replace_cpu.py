"""CPU checks of the replacement splice (acx_splice_host, the host route of acx_replace): a plain-Python splice of the
oracle's matches is the definition it must meet, and invalid match lists are refused."""
import random

import numpy as np
import pytest

import gen
from oracle_lib import KIND_DFA, Oracle

capi = pytest.importorskip("ahocorasick_rs_amd.capi")


def py_splice(hay: bytes, matches, repl) -> bytes:
    out, at = [], 0
    for p, s, e in matches:
        out.append(hay[at:s])
        out.append(repl[p])
        at = e
    out.append(hay[at:])
    return b"".join(out)


def seeded_repl(n: int, seed: int):
    rng = random.Random(seed)
    lens = [0, 1, 3, 5, 8, 12, 40, 300]
    return [bytes(rng.randrange(32, 127) for _ in range(rng.choice(lens))) for _ in range(n)]


@pytest.mark.parametrize("mk", [0, 1, 2])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_splice_host_equals_oracle_splice(mk, seed):
    pats = gen.gen_patterns(300, 2, 7, b"abcd", seed)
    hay = gen.gen_uniform(20000, b"abcde", seed + 10).tobytes()
    m = Oracle(pats, mk, KIND_DFA).find_raw(hay)
    assert len(m) > 100
    repl = seeded_repl(len(pats), seed)
    want = py_splice(hay, [tuple(int(v) for v in r) for r in m], repl)
    assert capi.splice_host(hay, m, repl) == want


def test_splice_host_edges():
    hay = b"abcXYZabcabc"
    m = [(0, 0, 3), (1, 3, 6), (0, 6, 9), (0, 9, 12)]  # a match at byte 0, adjacent matches, one ending the haystack
    for repl in ([b"", b""], [b"1", b"2"], [b"123", b"456"], [b"L" * 5000, b"M"]):  # empty, shorter, equal, much longer
        assert capi.splice_host(hay, m, repl) == py_splice(hay, m, repl)
    assert capi.splice_host(hay, [], [b"q", b"r"]) == hay  # no matches
    assert capi.splice_host(b"", [], [b"q"]) == b""  # empty haystack
    assert capi.splice_host(b"ab", [(0, 0, 2)], [b""]) == b""  # everything deleted


def test_splice_host_duplicate_patterns():
    pats = [b"ab", b"cd", b"ab"]
    hay = b"xxabyycdab"
    m = Oracle(pats, 0, KIND_DFA).find_raw(hay)
    assert [int(r[0]) for r in m] == [0, 1, 0]  # the lower index of a duplicate is reported
    repl = [b"<0>", b"<1>", b"<2>"]
    assert capi.splice_host(hay, m, repl) == b"xx<0>yy<1><0>"


@pytest.mark.parametrize("bad", [
    [(0, 4, 6), (0, 2, 3)],   # unsorted
    [(0, 2, 5), (0, 4, 6)],   # overlapping
    [(0, 8, 12)],             # beyond the haystack
    [(0, 5, 4)],              # end before start
    [(2, 0, 2)],              # a pattern >= n_repl
])
def test_splice_host_rejects_invalid_matches(bad):
    with pytest.raises(ValueError) as ei:
        capi.splice_host(b"0123456789", bad, [b"a", b"b"])
    assert ei.value.code == capi.EINVAL


def test_replace_abi_is_declared():
    L = capi.lib()
    for name in ("acx_replace", "acx_replace_device", "acx_replaced_len", "acx_replaced_offsets", "acx_replaced_copy",
                 "acx_replaced_device_bytes", "acx_free_replaced", "acx_splice_host"):
        assert hasattr(L, name), name
    assert "replaced_on_device" in capi.Automaton.PATH_STATS
    np.testing.assert_equal(capi.splice_host(b"abc", np.array([[0, 1, 2]], dtype=np.uint64), [b"XY"]), b"aXYc")
