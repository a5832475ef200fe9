"""WordPiece tokenization on the device (acx_wordpiece / acx_wordpiece_device / acx_wordpiece_into_device; wordpiece /
wordpiece_batch): the raw form at the seams of its kernels -- data lengths around the tile; words that start on a tile's last
byte, end on its end, continue into the next tile or start on its first byte; words longer than a tile, whose end comes from
the carry, ended by a separator and by a row start; tiles with no word, a word per byte and a word per wave; words of M and
M + 1 bytes, M = WP_MAX_WORD, a pattern longer than M; a node at depth 2 -- under the root and under C's node -- with AT_PROBE
children and with one more, at every outcome of at_child's probe and search; C's node with AT_PROBE, one more and 256 children;
a root with 256 children and an entry that stands four times in the list; row starts at both ends of a tile, runs of empty rows, the three row
cuts; every alignment of the data; caps; more tiles than one block of the library's scan -- with 64 guard bytes around all
five outputs and every input verified unwritten; the kinds and routes through the C ABI against acx_wordpiece_host and the
definition; the Python methods with bytes, str (characters), sequences and tensors in HBM, torch as the consumer.

THE DEFINITION (wp.hpp; tests/wp_definition.py restates it in plain Python -- the dictionary against the current position, no
trie -- and every expected value comes from there, never from the library).  The patterns are the vocabulary; C the
continuation prefix; cls a class per byte value (WORD, SPACE, ALONE); M the word limit in bytes.  Every ALONE byte is a word,
every maximal run of WORD bytes inside a row is a word.  A word longer than M is ONE piece (unk_id, ws, we); else the first
piece is the entry the match kind prefers among those that stand at ws and end inside the word, the following ones among the
entries C + x with x standing at p; a step without a candidate makes the WHOLE word one unknown piece.  The sizes are read
from the kernel's header."""
import gc
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import wp_definition as wpd

pytestmark = pytest.mark.gpu
capi = pytest.importorskip("ahocorasick_rs_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ahocorasick_rs_amd", "csrc")

STD, LF, LL = capi.MATCH_STANDARD, capi.MATCH_LEFTMOST_FIRST, capi.MATCH_LEFTMOST_LONGEST
KINDS = (STD, LF, LL)
PY_KINDS = ("Standard", "LeftmostFirst", "LeftmostLongest")
GUARD = 0xC3
NAMES = ("id", "start", "end", "first", "row_offsets")


def hip_constants(path, names):
    src = open(os.path.join(CSRC, path)).read()
    out = {}
    for n in names:
        m = re.search(r"\b%s\s*=\s*(\d+)\s*[,;]" % n, src)
        assert m, f"{n} is no longer a plain constant of {path}"
        out[n] = int(m.group(1))
    return out


_C = hip_constants("wp.hpp", ("WP_THREADS", "WP_TILE", "WP_MAX_WORD"))
THREADS, TILE, MAX_WORD = _C["WP_THREADS"], _C["WP_TILE"], _C["WP_MAX_WORD"]
_S = hip_constants("replace.hip", ("RS_THREADS", "RS_PER"))
SCAN_ITEMS = _S["RS_THREADS"] * _S["RS_PER"]  # the tile counts one workgroup of replace_scan takes

CLS = wpd.classes(b" \n", b",")
VOCAB = [b"a", b"##a", b"ab", b"##b", b"abc", b"##ca", b"b", b"##ab", b",", b"c", b"##bc", b"ba", b"##", b"##cab"]


def test_constants_are_what_the_sizes_below_assume():
    assert TILE % THREADS == 0 and THREADS % 64 == 0 and TILE // THREADS == 16 and 256 <= MAX_WORD < TILE
    assert SCAN_ITEMS * TILE <= 1 << 24 and MAX_WORD == capi.WP_MAX_WORD


def text(n, seed, space=0.2):
    """n bytes: words over "abc" with a "d" now and then (no entry has one), commas, spaces and newlines"""
    rng = np.random.default_rng(seed)
    a = rng.choice(list(b"aaabbbccd"), size=n).astype(np.uint8)
    r = rng.random(n)
    a[r < space] = 32
    a[r < space / 8] = 10
    a[(r > 0.97)] = 44
    return a.tobytes()


def same(got, want, what):
    for g, w, name in zip(got, want, NAMES):
        assert g.dtype == w.dtype and len(g) == len(w), (what, name, len(g), len(w))
        bad = np.flatnonzero(g != w)
        assert not len(bad), (what, name, int(bad[0]), g[bad[:8]], w[bad[:8]])


# ---------------------------------------------------------------------------
# the raw form: acx_wordpiece_into_device with guards
# ---------------------------------------------------------------------------
def run_raw(a, hay, cls, cap, *, prefix=b"##", M=100, unk=-1, offsets=None, uniform=0, base_res=0):
    """hay at base_res modulo 16; the five outputs each between 64 guard bytes, sized for `cap` pieces -> (T, the five as they
    lie in memory behind the call); the guards and every input checked unwritten"""
    hay = np.frombuffer(bytes(hay), dtype=np.uint8)
    n = len(hay)
    rows = (len(offsets) - 1) if offsets is not None else (n // uniform if uniform else 1)
    img_h = np.full(n + 48, GUARD, dtype=np.uint8)
    img_h[base_res:base_res + n] = hay
    d_hay = capi.DeviceBuffer(len(img_h)).upload(img_h)
    assert d_hay.ptr % 16 == 0
    sizes = (8 * cap, 8 * cap, 8 * cap, cap, 8 * (rows + 1))
    imgs = [np.full(64 + k + 64, GUARD, dtype=np.uint8) for k in sizes]
    bufs = [capi.DeviceBuffer(len(img) + 16).upload(img) for img in imgs]
    d_off = None
    if offsets is not None:
        off = np.ascontiguousarray(np.asarray(offsets, dtype=np.uint64))
        d_off = capi.DeviceBuffer(8 * len(off)).upload(off)
    try:
        T = a.wordpiece_into_device(d_hay.ptr + base_res, n, cls, cap, *[b.ptr + 64 for b in bufs], prefix=prefix, max_word=M,
                                    unk_id=unk, d_offsets=d_off.ptr if d_off else 0, n_hay=rows if (d_off or uniform) else 0,
                                    uniform_len=uniform)
        got = [b.download(len(img)) for b, img in zip(bufs, imgs)]
        assert np.array_equal(d_hay.download(len(img_h)), img_h), "the data (or a byte around it) was written"
        if d_off:
            assert np.array_equal(d_off.download(8 * len(off)).view(np.uint64), off), "the offsets were written"
    finally:
        for b in [d_hay, d_off] + bufs:
            if b:
                b.free()
    return T, got, sizes


def check_raw(patterns, kind, hay, cls=CLS, *, prefix=b"##", M=100, unk=-1, offsets=None, uniform=0, fold=False, what=None,
              automaton=None, base_res=0, want=None):
    """want: the expected columns when they are not the definition's (the host form's)"""
    cut = offsets if offsets is not None else (np.arange(0, len(hay) + 1, uniform) if uniform else None)
    if want is None:
        want = wpd.definition(patterns, hay, kind, cls, prefix=prefix, M=M, unk=unk, offsets=cut, fold=fold)
    a = automaton or capi.Automaton(patterns, kind, ascii_case_insensitive=fold)
    try:
        cap = max(len(want[0]), 1)  # (cap 0 is the count pass alone)
        T, got, sizes = run_raw(a, hay, cls, cap, prefix=prefix, M=M, unk=unk, offsets=offsets, uniform=uniform, base_res=base_res)
    finally:
        if not automaton:
            a.close()
    assert T == len(want[0]), (what, T, len(want[0]))
    out = []
    for g, k, name, w in zip(got, sizes, NAMES, want):
        assert (g[:64] == GUARD).all(), ("a byte before the output was written", what, name)
        assert (g[64 + k:] == GUARD).all(), ("a byte behind the output was written", what, name)
        used = w.nbytes  # exactly T, T, T, T and rows + 1 entries are written
        assert (g[64 + used:64 + k] == GUARD).all(), ("an entry at or behind T was written", what, name)
        out.append(g[64:64 + used].copy().view(w.dtype))
    same(out, want, what)
    return want


def pieces(want):
    return [(int(i), int(s), int(e), int(f)) for i, s, e, f in zip(*want[:4])]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [0, 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
def test_raw_data_lengths_around_the_tile(kind, n):
    check_raw(VOCAB, kind, text(n, n), what=n)
    check_raw(VOCAB, kind, text(n, n + 1, space=0.0), what=(n, "dense"))


def planted(n, words, fill=b" "):
    hay = bytearray(fill * n)
    for p, w in words:
        hay[p:p + len(w)] = w
    assert len(hay) == n
    return bytes(hay)


@pytest.mark.parametrize("kind", KINDS)
def test_raw_words_at_a_tile_boundary(kind):
    n = 2 * TILE + 50
    # a word that starts on the last byte of a tile (and one on the last byte of the data)
    want = check_raw(VOCAB, kind, planted(n, [(TILE - 1, b"abcab"), (2 * TILE - 1, b"a"), (n - 1, b"b")]), what="last byte")
    assert {TILE - 1, 2 * TILE - 1, n - 1} <= set(want[1][want[3] == 1].tolist())
    # a word that ends exactly on a tile's end; the next tile's first byte follows a separator and starts a word
    want = check_raw(VOCAB, kind, planted(n, [(TILE - 3, b"abc"), (2 * TILE - 3, b"ab"), (2 * TILE, b"ab")]), what="ends on the end")
    assert TILE in want[2].tolist() and 2 * TILE in want[1][want[3] == 1].tolist()
    # a tile whose first byte continues a word from the previous tile: no word start there
    want = check_raw(VOCAB, kind, planted(n, [(TILE - 2, b"abcab"), (2 * TILE - 1, b"ab,")]), what="continues")
    firsts = want[1][want[3] == 1].tolist()
    assert TILE not in firsts and 2 * TILE not in firsts and TILE - 2 in firsts and 2 * TILE + 1 in firsts
    # ... and one that follows an isolated byte, which is the tile's last
    check_raw(VOCAB, kind, planted(n, [(TILE - 1, b",ab"), (2 * TILE - 2, b"a,,b")]), what="isolated")
    # an unknown word across the boundary: the failed step lies in the next tile
    want = check_raw(VOCAB, kind, planted(n, [(TILE - 2, b"abd"), (2 * TILE - 1, b"da")]), what="fails behind the boundary")
    assert (-1, TILE - 2, TILE + 1, 1) in pieces(want)


@pytest.mark.parametrize("kind", KINDS)
def test_raw_words_longer_than_a_tile_end_at_the_carry(kind):
    n = 3 * TILE + 64
    # across two tile boundaries: the tile between has no word and no boundary
    want = check_raw(VOCAB, kind, planted(n, [(TILE - 5, b"a" * (TILE + 12)), (3 * TILE, b"ab")]), what="separator")
    assert (-1, TILE - 5, 2 * TILE + 7, 1) in pieces(want)
    # the same word ended by a row start instead of a separator, by each of the cuts
    hay = planted(n, [(TILE - 5, b"a" * (n - TILE + 5))])
    want = check_raw(VOCAB, kind, hay, offsets=[0, 2 * TILE + 7, n], what="row start")
    assert pieces(want) == [(-1, TILE - 5, 2 * TILE + 7, 1), (-1, 2 * TILE + 7, n, 1)]
    want = check_raw(VOCAB, kind, hay, offsets=[0, 2 * TILE, 2 * TILE, n], what="row start on a tile")
    assert pieces(want) == [(-1, TILE - 5, 2 * TILE, 1), (-1, 2 * TILE, n, 1)]
    want = check_raw(VOCAB, kind, hay[:3 * TILE], uniform=3 * TILE // 2, what="row length")
    assert pieces(want) == [(-1, TILE - 5, 3 * TILE // 2, 1), (-1, 3 * TILE // 2, 3 * TILE, 1)]
    want = check_raw(VOCAB, kind, hay, what="the data's end")
    assert pieces(want) == [(-1, TILE - 5, n, 1)]


@pytest.mark.parametrize("kind", KINDS)
def test_raw_word_density(kind):
    # a tile with no word between two that have one
    check_raw(VOCAB, kind, planted(3 * TILE, [(7, b"ab"), (2 * TILE + 9, b"abc")]), what="no word")
    check_raw(VOCAB, kind, b" " * (2 * TILE + 3), what="no word at all")
    # a word per byte: a tile of isolated bytes, known and unknown
    want = check_raw(VOCAB, kind, b"," * TILE + b"ab", what="a word per byte")
    assert len(want[0]) >= TILE + 1 and np.all(want[3][:TILE] == 1)
    check_raw(VOCAB, kind, b";" * (TILE + 5), wpd.classes(b" ", b",;"), what="a word per byte, unknown")
    # a word per wave
    check_raw(VOCAB, kind, planted(2 * TILE, [(w * 16 * 64 + 3, b"abcab") for w in range(2 * TILE // (16 * 64))]), what="a word per wave")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("M", [1, 7, 100, MAX_WORD])
def test_raw_words_of_m_and_m_plus_one_bytes(kind, M):
    vocab = [b"a", b"##a", b"a" * (M + 5), b"##" + b"a" * (M + 5), b"##aa"]  # two patterns longer than M
    n = 4 * TILE
    words = [(3, b"a" * M), (TILE // 2, b"a" * (M + 1)),
             (TILE - 10, b"a" * M), (2 * TILE - 10, b"a" * (M + 1)),        # across a boundary: the scan decides
             (3 * TILE - M, b"a" * M), (4 * TILE - M - 1, b"a" * (M + 1))]  # they end on a tile's end and on the data's
    want = check_raw(vocab, kind, planted(n, words), M=M, unk=-9, what=M)
    got = pieces(want)
    for p, w in words:
        one = [x for x in got if x[1] == p and x[3] == 1]
        assert len(one) == 1 and (one[0][0] == -9) == (len(w) > M), (p, len(w), one)


PROBE = hip_constants("at.hpp", ("AT_PROBE",))["AT_PROBE"]  # children up to which at_child probes a node linearly


def deep_node(m, head):
    """entries that put a node with exactly m children at depth len(head) -- child bytes 0x30, 0x34, .. -- and behind every
    child a short and a long entry, in either index order: the three kinds pick differently, and all of them search the node"""
    pats = []
    for k in range(m):
        c = head + bytes([0x30 + 4 * k])
        pats += [c + b"xy", c] if k % 2 else [c, c + b"xy"]
    return pats


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("m", [PROBE, PROBE + 1])
def test_raw_a_node_at_depth_2_with_probe_and_one_more_children(kind, m):
    """at_child below depth 1 inside k_wp, on the first piece's walk (the node of "qw") and on a continuation's (the node of
    "##qw", two levels below C's): the linear probe at AT_PROBE children, the binary search at one more, at the first, a middle
    and the last child, below, between and above them; one word reads the node's byte from the last byte of a tile, one from the
    next tile"""
    vocab = deep_node(m, b"qw") + [b"a", b"##xy"] + deep_node(m, b"##qw")
    child = [0x30 + 4 * k for k in range(m)]
    hits, misses = [child[0], child[m // 2], child[-1]], [child[0] - 1, child[1] + 1, child[-1] + 1]
    words = [(3 + 16 * k, b"qw" + bytes([b]) + b"xy") for k, b in enumerate(hits + misses)]
    words += [(11 + 16 * k, b"aqw" + bytes([b]) + b"xy") for k, b in enumerate(hits + misses)]
    words += [(TILE - 3, b"qw" + bytes([hits[2]]) + b"xy"), (2 * TILE - 2, b"qw" + bytes([hits[1]]) + b"xy"),
              (3 * TILE - 4, b"aqw" + bytes([hits[0]]) + b"xy"), (4 * TILE - 3, b"aqw" + bytes([hits[2]]) + b"xy")]
    want = check_raw(vocab, kind, planted(4 * TILE + 40, words), what=m)
    got = pieces(want)
    n = 2 * m  # (the entries of "qw": 0 .. 2m - 1; "a", "##xy"; those of "##qw" from 2m + 2)
    for k, b in enumerate(hits):
        c = (b - 0x30) // 4
        short, long_ = (2 * c + 1, 2 * c) if c % 2 else (2 * c, 2 * c + 1)
        whole = [(long_, 0, 5)] if kind == LL or (kind == LF and long_ < short) else [(short, 0, 3), (n + 1, 3, 5)]
        p = 3 + 16 * k
        assert [x for x in got if p <= x[1] < p + 5] == [(i, p + s, p + e, int(s == 0)) for i, s, e in whole], (m, k)
        p = 11 + 16 * k
        assert [x for x in got if p <= x[1] < p + 6] == [(n, p, p + 1, 1)] + [(i + n + 2 if i < n else i, p + 1 + s, p + 1 + e, 0) for i, s, e in whole], (m, k)
    for k in range(3, 6):
        assert (-1, 3 + 16 * k, 8 + 16 * k, 1) in got and (-1, 11 + 16 * k, 17 + 16 * k, 1) in got, (m, k)
    assert not any(x[0] == -1 and x[1] > TILE - 8 for x in got) and sum(x[3] for x in got) == 16


def fan_of(prefix, children):
    return [prefix + bytes([b]) for b in children]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("m", [PROBE, PROBE + 1, 256])
def test_raw_the_node_of_the_prefix_with_probe_one_more_and_256_children(kind, m):
    """cont_next is filled by 256 at_child calls on C's node: a vocabulary with C + b for m byte values b -- every byte value
    whose class is WORD among them when m == 256 -- and a word whose every continuation byte takes a different child"""
    word_bytes = [b for b in range(256) if CLS[b] == wpd.WORD]
    children = list(range(256)) if m == 256 else [0x31 + 5 * k for k in range(m)]
    assert set(children) <= set(word_bytes) or m == 256
    vocab = [b"a", b"##"] + fan_of(b"##", children)
    inside = [b for b in children if CLS[b] == wpd.WORD]
    every = b"a" + bytes(inside)                      # every continuation byte takes a different child
    back = b"a" + bytes(inside[::-1])
    edges = [b"a" + bytes([inside[0], inside[len(inside) // 2], inside[-1]])]
    misses = [] if m == 256 else [b"a" + bytes([children[0] - 1]), b"a" + bytes([children[1] + 1]), b"a" + bytes([children[-1] + 1]),
                                  b"a" + bytes([children[0], children[-1] + 1])]
    words, p = [], 5
    for w in [every, back] + edges + misses + [b"##", b"a##"]:
        words.append((p, w))
        p += len(w) + 2
    words += [(TILE - 2, edges[0]), (2 * TILE - 1, edges[0])]
    want = check_raw(vocab, kind, planted(2 * TILE + 30, words), M=MAX_WORD, what=m)
    got = pieces(want)
    assert [x[0] for x in got if 5 <= x[1] < 5 + len(every)] == [0] + [2 + children.index(b) for b in inside], m
    assert sum(x[0] == -1 for x in got) == len(misses) + (m != 256) and (1, words[-4][0], words[-4][0] + 2, 1) in got, m
    a3 = words[-3][0]  # "a##": "a", then C + "#" twice -- when "#" is a child of C's node
    assert [x for x in got if a3 <= x[1] < a3 + 3] == ([(0, a3, a3 + 1, 1), (2 + 35, a3 + 1, a3 + 2, 0), (2 + 35, a3 + 2, a3 + 3, 0)] if m == 256
                                                       else [(-1, a3, a3 + 3, 1)])


@pytest.mark.parametrize("kind", KINDS)
def test_raw_a_root_with_256_children_and_an_entry_four_times(kind):
    """every first byte of a word has a depth-1 state; "dup" and "##dup" stand four times each in the vocabulary (own1 says
    "many": the first of the state's list is read) behind an extension of each with a lower index: the lowest of the four comes
    back under every kind"""
    fan = [bytes([b]) + b"z" for b in range(256)]
    vocab = fan[:100] + [b"dup!", b"##dup!"] + fan[100:200] + [b"dup", b"##dup", b"dup", b"##dup"] + fan[200:] + [b"dup", b"##dup", b"dup", b"##dup"]
    assert vocab.count(b"dup") == 4 == vocab.count(b"##dup") and len({v[0] for v in vocab}) == 256
    cls = wpd.classes(b" \n")
    low, low_c = vocab.index(b"dup"), vocab.index(b"##dup")
    words = [(3, b"dup"), (8, b"dupdup"), (16, b"dup!dup!"), (26, b"dupdupdup"), (40, b"\x00z"), (44, b"\xffz"), (48, b"\x80z\x7fz"),
             (TILE - 2, b"dupdup"), (2 * TILE - 4, b"dupdup")]
    want = check_raw(vocab, kind, planted(2 * TILE + 20, words), cls, what="256 children")
    got = pieces(want)
    assert [x for x in got if 3 <= x[1] < 14] == [(low, 3, 6, 1), (low, 8, 11, 1), (low_c, 11, 14, 0)]
    assert [x[0] for x in got if 26 <= x[1] < 35] == [low, low_c, low_c]
    assert [x for x in got if x[1] >= TILE - 2] == [(low, TILE - 2, TILE + 1, 1), (low_c, TILE + 1, TILE + 4, 0),
                                                   (low, 2 * TILE - 4, 2 * TILE - 1, 1), (low_c, 2 * TILE - 1, 2 * TILE + 2, 0)]
    # "dup!dup!": Standard stops at "dup" and has no "##!" to go on with; the others take the extension, whose index is lower
    assert [x[0] for x in got if 16 <= x[1] < 24] == ([-1] if kind == STD else [vocab.index(b"dup!"), vocab.index(b"##dup!")])
    assert (0, 40, 42, 1) in got and (vocab.index(b"\xffz"), 44, 46, 1) in got and (-1, 48, 52, 1) in got


@pytest.mark.parametrize("kind", KINDS)
def test_raw_row_starts_and_empty_rows(kind):
    n = 2 * TILE + 100
    dense = text(n, 5, space=0.02)
    # row starts at both ends of a tile
    check_raw(VOCAB, kind, dense, offsets=[0, 1, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, n], what="both ends")
    # runs of empty rows across a boundary and at the end of the data
    check_raw(VOCAB, kind, dense, offsets=[0, 0, 5, TILE, TILE, TILE, TILE + 3, n, n, n], what="empty rows")
    check_raw(VOCAB, kind, dense, offsets=[0, TILE - 1, TILE - 1, TILE + 1, TILE + 1, n], what="empty rows beside a boundary")
    # the three cuts
    cuts = np.sort(np.random.default_rng(9).integers(0, n + 1, size=300))
    check_raw(VOCAB, kind, dense, offsets=np.concatenate([[0], cuts, [n]]), what="offsets")
    for u in (1, 3, 64, TILE, 2 * TILE + 100):
        m = n // u * u
        check_raw(VOCAB, kind, dense[:m], uniform=u, what=("row length", u))
    check_raw(VOCAB, kind, dense, what="neither")


@pytest.mark.parametrize("u", [1, 16, TILE - 1, TILE, TILE + 1, 2 * TILE])
def test_raw_rows_of_one_length_that_begin_on_before_and_behind_a_tile_boundary(u):
    """Exactly u * n bytes, n the smallest number of rows that gives more than two tiles (3 for the three lengths around the
    tile): row starts fall on a tile's first byte, one byte before it and one byte behind it -- the marks of k_wp include the
    one ON the first byte.  Dense words over the vocabulary's letters with a "d" now and then, which no entry begins with, so
    that the row starts cut words; against acx_wordpiece_host over the same cut written as offsets, entry for entry."""
    n = {1: 2 * TILE + 1, 16: 2 * TILE // 16 + 1, 2 * TILE: 2}.get(u, 3)
    assert u * n > 2 * TILE
    hay = text(u * n, u, space=0.02)
    h = capi.HostAutomaton(VOCAB, LL, 0)
    try:
        want = capi.wordpiece_host(h, hay, CLS, offsets=np.arange(n + 1, dtype=np.uint64) * u, match_kind=LL, prefix=b"##",
                                   max_word=100, unk_id=-1)
    finally:
        h.close()
    assert len(want[4]) == n + 1 and (want[0] == -1).any() and (want[0] >= 0).any()
    check_raw(VOCAB, LL, hay, uniform=u, what=("row length", u), want=want)


def test_raw_every_alignment_of_the_data():
    hay = text(TILE + 37, 3)
    a = capi.Automaton(VOCAB, LL)
    try:
        for r in range(16):
            check_raw(VOCAB, LL, hay[r:], automaton=a, base_res=r, what=("alignment", r))
            check_raw(VOCAB, LL, hay[:17 + r], automaton=a, base_res=15 - r, what=("short", r))
    finally:
        a.close()


def test_raw_caps():
    hay = text(TILE + 100, 12)
    want = wpd.definition(VOCAB, hay, LL, CLS)
    T0 = len(want[0])
    a = capi.Automaton(VOCAB, LL)
    try:
        for cap in (T0 - 1, 1):  # a cap below T writes nothing and reports T
            T, got, sizes = run_raw(a, hay, CLS, cap)
            assert T == T0 and all((g == GUARD).all() for g in got), cap
        T, got, sizes = run_raw(a, hay, CLS, T0 + 3)  # room to spare: exactly T entries are written
        assert T == T0 and all((g[64 + w.nbytes:] == GUARD).all() for g, w in zip(got, want))
        # cap 0: the count pass alone, nothing to write to
        assert a.wordpiece_into_device(0, 0, CLS, 0, 0, 0, 0, 0, 0) == 0
        d = capi.DeviceBuffer(len(hay)).upload(np.frombuffer(hay, dtype=np.uint8))
        try:
            assert a.wordpiece_into_device(d.ptr, len(hay), CLS, 0, 0, 0, 0, 0, 0) == T0
        finally:
            d.free()
    finally:
        a.close()


def test_raw_more_tiles_than_one_block_of_the_scan():
    """SCAN_ITEMS + 4 tiles, mostly separators: a few words per 64 KiB, words at tile boundaries behind the scan's first block,
    and one word longer than a tile there"""
    n = (SCAN_ITEMS + 3) * TILE + 1
    words = [(int(p), (b"abcab", b"ab,", b"abd", b"a" * 120)[k % 4]) for k, p in enumerate(range(100, n - 200, 50_021))]
    words += [(SCAN_ITEMS * TILE - 2, b"abcab"), ((SCAN_ITEMS + 1) * TILE - 7, b"ab" * (TILE // 2 + 9)), (n - 1, b"a")]
    hay = planted(n, words)
    want = check_raw(VOCAB, LL, hay, what="big")
    assert (-1, (SCAN_ITEMS + 1) * TILE - 7, (SCAN_ITEMS + 2) * TILE + 11, 1) in pieces(want) and pieces(want)[-1] == (0, n - 1, n, 1)
    check_raw(VOCAB, LL, hay[:SCAN_ITEMS * TILE + TILE], uniform=(SCAN_ITEMS + 1) * TILE // 4, what="big, rows")


# ---------------------------------------------------------------------------
# handles and routes through the C ABI
# ---------------------------------------------------------------------------
def device_call(a, hay, cls, kw, offsets=None, uniform=0):
    hay = np.frombuffer(bytes(hay), dtype=np.uint8)
    d_hay = capi.DeviceBuffer(len(hay) + 16)
    if len(hay):
        d_hay.upload(hay)
    d_off, rows = None, 0
    if offsets is not None:
        off = np.ascontiguousarray(np.asarray(offsets, dtype=np.uint64))
        d_off = capi.DeviceBuffer(8 * len(off)).upload(off)
        rows = len(off) - 1
    elif uniform:
        rows = len(hay) // uniform
    try:
        r = a.wordpiece_device(d_hay.ptr, len(hay), cls, d_offsets=d_off.ptr if d_off else 0, n_hay=rows, uniform_len=uniform, **kw)
        try:
            assert r.on_device and r.id_ptr() and r.start_ptr() and r.end_ptr() and r.first_ptr() and r.row_offsets_ptr()
            out = (r.id(), r.start(), r.end(), r.first(), r.row_offsets())
            assert r.count == len(out[0]) and r.rows == len(out[4]) - 1
            assert np.array_equal(d_hay.download(len(hay)), hay), "the data was written"
        finally:
            r.free()
    finally:
        for b in (d_hay, d_off):
            if b:
                b.free()
    return out


def host_call(a, hay, cls, kw, offsets=None, codepoints=False):
    if offsets is None:
        r = a.wordpiece(None, cls, codepoints=codepoints, single=bytes(hay), **kw)
    else:
        r = a.wordpiece([bytes(hay[int(offsets[i]):int(offsets[i + 1])]) for i in range(len(offsets) - 1)], cls, codepoints=codepoints, **kw)
    try:
        assert not r.on_device
        return r.id(), r.start(), r.end(), r.first(), r.row_offsets()
    finally:
        r.free()


def check_abi(patterns, kind, hay, cls=CLS, *, prefix=b"##", M=100, unk=-1, offsets=None, fold=False, what=None):
    want = wpd.definition(patterns, hay, kind, cls, prefix=prefix, M=M, unk=unk, offsets=offsets, fold=fold)
    kw = dict(prefix=prefix, max_word=M, unk_id=unk)
    a = capi.Automaton(patterns, kind, ascii_case_insensitive=fold)
    try:
        legs = [("device", device_call(a, hay, cls, kw, offsets)), ("host", host_call(a, hay, cls, kw, offsets))]
    finally:
        a.close()
    h = capi.HostAutomaton(patterns, kind, capi.BUILD_ASCII_CASE_INSENSITIVE if fold else 0)
    try:
        legs.append(("acx_wordpiece_host", capi.wordpiece_host(h, hay, cls, offsets=offsets, match_kind=kind, **kw)))
    finally:
        h.close()
    for leg, got in legs:
        same(got, want, (what, leg))
    return want


@pytest.mark.parametrize("fold", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_abi_kinds_and_fold_host_and_device_inputs(kind, fold):
    hay = text(TILE + 700, 21)
    vocab = VOCAB + [b"a", b"##b"]  # copies: the lowest index is reported
    if fold:
        a = np.frombuffer(hay, dtype=np.uint8).copy()
        up = (np.random.default_rng(2).random(len(a)) < 0.4) & (a >= 97)
        a[up] -= 32
        hay = a.tobytes()
        vocab = [v.upper() if k % 2 else v for k, v in enumerate(vocab)]
    cuts = np.sort(np.random.default_rng(3).integers(0, len(hay) + 1, size=60))
    off = np.concatenate([[0], cuts, [len(hay)]])
    check_abi(vocab, kind, hay, fold=fold, what="one haystack")
    check_abi(vocab, kind, hay, offsets=off, fold=fold, M=9, unk=77, what="rows")
    check_abi(vocab, kind, hay, prefix=b"", fold=fold, what="an empty prefix")
    check_abi(vocab, kind, hay, prefix=b"@@", fold=fold, what="a prefix that is not in the trie")
    check_abi(vocab, kind, b"", fold=fold, what="no data")
    check_abi(vocab, kind, b"", offsets=[0, 0, 0], fold=fold, what="empty rows only")
    check_abi(vocab, kind, b"  \n ", offsets=[0, 2, 4], fold=fold, what="no word")


def test_abi_codepoints_and_refusals():
    text_ = "übergrößenträger, 日本語のテキスト ok"
    pats = ["über".encode(), "##größen".encode(), "##träger".encode(), b",", "日本語".encode(), "##のテキスト".encode(), b"ok"]
    cls = wpd.classes(wpd.WHITESPACE, wpd.PUNCTUATION)
    a = capi.Automaton(pats, LL)
    try:
        ids, start, end, first, ro = host_call(a, text_.encode(), cls, {}, codepoints=True)
        want = wpd.definition(pats, text_.encode(), LL, cls)
        chars = lambda col: [len(text_.encode()[:b].decode()) for b in col]
        assert list(ids) == list(want[0]) == [0, 1, 2, 3, 4, 5, 6] and list(start) == chars(want[1]) and list(end) == chars(want[2])

        def code(fn):
            with pytest.raises(ValueError) as e:
                fn()
            return e.value.code

        bad = cls.copy()
        bad[0] = 3
        assert code(lambda: a.wordpiece(None, bad, single=b"ab")) == capi.EINVAL
        assert code(lambda: a.wordpiece_device(0, 0, bad)) == capi.EINVAL
        assert code(lambda: a.wordpiece(None, cls, max_word=0, single=b"ab")) == capi.EINVAL
        assert code(lambda: a.wordpiece_device(0, 0, cls, max_word=MAX_WORD + 1)) == capi.EINVAL
        assert code(lambda: a.wordpiece_device(0, 5, cls)) == capi.EINVAL  # bytes and nowhere to read them
        L = capi.lib()
        off = np.asarray([0, 2, 1, 3], dtype=np.uint64)
        hay = np.frombuffer(b"abc", dtype=np.uint8)
        out = capi.ctypes.c_void_p()
        tail = (cls.ctypes.data, None, 0, 100, -1)
        assert L.acx_wordpiece(a._h, hay.ctypes.data, 3, off.ctypes.data, 3, *tail, 0, 0, capi.ctypes.byref(out)) == capi.EINVAL
        assert L.acx_wordpiece(a._h, hay.ctypes.data, 3, None, 0, *tail, 4, 0, capi.ctypes.byref(out)) == capi.EINVAL  # a flag
        assert L.acx_wordpiece(a._h, hay.ctypes.data, 3, None, 0, *tail, 0, 0, None) == capi.EINVAL
        one = np.zeros(4, dtype=np.int64)
        assert L.acx_wp_copy(None, 0, one.ctypes.data) == capi.EINVAL and L.acx_wp_count(None) == 0
        r = a.wordpiece(None, cls, single=b"ok ok")
        assert L.acx_wp_copy(r._h, 5, one.ctypes.data) == capi.EINVAL
        assert r.count == 2 and r.rows == 1 and list(r.start()) == [0, 3] and list(r.row_offsets()) == [0, 2]
        r.free()
    finally:
        a.close()


@pytest.mark.parametrize("seed", range(8))
def test_seeded_slice_of_the_fuzz(seed):
    case = wpd.fuzz_case(seed, size=TILE + 300)
    kw = dict(prefix=case["prefix"], M=case["M"], offsets=case["offsets"], fold=case["fold"])
    want = check_raw(case["patterns"], case["kind"], case["hay"], case["cls"], what=seed, **kw)
    assert wpd.fuzz_shows_all_three(case, want) == (True, True, True), seed
    check_abi(case["patterns"], case["kind"], case["hay"], case["cls"], what=seed, **kw)


# ---------------------------------------------------------------------------
# the Python methods
# ---------------------------------------------------------------------------
def quads(want, off=None, chars=None):
    """what tolist() gives: (id, start, end, first) local to the row, one list per row when there are rows"""
    ids, start, end, first, ro = want
    pos = (lambda b: int(b)) if chars is None else (lambda b: chars[int(b)])
    begins = [0] if off is None else [pos(b) for b in off]
    rows = [[(int(ids[k]), pos(start[k]) - begins[r], pos(end[k]) - begins[r], int(first[k])) for k in range(ro[r], ro[r + 1])]
            for r in range(len(ro) - 1)]
    return rows if off is not None else rows[0]


def test_python_bytes_and_sequences():
    import ahocorasick_rs as ar
    hay = text(TILE + 333, 8)
    for k, kind in enumerate(KINDS):
        b = ar.BytesAhoCorasick(VOCAB, matchkind=getattr(ar.MatchKind, PY_KINDS[k]))
        want = wpd.definition(VOCAB, hay, kind, CLS)
        s = b.wordpiece(hay, separators=b" \n", isolated=b",")
        assert isinstance(s, ar.WordPieces) and len(s) == len(want[0]) and s.row_offsets is None and s.device is None
        assert s.tolist() == quads(want)
        for col, w in zip((s.id, s.start, s.end, s.first), want):
            got = np.from_dlpack(col)
            assert got.dtype == w.dtype and np.array_equal(got, w)
        # first against the word starts
        raw = np.frombuffer(hay, dtype=np.uint8)
        c = CLS[raw]
        starts = np.flatnonzero((c != wpd.SPACE) & ((c == wpd.ALONE) | (np.concatenate([[wpd.SPACE], c[:-1]]) != wpd.WORD)))
        assert np.array_equal(np.from_dlpack(s.start)[np.from_dlpack(s.first) == 1], starts)
        assert s.tolist() == b.wordpiece(bytearray(hay), separators=b" \n", isolated=b",").tolist()
        # the defaults: whitespace separates, nothing is isolated, M = 100, unk_id = -1
        assert b.wordpiece(hay).tolist() == quads(wpd.definition(VOCAB, hay, kind, wpd.classes()))
        rows = [hay[:10], b"", hay[10:TILE + 1], b"", b"", hay[TILE + 1:], b""]
        off = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
        want = wpd.definition(VOCAB, hay, kind, CLS, M=5, unk=99, offsets=off)
        s = b.wordpiece_batch(rows, separators=b" \n", isolated=b",", max_word_bytes=5, unk_id=99)
        assert len(s) == len(want[0]) and s.tolist() == quads(want, off)
        assert np.array_equal(np.from_dlpack(s.row_offsets), want[4]) and np.array_equal(np.from_dlpack(s.start), want[1])
        assert b.wordpiece_batch([]).tolist() == [] and b.wordpiece(b"").tolist() == [] and b.wordpiece_batch([b"", b" "]).tolist() == [[], []]
        host = np.frombuffer(hay[:4096], dtype=np.uint8).copy()
        want = wpd.definition(VOCAB, hay[:4096], kind, wpd.classes(), offsets=np.arange(0, 4097, 64))
        assert b.wordpiece_batch(host, row_length=64).tolist() == quads(want, np.arange(0, 4097, 64))
    bert = ar.BytesAhoCorasick([b"[UNK]", b"fox", b"##es", b",", b"jump", b"##ed"], matchkind=ar.MatchKind.LeftmostLongest)
    got = bert.wordpiece(b"foxes, jumped over", isolated=ar.ASCII_PUNCTUATION, unk_id=0).tolist()
    assert got == [(1, 0, 3, 1), (2, 3, 5, 0), (3, 5, 6, 1), (4, 7, 11, 1), (5, 11, 13, 0), (0, 14, 18, 1)]


def test_python_str_in_characters_with_multi_byte_text():
    import ahocorasick_rs as ar
    words = ["über", "##größen", "##träger", "日本", "##語", "ok", "un", "##able", ",", "##ö"]
    text_ = "übergrößenträger, 日本語 ok unable nö"
    raw = text_.encode()
    chars = {b: len(raw[:b].decode()) for b in range(len(raw) + 1) if b == len(raw) or (raw[b] & 0xC0) != 0x80}
    for k, kind in enumerate(KINDS):
        a = ar.AhoCorasick(words, matchkind=getattr(ar.MatchKind, PY_KINDS[k]))
        want = wpd.definition([w.encode() for w in words], raw, kind, wpd.classes(wpd.WHITESPACE, b","))
        s = a.wordpiece(text_, isolated=",")
        assert s.tolist() == quads(want, chars=chars)
        assert s.tolist() == a.wordpiece(text_, continuation_prefix=b"##", separators=wpd.WHITESPACE, isolated=b",").tolist()
        rows = [text_, "", "日本語ok", "nö"]
        got = a.wordpiece_batch(rows, isolated=",").tolist()
        assert got == [a.wordpiece(r, isolated=",").tolist() for r in rows]
        assert a.wordpiece("plain ok").tolist()[-1] == (5, 6, 8, 1)


def test_python_errors():
    import ahocorasick_rs as ar
    a = ar.AhoCorasick(["ab"], matchkind=ar.MatchKind.LeftmostLongest)
    b = ar.BytesAhoCorasick([b"ab"], matchkind=ar.MatchKind.LeftmostLongest)
    for ac, hay in ((a, "abc"), (b, b"abc")):
        for bad in (True, 1.0, "7", None.__class__):
            with pytest.raises(TypeError):
                ac.wordpiece(hay, max_word_bytes=bad)
            with pytest.raises(TypeError):
                ac.wordpiece_batch([hay], unk_id=bad)
        for bad in (0, -3, MAX_WORD + 1, 2 ** 70):
            with pytest.raises(ValueError):
                ac.wordpiece(hay, max_word_bytes=bad)
        with pytest.raises(ValueError):
            ac.wordpiece(hay, unk_id=2 ** 63)
        with pytest.raises(ValueError):
            ac.wordpiece(hay, separators=b" ,", isolated=b",")
        with pytest.raises(TypeError):
            ac.wordpiece(hay, b"##")  # keyword-only
        with pytest.raises(TypeError):
            ac.wordpiece_batch([hay], offsets=[0, 3])  # offsets / row_length cut ONE tensor, not a sequence
        with pytest.raises(TypeError):
            ac.wordpiece()
    for name in ("continuation_prefix", "separators", "isolated"):
        with pytest.raises(TypeError):
            b.wordpiece(b"abc", **{name: "#"})
    with pytest.raises(ValueError):
        a.wordpiece("abc", separators="ä")
    with pytest.raises(ValueError):
        a.wordpiece("abc", isolated="„")
    with pytest.raises(TypeError):
        a.wordpiece(b"abc")
    with pytest.raises(TypeError):
        b.wordpiece("abc")
    host = np.frombuffer(b"abcabc", dtype=np.uint8).copy()
    with pytest.raises(TypeError):
        b.wordpiece_batch(host, offsets=np.asarray([0, 3, 6]), row_length=3)  # exactly one of the two
    with pytest.raises(ValueError):
        b.wordpiece_batch(host, row_length=4)
    with pytest.raises(ValueError):
        b.wordpiece_batch(host, offsets=np.asarray([0, 4, 3, 6]))
    assert b.wordpiece_batch(host, offsets=np.asarray([0, 2, 6])).tolist() == [[(0, 0, 2, 1)], [(-1, 0, 4, 1)]]
    with pytest.raises(TypeError):
        ar.WordPieces()


def test_python_host_columns_outlive_the_result_and_the_automaton():
    import ahocorasick_rs as ar
    hay = text(TILE + 400, 4)
    want = wpd.definition(VOCAB, hay, STD, wpd.classes())
    b = ar.BytesAhoCorasick(VOCAB)
    s = b.wordpiece(hay)
    cols = [np.from_dlpack(c) for c in (s.id, s.start, s.end, s.first)]
    del s, b
    gc.collect()
    other = ar.BytesAhoCorasick(VOCAB)
    for k in range(20):  # (other results come and go where the columns would be if they had been freed)
        other.wordpiece(text(TILE + 400, 50 + k))
    for c, w in zip(cols, want):
        assert np.array_equal(c, w)


_TENSOR_SCRIPT = r"""
import gc
import sys
import torch  # first: one process holds ONE HIP runtime, and torch must be the one to load it
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import numpy as np
import ahocorasick_rs as ar
import wp_definition as wpd
from test_gpu_wp import VOCAB, KINDS, PY_KINDS, TILE, text, quads

dev = "cuda:0"
CLS = wpd.classes(wpd.WHITESPACE, b",")
lines = [b"abc ab,cab", b"", b"abd a", b"a" * 130, b"ab", b"", b"", b"bca,", b" ", text(700, 3).replace(b"\n", b" ")] * 12
data = b"\n".join(lines) + b"\n"
assert len(data) > 2 * TILE
t = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to(dev)
ro = ar.split_rows(t)
off = torch.from_dlpack(ro.offsets)
off_np = off.cpu().numpy()
DT = (torch.int64, torch.int64, torch.int64, torch.uint8)

def same(s, want, where):
    cols = [torch.from_dlpack(c) for c in (s.id, s.start, s.end, s.first)]  # every column, without a copy
    for c, w, dt in zip(cols, want, DT):
        assert c.dtype == dt and c.is_contiguous() and c.device.type == "cuda", where
        assert torch.equal(c.cpu(), torch.from_numpy(w)), where
    assert s.device == 0 and len(s) == len(want[0]), where

for k, kind in enumerate(KINDS):
    b = ar.BytesAhoCorasick(VOCAB, matchkind=getattr(ar.MatchKind, PY_KINDS[k]))
    # one haystack: no rows
    s = b.wordpiece(t, isolated=b",")
    want = wpd.definition(VOCAB, data, kind, CLS)
    same(s, want, ("one", k))
    assert s.row_offsets is None and s.tolist() == quads(want)
    # first against the word starts
    c = torch.from_numpy(CLS)[t.cpu().long()]
    prev = torch.cat([torch.tensor([wpd.SPACE], dtype=c.dtype), c[:-1]])
    starts = torch.nonzero((c != wpd.SPACE) & ((c == wpd.ALONE) | (prev != wpd.WORD))).flatten()
    assert torch.equal(torch.from_dlpack(s.start)[torch.from_dlpack(s.first) == 1].cpu(), starts)
    # split_rows' offsets, a tensor of offsets, a row length
    want = wpd.definition(VOCAB, data, kind, CLS, offsets=off_np)
    for o, where in ((ro.offsets, "split_rows"), (off, "tensor")):
        s = b.wordpiece_batch(t, isolated=b",", offsets=o)
        same(s, want, (where, k))
        assert torch.equal(torch.from_dlpack(s.row_offsets).cpu(), torch.from_numpy(want[4])), where
    assert s.tolist() == quads(want, off_np)
    n = len(data) // 64 * 64
    cut = np.arange(0, n + 1, 64)
    s = b.wordpiece_batch(t[:n], isolated=b",", max_word_bytes=20, unk_id=5, row_length=64)
    want64 = wpd.definition(VOCAB, data[:n], kind, CLS, M=20, unk=5, offsets=cut)
    same(s, want64, ("row_length", k))
    assert s.tolist() == quads(want64, cut)
    # host tensors take the host route
    s = b.wordpiece_batch(t.cpu(), isolated=b",", offsets=off.cpu())
    assert s.device is None and s.tolist() == quads(want, off_np)

# a case-insensitive handle leaves the tensor as it is
ci = ar.BytesAhoCorasick([b"AB", b"##C", b"a"], ascii_case_insensitive=True, matchkind=ar.MatchKind.LeftmostLongest)
same(ci.wordpiece(t), wpd.definition([b"AB", b"##C", b"a"], data, KINDS[2], wpd.classes(), fold=True), "fold")
assert torch.equal(t.cpu(), torch.from_numpy(np.frombuffer(data, dtype=np.uint8)))

# errors
def raises(exc, fn):
    try:
        fn()
    except exc:
        return
    raise AssertionError(f"{exc.__name__} not raised")

b = ar.BytesAhoCorasick(VOCAB)
raises(TypeError, lambda: b.wordpiece_batch(t))                                      # a tensor needs one of the two
raises(TypeError, lambda: b.wordpiece_batch(t, offsets=off, row_length=8))
raises(TypeError, lambda: b.wordpiece_batch(t, offsets=off.to(torch.int32)))
raises(ValueError, lambda: b.wordpiece_batch(t, offsets=off.cpu()))                  # on another device
raises(ValueError, lambda: b.wordpiece_batch(t, offsets=off[:-1]))                   # they do not end at len
raises(ValueError, lambda: b.wordpiece(t, max_word_bytes=0))

# empty inputs
e = b.wordpiece(torch.zeros(0, dtype=torch.uint8, device=dev))
assert len(e) == 0 and e.tolist() == [] and torch.from_dlpack(e.start).numel() == 0
e = b.wordpiece_batch(torch.zeros(0, dtype=torch.uint8, device=dev), offsets=torch.zeros(3, dtype=torch.int64, device=dev))
assert e.tolist() == [[], []] and torch.from_dlpack(e.row_offsets).tolist() == [0, 0, 0]
e = b.wordpiece(torch.full((100,), 32, dtype=torch.uint8, device=dev))
assert len(e) == 0 and e.tolist() == []

# lifetime: the columns outlive the result, the inputs and the automaton; the inputs stay alive while kernels read them
want = wpd.definition(VOCAB, data, KINDS[0], wpd.classes(), offsets=off_np)
s = b.wordpiece_batch(t, offsets=ro.offsets)
cols = [torch.from_dlpack(c) for c in (s.id, s.start, s.end, s.first)]
del s, b, t, ro, off
gc.collect()
for k in range(8):
    other = torch.from_numpy(np.frombuffer(text(len(data), 40 + k), dtype=np.uint8).copy()).to(dev)
torch.cuda.synchronize()
for c, w in zip(cols, want):
    assert torch.equal(c.cpu(), torch.from_numpy(w))
print("OK")
"""


def test_tensors_in_and_torch_out():
    """wordpiece and wordpiece_batch on tensors in HBM with split_rows' offsets, a tensor of offsets, row_length and neither,
    all kinds; torch.from_dlpack of every column on the automaton's device; first against the word starts; a
    case-insensitive handle leaves the tensor as it is; errors; empty inputs; lifetime.  In a process of its own: torch has
    to be the first to load the HIP runtime."""
    pytest.importorskip("torch")
    p = subprocess.run([sys.executable, "-c", _TENSOR_SCRIPT, ROOT, os.path.join(ROOT, "tests")], capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
