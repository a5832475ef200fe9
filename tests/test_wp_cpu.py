"""CPU checks of the WordPiece tokenization (acx_wordpiece_host: the definition of wp.hpp walked over the tables
acx_compile_host(_ex) makes, the tables the device chains read -- and what the header, the binding, the stubs and the
extension classes declare for wordpiece / wordpiece_batch, with the argument checks of the Python methods).  Expected values
come from plain Python (tests/wp_definition.py restates the definition: the dictionary against the current position with
startswith, no trie), never from the library.  tests/test_gpu_wp.py has the device side."""
import ctypes
import os
import re

import numpy as np
import pytest

import wp_definition as wpd

capi = pytest.importorskip("ahocorasick_rs_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STD, LF, LL = capi.MATCH_STANDARD, capi.MATCH_LEFTMOST_FIRST, capi.MATCH_LEFTMOST_LONGEST
KINDS = (STD, LF, LL)
DEFAULT = wpd.classes()
NEW_EXPORTS = ("acx_wordpiece", "acx_wordpiece_device", "acx_wordpiece_into_device", "acx_wordpiece_host", "acx_wp_count",
               "acx_wp_rows", "acx_wp_on_device", "acx_wp_id", "acx_wp_start", "acx_wp_end", "acx_wp_first", "acx_wp_row_offsets",
               "acx_wp_copy", "acx_free_wp")
NAMES = ("id", "start", "end", "first", "row_offsets")


def check(patterns, hay, kind=LL, cls=DEFAULT, *, prefix=b"##", M=100, unk=-1, offsets=None, fold=False, what=None):
    assert (STD, LF, LL) == (wpd.STD, wpd.LF, wpd.LL) and (capi.WP_WORD, capi.WP_SPACE, capi.WP_ALONE) == (wpd.WORD, wpd.SPACE, wpd.ALONE)
    h = capi.HostAutomaton(patterns, kind, capi.BUILD_ASCII_CASE_INSENSITIVE if fold else 0)
    try:
        got = capi.wordpiece_host(h, hay, cls, prefix=prefix, max_word=M, unk_id=unk, offsets=offsets, match_kind=kind)
    finally:
        h.close()
    want = wpd.definition(patterns, hay, kind, cls, prefix=prefix, M=M, unk=unk, offsets=offsets, fold=fold)
    for g, w, name in zip(got, want, NAMES):
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, name, g[:40], w[:40])
    ids, start, end, first, ro = got
    assert np.all(np.diff(start) > 0) and np.all(end > start) and np.all(start[1:] >= end[:-1])
    return [(int(i), int(s), int(e), int(f)) for i, s, e, f in zip(ids, start, end, first)]


@pytest.mark.parametrize("kind", KINDS)
def test_the_three_kinds_pick_as_match_at_does(kind):
    vocab = [b"a", b"ab", b"abc", b"##c", b"##b", b"##bc"]
    got = check(vocab, b"abc ab a", kind)
    word = {STD: [(0, 0, 1, 1), (4, 1, 2, 0), (3, 2, 3, 0)], LF: [(0, 0, 1, 1), (4, 1, 2, 0), (3, 2, 3, 0)], LL: [(2, 0, 3, 1)]}[kind]
    assert got[:len(word)] == word
    # LeftmostFirst: the smallest index, not the shortest
    assert check([b"ab", b"a", b"##b"], b"ab", LF) == [(0, 0, 2, 1)]
    assert check([b"ab", b"a", b"##b"], b"ab", STD) == [(1, 0, 1, 1), (2, 1, 2, 0)]
    for k in KINDS:
        check(vocab[::-1], b"abcabc cab abcb", k)


@pytest.mark.parametrize("kind", KINDS)
def test_a_folding_handle_folds_the_patterns_and_the_prefix_but_not_the_classes(kind):
    vocab = [b"Un", b"xxABLE", b"xx", b"a"]
    got = check(vocab, b"uNaBlE UNABLE", kind, prefix=b"XX", fold=True)
    assert got == [(0, 0, 2, 1), (1, 2, 6, 0), (0, 7, 9, 1), (1, 9, 13, 0)]
    # the classes see the raw byte: "A" separates, "a" does not
    cls = wpd.classes(b" A")
    assert check([b"b", b"##a", b"a"], b"bAb ba", kind, cls, fold=True) == [(0, 0, 1, 1), (0, 2, 3, 1), (0, 4, 5, 1), (1, 5, 6, 0)]
    assert check([b"b", b"##a"], b"bAb", kind, fold=False) == [(-1, 0, 3, 1)]


def test_a_continuation_needs_the_prefix():
    assert check([b"un", b"able"], b"unable") == [(-1, 0, 6, 1)]
    assert check([b"un", b"##able"], b"unable") == [(0, 0, 2, 1), (1, 2, 6, 0)]


def test_a_word_whose_last_step_fails_is_one_piece():
    assert check([b"un", b"##ab", b"##l"], b"unable unabl") == [(-1, 0, 6, 1), (0, 7, 9, 1), (1, 9, 11, 0), (2, 11, 12, 0)]


def test_the_bare_substring_is_looked_up_at_a_word_start():
    assert check([b"##ing", b"s"], b"##ing s##ing sing") == [(0, 0, 5, 1), (-1, 6, 12, 1), (1, 13, 14, 1), (0, 14, 17, 0)]


def test_an_entry_equal_to_the_prefix_is_never_a_continuation():
    # at a word start "##" is an entry like any other; behind a piece it would match the empty string
    assert check([b"##", b"a", b"##b"], b"## a## ab") == [(0, 0, 2, 1), (-1, 3, 6, 1), (1, 7, 8, 1), (2, 8, 9, 0)]
    assert check([b"##", b"a", b"###"], b"a##") == [(1, 0, 1, 1), (2, 1, 2, 0), (2, 2, 3, 0)]  # "###" is C + "#"
    assert check([b"##", b"a"], b"aa") == [(-1, 0, 2, 1)]


def test_an_isolated_byte_ends_the_word_in_front_of_it():
    cls = wpd.classes(isolated=b",")
    assert check([b"ab,", b"ab", b","], b"ab, ab,", cls=cls) == [(1, 0, 2, 1), (2, 2, 3, 1), (1, 4, 6, 1), (2, 6, 7, 1)]
    assert check([b"ab,"], b"ab,", cls=cls) == [(-1, 0, 2, 1), (-1, 2, 3, 1)]
    assert check([b",", b"##,"], b",,,", cls=cls) == [(0, 0, 1, 1), (0, 1, 2, 1), (0, 2, 3, 1)]  # each its own word: all first


@pytest.mark.parametrize("kind", KINDS)
def test_a_prefix_that_is_not_in_the_trie(kind):
    # no continuation ever matches: a word is one entry or unknown (Standard stops at "a" and cannot go on)
    first = (-1, 0, 2, 1) if kind == STD else (0, 0, 2, 1)
    assert check([b"ab", b"a", b"##b"], b"ab a abb", kind, prefix=b"@@") == [first, (1, 3, 4, 1), (-1, 5, 8, 1)]
    assert check([b"ab", b"#x"], b"abab", kind, prefix=b"##") == [(-1, 0, 4, 1)]  # "#" is a node, "##" is not


@pytest.mark.parametrize("kind", KINDS)
def test_an_empty_prefix_makes_every_entry_a_continuation(kind):
    got = check([b"ab", b"c", b"abc"], b"abcab cc", kind, prefix=b"")
    assert [x[3] for x in got].count(1) == 2 and got[-1] == (1, 7, 8, 0)


@pytest.mark.parametrize("kind", KINDS)
def test_words_of_m_and_m_plus_one_bytes(kind):
    vocab = [b"a", b"##a"]
    for M in (1, 2, 5, 100, capi.WP_MAX_WORD):
        got = check(vocab, b"a" * M + b" " + b"a" * (M + 1) + b" a", kind, M=M, unk=-7)
        assert len(got) == M + 2 and got[M] == (-7, M + 1, 2 * M + 2, 1) and got[-1] == (0, 2 * M + 3, 2 * M + 4, 1)
    check([b"a" * 300, b"##" + b"a" * 299], b"a" * 300 + b" " + b"a" * 599, kind, M=capi.WP_MAX_WORD)  # no limit on pattern length


CUTS = (None, [0, 19], [0, 0, 0, 5, 9, 19], [0, 5, 5, 5, 9, 19, 19, 19], [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 19], [0, 0, 19, 19])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("offsets", CUTS)
def test_row_cuts_empty_rows_and_a_row_start_inside_a_word(kind, offsets):
    vocab = [b"un", b"##able", b"able", b"a", b"##b", b"##le", b"u", b"##n", b"n", b"b", b"l", b"e", b"##l", b"##e", b"##a"]
    hay = b"unable, unable able"
    got = check(vocab, hay, kind, wpd.classes(isolated=b","), offsets=offsets)
    if offsets and 5 in offsets:  # the row start at 5 cuts "unable" into "unabl" and "e": both begin a word
        assert any(s == 5 and f == 1 for _, s, _, f in got)
    check(vocab, b"", kind, offsets=[0, 0, 0])
    check(vocab, b"", kind)
    check(vocab, b"   ", kind, offsets=[0, 1, 3])


def test_the_row_length_cut_is_the_offsets_cut():
    vocab = [b"ab", b"##ab", b"a", b"b", b"##b"]
    hay = b"abab ababab b ab"
    for u in (1, 2, 4, 8, 16):
        check(vocab, hay, LL, offsets=list(range(0, len(hay) + 1, u)))


def test_bert_recipe_against_a_hand_tokenization():
    vocab = [b"[UNK]", b"the", b"quick", b"brown", b"fox", b"##es", b"jump", b"##ed", b",", b".", b"un", b"##aff", b"##able"]
    cls = wpd.classes(wpd.WHITESPACE, wpd.PUNCTUATION)
    got = check(vocab, b"the quick brown foxes jumped, unaffable\txyz.", LL, cls, unk=0)
    assert [vocab[i] for i, _, _, _ in got] == [b"the", b"quick", b"brown", b"fox", b"##es", b"jump", b"##ed", b",", b"un", b"##aff",
                                               b"##able", b"[UNK]", b"."]
    assert capi.ASCII_WHITESPACE == wpd.WHITESPACE and capi.ASCII_PUNCTUATION == wpd.PUNCTUATION and len(wpd.PUNCTUATION) == 32


@pytest.mark.parametrize("seed", range(24))
def test_seeded_fuzz(seed):
    case = wpd.fuzz_case(seed)
    want = wpd.definition(case["patterns"], case["hay"], case["kind"], case["cls"], prefix=case["prefix"], M=case["M"],
                          offsets=case["offsets"], fold=case["fold"])
    assert wpd.fuzz_shows_all_three(case, want) == (True, True, True), seed  # the generator's promise, per seed
    check(case["patterns"], case["hay"], case["kind"], case["cls"], prefix=case["prefix"], M=case["M"], offsets=case["offsets"],
          fold=case["fold"], what=seed)


def test_argument_errors_of_the_host_form():
    h = capi.HostAutomaton([b"a", b"##b"], LL)
    try:
        def code(fn):
            with pytest.raises(ValueError) as e:
                fn()
            return e.value.code

        bad = DEFAULT.copy()
        bad[65] = 3
        assert code(lambda: capi.wordpiece_host(h, b"ab", bad)) == capi.EINVAL                      # a class above 2
        assert code(lambda: capi.wordpiece_host(h, b"ab", DEFAULT, max_word=0)) == capi.EINVAL
        assert code(lambda: capi.wordpiece_host(h, b"ab", DEFAULT, max_word=capi.WP_MAX_WORD + 1)) == capi.EINVAL
        assert code(lambda: capi.wordpiece_host(h, b"abc", DEFAULT, offsets=[0, 2, 1, 3])) == capi.EINVAL
        assert code(lambda: capi.wordpiece_host(h, b"abc", DEFAULT, offsets=[0, 2])) == capi.EINVAL
        assert code(lambda: capi.wordpiece_host(h, b"abc", DEFAULT, offsets=[1, 3])) == capi.EINVAL
        assert code(lambda: capi.wordpiece_host(h, b"abc", DEFAULT, match_kind=3)) == capi.EINVAL
        L = capi.lib()
        n = ctypes.c_uint64(7)
        hay = np.frombuffer(b"ab ab", dtype=np.uint8)
        out = np.full(40, -7, dtype=np.int64)
        fo = np.full(8, 9, dtype=np.uint8)
        pre = np.frombuffer(b"##", dtype=np.uint8)
        head = (hay.ctypes.data, 5, None, 0, DEFAULT.ctypes.data, pre.ctypes.data, 2, 100, -1)
        cols = (out.ctypes.data, out[8:].ctypes.data, out[16:].ctypes.data, fo.ctypes.data, out[24:].ctypes.data)
        assert L.acx_wordpiece_host(None, *head, 0, LL, 0, None, None, None, None, None, ctypes.byref(n)) == capi.EINVAL
        assert L.acx_wordpiece_host(h._h, *head, 0, LL, 0, None, None, None, None, None, None) == capi.EINVAL
        assert L.acx_wordpiece_host(h._h, *head, 1, LL, 0, None, None, None, None, None, ctypes.byref(n)) == capi.EINVAL  # a flag
        assert L.acx_wordpiece_host(h._h, *head[:4], None, *head[5:], 0, LL, 0, None, None, None, None, None, ctypes.byref(n)) == capi.EINVAL
        assert L.acx_wordpiece_host(h._h, *head, 0, LL, 8, None, *cols[1:], ctypes.byref(n)) == capi.EINVAL  # a column is missing
        assert L.acx_wordpiece_host(h._h, *head, 0, LL, 0, None, None, None, None, None, ctypes.byref(n)) == capi.OK and n.value == 4
        # a cap smaller than T: T is reported, nothing is written
        assert L.acx_wordpiece_host(h._h, *head, 0, LL, 3, *cols, ctypes.byref(n)) == capi.OK
        assert n.value == 4 and np.all(out == -7) and np.all(fo == 9)
        assert L.acx_wordpiece_host(h._h, *head, 0, LL, 4, *cols, ctypes.byref(n)) == capi.OK
        assert n.value == 4 and list(out[:5]) == [0, 1, 0, 1, -7] and list(out[8:13]) == [0, 1, 3, 4, -7]
        assert list(out[16:21]) == [1, 2, 4, 5, -7] and list(fo[:5]) == [1, 0, 1, 0, 9] and list(out[24:27]) == [0, 4, -7]
    finally:
        h.close()


def test_argument_checks_of_the_python_methods():
    import ahocorasick_rs_amd as ac
    args = ac.ahocorasick_rs._wordpiece_args
    cls, prefix, m, unk = args(False)
    assert bytes(cls) == bytes(DEFAULT) and prefix == b"##" and m == 100 and unk == -1
    assert args(True) == args(False)
    cls, prefix, m, unk = args(False, b"@", b" ,", ac.ASCII_PUNCTUATION[:11] + ac.ASCII_PUNCTUATION[12:], 1, -2 ** 63)
    assert prefix == b"@" and m == 1 and unk == -2 ** 63 and cls[32] == cls[44] == 1 and cls[33] == 2 and cls[9] == 0
    assert args(False, bytearray(b""), memoryview(b"\n"), None, 1024, 2 ** 63 - 1)[1:] == (b"", 1024, 2 ** 63 - 1)
    assert ac.ASCII_WHITESPACE == b" \t\n\r\x0b\x0c" and ac.ASCII_PUNCTUATION == wpd.PUNCTUATION
    # str for the str class only; the sets ASCII
    assert args(True, "##", " \n", ",.") == args(False, b"##", b" \n", b",.")
    assert args(True, "ä")[1] == "ä".encode()
    for k, v in ((1, "##"), (2, " "), (3, ",")):
        with pytest.raises(TypeError):
            args(False, *([None] * (k - 1)), v)
    for k in (2, 3):
        with pytest.raises(ValueError):
            args(True, *([None] * (k - 1)), "ä")
    with pytest.raises(ValueError):
        args(False, None, b" ,", b",")  # a byte in both sets
    with pytest.raises(TypeError):
        args(False, None, 5)
    for bad in (True, 1.0, "1", b"1"):
        with pytest.raises(TypeError):
            args(False, None, None, None, bad)
        with pytest.raises(TypeError):
            args(False, None, None, None, None, bad)
    for bad in (0, -1, 1025, 2 ** 64):
        with pytest.raises(ValueError):
            args(False, None, None, None, bad)
    for bad in (2 ** 63, -2 ** 63 - 1):
        with pytest.raises(ValueError):
            args(False, None, None, None, None, bad)
    # the binding's class table
    with pytest.raises(ValueError):
        capi.wp_classes(b" ,", b",")
    with pytest.raises(TypeError):
        capi.wp_classes(" ")
    assert np.array_equal(capi.wp_classes(), DEFAULT)
    assert np.array_equal(capi.wp_classes(capi.ASCII_WHITESPACE, capi.ASCII_PUNCTUATION), wpd.classes(wpd.WHITESPACE, wpd.PUNCTUATION))


def test_the_binding_and_the_extension_declare_the_new_names():
    L = capi.lib()
    with open(os.path.join(ROOT, "include", "acx.h")) as f:
        header = f.read()
    for name in NEW_EXPORTS:
        assert hasattr(L, name), name
        assert re.search(r"\b" + name + r"\s*\(", header), name
    for name in ("wordpiece", "wordpiece_device", "wordpiece_into_device"):
        assert callable(getattr(capi.Automaton, name)), name
    assert callable(capi.wordpiece_host) and capi.DeviceWordPieces._PREFIX == "wp"
    assert (capi.WP_WORD, capi.WP_SPACE, capi.WP_ALONE) == tuple(
        int(re.search(r"#define\s+ACX_WP_" + n + r"\s+(\d+)", header).group(1)) for n in ("WORD", "SPACE", "ALONE"))
    assert (capi.WP_ID, capi.WP_START, capi.WP_END, capi.WP_FIRST, capi.WP_ROW_OFFSETS) == tuple(
        int(re.search(r"#define\s+ACX_WP_" + n + r"\s+(\d+)", header).group(1)) for n in ("ID", "START", "END", "FIRST", "ROW_OFFSETS"))
    assert capi.WP_MAX_WORD == int(re.search(r"#define\s+ACX_WP_MAX_WORD\s+(\d+)u", header).group(1))
    assert int(re.search(r"#define\s+ACX_VERSION\s+(\d+)", header).group(1)) == 11 == capi.ABI_VERSION  # additive
    import ahocorasick_rs
    import ahocorasick_rs_amd
    for mod in (ahocorasick_rs, ahocorasick_rs_amd):
        assert "WordPieces" in mod.__all__ and isinstance(mod.WordPieces, type)
        assert "ASCII_WHITESPACE" in mod.__all__ and "ASCII_PUNCTUATION" in mod.__all__
        for cls in (mod.AhoCorasick, mod.BytesAhoCorasick):
            assert callable(cls.wordpiece) and callable(cls.wordpiece_batch)
    assert ahocorasick_rs.WordPieces is ahocorasick_rs_amd.WordPieces
    with open(os.path.join(ROOT, "ahocorasick_rs_amd", "ahocorasick_rs.pyi")) as f:
        stubs = f.read()
    assert "class WordPieces" in stubs and stubs.count("def wordpiece(") == 2 and stubs.count("def wordpiece_batch(") == 2


def test_constants_of_the_kernel_header():
    with open(os.path.join(ROOT, "ahocorasick_rs_amd", "csrc", "wp.hpp")) as f:
        text = f.read()
    c = {n: int(re.search(r"constexpr uint32_t WP_" + n + r"\s*=\s*(\d+)", text).group(1)) for n in ("THREADS", "TILE", "MAX_WORD")}
    assert c["THREADS"] == 256 and c["TILE"] == 4096 and 256 <= c["MAX_WORD"] == capi.WP_MAX_WORD
    assert c["TILE"] + c["MAX_WORD"] < 1 << 15  # a tile's pieces and a word's fit the 16-bit words in LDS
    assert "THE DEFINITION" in text and "STARTING SIZES, NOT MEASURED ONES" in text
