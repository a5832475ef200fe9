"""CPU checks of the cover of a search's matches (acx_mask_host: every byte that a record covers becomes the fill byte, every
other byte stays or becomes 0, and what the header, the binding, the stubs and the extension classes declare for mask_all /
match_mask and their _batch forms).  Expected values come from numpy (the definition restated below over synthetic
records), never from the library.  tests/test_gpu_mask.py has the device side."""
import ast
import os
import re

import numpy as np
import pytest

capi = pytest.importorskip("ahocorasick_rs_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_EXPORTS = ("acx_mask", "acx_mask_device", "acx_mask_host", "acx_mask_rows_device", "acx_masked_bytes", "acx_masked_rows",
               "acx_masked_on_device", "acx_masked_data", "acx_masked_offsets", "acx_masked_copy", "acx_masked_copy_offsets",
               "acx_free_masked")
ZERO = 1  # ACX_MASK_ZERO


def definition(hay, offsets, records, counts, fill, flags):
    """out[off[h] + i] = fill where a record of row h, clipped to the row (end' = min(end, row length), start' = min(start,
    end')), has start' <= i < end'; elsewhere the haystack's byte, or 0 with ACX_MASK_ZERO"""
    hay = np.frombuffer(bytes(hay), dtype=np.uint8)
    out = np.zeros(len(hay), dtype=np.uint8) if flags & ZERO else hay.copy()
    offsets = [0, len(hay)] if offsets is None else [int(x) for x in offsets]
    counts = [len(records)] if counts is None else [int(c) for c in counts]
    at = 0
    for h, c in enumerate(counts):
        b, rowlen = offsets[h], offsets[h + 1] - offsets[h]
        for _, s, e in records[at:at + c]:
            e = min(int(e), rowlen)
            s = min(int(s), e)
            out[b + s:b + e] = fill
        at += c
    return out


def check(hay, offsets, records, counts, fill=0x2A, flags=0, what=None):
    records = [tuple(r) for r in records]
    got = capi.mask_host(hay, offsets, np.asarray(records, dtype=np.uint64).reshape(-1, 3), counts, fill, flags)
    want = definition(hay, offsets, records, counts, fill, flags)
    assert got.dtype == np.uint8 and np.array_equal(got, want), (what, fill, flags, bytes(got[:80]), bytes(want[:80]))
    return got


def random_case(rng, row_lens, per_row=(0, 0, 1, 2, 5), longest=12, beyond=False):
    """a batch of rows of the given lengths with a few records each, ordered by end within a row as a search reports them;
    beyond: some records end behind their row or begin behind it"""
    hay = rng.integers(97, 123, size=int(sum(row_lens)), dtype=np.uint8).tobytes()
    offsets = np.concatenate([[0], np.cumsum(row_lens)]).astype(np.int64)
    records, counts = [], []
    for n in row_lens:
        k = int(rng.choice(per_row))
        rec = []
        for _ in range(k):
            s = int(rng.integers(0, n + 1 + (3 if beyond else 0)))
            e = s + int(rng.integers(1, longest + 1))
            if not beyond:
                e = min(e, n)
            rec.append((int(rng.integers(0, 1 << 20)), s, e))
        rec.sort(key=lambda r: (r[2], r[1]))
        records += rec
        counts.append(k)
    return hay, offsets, records, counts


@pytest.mark.parametrize("flags", [0, ZERO])
@pytest.mark.parametrize("fill", [0x00, 0xFF, 0x2A, ord("q")])  # ('q': a fill that is a byte of the haystack)
def test_mask_host_on_seeded_batches(fill, flags):
    rng = np.random.default_rng(20261018)
    for rows in (1, 2, 7, 64, 301):
        lens = rng.choice([0, 0, 1, 5, 17, 64, 300], size=rows)
        check(*random_case(rng, lens), fill, flags, ("ragged", rows))
        check(*random_case(rng, [33] * rows), fill, flags, ("uniform", rows))
        check(*random_case(rng, lens, beyond=True), fill, flags, ("clipped", rows))


def test_mask_host_one_row_empty_rows_and_nothing():
    rng = np.random.default_rng(1)
    hay, _, rec, _ = random_case(rng, [500], per_row=(9,))
    for flags in (0, ZERO):
        check(hay, None, rec, None, 1, flags, "one row: no offsets, no counts")
        check(hay, None, rec, [len(rec)], 1, flags, "one row with its count")
        check(hay, [0, 500], rec, None, 1, flags, "one row with its offsets")
        check(b"", None, [], None, 1, flags, "len = 0")
        check(b"", [0], [], [], 1, flags, "no row at all")
        check(b"", [0, 0, 0], [], [0, 0], 1, flags, "empty rows only")
        check(b"abc", [0, 0, 3, 3], [(0, 1, 2)], [0, 1, 0], 1, flags, "empty rows around one")
        check(b"abcdef", [0, 3, 6], [], [0, 0], 1, flags, "no record: a copy, or a clear")
        check(b"abcdef", [0, 3, 6], [(0, 0, 3), (0, 0, 3)], [1, 1], 1, flags, "every byte covered")


@pytest.mark.parametrize("flags", [0, ZERO])
def test_mask_host_overlapping_records_ordered_by_end(flags):
    hay = b"0123456789abcdefghij"
    nested = [(0, 4, 6), (1, 3, 7), (2, 2, 8), (3, 0, 9)]       # each one inside the next
    same = [(0, 5, 9), (1, 5, 9), (2, 5, 9)]                    # copies of a pattern cover the same bytes once
    chained = [(0, 0, 4), (1, 2, 6), (2, 5, 9), (3, 8, 12), (4, 12, 13)]
    for rec in (nested, same, chained, nested + same + chained):
        got = check(hay, None, rec, None, ord("*"), flags, rec)
        covered = set()
        for _, s, e in rec:
            covered |= set(range(s, e))
        assert {i for i in range(len(hay)) if got[i] == ord("*")} == covered
    two = check(hay, [0, 10, 20], nested + chained, [4, 5], ord("*"), flags)
    assert bytes(two[9:10]) == (b"9", b"\0")[flags] and bytes(two[10:14]) == b"****"


@pytest.mark.parametrize("flags", [0, ZERO])
def test_mask_host_clips_every_record_to_its_row(flags):
    hay = b"aaaaabbbbbccccc"
    off = [0, 5, 10, 15]
    for rec, counts, painted in (
            ([(0, 3, 8)], [1, 0, 0], {3, 4}),                    # an end behind the row: the next row stays
            ([(0, 3, 1 << 63)], [0, 1, 0], {8, 9}),
            ([(0, 7, 9)], [1, 0, 0], set()),                     # a start behind the row
            ([(0, 1 << 62, 1 << 63)], [0, 0, 1], set()),
            ([(0, 4, 2)], [0, 1, 0], set()),                     # start > end: nothing
            ([(0, 5, 5)], [1, 0, 0], set()),                     # an empty match covers nothing
            ([(0, 0, 99)], [0, 0, 1], {10, 11, 12, 13, 14}),     # the last row: the buffer's end
    ):
        got = check(hay, off, rec, counts, 0xFF, flags, rec)
        assert {i for i in range(15) if got[i] == 0xFF} == painted, rec


def test_mask_host_in_place_and_exactly_its_output():
    L = capi.lib()
    buf = np.frombuffer(b"\xc3" * 8 + b"hello world" + b"\xc3" * 8, dtype=np.uint8).copy()
    m = np.asarray([[0, 0, 5], [1, 6, 11]], dtype=np.uint64)
    before = m.copy()
    p = buf.ctypes.data + 8
    assert L.acx_mask_host(p, 11, None, 1, m.ctypes.data, 2, None, ord("#"), 0, p) == capi.OK  # dst == hay
    assert buf.tobytes() == b"\xc3" * 8 + b"##### #####" + b"\xc3" * 8 and np.array_equal(m, before)
    assert L.acx_mask_host(p, 11, None, 1, m.ctypes.data, 2, None, 1, ZERO, p) == capi.EINVAL       # no 0 / 1 mask in place
    src = np.frombuffer(b"hello world", dtype=np.uint8).copy()
    assert L.acx_mask_host(src.ctypes.data, 11, None, 1, m.ctypes.data, 2, None, 1, ZERO, p) == capi.OK
    assert buf.tobytes() == b"\xc3" * 8 + b"\1\1\1\1\1\0\1\1\1\1\1" + b"\xc3" * 8 and src.tobytes() == b"hello world"
    assert L.acx_mask_host(None, 11, None, 1, m.ctypes.data, 2, None, 1, ZERO, p) == capi.OK        # the mask reads no haystack


def test_mask_host_refuses_bad_arguments():
    hay, rec = b"abcdefghij", [(0, 1, 2), (0, 3, 4), (0, 5, 6)]
    for flags in (2, 3, 4, 1 << 31):  # an unknown flag bit
        with pytest.raises(ValueError) as ei:
            capi.mask_host(hay, None, rec, None, 1, flags)
        assert ei.value.code == capi.EINVAL, flags
    for off in ([1, 5, 10], [0, 5, 9], [0, 5, 11], [0, 7, 5, 10][:3], [0, 11, 10]):  # offsets that do not rise from 0 to len
        with pytest.raises(ValueError) as ei:
            capi.mask_host(hay, off, rec, [1, 2], 1)
        assert ei.value.code == capi.EINVAL, off
    with pytest.raises(ValueError) as ei:
        capi.mask_host(hay, [0, 4, 2, 10], rec, [1, 1, 1], 1)
    assert ei.value.code == capi.EINVAL
    for counts in ([1, 1], [2, 2], [4, 0], [0, 0], [(1 << 64) - 1, 4]):  # the counts do not sum to the records
        with pytest.raises(ValueError) as ei:
            capi.mask_host(hay, [0, 5, 10], rec, counts, 1)
        assert ei.value.code == capi.EINVAL, counts
    L = capi.lib()
    m = np.asarray(rec, dtype=np.uint64)
    h = np.frombuffer(hay, dtype=np.uint8).copy()
    out = np.zeros(10, dtype=np.uint8)
    off = np.asarray([0, 5, 10], dtype=np.uint64)
    c = np.asarray([1, 2], dtype=np.uint64)
    assert L.acx_mask_host(h.ctypes.data, 10, off.ctypes.data, 2, m.ctypes.data, 3, c.ctypes.data, 1, 0, out.ctypes.data) == capi.OK
    assert L.acx_mask_host(h.ctypes.data, 10, off.ctypes.data, 2, None, 3, c.ctypes.data, 1, 0, out.ctypes.data) == capi.EINVAL  # no records
    assert L.acx_mask_host(h.ctypes.data, 10, off.ctypes.data, 2, m.ctypes.data, 3, c.ctypes.data, 1, 0, None) == capi.EINVAL     # no output
    assert L.acx_mask_host(None, 10, off.ctypes.data, 2, m.ctypes.data, 3, c.ctypes.data, 1, 0, out.ctypes.data) == capi.EINVAL   # no haystack
    assert L.acx_mask_host(h.ctypes.data, 10, off.ctypes.data, 2, m.ctypes.data, 3, None, 1, 0, out.ctypes.data) == capi.EINVAL   # two rows, no counts
    assert L.acx_mask_host(h.ctypes.data, 10, None, 2, m.ctypes.data, 3, c.ctypes.data, 1, 0, out.ctypes.data) == capi.EINVAL     # two rows, no offsets


def test_header_and_binding_agree_on_the_mask_abi():
    hdr = open(os.path.join(ROOT, "include", "acx.h")).read()
    L = capi.lib()
    for name in NEW_EXPORTS:
        decl = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert decl, name
        assert hasattr(L, name), name
        n_args = len([a for a in re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",") if a.strip()])
        assert len(getattr(L, name).argtypes) == n_args, (name, n_args)  # bound with its argument types, one per argument
    assert int(re.search(r"#define ACX_MASK_ZERO (\d+)", hdr).group(1)) == capi.MASK_ZERO == ZERO
    # acx_mask* take acx_filter*'s haystack arguments, then (fill, flags) in place of (min_matches, flags)
    u8, u64 = capi.ctypes.c_uint8, capi.ctypes.c_uint64
    for mine, plain in (("acx_mask", "acx_filter"), ("acx_mask_device", "acx_filter_device")):
        want = list(getattr(L, plain).argtypes)
        at = want.index(capi.ctypes.c_uint32) - 1
        assert want[at] is u64
        want[at] = u8
        assert list(getattr(L, mine).argtypes) == want, mine
    # additive: the version and the path counters are the parent's
    assert L.acx_version() == capi.ABI_VERSION == int(re.search(r"#define ACX_VERSION (\d+)", hdr).group(1)) == 11
    assert len(capi.Automaton.PATH_STATS) == int(re.search(r"#define ACX_PATH_STATS (\d+)", hdr).group(1)) == 14
    for name in ("mask", "mask_device"):
        assert callable(getattr(capi.Automaton, name))
    assert callable(capi.mask_host) and callable(capi.mask_rows_device) and capi.DeviceMasked


def test_the_stage_is_in_the_build_list_and_the_other_kernel_files_are_the_parents():
    from ahocorasick_rs_amd import _build
    assert "mask.hip" in _build.LIB_SOURCES and "mask_api.cpp" in _build.LIB_SOURCES and "mask.hpp" in _build.LIB_HEADERS
    for f in ("mask.hip", "mask_api.cpp", "mask.hpp"):
        assert os.path.exists(os.path.join(ROOT, "ahocorasick_rs_amd", "csrc", f)), f
    hpp = open(os.path.join(ROOT, "ahocorasick_rs_amd", "csrc", "mask.hpp")).read()
    for name in ("MASK_THREADS", "MASK_TILE", "MASK_LONG"):  # plain constants: the seam tests read them
        assert re.search(r"constexpr uint32_t %s\s*=\s*\d+\s*;" % name, hpp), name
    hip = open(os.path.join(ROOT, "ahocorasick_rs_amd", "csrc", "mask.hip")).read()
    assert re.findall(r"\batomic\w+\(([^,)]*)", hip) == ["&s_nlong"], "the paint needs no atomic on global memory"
    assert "asm" not in hip, "plain C++ stores only"


def test_pyi_declares_the_methods_and_the_class():
    tree = ast.parse(open(os.path.join(ROOT, "ahocorasick_rs_amd", "ahocorasick_rs.pyi")).read())
    classes = {c.name: c for c in tree.body if isinstance(c, ast.ClassDef)}
    want = {
        "mask_all": (["self", "haystack", "fill", "overlapping"], [], None),
        "match_mask": (["self", "haystack", "overlapping"], [], "bytes"),
        "mask_all_batch": (["self", "haystacks", "fill", "overlapping"], ["offsets", "row_length"], "MaskedRows"),
        "match_mask_batch": (["self", "haystacks", "overlapping"], ["offsets", "row_length"], "MaskedRows"),
    }
    for cls in ("AhoCorasick", "BytesAhoCorasick"):
        for method, (pos, kwonly, returns) in want.items():
            mine = [f for f in classes[cls].body if isinstance(f, ast.FunctionDef) and f.name == method]
            assert len(mine) == 1, (cls, method)
            a = mine[0].args
            assert [x.arg for x in a.args] == pos, (cls, method)
            assert [x.arg for x in a.kwonlyargs] == kwonly, (cls, method)
            assert a.vararg is None and a.kwarg is None, (cls, method)
            assert [ast.unparse(d) for d in a.defaults] == ["False"], (cls, method)
            assert [ast.unparse(d) for d in a.kw_defaults] == ["None"] * len(kwonly), (cls, method)
            assert ast.unparse(mine[0].returns) == (returns or ("str" if cls == "AhoCorasick" else "bytes")), (cls, method)
        fill = [x for f in classes[cls].body if isinstance(f, ast.FunctionDef) and f.name == "mask_all" for x in f.args.args][2]
        assert ast.unparse(fill.annotation) == ("str" if cls == "AhoCorasick" else "Any")
    names = {f.name for f in classes["MaskedRows"].body if isinstance(f, ast.FunctionDef)}
    assert names >= {"data", "offsets", "device", "nbytes", "__len__", "tolist"}
    text = open(os.path.join(ROOT, "ahocorasick_rs_amd", "ahocorasick_rs.pyi")).read()
    assert "one entry per CHARACTER" in text and "byte for" in text and "TypeError" in text and "ValueError" in text


def test_extension_classes_have_the_methods():
    import ahocorasick_rs
    import ahocorasick_rs_amd
    for mod in (ahocorasick_rs, ahocorasick_rs_amd, ahocorasick_rs.ahocorasick_rs):
        for cls in (mod.AhoCorasick, mod.BytesAhoCorasick):
            for method, sig in (("mask_all", "(haystack, fill, overlapping=False)"), ("match_mask", "(haystack, overlapping=False)"),
                                ("mask_all_batch", "(haystacks, fill, overlapping=False, *, offsets=None, row_length=None)"),
                                ("match_mask_batch", "(haystacks, overlapping=False, *, offsets=None, row_length=None)")):
                assert callable(getattr(cls, method)), (cls, method)
                assert method + sig in getattr(cls, method).__doc__, (cls, method)
        assert isinstance(mod.MaskedRows, type) and "MaskedRows" in mod.__all__
        with pytest.raises(TypeError):
            mod.MaskedRows()  # (made by the methods only)
    assert ahocorasick_rs.MaskedRows is ahocorasick_rs_amd.MaskedRows
    for name in ("data", "offsets", "device", "nbytes", "tolist", "__len__"):
        assert hasattr(ahocorasick_rs.MaskedRows, name)
    # the parent's methods keep their signatures
    assert "score_batch(haystacks, weights, overlapping=False, *" in ahocorasick_rs.AhoCorasick.score_batch.__doc__
    assert "RowScores" in ahocorasick_rs.__all__ and "FilteredRows" in ahocorasick_rs.__all__


def test_the_fill_argument_of_both_classes():
    """the one check both classes' mask_all and mask_all_batch make of `fill` (the extension's _mask_fill: no automaton)"""
    from ahocorasick_rs_amd.ahocorasick_rs import _mask_fill
    # BytesAhoCorasick: an int in range(256) or a one-byte buffer
    for fill, want in ((0, 0), (42, 42), (255, 255), (b"*", 42), (bytearray(b"\xff"), 255), (memoryview(b"\0"), 0),
                       (np.asarray([9], dtype=np.uint8), 9)):
        assert _mask_fill(fill, False) == want, fill
    for bad in (-1, 256, 1 << 70, -(1 << 70), b"", b"**", bytearray(b"ab"), np.asarray([1, 2], dtype=np.uint8)):
        with pytest.raises(ValueError):
            _mask_fill(bad, False)
    for bad in ("*", 1.0, None, True, [42], (42,), np.asarray([[1]], dtype=np.uint8)):
        with pytest.raises(TypeError):
            _mask_fill(bad, False)
    # AhoCorasick: a one-character ASCII str, so the output stays valid UTF-8
    for fill, want in (("*", 42), ("\0", 0), ("\x7f", 127), (" ", 32)):
        assert _mask_fill(fill, True) == want, fill
    for bad in ("", "**", "\x80", "é", "€", "\U0001F600"):
        with pytest.raises(ValueError):
            _mask_fill(bad, True)
    for bad in (42, b"*", None, True, 1.0, ["*"]):
        with pytest.raises(TypeError):
            _mask_fill(bad, True)


def test_the_per_character_rule_of_the_str_class():
    """mask_all / match_mask of a str give one entry per character: the entries of a covered character's continuation bytes
    are dropped (the extension's _mask_per_character: no device).  The masked row is made by acx_mask_host here, from matches
    in UTF-8 bytes that cover whole characters."""
    from ahocorasick_rs_amd.ahocorasick_rs import _mask_per_character
    s = "aé€\U0001F600b-éé-€€-\U0001F600\U0001F600z"   # 1-, 2-, 3- and 4-byte characters
    raw = s.encode()
    at = np.cumsum([0] + [len(c.encode()) for c in s])   # the byte every character begins at
    for chars in ([(1, 2)], [(2, 3)], [(3, 4)], [(1, 4)], [(0, len(s))], [], [(6, 8), (9, 10), (12, 14)], [(3, 4), (4, 5), (13, 14)]):
        rec = [(0, int(at[a]), int(at[b])) for a, b in chars]
        covered = set()
        for a, b in chars:
            covered |= set(range(a, b))
        text = _mask_per_character(s, capi.mask_host(raw, None, rec, None, ord("*")).tobytes(), True)
        assert isinstance(text, str) and len(text) == len(s), (chars, text)
        assert text == "".join("*" if i in covered else c for i, c in enumerate(s)), (chars, text)
        mask = _mask_per_character(s, capi.mask_host(raw, None, rec, None, 1, ZERO).tobytes(), False)
        assert isinstance(mask, bytes) and len(mask) == len(s)
        assert mask == bytes(1 if i in covered else 0 for i in range(len(s))), (chars, mask)
    assert _mask_per_character("", b"", True) == "" and _mask_per_character("", b"", False) == b""
    assert _mask_per_character("abc", b"a*c", True) == "a*c"   # ASCII: byte for byte
    with pytest.raises(ValueError):
        _mask_per_character("é", b"*", True)                   # one entry per UTF-8 byte is needed
