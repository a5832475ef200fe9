"""CPU checks of the row cut (acx_split_rows_host / acx_split_rows: a delimited buffer becomes the offsets the batch entry
points take, and what the header, the binding, the stubs and both packages declare for split_rows / RowOffsets).  Expected
values come from numpy (the definition restated below), never from the library, and equality is exact.
tests/test_gpu_rows.py has the device side."""
import ast
import ctypes
import os
import re

import numpy as np
import pytest

capi = pytest.importorskip("ahocorasick_rs_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ahocorasick_rs_amd", "csrc")

NEW_EXPORTS = ("acx_split_rows", "acx_split_rows_device", "acx_rows_count", "acx_rows_bytes", "acx_rows_on_device",
               "acx_rows_device", "acx_rows_offsets", "acx_rows_copy", "acx_free_rows", "acx_split_rows_host",
               "acx_split_rows_into_device")
DELIMITERS = (0x0A, 0x00, 0xFF, 0x80)
GUARD = -0x3C3C3C3C3C3C3C3D


def definition(data, d):
    """0; p + 1 for every position p with data[p] == d, ascending; len(data) if it is not empty and its last byte is not d"""
    a = np.frombuffer(bytes(data), dtype=np.uint8)
    cuts = np.flatnonzero(a == d).astype(np.int64) + 1
    tail = [len(a)] if len(a) and a[-1] != d else []
    return np.concatenate([np.zeros(1, np.int64), cuts, np.asarray(tail, dtype=np.int64)])


def trap_alphabet(d):
    """the bytes an inexact SWAR compare confuses with d: a borrow out of a matching byte makes d ^ 1 behind it look equal"""
    return np.asarray([d, d ^ 1, d ^ 0x80, (d + 1) & 0xFF, (d - 1) & 0xFF], dtype=np.uint8)


def cases(d):
    """(name, bytes) at the seams of the definition"""
    o = (d ^ 0x55) or 1  # a byte that is not the delimiter
    assert o != d
    rng = np.random.default_rng(20261019 + d)
    for n in (0, 1, 2, 15, 16, 17, 3000, 4099):
        yield ("no delimiter", n), bytes([o]) * n
        yield ("every byte", n), bytes([d]) * n
        if n:
            yield ("first byte only", n), bytes([d]) + bytes([o]) * (n - 1)
            yield ("last byte only", n), bytes([o]) * (n - 1) + bytes([d])
        if n >= 15:
            yield ("runs", n), (bytes([o]) * 3 + bytes([d]) * 4 + bytes([o]) + bytes([d]) * 2) * (n // 10) + bytes([o]) * (n % 10)
        for p in (2, 64, 1000):
            a = np.full(n, o, dtype=np.uint8)
            a[rng.integers(0, p, size=n) == 0] = d
            yield ("density 1/%d" % p, n), a.tobytes()
        yield ("the SWAR trap's alphabet", n), trap_alphabet(d)[rng.integers(0, 5, size=n)].tobytes()
    # d ^ 1 right behind a d, at every place of a 16-byte line
    for at in range(16):
        a = np.full(40, o, dtype=np.uint8)
        a[at], a[at + 1] = d, d ^ 1
        yield ("d ^ 1 behind d", at), a.tobytes()


@pytest.mark.parametrize("d", DELIMITERS)
def test_split_rows_host_is_the_definition(d):
    L = capi.lib()
    for what, data in cases(d):
        want = definition(data, d)
        got = capi.split_rows_host(data, d)
        assert got.dtype == np.int64 and np.array_equal(got, want), (what, d, got[:20], want[:20])
        assert capi.split_rows_host(data, d, count_only=True) == len(want) - 1, (what, d)  # offsets == NULL agrees
        # what the batch entry points require of offsets: strictly ascending from 0 to len, no empty row
        assert got[0] == 0 and int(got[-1]) == len(data) and (np.diff(got) > 0).all(), (what, d)
        # the owning call
        h = np.frombuffer(data, dtype=np.uint8)
        out = ctypes.c_void_p()
        assert L.acx_split_rows(h.ctypes.data if len(h) else None, len(h), d, ctypes.byref(out)) == capi.OK
        r = capi.DeviceRows(out.value)
        assert r.rows == len(want) - 1 and r.nbytes == len(data) and not r.on_device and r.offsets_ptr(), (what, d)
        assert np.array_equal(r.offsets(), want), (what, d)
        inplace = np.ctypeslib.as_array(ctypes.cast(r.offsets_ptr(), ctypes.POINTER(ctypes.c_int64)), shape=(len(want),))
        assert np.array_equal(inplace, want), (what, d)
        r.free()


def test_rows_of_text_are_splitlines_keepends():
    text = b"alpha\nbeta\n\n\ngamma delta\n" * 7 + b"no newline at the end"
    off = capi.split_rows_host(text)
    assert [text[off[i]:off[i + 1]] for i in range(len(off) - 1)] == text.splitlines(keepends=True)
    assert capi.split_rows_host(b"").tolist() == [0] and capi.split_rows_host(b"\n").tolist() == [0, 1]
    assert capi.split_rows_host(b"a").tolist() == [0, 1] and capi.split_rows_host(b"\n\n").tolist() == [0, 1, 2]


def test_capacity_one_word_short_writes_nothing_and_says_what_is_needed():
    L = capi.lib()
    for data in (b"a\nb\nc", b"a\nb\nc\n", b"x", b"\n" * 9):
        want = definition(data, 10)
        h = np.frombuffer(data, dtype=np.uint8)
        for capacity in (len(want) - 1, 1, 0):
            buf = np.full(len(want) + 2, GUARD, dtype=np.int64)
            n = ctypes.c_uint64(99)
            rc = L.acx_split_rows_host(h.ctypes.data, len(h), 10, buf.ctypes.data, capacity, ctypes.byref(n))
            assert rc == capi.EINVAL and n.value == len(want) - 1, (data, capacity)
            assert (buf == GUARD).all(), "a word was written although the buffer is too small"
            assert str(len(want)) in L.acx_last_error().decode(), L.acx_last_error()
        buf = np.full(len(want) + 2, GUARD, dtype=np.int64)
        n = ctypes.c_uint64(99)
        assert L.acx_split_rows_host(h.ctypes.data, len(h), 10, buf.ctypes.data, len(want), ctypes.byref(n)) == capi.OK
        assert np.array_equal(buf[:len(want)], want) and (buf[len(want):] == GUARD).all() and n.value == len(want) - 1


def test_null_arguments_and_zero_length():
    L = capi.lib()
    n = ctypes.c_uint64(99)
    buf = np.full(3, GUARD, dtype=np.int64)
    h = np.frombuffer(b"a\nb", dtype=np.uint8)
    # len == 0: 0 rows and the one word 0, a null pointer allowed
    assert L.acx_split_rows_host(None, 0, 10, buf.ctypes.data, 1, ctypes.byref(n)) == capi.OK
    assert n.value == 0 and buf.tolist() == [0, GUARD, GUARD]
    n.value = 99
    assert L.acx_split_rows_host(None, 0, 10, None, 0, ctypes.byref(n)) == capi.OK and n.value == 0
    assert L.acx_split_rows_host(h.ctypes.data, 0, 10, buf.ctypes.data, 0, ctypes.byref(n)) == capi.EINVAL  # no room for the one word
    # a null haystack with len > 0, no place for the count
    assert L.acx_split_rows_host(None, 3, 10, buf.ctypes.data, 3, ctypes.byref(n)) == capi.EINVAL
    assert L.acx_split_rows_host(h.ctypes.data, 3, 10, buf.ctypes.data, 3, None) == capi.EINVAL
    out = ctypes.c_void_p()
    assert L.acx_split_rows(None, 3, 10, ctypes.byref(out)) == capi.EINVAL and not out.value
    assert L.acx_split_rows(h.ctypes.data, 3, 10, None) == capi.EINVAL
    assert L.acx_split_rows(None, 0, 10, ctypes.byref(out)) == capi.OK
    r = capi.DeviceRows(out.value)
    assert r.rows == 0 and r.nbytes == 0 and r.offsets().tolist() == [0]
    r.free()
    # the accessors of no result
    assert L.acx_rows_count(None) == 0 and L.acx_rows_bytes(None) == 0 and L.acx_rows_on_device(None) == 0
    assert not L.acx_rows_offsets(None) and L.acx_rows_copy(None, buf.ctypes.data) == capi.EINVAL
    L.acx_free_rows(None)
    # the device entry points' argument checks come before any device state
    assert L.acx_split_rows_into_device(None, 3, 10, None, 0, ctypes.byref(n)) == capi.EINVAL
    assert L.acx_split_rows_into_device(None, 0, 10, 4, 1, ctypes.byref(n)) == capi.EINVAL  # misaligned offsets
    assert L.acx_split_rows_into_device(None, 0, 10, None, 0, None) == capi.EINVAL
    assert L.acx_split_rows_device(None, 3, 10, ctypes.byref(out)) == capi.EINVAL
    assert L.acx_split_rows_device(None, 0, 10, None) == capi.EINVAL


def test_header_and_binding_agree_on_the_rows_abi():
    hdr = open(os.path.join(ROOT, "include", "acx.h")).read()
    L = capi.lib()
    for name in NEW_EXPORTS:
        decl = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert decl, name
        assert hasattr(L, name), name
        n_args = len([a for a in re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",") if a.strip()])
        assert len(getattr(L, name).argtypes) == n_args, (name, n_args)  # bound with its argument types, one per argument
    assert "typedef struct acx_rows acx_rows_t;" in hdr
    u8, u64, vp = ctypes.c_uint8, ctypes.c_uint64, ctypes.c_void_p
    assert list(L.acx_split_rows.argtypes) == list(L.acx_split_rows_device.argtypes) == [vp, u64, u8, ctypes.POINTER(vp)]
    assert list(L.acx_split_rows_host.argtypes) == list(L.acx_split_rows_into_device.argtypes) == [vp, u64, u8, vp, u64, ctypes.POINTER(u64)]
    assert L.acx_rows_count.restype is u64 and L.acx_rows_bytes.restype is u64 and L.acx_rows_offsets.restype is vp
    # additive: the version and the path counters are the parent's
    assert L.acx_version() == capi.ABI_VERSION == int(re.search(r"#define ACX_VERSION (\d+)", hdr).group(1)) == 11
    assert len(capi.Automaton.PATH_STATS) == int(re.search(r"#define ACX_PATH_STATS (\d+)", hdr).group(1)) == 14
    for name in ("split_rows", "split_rows_device", "split_rows_host", "split_rows_into_device"):
        assert callable(getattr(capi, name)), name
    assert capi.DeviceRows


def test_the_stage_is_in_the_build_lists_and_its_sizes_are_plain_constants():
    from ahocorasick_rs_amd import _build
    assert "rows.hip" in _build.LIB_SOURCES and "rows_api.cpp" in _build.LIB_SOURCES and "rows.hpp" in _build.LIB_HEADERS
    for f in ("rows.hip", "rows_api.cpp", "rows.hpp"):
        assert os.path.exists(os.path.join(CSRC, f)), f
    hpp = open(os.path.join(CSRC, "rows.hpp")).read()
    sizes = {}
    for name in ("ROWS_THREADS", "ROWS_TILE"):  # plain constants: the seam tests read them
        m = re.search(r"constexpr uint32_t %s\s*=\s*(\d+)\s*;" % name, hpp)
        assert m, name
        sizes[name] = int(m.group(1))
    assert sizes["ROWS_THREADS"] % 64 == 0 and sizes["ROWS_TILE"] % (16 * sizes["ROWS_THREADS"]) == 0
    hip = open(os.path.join(CSRC, "rows.hip")).read()
    assert not re.findall(r"\batomic\w+\(", hip), "ranks come from scans: the stage needs no atomic"
    assert "asm" not in hip, "plain C++ stores only"
    assert "replace_scan(" in open(os.path.join(CSRC, "rows_api.cpp")).read(), "the scan between the kernels is the library's own"


def test_pyi_declares_the_function_and_the_class():
    tree = ast.parse(open(os.path.join(ROOT, "ahocorasick_rs_amd", "ahocorasick_rs.pyi")).read())
    fn = [f for f in tree.body if isinstance(f, ast.FunctionDef) and f.name == "split_rows"]
    assert len(fn) == 1
    a = fn[0].args
    assert [x.arg for x in a.args] == ["data", "delimiter"] and not a.kwonlyargs and a.vararg is None and a.kwarg is None
    assert [ast.unparse(x) for x in a.defaults] == ["b'\\n'"] and ast.unparse(fn[0].returns) == "RowOffsets"
    cls = [c for c in tree.body if isinstance(c, ast.ClassDef) and c.name == "RowOffsets"]
    assert len(cls) == 1
    names = {f.name for f in cls[0].body if isinstance(f, ast.FunctionDef)}
    assert names >= {"offsets", "device", "nbytes", "__len__", "tolist"}


def test_both_packages_export_the_function_and_the_class():
    import ahocorasick_rs
    import ahocorasick_rs_amd
    for mod in (ahocorasick_rs, ahocorasick_rs_amd, ahocorasick_rs.ahocorasick_rs):
        assert callable(mod.split_rows) and isinstance(mod.RowOffsets, type)
        assert "split_rows" in mod.__all__ and "RowOffsets" in mod.__all__
        assert "split_rows(data, delimiter=" in mod.split_rows.__doc__
        with pytest.raises(TypeError):
            mod.RowOffsets()  # (made by split_rows only)
    assert set(ahocorasick_rs.__all__) == set(ahocorasick_rs_amd.__all__)
    assert ahocorasick_rs.RowOffsets is ahocorasick_rs_amd.RowOffsets and ahocorasick_rs.split_rows is ahocorasick_rs_amd.split_rows
    for name in ("offsets", "device", "nbytes", "tolist", "__len__"):
        assert hasattr(ahocorasick_rs.RowOffsets, name)
    # the parent's exports stay
    assert {"MaskedRows", "RowScores", "FilteredRows", "PatternCounts", "MatchColumns", "Column"} <= set(ahocorasick_rs.__all__)


def test_split_rows_on_host_objects():
    import ahocorasick_rs as ar
    text = b"first line\nsecond\n\nfourth, and then an unterminated fifth"
    want = definition(text, 10)
    for data in (text, bytearray(text), memoryview(text), np.frombuffer(text, dtype=np.uint8)):
        ro = ar.split_rows(data)
        assert isinstance(ro, ar.RowOffsets) and ro.device is None and ro.nbytes == len(text) and len(ro) == len(want) - 1
        col = ro.offsets
        assert isinstance(col, ar.Column) and len(col) == len(want) and col.__dlpack_device__() == (1, 0)
        got = np.from_dlpack(col)
        assert got.dtype == np.int64 and np.array_equal(got, want)
        assert np.array_equal(np.asarray(memoryview(col)), want) and memoryview(col).format == "q"  # host columns are buffers too
        assert ro.tolist() == want.tolist()
    assert bytes(text) == b"first line\nsecond\n\nfourth, and then an unterminated fifth"  # never written
    # the offsets outlive the RowOffsets and its input
    data = bytearray(b"a,b,,c")
    ro = ar.split_rows(data, ",")
    got = np.from_dlpack(ro.offsets)
    del ro, data
    assert got.tolist() == [0, 2, 4, 5, 6]
    # other delimiters, the empty input, keyword form
    assert ar.split_rows(b"a\0b\0", 0).tolist() == [0, 2, 4] and ar.split_rows(b"a\0b\0", delimiter=b"\0").tolist() == [0, 2, 4]
    assert ar.split_rows(b"\xffa\x80", 0xFF).tolist() == [0, 1, 3] and ar.split_rows(b"\xffa\x80", 0x80).tolist() == [0, 3]
    empty = ar.split_rows(b"")
    assert len(empty) == 0 and empty.tolist() == [0] and empty.nbytes == 0 and np.from_dlpack(empty.offsets).tolist() == [0]
    for d in DELIMITERS:
        data = trap_alphabet(d)[np.random.default_rng(d).integers(0, 5, size=777)]
        assert np.array_equal(np.from_dlpack(ar.split_rows(data, d).offsets), definition(data, d)), d
    # what is no byte buffer
    for bad in ("text\n", 12, None, [b"a\n"], np.zeros((2, 2), dtype=np.uint8)):
        with pytest.raises(TypeError):
            ar.split_rows(bad)
    with pytest.raises((BufferError, TypeError)):
        ar.split_rows(np.zeros(4, dtype=np.int32))
    with pytest.raises(TypeError):
        ar.split_rows(np.zeros(8, dtype=np.uint8)[::2])  # not contiguous
    with pytest.raises(TypeError):
        ar.split_rows()
    with pytest.raises(TypeError):
        ar.split_rows(b"a", 10, 3)


def test_the_delimiter_argument():
    """the rules of mask_all's fill, restated: an int in range(256) or a one-byte buffer, or a one-character ASCII str"""
    import ahocorasick_rs as ar
    data = bytes(range(256)) * 2
    for delim, want in ((0, 0), (42, 42), (255, 255), (b"*", 42), (bytearray(b"\xff"), 255), (memoryview(b"\0"), 0),
                        (np.asarray([9], dtype=np.uint8), 9), ("*", 42), ("\0", 0), ("\x7f", 127), (" ", 32), ("\n", 10)):
        assert ar.split_rows(data, delim).tolist() == [0, want + 1, want + 257, 512][:4 if want != 255 else 3], delim
    assert ar.split_rows(data).tolist() == ar.split_rows(data, b"\n").tolist() == [0, 11, 267, 512]
    for bad in (-1, 256, 1 << 70, -(1 << 70), b"", b"**", bytearray(b"ab"), np.asarray([1, 2], dtype=np.uint8), "", "**", "\x80", "é",
                "€", "\U0001F600"):
        with pytest.raises(ValueError) as e:
            ar.split_rows(data, bad)
        assert "delimiter" in str(e.value), bad
    for bad in (1.0, None, True, [42], (42,), np.asarray([[1]], dtype=np.uint8), ["*"]):
        with pytest.raises(TypeError):
            ar.split_rows(data, bad)
