"""CPU checks of ascii_case_insensitive (acx_build_ex / acx_compile_host_ex with ACX_BUILD_ASCII_CASE_INSENSITIVE): the
case-insensitive tables are the case-sensitive tables of the folded patterns (the crate adds the opposite-case edge to the
same trie node), unknown flag bits are refused, the Python classes validate the keyword before any device work, and the
binding agrees with the header."""
import ast
import ctypes
import os
import re

import numpy as np
import pytest

import gen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
capi = pytest.importorskip("ahocorasick_rs_amd.capi")

FOLD = bytes.maketrans(bytes(range(65, 91)), bytes(range(97, 123)))


def fold(b: bytes) -> bytes:
    return bytes(b).translate(FOLD)


MIXED = [b"Hello", b"WORLD", b"abc", b"ABC", b"aBc", b"caf\xc3\xa9", b"CAF\xc3\x89", b"x1_Y2", b"[Z]@`{", b"Q"] + \
    gen.gen_patterns(400, 2, 9, b"aAbBcCdD xyzXYZ@[`{\xc3\x89", 3)


@pytest.mark.parametrize("mk", [0, 1, 2])
def test_folded_tables_equal_tables_of_folded_patterns(mk):
    ci = capi.HostAutomaton(MIXED, mk, flags=capi.BUILD_ASCII_CASE_INSENSITIVE)
    cs = capi.HostAutomaton([fold(p) for p in MIXED], mk)
    assert ci.n_states == cs.n_states and ci.n_classes == cs.n_classes
    for name in ("classes", "prefix_table", "table", "own_off", "own_pid", "pattern_len", "in_byte", "fail"):
        np.testing.assert_array_equal(getattr(ci, name), getattr(cs, name), err_msg=name)
    # the flag changed something: the plain tables of the mixed-case patterns are another automaton
    plain = capi.HostAutomaton(MIXED, mk)
    assert plain.n_states > cs.n_states
    # no upper-case letter is on any trie edge of the folded automaton; no other byte moved
    assert not any(65 <= int(b) <= 90 for b in ci.in_byte[1:])
    assert sorted(set(int(b) for b in ci.in_byte[1:])) == sorted(set(fold(b"".join(MIXED))))


def test_fold_keeps_non_letters():
    # digits, punctuation next to the letters ('@' 0x40, '[' 0x5B, '`' 0x60, '{' 0x7B) and UTF-8 bytes whose low seven
    # bits are those of a capital letter (0xC1 .. 0xDA) are not folded
    pats = [bytes([b]) for b in range(1, 256)]
    ci = capi.HostAutomaton(pats, 0, flags=capi.BUILD_ASCII_CASE_INSENSITIVE)
    got = sorted(int(b) for b in ci.in_byte[1:])
    assert got == sorted(set(b for b in range(1, 256) if not 65 <= b <= 90))


def test_unknown_flag_bits_are_refused():
    blob, off = capi.pack([b"abc"])
    for bad in (2, 3, 4, 0x80000000):
        with pytest.raises(ValueError) as e:
            capi.HostAutomaton([b"abc"], 0, flags=bad)
        assert e.value.code == capi.EINVAL and "flags" in str(e.value)
        h = ctypes.c_void_p()
        rc = capi.lib().acx_build_ex(blob.ctypes.data, off.ctypes.data, 1, 0, -1, bad, ctypes.byref(h))
        assert rc == capi.EINVAL and not h.value


@pytest.mark.parametrize("name", ["ahocorasick_rs", "ahocorasick_rs_amd"])
def test_keyword_must_be_a_real_bool(name):
    ac = pytest.importorskip(name)
    for bad in (1, 0, "yes", None, 1.0):
        with pytest.raises(TypeError, match="ascii_case_insensitive"):
            ac.AhoCorasick(["a"], ascii_case_insensitive=bad)
        with pytest.raises(TypeError, match="ascii_case_insensitive"):
            ac.BytesAhoCorasick([b"a"], ascii_case_insensitive=bad)
    # positional, after implementation
    with pytest.raises(TypeError, match="ascii_case_insensitive"):
        ac.AhoCorasick(["a"], ac.MatchKind.Standard, None, None, 1)
    with pytest.raises(TypeError, match="ascii_case_insensitive"):
        ac.BytesAhoCorasick([b"a"], ac.MatchKind.Standard, None, 1)


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_keyword_reaches_the_device_check():
    ac = pytest.importorskip("ahocorasick_rs_amd")
    for make in (lambda: ac.AhoCorasick(["Abc"], ascii_case_insensitive=True),
                 lambda: ac.BytesAhoCorasick([b"Abc"], ascii_case_insensitive=True)):
        with pytest.raises(RuntimeError) as e:
            make()
        assert "no HIP device" in str(e.value)


def test_binding_agrees_with_the_header():
    hdr = open(os.path.join(ROOT, "include", "acx.h")).read()
    assert capi.ABI_VERSION == int(re.search(r"#define ACX_VERSION (\d+)", hdr).group(1)) == 11
    assert capi.BUILD_ASCII_CASE_INSENSITIVE == int(re.search(r"#define ACX_BUILD_ASCII_CASE_INSENSITIVE (\d+)", hdr).group(1))
    body = hdr[hdr.index("typedef struct acx_info {"):]
    body = body[:body.index("} acx_info_t;")]
    types = {"uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32, "int32_t": ctypes.c_int32}
    fields = [(n, types[t]) for t, n in re.findall(r"\b(u?int(?:32|64)_t)\s+(\w+);", body)]
    assert fields == list(capi.Info._fields_)
    assert fields[-1][0] == "flags"
    assert len(capi.Automaton.PATH_STATS) == int(re.search(r"#define ACX_PATH_STATS (\d+)", hdr).group(1)) == 14
    assert capi.Automaton.PATH_STATS[13] == "folded_on_device"
    L = capi.lib()
    assert hasattr(L, "acx_build_ex") and hasattr(L, "acx_compile_host_ex")


def test_pyi_declares_each_method_once():
    tree = ast.parse(open(os.path.join(ROOT, "ahocorasick_rs_amd", "ahocorasick_rs.pyi")).read())
    classes = {c.name: c for c in tree.body if isinstance(c, ast.ClassDef)}
    for cls in ("AhoCorasick", "BytesAhoCorasick"):
        names = [f.name for f in classes[cls].body if isinstance(f, ast.FunctionDef)]
        assert len(names) == len(set(names)), (cls, names)
        init = next(f for f in classes[cls].body if isinstance(f, ast.FunctionDef) and f.name == "__init__")
        assert init.args.args[-1].arg == "ascii_case_insensitive"
