"""ctypes binding of the C ABI (include/acx.h -> libacx_hip.so).

This is the thin Python view of the drop-in boundary used by the device-pointer
workflows (bench.py, the multi-GPU harness, tests).  The reference-shaped
classes (`AhoCorasick`, `BytesAhoCorasick`) live in the C++ CPython extension
`ahocorasick_rs_amd.ahocorasick_rs`; both sit on the same shared library.

There is no CPU fallback: if libacx_hip.so is missing this module raises
ImportError, and without a HIP device every matching call raises RuntimeError.
"""
from __future__ import annotations

import ctypes
import os
import sys
import weakref
from typing import List, Optional, Sequence, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "libacx_hip.so")

OK, EINVAL, EEMPTY, EOVERLAP, ENOMEM, EDEVICE, ETOOBIG = 0, -1, -2, -3, -4, -5, -6
MATCH_STANDARD, MATCH_LEFTMOST_FIRST, MATCH_LEFTMOST_LONGEST = 0, 1, 2
IMPL_AUTO, IMPL_NONCONTIGUOUS_NFA, IMPL_CONTIGUOUS_NFA, IMPL_DFA = -1, 0, 1, 2
KERNEL_AUTO, KERNEL_DFA_WALK, KERNEL_PREFILTER = 0, 1, 2
KERNEL_NAMES = {1: "dfa_walk", 2: "prefilter"}
BUILD_ASCII_CASE_INSENSITIVE = 1  # build flag (acx_build_ex)
SUM_FIRST, SUM_BY_PATTERN = 1, 2  # acx_summarize: the parts beyond the total and the counts (ACX_SUM_*)
NO_MATCH = (1 << 64) - 1  # the pattern of a haystack's first match when it has none
COL_PATTERN, COL_START, COL_END, COL_ROW_OFFSETS = 0, 1, 2, 3  # acx_columns_data / acx_columns_copy (ACX_COL_*)
TALLY_ROW_OFFSETS, TALLY_PATTERN, TALLY_COUNT = 0, 1, 2  # acx_tally_data / acx_tally_copy (ACX_TALLY_*)
FILT_ROWS, FILT_OFFSETS, FILT_DATA = 0, 1, 2  # acx_filtered_data / acx_filtered_copy (ACX_FILT_*)
FILTER_KEEP_MATCHED = 1  # acx_filter* flags (ACX_FILTER_KEEP_MATCHED); 0 keeps the unmatched rows
SPAN_START, SPAN_END, SPAN_ROW_OFFSETS = 0, 1, 2  # acx_spans_data / acx_spans_copy (ACX_SPAN_*)
SNIP_DATA, SNIP_OFFSETS, SNIP_PATTERN, SNIP_LEAD, SNIP_ROW_OFFSETS = 0, 1, 2, 3, 4  # acx_snippets_data / _copy (ACX_SNIP_*)
SNIPPET_UTF8 = 1  # acx_snippets* flags (ACX_SNIPPET_UTF8): the ends move inward to a character boundary
AT_OVERLAPPING, AT_FULL, AT_ROW_STARTS = 1, 2, 4  # acx_match_at* flags (ACX_AT_*)
AT_PATTERN, AT_END, AT_ROW_OFFSETS = 0, 1, 2  # acx_at_copy (ACX_AT_PATTERN ..)
SEG_UTF8 = 1  # acx_segment* flags (ACX_SEG_UTF8): an unknown piece is a whole UTF-8 character
SEG_PATTERN, SEG_OFFSETS, SEG_ROW_OFFSETS = 0, 1, 2  # acx_seg_copy (ACX_SEG_PATTERN ..)
WP_WORD, WP_SPACE, WP_ALONE = 0, 1, 2  # acx_wordpiece*: the classes of the byte values (ACX_WP_WORD ..)
WP_MAX_WORD = 1024  # ... and the largest max_word (ACX_WP_MAX_WORD)
WP_ID, WP_START, WP_END, WP_FIRST, WP_ROW_OFFSETS = 0, 1, 2, 3, 4  # acx_wp_copy (ACX_WP_ID ..)
MASK_ZERO = 1  # acx_mask* flags (ACX_MASK_ZERO): uncovered bytes become 0 instead of the haystack's own
ABI_VERSION = 11  # ACX_VERSION of include/acx.h this binding was written against

MATCH_DTYPE = np.dtype([("pattern", "<u8"), ("start", "<u8"), ("end", "<u8")])


class Info(ctypes.Structure):
    _fields_ = [("n_patterns", ctypes.c_uint64), ("n_states", ctypes.c_uint64),
                ("n_classes", ctypes.c_uint32), ("stride", ctypes.c_uint32),
                ("min_pattern_len", ctypes.c_uint32), ("max_pattern_len", ctypes.c_uint32),
                ("table_bytes", ctypes.c_uint64), ("lds_hot_rows", ctypes.c_uint32),
                ("kernel", ctypes.c_int32), ("match_kind", ctypes.c_int32),
                ("device", ctypes.c_int32), ("filter_q", ctypes.c_uint32), ("flags", ctypes.c_uint32)]


class HostTables(ctypes.Structure):
    _fields_ = [("n_patterns", ctypes.c_uint64), ("n_states", ctypes.c_uint64),
                ("n_classes", ctypes.c_uint32), ("stride", ctypes.c_uint32),
                ("min_pattern_len", ctypes.c_uint32), ("max_pattern_len", ctypes.c_uint32),
                ("classes", ctypes.c_void_p), ("table", ctypes.c_void_p),
                ("own_off", ctypes.c_void_p), ("own_pid", ctypes.c_void_p),
                ("dlink", ctypes.c_void_p), ("level_start", ctypes.c_void_p),
                ("pattern_len", ctypes.c_void_p), ("rank", ctypes.c_void_p),
                ("filter_xy", ctypes.c_void_p), ("prefix_table", ctypes.c_void_p),
                ("prefix_lists", ctypes.c_void_p),
                ("filter_q", ctypes.c_uint32), ("filter_q2", ctypes.c_uint32),
                ("filter_entries_log2", ctypes.c_uint32), ("prefix_table_log2", ctypes.c_uint32),
                ("filter_density", ctypes.c_double),
                ("n_prefix_keys", ctypes.c_uint32), ("n_prefix_lists", ctypes.c_uint32),
                ("prefix_bitmap", ctypes.c_void_p),
                ("dense", ctypes.c_uint32), ("first_child", ctypes.c_void_p), ("in_byte", ctypes.c_void_p),
                ("fail", ctypes.c_void_p), ("state_flags", ctypes.c_void_p),
                ("walk_t3b", ctypes.c_void_p), ("walk_t3r", ctypes.c_void_p), ("walk_grec", ctypes.c_void_p),
                ("long_min_len", ctypes.c_uint32), ("n_short", ctypes.c_uint32), ("short_min_len", ctypes.c_uint32),
                ("short_xy", ctypes.c_void_p), ("short_codes", ctypes.c_void_p),
                ("max_shift", ctypes.c_uint32), ("pattern_shift", ctypes.c_void_p), ("pattern_head", ctypes.c_void_p)]


class Profile(ctypes.Structure):
    _fields_ = [("scan_ms", ctypes.c_double), ("scan_launches", ctypes.c_uint64),
                ("post_ms", ctypes.c_double), ("scan_bytes", ctypes.c_uint64),
                ("raw_occurrences", ctypes.c_uint64), ("prefix_hits", ctypes.c_uint64),
                ("small_calls", ctypes.c_uint64)]


def _preload_hip_runtime() -> None:
    # One process holds ONE HIP runtime: PyTorch wheels bundle their own libamdhip64 with the
    # same SONAME as /opt/rocm's, and whichever is loaded first serves both libraries.  Nothing
    # is imported here unless asked for (ACX_PRELOAD_TORCH=1): a plain AhoCorasick user needs
    # no torch, and a process that already imported torch already has its runtime loaded.
    if os.environ.get("ACX_PRELOAD_TORCH") != "1" or "torch" in sys.modules:
        return
    try:
        import torch  # noqa: F401
    except Exception:
        pass


vp, u64, i64, u32, i32, u8 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int64, ctypes.c_uint32, ctypes.c_int, ctypes.c_uint8
_out, _u64p = ctypes.POINTER(vp), ctypes.POINTER(u64)  # where a call leaves a handle / a count

# ---- the declarations of include/acx.h, as data (tests/test_capi_abi_cpu.py holds them against the header)
# A stage with a host and a device form: name -> the arguments between the haystack and `out`.  _declare_pair makes
#   acx_<name>(a, hay, len, offsets, n_hay, *tail, out)
#   acx_<name>_device(a, d_hay, len, d_offsets, n_hay, uniform_len, *tail, out)
_PAIRS = {
    "replace": [vp, vp, u64], "summarize": [i32, i32, u32], "find_columns": [i32, i32], "tally": [i32],
    "filter": [i32, u64, u32], "score": [i32, vp, u64], "filter_scored": [i32, vp, u64, i64, u32], "mask": [i32, u8, u32],
    "spans": [i32, i32, u64], "snippets": [i32, u64, u32],
    "find_words": [i32, i32, vp], "filter_words": [i32, i32, vp, u64, u32],
}
# A result type: prefix -> (its size getters, whether _data / _copy take a `which`; None: it has no such pair).  _declare_result
# adds acx_<prefix>_on_device and acx_free_<prefix>.
_RESULTS = {
    "summary": (("total",), None), "columns": (("count", "rows"), True), "tally": (("nnz", "rows"), True),
    "filtered": (("rows", "bytes"), True), "scores": (("rows",), False), "masked": (("bytes", "rows"), False),
    "rows": (("count", "bytes"), None), "spans": (("count", "rows"), True), "snippets": (("count", "rows", "nbytes"), True),
    "token_labels": (("count",), None), "at": (("count", "entries"), None),
    "seg": (("count", "rows"), None), "wp": (("count", "rows"), None),
}
# Everything else, one row each: name -> arguments, or (arguments, what it returns) where that is no status.  (acx_version is
# declared by lib() itself, ahead of the version check.)
_SINGLES = {
    "acx_last_error": ([], ctypes.c_char_p),
    "acx_device_count": [ctypes.POINTER(i32)],
    "acx_set_device": [i32],
    "acx_build": [vp, vp, u64, i32, i32, _out],
    "acx_build_ex": [vp, vp, u64, i32, i32, u32, _out],
    "acx_free_automaton": ([vp], None),
    "acx_automaton_info": [vp, ctypes.POINTER(Info)],
    "acx_set_kernel": [vp, i32],
    "acx_compile_host": [vp, vp, u64, i32, _out],
    "acx_compile_host_ex": [vp, vp, u64, i32, u32, _out],
    "acx_host_tables": [vp, ctypes.POINTER(HostTables)],
    "acx_free_host": ([vp], None),
    "acx_filter_hash": ([u32], u32),
    "acx_prefix_slot": ([u64, u32, u32], u32),
    "acx_find": [vp, vp, u64, i32, i32, _out, _u64p],
    "acx_free_matches": ([vp], None),
    "acx_find_batch": [vp, vp, vp, u64, i32, i32, _out, _u64p, vp],
    "acx_find_device": [vp, vp, u64, vp, u64, u64, i32, i32, _out],
    "acx_replicate": [vp, i32, _out],
    "acx_automaton_device": [vp],
    "acx_shard_range": ([u64, i32, i32, _u64p, _u64p], None),
    "acx_find_batch_multi": [vp, i32, vp, vp, u64, i32, i32, _out, _u64p, vp],
    "acx_result_count": ([vp], u64),
    "acx_result_device_matches": ([vp], vp),
    "acx_result_device_counts": ([vp], vp),
    "acx_result_copy": [vp, vp],
    "acx_result_copy_counts": [vp, vp],
    "acx_free_result": ([vp], None),
    "acx_profile_enable": [vp, i32],
    "acx_profile_read": [vp, ctypes.POINTER(Profile), i32],
    "acx_path_stats": [vp, _u64p, i32],
    "acx_device_alloc": [_out, u64],
    "acx_device_free": [vp],
    "acx_device_upload": [vp, vp, u64],
    "acx_device_download": [vp, vp, u64],
    "acx_device_synchronize": [],
    "acx_device_synchronize_on": [i32],
    "acx_comm_init_all": [ctypes.POINTER(i32), i32, _out],
    "acx_comm_unique_id": [vp],
    "acx_comm_init_rank": [vp, i32, i32, i32, _out],
    "acx_comm_world": [vp],
    "acx_comm_local_ranks": [vp],
    "acx_comm_allgather_counts": [vp, vp, vp],
    "acx_comm_free": ([vp], None),
    "acx_output_offsets": ([vp, i32, vp], None),
    "acx_generate_haystack": [vp, vp, u64, i32, u64, u64],
    "acx_replaced_len": ([vp], u64),
    "acx_replaced_offsets": [vp, vp],
    "acx_replaced_copy": [vp, vp],
    "acx_replaced_device_bytes": ([vp], vp),
    "acx_free_replaced": ([vp], None),
    "acx_splice_host": [vp, u64, vp, u64, vp, vp, u64, vp, _u64p],
    **{"acx_summary_" + part: [vp, vp] for part in ("counts", "any", "first", "by_pattern")},
    **{"acx_summary_device_" + part: ([vp], vp) for part in ("counts", "any", "first", "by_pattern")},
    "acx_summarize_host": [vp, u64, vp, u64, u64, u32, vp, vp, vp],
    "acx_split_host": [vp, u64, vp, vp, vp],
    "acx_split_device": [vp, u64, vp, vp, vp],
    "acx_tally_host": [vp, u64, vp, u64, vp, vp, vp, _u64p],
    "acx_tally_rows_device": [vp, u64, vp, u64, u64, vp, vp, vp, _u64p],
    "acx_filter_host": [vp, u64, vp, u64, vp, u64, u32, vp, vp, vp, _u64p, _u64p],
    "acx_filter_rows_device": [vp, u64, vp, u64, u64, vp, u64, u32, vp, vp, vp, _u64p, _u64p],
    "acx_score_host": [vp, u64, vp, u64, vp, u64, vp],
    "acx_score_rows_device": [vp, u64, vp, u64, vp, u64, vp],
    "acx_masked_offsets": ([vp], vp),
    "acx_masked_copy_offsets": [vp, vp],
    "acx_mask_host": [vp, u64, vp, u64, vp, u64, vp, u8, u32, vp],
    "acx_mask_rows_device": [vp, u64, vp, u64, u64, vp, u64, vp, u8, u32, vp],
    "acx_split_rows": [vp, u64, u8, _out],
    "acx_split_rows_device": [vp, u64, u8, _out],
    "acx_rows_device": [vp],
    "acx_rows_offsets": ([vp], vp),
    "acx_rows_copy": [vp, vp],
    "acx_split_rows_host": [vp, u64, u8, vp, u64, _u64p],
    "acx_split_rows_into_device": [vp, u64, u8, vp, u64, _u64p],
    "acx_spans_host": [vp, u64, vp, u64, u64, vp, vp, vp, _u64p],
    "acx_spans_rows_device": [vp, u64, vp, u64, u64, vp, vp, vp, _u64p],
    "acx_snippets_host": [vp, u64, vp, u64, vp, u64, vp, u64, u32, vp, vp, vp, vp, vp, _u64p],
    "acx_snippets_rows_device": [vp, u64, vp, u64, vp, u64, vp, u64, u64, u32, vp, vp, vp, vp, vp, u64, _u64p],
    "acx_words_host": [vp, u64, vp, u64, vp, u64, vp, i32, i32, vp, vp, vp, _u64p],
    "acx_words_rows_device": [vp, u64, vp, u64, u64, vp, u64, vp, i32, i32, vp, vp, vp, _u64p],
    # (no _PAIRS row: the host form alone takes `codepoints`)
    "acx_tokens": [vp, vp, u64, vp, u64, i32, i32, vp, vp, u64, _out],
    "acx_tokens_device": [vp, vp, u64, vp, u64, u64, i32, vp, vp, u64, _out],
    "acx_token_labels_pattern": ([vp], vp),
    "acx_token_labels_begin": ([vp], vp),
    "acx_token_labels_copy_pattern": [vp, vp],
    "acx_token_labels_copy_begin": [vp, vp],
    "acx_tokens_host": [vp, u64, vp, u64, vp, u64, vp, vp, u64, vp, vp],
    "acx_tokens_rows_device": [u64, vp, u64, u64, vp, u64, vp, vp, vp, u64, vp, vp],
    # (no _PAIRS row: positions and flags lie between the haystack and `out`, and the host form alone takes `codepoints`)
    "acx_match_at": [vp, vp, u64, vp, u64, vp, u64, u32, i32, _out],
    "acx_match_at_device": [vp, vp, u64, vp, u64, u64, vp, u64, u32, _out],
    "acx_match_at_into_device": [vp, vp, u64, vp, u64, u64, vp, u64, u32, vp, vp],
    "acx_match_at_host": [vp, vp, u64, vp, u64, vp, u64, u32, i32, vp, vp, vp],
    "acx_at_pattern": ([vp], vp),
    "acx_at_end": ([vp], vp),
    "acx_at_row_offsets": ([vp], vp),
    "acx_at_copy": [vp, i32, vp],
    # (no _PAIRS row: the host form alone takes `codepoints`)
    "acx_segment": [vp, vp, u64, vp, u64, u32, i32, _out],
    "acx_segment_device": [vp, vp, u64, vp, u64, u64, u32, _out],
    "acx_segment_into_device": [vp, vp, u64, vp, u64, u64, u32, u64, vp, vp, vp, _u64p],
    "acx_segment_host": [vp, vp, u64, vp, u64, u32, i32, u64, vp, vp, vp, _u64p],
    "acx_seg_pattern": ([vp], vp),
    "acx_seg_offsets": ([vp], vp),
    "acx_seg_row_offsets": ([vp], vp),
    "acx_seg_copy": [vp, i32, vp],
    "acx_wordpiece": [vp, vp, u64, vp, u64, vp, vp, u64, u64, i64, u32, i32, _out],
    "acx_wordpiece_device": [vp, vp, u64, vp, u64, u64, vp, vp, u64, u64, i64, u32, _out],
    "acx_wordpiece_into_device": [vp, vp, u64, vp, u64, u64, vp, vp, u64, u64, i64, u32, u64, vp, vp, vp, vp, vp, _u64p],
    "acx_wordpiece_host": [vp, vp, u64, vp, u64, vp, vp, u64, u64, i64, u32, i32, u64, vp, vp, vp, vp, vp, _u64p],
    "acx_wp_id": ([vp], vp),
    "acx_wp_start": ([vp], vp),
    "acx_wp_end": ([vp], vp),
    "acx_wp_first": ([vp], vp),
    "acx_wp_row_offsets": ([vp], vp),
    "acx_wp_copy": [vp, i32, vp],
}


def _declare(L, name: str, argtypes, restype=i32) -> None:
    fn = getattr(L, name)
    fn.argtypes, fn.restype = list(argtypes), restype


def _declare_pair(L, name: str, tail) -> None:
    _declare(L, "acx_" + name, [vp, vp, u64, vp, u64, *tail, _out])
    _declare(L, f"acx_{name}_device", [vp, vp, u64, vp, u64, u64, *tail, _out])


def _declare_result(L, prefix: str, sizes, which: Optional[bool]) -> None:
    for size in sizes:
        _declare(L, f"acx_{prefix}_{size}", [vp], u64)
    _declare(L, f"acx_{prefix}_on_device", [vp])
    _declare(L, "acx_free_" + prefix, [vp], None)
    if which is not None:
        _declare(L, f"acx_{prefix}_data", [vp, i32] if which else [vp], vp)
        _declare(L, f"acx_{prefix}_copy", [vp, i32, vp] if which else [vp, vp])


_lib: Optional[ctypes.CDLL] = None


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_SO):
        raise ImportError(
            f"{_SO} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`"
            " (hipcc --offload-arch=gfx950).  There is no CPU fallback.")
    _preload_hip_runtime()
    L = ctypes.CDLL(os.environ.get("ACX_LIB", _SO), mode=ctypes.RTLD_GLOBAL)  # ACX_LIB: experiments with variant builds
    _declare(L, "acx_version", [])
    # (ACX_LIB_ANY_ABI=1 with ACX_LIB: same-box measurements against an older build of the library)
    if L.acx_version() != ABI_VERSION and not (os.environ.get("ACX_LIB") and os.environ.get("ACX_LIB_ANY_ABI")):
        raise ImportError(f"libacx_hip.so speaks C ABI version {L.acx_version()}, this binding version {ABI_VERSION}: "
                          "rebuild (python -c 'import __graft_entry__ as g; g.build()')")
    for name, tail in _PAIRS.items():
        _declare_pair(L, name, tail)
    for prefix, (sizes, which) in _RESULTS.items():
        _declare_result(L, prefix, sizes, which)
    for name, row in _SINGLES.items():
        _declare(L, name, *(row if isinstance(row, tuple) else (row,)))
    _lib = L
    return L


class AcxError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"acx error {code}: {msg}")
        self.code = code
        self.msg = msg


def _check(rc: int) -> None:
    if rc != OK:
        msg = lib().acx_last_error().decode("utf-8", "replace")
        if rc in (EINVAL, EEMPTY, EOVERLAP, ETOOBIG):
            e = ValueError(msg)
            e.code = rc  # type: ignore[attr-defined]
            raise e
        if rc == ENOMEM:
            raise MemoryError(msg)
        raise AcxError(rc, msg)


def shard_range(n_items: int, shard: int, n_shards: int) -> Tuple[int, int]:
    lo, hi = ctypes.c_uint64(), ctypes.c_uint64()
    lib().acx_shard_range(n_items, shard, n_shards, ctypes.byref(lo), ctypes.byref(hi))
    return int(lo.value), int(hi.value)


def device_count() -> int:
    n = ctypes.c_int(0)
    rc = lib().acx_device_count(ctypes.byref(n))
    return n.value if rc == OK else 0


def set_device(ordinal: int) -> None:
    _check(lib().acx_set_device(ordinal))


def pack(patterns: Sequence[bytes]) -> Tuple[np.ndarray, np.ndarray]:
    off = np.zeros(len(patterns) + 1, dtype=np.uint64)
    if len(patterns):
        off[1:] = np.cumsum([len(p) for p in patterns], dtype=np.uint64)
    blob = np.frombuffer(b"".join(bytes(p) for p in patterns) + b"\0" * 16, dtype=np.uint8).copy()
    return blob, off


class _Handle:
    """The one owner of a handle of the C ABI: `_h`, given back exactly once through the C function that _FREE names -- by
    free() (close() where a class spells it so), or when the object goes; afterwards `_h` is None."""
    _FREE = ""
    _h: Optional[int] = None  # (a constructor that raised leaves nothing to give back)

    def __init__(self, handle: Optional[int]):
        self._h = handle

    def free(self) -> None:
        if self._h:
            getattr(lib(), self._FREE)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class _Size:
    """a size of a result as an attribute: asked of the C getter acx_<prefix>_<getter> whenever it is read"""

    def __init__(self, getter: str):
        self.getter = getter

    def __get__(self, obj, cls=None):
        return self if obj is None else int(obj._fn(self.getter)(obj._h))


class _Result(_Handle):
    """... of a result whose parts lie in HBM or in host memory (on_device tells which).  A subclass names its C prefix
    (_PREFIX: its functions are acx_<prefix>_<name>, its free is acx_free_<prefix>) and its sizes (_Size); _address and
    _copy_out are the two ways to a part."""
    _PREFIX = ""

    def __init_subclass__(cls):
        cls._FREE = "acx_free_" + cls._PREFIX

    def _fn(self, name: str):
        return getattr(lib(), f"acx_{self._PREFIX}_{name}")

    @property
    def on_device(self) -> bool:
        return bool(self._fn("on_device")(self._h))

    def _address(self, name: str, *which: int) -> int:
        """host or device address of a part (by on_device), behind the device work; 0: the result has no such part"""
        return self._fn(name)(self._h, *which) or 0

    def _copy_out(self, name: str, n: int, dtype, *which: int) -> np.ndarray:
        """n elements copied out by acx_<prefix>_<name>; nothing to copy: a null destination"""
        out = np.zeros(n, dtype=dtype)
        _check(self._fn(name)(self._h, *which, out.ctypes.data if out.size else None))
        return out


class HostAutomaton(_Handle):
    """acx_host_automaton_t: the compiled tables on the host (no device needed).
    Arrays are numpy views valid while this object is alive."""
    _FREE = "acx_free_host"
    close = _Handle.free

    def __init__(self, patterns: Sequence[bytes], match_kind: int = MATCH_STANDARD, flags: int = 0):
        blob, off = pack(patterns)
        h = ctypes.c_void_p()
        _check(lib().acx_compile_host_ex(blob.ctypes.data, off.ctypes.data, len(patterns),
                                         match_kind, flags, ctypes.byref(h)))
        self._h = h.value
        t = HostTables()
        _check(lib().acx_host_tables(self._h, ctypes.byref(t)))
        self.t = t

        def view(ptr, n, dtype):
            if not n:
                return np.zeros(0, dtype=dtype)
            size = n * np.dtype(dtype).itemsize
            buf = (ctypes.c_uint8 * size).from_address(ptr)
            return np.frombuffer(buf, dtype=dtype, count=n)

        self.n_states = int(t.n_states)
        self.stride = int(t.stride)
        self.classes = view(t.classes, 256, np.uint8)
        self.dense = bool(t.dense)
        self.table = view(t.table, self.n_states * self.stride if t.dense else 0, np.uint32).reshape(-1, self.stride)
        self.first_child = view(t.first_child, self.n_states + 1, np.uint32)
        self.in_byte = view(t.in_byte, self.n_states, np.uint8)
        self.fail = view(t.fail, self.n_states, np.uint32)
        self.state_flags = view(t.state_flags, self.n_states, np.uint8)
        self.own_off = view(t.own_off, self.n_states + 1, np.uint32)
        self.own_pid = view(t.own_pid, int(t.n_patterns), np.uint32)
        self.dlink = view(t.dlink, self.n_states, np.uint32)
        self.level_start = view(t.level_start, int(t.max_pattern_len) + 2, np.uint32)
        self.pattern_len = view(t.pattern_len, int(t.n_patterns), np.uint32)
        self.rank = view(t.rank, int(t.n_patterns), np.uint32)
        self.filter_xy = view(t.filter_xy, (2 << int(t.filter_entries_log2)) if t.filter_q else 0,
                              np.uint32).reshape(-1, 2)
        self.prefix_table = view(t.prefix_table, (4 << int(t.prefix_table_log2)) if t.filter_q else 0,
                                 np.uint32).reshape(-1, 4)
        self.prefix_lists = view(t.prefix_lists, int(t.n_prefix_lists), np.uint32)
        self.prefix_bitmap = view(t.prefix_bitmap, (8 << int(t.prefix_table_log2)) // 32 if t.filter_q else 0, np.uint32)
        # K1a's failureless walk (automata of at most 32 byte classes, else empty)
        nc = int(t.n_classes)
        self.n_classes = nc
        self.walk_t3b = view(t.walk_t3b, 33 * 1024 if t.walk_t3b else 0, np.uint32)
        self.walk_t3r = view(t.walk_t3r, 2 * nc ** 3 if t.walk_t3r else 0, np.uint32).reshape(-1, 2)
        self.walk_grec = view(t.walk_grec, 4 * self.n_states if t.walk_grec else 0, np.uint32).reshape(-1, 4)
        # K1b's side test for patterns of 1 and 2 bytes (empty without such patterns)
        self.short_xy = view(t.short_xy, 512 if t.short_xy else 0, np.uint32).reshape(-1, 2)
        self.short_codes = view(t.short_codes, 256 + 65536 if t.short_codes else 0, np.uint32)
        # anchors: where every pattern is filed (a code of the prefix table is pattern id | shift << 24)
        self.pattern_shift = view(t.pattern_shift, int(t.n_patterns), np.uint8)
        self.pattern_head = view(t.pattern_head, 4 * int(t.n_patterns) if t.pattern_head else 0, np.uint32).reshape(-1, 4)


def filter_hash(gram: bytes) -> int:
    """level-1 hash H of a (Q-1)-byte gram: entry = H >> 18, signature bits from H >> 9."""
    return int(lib().acx_filter_hash(int.from_bytes(gram[:4], "little")))


def prefix_hash(gram: bytes, salt: int) -> int:
    """32-bit hash of the first `salt` bytes of `gram` (the slot is its top bits)."""
    return int(lib().acx_prefix_slot(int.from_bytes(gram[:salt], "little"), salt, 32))


def prefix_slot(gram: bytes, salt: int, log2: int) -> int:
    """home slot of the first `salt` bytes of `gram` in the prefix table."""
    return int(lib().acx_prefix_slot(int.from_bytes(gram[:salt], "little"), salt, log2))


COMM_ID_BYTES = 128


def comm_unique_id() -> bytes:
    """acx_comm_unique_id: the 128 bytes rank 0 creates and every rank passes to Comm.init_rank."""
    buf = (ctypes.c_uint8 * COMM_ID_BYTES)()
    _check(lib().acx_comm_unique_id(buf))
    return bytes(buf)


def output_offsets(counts: Sequence[int]) -> List[int]:
    """acx_output_offsets: exclusive prefix of the ranks' match counts (+ the total)."""
    c = np.asarray(counts, dtype=np.uint64)
    out = np.zeros(len(c) + 1, dtype=np.uint64)
    lib().acx_output_offsets(c.ctypes.data, len(c), out.ctypes.data)
    return [int(x) for x in out]


class Comm(_Handle):
    """acx_comm_t: the count exchange over RCCL, without torch (include/acx.h)."""
    _FREE = "acx_comm_free"
    close = _Handle.free

    @classmethod
    def init_all(cls, devices: Sequence[int]) -> "Comm":
        arr = (ctypes.c_int * len(devices))(*devices)
        h = ctypes.c_void_p()
        _check(lib().acx_comm_init_all(arr, len(devices), ctypes.byref(h)))
        return cls(h.value)

    @classmethod
    def init_rank(cls, uid: bytes, world: int, rank: int, device: int) -> "Comm":
        assert len(uid) == COMM_ID_BYTES
        buf = (ctypes.c_uint8 * COMM_ID_BYTES).from_buffer_copy(uid)
        h = ctypes.c_void_p()
        _check(lib().acx_comm_init_rank(buf, world, rank, device, ctypes.byref(h)))
        return cls(h.value)

    @property
    def world(self) -> int:
        return int(lib().acx_comm_world(self._h))

    @property
    def local_ranks(self) -> int:
        return int(lib().acx_comm_local_ranks(self._h))

    def allgather_counts(self, local_counts: Sequence[int]) -> List[int]:
        loc = np.asarray(local_counts, dtype=np.uint64)
        assert len(loc) == self.local_ranks
        out = np.zeros(self.world, dtype=np.uint64)
        _check(lib().acx_comm_allgather_counts(self._h, loc.ctypes.data, out.ctypes.data))
        return [int(x) for x in out]


class DeviceBuffer(_Handle):
    """hipMalloc'ed bytes owned by this object (for hosts without torch)."""
    _FREE = "acx_device_free"

    def __init__(self, nbytes: int):
        p = ctypes.c_void_p()
        _check(lib().acx_device_alloc(ctypes.byref(p), nbytes))
        super().__init__(p.value)
        self.nbytes = nbytes

    @property
    def ptr(self) -> Optional[int]:
        """the device address; None once freed"""
        return self._h

    def upload(self, arr: np.ndarray) -> "DeviceBuffer":
        a = np.ascontiguousarray(arr)
        assert a.nbytes <= self.nbytes
        _check(lib().acx_device_upload(self.ptr, a.ctypes.data, a.nbytes))
        return self

    def download(self, nbytes: Optional[int] = None) -> np.ndarray:
        n = self.nbytes if nbytes is None else nbytes
        out = np.empty(n, dtype=np.uint8)
        _check(lib().acx_device_download(out.ctypes.data, self.ptr, n))
        return out


class DeviceResult(_Handle):
    """Matches resident in HBM (acx_result_t)."""
    _FREE = "acx_free_result"

    def __init__(self, handle: int, n_hay: int):
        super().__init__(handle)
        self.n_hay = n_hay

    @property
    def count(self) -> int:
        return int(lib().acx_result_count(self._h))

    @property
    def device_ptr(self) -> int:
        return lib().acx_result_device_matches(self._h) or 0

    def matches(self) -> np.ndarray:
        out = np.empty(self.count, dtype=MATCH_DTYPE)
        if self.count:
            _check(lib().acx_result_copy(self._h, out.ctypes.data))
        return out

    def counts(self) -> np.ndarray:
        out = np.zeros(self.n_hay, dtype=np.uint64)
        if self.n_hay:
            _check(lib().acx_result_copy_counts(self._h, out.ctypes.data))
        return out


class DeviceReplaced(_Handle):
    """The output of Automaton.replace_device, resident in HBM (acx_replaced_t)."""
    _FREE = "acx_free_replaced"

    def __init__(self, handle: int, n_hay: int):
        super().__init__(handle)
        self.n_hay = n_hay

    @property
    def nbytes(self) -> int:
        return int(lib().acx_replaced_len(self._h))

    @property
    def device_ptr(self) -> int:
        """the output bytes in HBM (waits for the splice)"""
        return lib().acx_replaced_device_bytes(self._h) or 0

    def offsets(self) -> np.ndarray:
        """every haystack's output bounds (n_hay + 1 entries; one haystack: [0, nbytes])"""
        out = np.zeros(max(self.n_hay, 1) + 1, dtype=np.uint64)
        _check(lib().acx_replaced_offsets(self._h, out.ctypes.data))
        return out

    def download(self) -> bytes:
        buf = bytearray(self.nbytes)
        if buf:
            _check(lib().acx_replaced_copy(self._h, (ctypes.c_uint8 * len(buf)).from_buffer(buf)))
        return bytes(buf)


class DeviceSummary(_Result):
    """The summaries of Automaton.summarize / summarize_batch / summarize_device (acx_summary_t): reduced in HBM
    (on_device) or on the host; every part is copied out when it is asked for.  A part that `what` did not name raises
    ValueError (code EINVAL)."""
    _PREFIX = "summary"
    total = _Size("total")

    def __init__(self, handle: int, n_hay: int, n_patterns: int):
        super().__init__(handle)
        self.n_hay = n_hay
        self.n_patterns = n_patterns

    def counts(self) -> np.ndarray:
        """matches per haystack"""
        return self._copy_out("counts", self.n_hay, np.uint64)

    def any_bits(self) -> np.ndarray:
        """the bitmap as the library keeps it: (n_hay + 63) // 64 words, LSB first"""
        return self._copy_out("any", (self.n_hay + 63) // 64, np.uint64)

    def any(self) -> np.ndarray:
        """one bool per haystack: it has a match"""
        bits = np.unpackbits(self.any_bits().view(np.uint8), bitorder="little")
        return bits[:self.n_hay].astype(bool)

    def first(self) -> np.ndarray:
        """every haystack's first match (MATCH_DTYPE; pattern == NO_MATCH: none)"""
        return self._copy_out("first", self.n_hay, MATCH_DTYPE)

    def by_pattern(self) -> np.ndarray:
        """matches of the whole call per pattern"""
        return self._copy_out("by_pattern", self.n_patterns, np.uint64)

    def device_ptr(self, name: str) -> int:
        """where the part ("counts", "any", "first", "by_pattern") lies in HBM (waits for the reduction); 0 on the host route"""
        return self._address("device_" + name)


def _records(matches) -> np.ndarray:
    """rows of (pattern, start, end) as a C-contiguous (n, 3) uint64 array"""
    return np.ascontiguousarray(np.asarray(matches, dtype=np.uint64).reshape(-1, 3))


def _u64(seq) -> Optional[np.ndarray]:
    """a C-contiguous flat uint64 array (None stays None: counts or offsets that were not given)"""
    return None if seq is None else np.ascontiguousarray(np.asarray(seq, dtype=np.uint64).reshape(-1))


def _ptr(arr: Optional[np.ndarray], empty: Optional[int] = None) -> Optional[int]:
    """the array's address; `empty` (NULL) when it has no element, NULL when there is no array.  An empty batch is still a
    batch: the *_host definitions take its counts from a non-null pointer, `empty` = the address of a spare word."""
    return None if arr is None else (arr.ctypes.data if len(arr) else empty)


_SPARE = np.zeros(1, dtype=np.uint64)


def summarize_host(matches, counts: Optional[Sequence[int]], n_patterns: int, what: int = SUM_FIRST | SUM_BY_PATTERN):
    """acx_summarize_host: the reduction of a match list (rows of pattern, start, end; all haystacks behind one another,
    counts[h] rows each -- None: one haystack) on the host, no device involved -> (any, first, by_pattern): one bool per
    haystack, MATCH_DTYPE rows, one count per pattern; a part `what` does not name is None.  ValueError (code EINVAL) when
    the counts do not sum to the rows or a row names a pattern >= n_patterns."""
    m, c = _records(matches), _u64(counts)
    n_hay = 1 if c is None else len(c)
    bits = np.zeros((n_hay + 63) // 64 + 1, dtype=np.uint64)
    first = np.zeros(n_hay + 1, dtype=MATCH_DTYPE)
    hist = np.zeros(n_patterns + 1, dtype=np.uint64)
    _check(lib().acx_summarize_host(_ptr(m), len(m), _ptr(c, _SPARE.ctypes.data), n_hay, n_patterns, what, bits.ctypes.data,
                                    first.ctypes.data, hist.ctypes.data))
    any_ = np.unpackbits(bits.view(np.uint8), bitorder="little")[:n_hay].astype(bool)
    return (any_ if what & SUM_FIRST else None, first[:n_hay] if what & SUM_FIRST else None,
            hist[:n_patterns] if what & SUM_BY_PATTERN else None)


class _PartsResult(_Result):
    """A result whose parts acx_<prefix>_data / acx_<prefix>_copy address by a `which`.  A subclass states them in _PARTS:
    which -> (the size the part goes by, its words beyond that size, its element type)."""
    _PARTS: dict = {}

    def data_ptr(self, which: int) -> int:
        """host or device address of the part (by on_device), behind the device work; 0: the result has no such part"""
        return self._address("data", which)

    def _copy_part(self, which: int) -> np.ndarray:
        # (a `which` the class does not state has no size here: the C side refuses it before it looks at the destination)
        size, beyond, dtype = self._PARTS.get(which, (None, 0, np.int64))
        return self._copy_out("copy", getattr(self, size) + beyond if size else 0, dtype, which)


class _BatchPartsResult(_PartsResult):
    """... and whose row offsets exist for a batch only (`batch`: the call was one)"""

    def __init__(self, handle: int, batch: bool):
        super().__init__(handle)
        self.batch = batch


class DeviceColumns(_BatchPartsResult):
    """The columns of Automaton.find_columns / find_columns_batch / find_columns_device (acx_columns_t): three int64
    columns of `count` words and, for a batch, n_hay + 1 row offsets -- in HBM (on_device) or in host memory.  column()
    copies one out; data_ptr() is where it lies (both wait for the split kernel)."""
    _PREFIX = "columns"
    count, rows = _Size("count"), _Size("rows")
    _PARTS = {COL_PATTERN: ("count", 0, np.int64), COL_START: ("count", 0, np.int64), COL_END: ("count", 0, np.int64),
              COL_ROW_OFFSETS: ("rows", 1, np.int64)}
    column = _PartsResult._copy_part

    def pattern(self) -> np.ndarray:
        return self.column(COL_PATTERN)

    def start(self) -> np.ndarray:
        return self.column(COL_START)

    def end(self) -> np.ndarray:
        return self.column(COL_END)

    def row_offsets(self) -> Optional[np.ndarray]:
        return self.column(COL_ROW_OFFSETS) if self.batch else None


def split_host(matches) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """acx_split_host: rows of (pattern, start, end) -> the three int64 columns, on the host, no device involved"""
    m = _records(matches)
    cols = [np.zeros(len(m), dtype=np.int64) for _ in range(3)]
    _check(lib().acx_split_host(_ptr(m), len(m), *[_ptr(c) for c in cols]))
    return cols[0], cols[1], cols[2]


def split_device(d_matches: int, n: int, d_pattern: int, d_start: int, d_end: int) -> None:
    """acx_split_device: n records of 24 bytes at d_matches -> n words at each of the three device addresses (8-byte
    alignment is all any of them needs); complete when it returns"""
    _check(lib().acx_split_device(d_matches or None, n, d_pattern or None, d_start or None, d_end or None))


class DeviceTally(_PartsResult):
    """The result of Automaton.tally / tally_device (acx_tally_t): per-haystack pattern counts in CSR form -- rows + 1 row
    offsets, nnz patterns (ascending within a row) and nnz counts, int64 -- in HBM (on_device) or in host memory.  part()
    copies one out; data_ptr() is where it lies (both wait for the device stage)."""
    _PREFIX = "tally"
    nnz, rows = _Size("nnz"), _Size("rows")
    _PARTS = {TALLY_ROW_OFFSETS: ("rows", 1, np.int64), TALLY_PATTERN: ("nnz", 0, np.int64), TALLY_COUNT: ("nnz", 0, np.int64)}
    part = _PartsResult._copy_part

    def row_offsets(self) -> np.ndarray:
        return self.part(TALLY_ROW_OFFSETS)

    def pattern(self) -> np.ndarray:
        return self.part(TALLY_PATTERN)

    def count(self) -> np.ndarray:
        return self.part(TALLY_COUNT)


def tally_host(matches, counts: Sequence[int]) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """acx_tally_host: rows of (pattern, start, end), counts[h] of them haystack h's -> (row_offsets, pattern, count) of the
    CSR matrix of per-haystack pattern counts, on the host, no device involved.  ValueError (code EINVAL) when the counts do
    not sum to the rows."""
    m, c = _records(matches), _u64(counts)
    ro = np.zeros(len(c) + 1, dtype=np.int64)
    pat, cnt = np.zeros(len(m), dtype=np.int64), np.zeros(len(m), dtype=np.int64)
    nnz = ctypes.c_uint64()
    _check(lib().acx_tally_host(_ptr(m), len(m), _ptr(c), len(c), ro.ctypes.data, _ptr(pat), _ptr(cnt), ctypes.byref(nnz)))
    return ro, pat[:nnz.value], cnt[:nnz.value]


def tally_rows_device(d_records: int, n: int, d_counts: int, n_hay: int, n_patterns: int, d_row_offsets: int, d_pattern: int,
                      d_count: int) -> int:
    """acx_tally_rows_device: the device stage alone -- n records of 24 bytes at d_records, n_hay counts at d_counts -> n_hay
    + 1 row offsets and nnz patterns and counts at the three device addresses (room for n words each); returns nnz;
    complete when it returns"""
    nnz = ctypes.c_uint64()
    _check(lib().acx_tally_rows_device(d_records or None, n, d_counts or None, n_hay, n_patterns, d_row_offsets or None,
                                       d_pattern or None, d_count or None, ctypes.byref(nnz)))
    return int(nnz.value)


class DeviceFiltered(_PartsResult):
    """The result of Automaton.filter / filter_device (acx_filtered_t): the kept rows of a batch -- k source row indexes
    and k + 1 offsets (int64) and the rows' bytes back to back (uint8) -- in HBM (on_device) or in host memory.  part()
    copies one out; data_ptr() is where it lies (both wait for the device stage)."""
    _PREFIX = "filtered"
    n_rows, nbytes = _Size("rows"), _Size("bytes")
    _PARTS = {FILT_ROWS: ("n_rows", 0, np.int64), FILT_OFFSETS: ("n_rows", 1, np.int64), FILT_DATA: ("nbytes", 0, np.uint8)}
    part = _PartsResult._copy_part

    def rows(self) -> np.ndarray:
        return self.part(FILT_ROWS)

    def offsets(self) -> np.ndarray:
        return self.part(FILT_OFFSETS)

    def data(self) -> np.ndarray:
        return self.part(FILT_DATA)


def filter_host(hay, offsets: Optional[Sequence[int]], counts: Sequence[int], min_matches: int = 1, flags: int = 0, *,
                sizes_only: bool = False):
    """acx_filter_host: the definition of the row filter on the host, no device involved.  hay: bytes-like; offsets: n + 1
    from 0 to len(hay), or None (one row); counts[h]: row h's matches.  Returns (rows, offsets, data) as int64 / int64 /
    uint8 arrays, or (n_rows, n_bytes) with sizes_only.  ValueError (code EINVAL) for a bad flag, min_matches = 0 or
    offsets that do not rise from 0 to len(hay)."""
    h = np.frombuffer(bytes(hay), dtype=np.uint8)
    c, off = _u64(counts), _u64(offsets)
    n = len(c)
    if off is not None and len(off) != n + 1:
        raise ValueError("offsets needs len(counts) + 1 entries")
    k, nb = ctypes.c_uint64(), ctypes.c_uint64()
    args = (_ptr(h), len(h), None if off is None else off.ctypes.data, n, _ptr(c), min_matches, flags)
    _check(lib().acx_filter_host(*args, None, None, None, ctypes.byref(k), ctypes.byref(nb)))
    if sizes_only:
        return int(k.value), int(nb.value)
    rows, oo = np.zeros(max(n, 1), dtype=np.int64), np.zeros(n + 1, dtype=np.int64)
    data = np.zeros(max(len(h), 1), dtype=np.uint8)
    _check(lib().acx_filter_host(*args, rows.ctypes.data, oo.ctypes.data, data.ctypes.data, ctypes.byref(k), ctypes.byref(nb)))
    return rows[:k.value], oo[:k.value + 1], data[:nb.value]


def filter_rows_device(d_hay: int, nbytes: int, d_offsets: int, n_hay: int, uniform_len: int, d_counts: int,
                       min_matches: int, flags: int, d_rows: int, d_out_offsets: int, d_data: int) -> Tuple[int, int]:
    """acx_filter_rows_device: the device stage alone -- nbytes at d_hay (any address) cut by n_hay + 1 offsets at d_offsets
    or by uniform_len, n_hay counts at d_counts -> the kept rows' indexes, offsets and bytes at the three device addresses
    (room for n_hay words, n_hay + 1 words and round_up(nbytes, 16) bytes; 8-, 8- and 16-byte aligned); returns (n_rows,
    n_bytes); complete when it returns"""
    k, nb = ctypes.c_uint64(), ctypes.c_uint64()
    _check(lib().acx_filter_rows_device(d_hay or None, nbytes, d_offsets or None, n_hay, uniform_len, d_counts or None,
                                        min_matches, flags, d_rows or None, d_out_offsets or None, d_data or None,
                                        ctypes.byref(k), ctypes.byref(nb)))
    return int(k.value), int(nb.value)


class DeviceScores(_Result):
    """The result of Automaton.score / score_device (acx_scores_t): one int64 score per row of the batch, in HBM (on_device)
    or in host memory.  scores() copies them out; data_ptr() is where they lie (both wait for the device stage)."""
    _PREFIX = "scores"
    rows = _Size("rows")

    def data_ptr(self) -> int:
        return self._address("data")

    def scores(self) -> np.ndarray:
        return self._copy_out("copy", self.rows, np.int64)


def _weights(weights) -> np.ndarray:
    """one int32 per pattern, contiguous; ValueError for a weight outside |w| < 2^31"""
    w = np.ascontiguousarray(np.asarray(weights, dtype=np.int64).reshape(-1))
    if len(w) and int(np.abs(w).max()) >= 1 << 31:
        raise ValueError("a weight is outside int32: |w| < 2^31 is needed")
    return np.ascontiguousarray(w.astype(np.int32))


def score_host(matches, counts: Optional[Sequence[int]], weights) -> np.ndarray:
    """acx_score_host: rows of (pattern, start, end), counts[h] of them haystack h's (None: one row holds them all) -> the
    int64 score of every row, on the host, no device involved.  ValueError (code EINVAL) when the counts do not sum to the
    rows."""
    m, c, w = _records(matches), _u64(counts), _weights(weights)
    n_hay = 1 if c is None else len(c)
    out = np.zeros(n_hay, dtype=np.int64)
    _check(lib().acx_score_host(_ptr(m), len(m), _ptr(c, _SPARE.ctypes.data), n_hay, _ptr(w), len(w), _ptr(out)))
    return out


def score_rows_device(d_records: int, n: int, d_counts: int, n_hay: int, d_weights: int, n_weights: int, d_scores: int) -> None:
    """acx_score_rows_device: the device stage alone -- n records of 24 bytes at d_records, n_hay counts at d_counts, n_weights
    int32 weights at d_weights -> n_hay int64 scores at d_scores; complete when it returns"""
    _check(lib().acx_score_rows_device(d_records or None, n, d_counts or None, n_hay, d_weights or None, n_weights,
                                       d_scores or None))


class DeviceMasked(_Result):
    """The result of Automaton.mask / mask_device (acx_masked_t): the batch's bytes with every covered byte filled (or the
    0 / 1 mask), nbytes of them in the input's own layout, and the rows' offsets (rows + 1 int64 words from 0) -- in HBM
    (on_device) or in host memory.  data() / offsets() copy them out; data_ptr() / offsets_ptr() are where they lie (all
    wait for the device stage)."""
    _PREFIX = "masked"
    rows, nbytes = _Size("rows"), _Size("bytes")

    def data_ptr(self) -> int:
        return self._address("data")

    def offsets_ptr(self) -> int:
        return self._address("offsets")

    def data(self) -> np.ndarray:
        return self._copy_out("copy", self.nbytes, np.uint8)

    def offsets(self) -> np.ndarray:
        return self._copy_out("copy_offsets", self.rows + 1, np.int64)


def mask_host(hay, offsets: Optional[Sequence[int]], matches, counts: Optional[Sequence[int]], fill: int,
              flags: int = 0) -> np.ndarray:
    """acx_mask_host: the definition of the cover on the host, no device involved.  hay: bytes-like; offsets: n + 1 from 0 to
    len(hay), or None (one row); matches: rows of (pattern, start, end), counts[h] of them row h's (None: one row holds them
    all), every one clipped to its row.  Returns len(hay) uint8: `fill` where a match covers a byte, elsewhere the haystack's
    own byte (flags = 0) or 0 (MASK_ZERO).  ValueError (code EINVAL) for a bad flag, offsets that do not rise from 0 to
    len(hay) or counts that do not sum to the rows."""
    h = np.frombuffer(bytes(hay), dtype=np.uint8)
    m, c, off = _records(matches), _u64(counts), _u64(offsets)
    n_hay = (1 if c is None else len(c)) if off is None else len(off) - 1
    if c is not None and off is not None and len(c) != n_hay:
        raise ValueError("offsets needs len(counts) + 1 entries")
    out = np.zeros(max(len(h), 1), dtype=np.uint8)
    _check(lib().acx_mask_host(_ptr(h), len(h), None if off is None else off.ctypes.data, n_hay, _ptr(m), len(m),
                               _ptr(c, _SPARE.ctypes.data), fill, flags, out.ctypes.data))
    return out[:len(h)]


def mask_rows_device(d_hay: int, nbytes: int, d_offsets: int, n_hay: int, uniform_len: int, d_records: int, n: int,
                     d_counts: int, fill: int, flags: int, d_out: int) -> None:
    """acx_mask_rows_device: the device stage alone -- nbytes at d_hay (any address) cut by n_hay + 1 offsets at d_offsets, by
    uniform_len or not at all (one row), n records of 24 bytes at d_records, n_hay counts at d_counts -> exactly nbytes at
    d_out (any address; d_out == d_hay: in place); complete when it returns"""
    _check(lib().acx_mask_rows_device(d_hay or None, nbytes, d_offsets or None, n_hay, uniform_len, d_records or None, n,
                                      d_counts or None, fill, flags, d_out or None))


class DeviceTokenLabels(_Result):
    """The result of Automaton.tokens / tokens_device (acx_token_labels_t): per token the owner's pattern (int64, -1: none) and
    the begin flag (uint8) -- in HBM (on_device) or in host memory.  pattern() / begin() copy them out; pattern_ptr() /
    begin_ptr() are where they lie (all wait for the device stage)."""
    _PREFIX = "token_labels"
    count = _Size("count")

    def pattern_ptr(self) -> int:
        return self._address("pattern")

    def begin_ptr(self) -> int:
        return self._address("begin")

    def pattern(self) -> np.ndarray:
        return self._copy_out("copy_pattern", self.count, np.int64)

    def begin(self) -> np.ndarray:
        return self._copy_out("copy_begin", self.count, np.uint8)


def _i64(values) -> np.ndarray:
    """int64 words, contiguous (an empty array still has an address to give)"""
    a = np.ascontiguousarray(np.asarray(values, dtype=np.int64).reshape(-1))
    return a if a.size else np.zeros(1, dtype=np.int64)[:0]


def tokens_host(matches, counts: Optional[Sequence[int]], offsets: Optional[Sequence[int]], length: int, ts, te
                ) -> Tuple[np.ndarray, np.ndarray]:
    """acx_tokens_host: the definition of the token labels on the host, no device involved, any unit.  matches: rows of
    (pattern, start, end), counts[h] of them row h's (None: one row holds them all); offsets: n + 1 from 0 to length, or None
    (one row of `length` positions); ts, te: the tokens' global starts and ends.  Returns (pattern int64, begin uint8), an entry
    per token.  ValueError (code EINVAL) for token arrays that do not rise or pass `length`, offsets that do not rise from 0 to
    `length` or counts that do not sum to the rows."""
    m, c, off, s, e = _records(matches), _u64(counts), _u64(offsets), _i64(ts), _i64(te)
    if len(s) != len(e):
        raise ValueError("ts and te need one entry per token each")
    n_hay = (1 if c is None else len(c)) if off is None else len(off) - 1
    if c is not None and off is not None and len(c) != n_hay:
        raise ValueError("offsets needs len(counts) + 1 entries")
    pattern, begin = np.zeros(max(len(s), 1), dtype=np.int64), np.zeros(max(len(s), 1), dtype=np.uint8)
    _check(lib().acx_tokens_host(_ptr(m), len(m), _ptr(c, _SPARE.ctypes.data), n_hay, None if off is None else off.ctypes.data,
                                 length, s.ctypes.data, e.ctypes.data, len(s), pattern.ctypes.data, begin.ctypes.data))
    return pattern[:len(s)], begin[:len(s)]


def tokens_rows_device(nbytes: int, d_offsets: int, n_hay: int, uniform_len: int, d_records: int, n: int, d_counts: int,
                       d_ts: int, d_te: int, n_tokens: int, d_pattern: int, d_begin: int) -> None:
    """acx_tokens_rows_device: the device stage alone -- nbytes cut by n_hay + 1 offsets at d_offsets, by uniform_len or not at
    all (one row), n records of 24 bytes at d_records, n_hay counts at d_counts, n_tokens int64 words at d_ts and at d_te ->
    n_tokens int64 words at d_pattern and n_tokens bytes at d_begin (any address); complete when it returns"""
    _check(lib().acx_tokens_rows_device(nbytes, d_offsets or None, n_hay, uniform_len, d_records or None, n, d_counts or None,
                                        d_ts or None, d_te or None, n_tokens, d_pattern or None, d_begin or None))


class DeviceMatchesAt(_Result):
    """The result of Automaton.match_at / match_at_device (acx_at_t): per anchor the pattern that begins there and its end
    (int64, -1: none) -- or, overlapping, every such pattern as a CSR over the anchors (row_offsets: anchors + 1 int64 words) --
    in HBM (on_device) or in host memory.  pattern() / end() / row_offsets() copy them out; the _ptr() forms are where they lie
    (all wait for the device stage; row_offsets: None / 0 unless the call was overlapping)."""
    _PREFIX = "at"
    count, entries = _Size("count"), _Size("entries")

    def pattern_ptr(self) -> int:
        return self._address("pattern")

    def end_ptr(self) -> int:
        return self._address("end")

    def row_offsets_ptr(self) -> int:
        return self._address("row_offsets")

    def pattern(self) -> np.ndarray:
        return self._copy_out("copy", self.entries, np.int64, AT_PATTERN)

    def end(self) -> np.ndarray:
        return self._copy_out("copy", self.entries, np.int64, AT_END)

    def row_offsets(self) -> Optional[np.ndarray]:
        return self._copy_out("copy", self.count + 1, np.int64, AT_ROW_OFFSETS) if self.row_offsets_ptr() else None


def match_at_host(h: "HostAutomaton", hay, positions, *, offsets: Optional[Sequence[int]] = None, flags: int = 0,
                  match_kind: int = MATCH_STANDARD):
    """acx_match_at_host: the definition of the anchored search walked over a HostAutomaton's tables, no device involved.  hay:
    bytes-like; positions: ints in 0 .. len(hay) (None with AT_ROW_STARTS); offsets: n + 1 from 0 to len(hay), or None (one
    row).  Returns (pattern, end) with an entry per anchor, or -- AT_OVERLAPPING -- (pattern, end, row_offsets).  ValueError
    (code EINVAL) for offsets that do not rise from 0 to len(hay), a position outside the data, AT_FULL without
    AT_ROW_STARTS."""
    a = np.ascontiguousarray(np.frombuffer(bytes(hay), dtype=np.uint8))
    off = _u64(offsets)
    pos = None if positions is None else _i64(positions)
    n_hay = 0 if off is None else len(off) - 1
    n_pos = 0 if pos is None else len(pos)
    anchors = (n_hay if off is not None else 1) if flags & AT_ROW_STARTS else n_pos
    args = (h._h, a.ctypes.data if a.size else None, a.size, None if off is None else off.ctypes.data, n_hay,
            None if pos is None else pos.ctypes.data, n_pos, flags, match_kind)
    if not flags & AT_OVERLAPPING:
        pattern, end = np.zeros(anchors + 1, dtype=np.int64), np.zeros(anchors + 1, dtype=np.int64)
        _check(lib().acx_match_at_host(*args, pattern.ctypes.data, end.ctypes.data, None))
        return pattern[:anchors], end[:anchors]
    ro = np.zeros(anchors + 1, dtype=np.int64)
    _check(lib().acx_match_at_host(*args, None, None, ro.ctypes.data))  # (count only)
    n = int(ro[anchors])
    pattern, end = np.zeros(n + 1, dtype=np.int64), np.zeros(n + 1, dtype=np.int64)
    _check(lib().acx_match_at_host(*args, pattern.ctypes.data, end.ctypes.data, ro.ctypes.data))
    return pattern[:n], end[:n], ro


class DeviceSegments(_Result):
    """The result of Automaton.segment / segment_device (acx_seg_t): the pieces of a greedy segmentation by the dictionary --
    pattern (count int64 words, -1: an unknown unit), offsets (count + 1 global boundaries, the last one the data's length)
    and row_offsets (rows + 1: the pieces that begin before every row) -- in HBM (on_device) or in host memory.  pattern() /
    offsets() / row_offsets() copy them out; the _ptr() forms are where they lie (all wait for the device stage)."""
    _PREFIX = "seg"
    count, rows = _Size("count"), _Size("rows")

    def pattern_ptr(self) -> int:
        return self._address("pattern")

    def offsets_ptr(self) -> int:
        return self._address("offsets")

    def row_offsets_ptr(self) -> int:
        return self._address("row_offsets")

    def pattern(self) -> np.ndarray:
        return self._copy_out("copy", self.count, np.int64, SEG_PATTERN)

    def offsets(self) -> np.ndarray:
        return self._copy_out("copy", self.count + 1, np.int64, SEG_OFFSETS)

    def row_offsets(self) -> np.ndarray:
        return self._copy_out("copy", self.rows + 1, np.int64, SEG_ROW_OFFSETS)


def segment_host(h: "HostAutomaton", hay, *, offsets: Optional[Sequence[int]] = None, flags: int = 0,
                 match_kind: int = MATCH_STANDARD) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """acx_segment_host: the definition of the greedy segmentation walked over a HostAutomaton's tables, no device involved.
    hay: bytes-like; offsets: n + 1 from 0 to len(hay), or None (one row); flags: SEG_UTF8.  Returns (pattern, offsets,
    row_offsets): T, T + 1 and rows + 1 int64 words.  ValueError for an unknown flag or offsets that do not rise from 0 to
    len(hay) (code EINVAL) and for a pattern longer than 256 bytes (code ETOOBIG)."""
    a = np.ascontiguousarray(np.frombuffer(bytes(hay), dtype=np.uint8))
    off = _u64(offsets)
    n_hay = 0 if off is None else len(off) - 1
    rows = n_hay if off is not None else 1
    args = (h._h, a.ctypes.data if a.size else None, a.size, None if off is None else off.ctypes.data, n_hay, flags, match_kind)
    n = ctypes.c_uint64(0)
    _check(lib().acx_segment_host(*args, 0, None, None, None, ctypes.byref(n)))  # (count only)
    t = int(n.value)
    pattern, bounds, ro = np.zeros(t + 1, dtype=np.int64), np.zeros(t + 1, dtype=np.int64), np.zeros(rows + 1, dtype=np.int64)
    _check(lib().acx_segment_host(*args, t + 1, pattern.ctypes.data, bounds.ctypes.data, ro.ctypes.data, ctypes.byref(n)))
    return pattern[:t], bounds, ro


ASCII_WHITESPACE = b" \t\n\r\x0b\x0c"  # the default separators of wordpiece: what bytes.split() splits at
# the 32 ASCII bytes BERT's _is_punctuation accepts: 33-47, 58-64, 91-96, 123-126 (isolated=ASCII_PUNCTUATION: BertTokenizer)
ASCII_PUNCTUATION = bytes(list(range(33, 48)) + list(range(58, 65)) + list(range(91, 97)) + list(range(123, 127)))


def wp_classes(separators=None, isolated=None) -> np.ndarray:
    """the 256 classes acx_wordpiece* take: WP_SPACE for the byte values in `separators` (None: ASCII_WHITESPACE), WP_ALONE
    for those in `isolated` (None: none), WP_WORD for the rest.  Both bytes-like (a str is a TypeError); a byte value in
    both is a ValueError."""
    sets = []
    for name, given, default in (("separators", separators, ASCII_WHITESPACE), ("isolated", isolated, b"")):
        if isinstance(given, str):
            raise TypeError(f"{name} must be bytes-like, not str")
        sets.append(frozenset(bytes(default if given is None else given)))
    both = sets[0] & sets[1]
    if both:
        raise ValueError(f"byte value {min(both)} is a separator and isolated")
    cls = np.full(256, WP_WORD, dtype=np.uint8)
    cls[list(sets[0])] = WP_SPACE
    cls[list(sets[1])] = WP_ALONE
    return cls


def _wp_args(cls, prefix, max_word: int, unk_id: int) -> tuple:
    """(cls, prefix, prefix_len, max_word, unk_id, flags) of an acx_wordpiece* call, with what must stay alive behind it"""
    c = np.ascontiguousarray(np.asarray(cls, dtype=np.uint8).reshape(-1))
    if c.size != 256:
        raise ValueError("cls needs 256 entries")
    pre = np.frombuffer(bytes(prefix) + b"\0", dtype=np.uint8)
    return c.ctypes.data, pre.ctypes.data, len(pre) - 1, max_word, unk_id, 0, c, pre


class DeviceWordPieces(_Result):
    """The result of Automaton.wordpiece / wordpiece_device (acx_wp_t): the pieces of a WordPiece tokenization by the
    dictionary -- id, start, end (count int64 words each, global positions) and first (count bytes: 1 on the first piece of
    its word) and row_offsets (rows + 1: the pieces that begin before every row) -- in HBM (on_device) or in host memory.
    id() .. row_offsets() copy them out; the _ptr() forms are where they lie (all wait for the device stage)."""
    _PREFIX = "wp"
    count, rows = _Size("count"), _Size("rows")

    def id_ptr(self) -> int:
        return self._address("id")

    def start_ptr(self) -> int:
        return self._address("start")

    def end_ptr(self) -> int:
        return self._address("end")

    def first_ptr(self) -> int:
        return self._address("first")

    def row_offsets_ptr(self) -> int:
        return self._address("row_offsets")

    def id(self) -> np.ndarray:
        return self._copy_out("copy", self.count, np.int64, WP_ID)

    def start(self) -> np.ndarray:
        return self._copy_out("copy", self.count, np.int64, WP_START)

    def end(self) -> np.ndarray:
        return self._copy_out("copy", self.count, np.int64, WP_END)

    def first(self) -> np.ndarray:
        return self._copy_out("copy", self.count, np.uint8, WP_FIRST)

    def row_offsets(self) -> np.ndarray:
        return self._copy_out("copy", self.rows + 1, np.int64, WP_ROW_OFFSETS)


def wordpiece_host(h: "HostAutomaton", hay, cls, *, prefix=b"##", max_word: int = 100, unk_id: int = -1,
                   offsets: Optional[Sequence[int]] = None, match_kind: int = MATCH_LEFTMOST_LONGEST):
    """acx_wordpiece_host: the definition of the WordPiece tokenization walked over a HostAutomaton's tables, no device
    involved.  hay: bytes-like; cls: 256 classes (wp_classes); offsets: n + 1 from 0 to len(hay), or None (one row).  Returns
    (id, start, end, first, row_offsets): T, T, T int64 words, T bytes and rows + 1 int64 words.  ValueError (code EINVAL) for
    a class above 2, max_word outside 1 .. WP_MAX_WORD or offsets that do not rise from 0 to len(hay)."""
    a = np.ascontiguousarray(np.frombuffer(bytes(hay), dtype=np.uint8))
    off = _u64(offsets)
    n_hay = 0 if off is None else len(off) - 1
    rows = n_hay if off is not None else 1
    w = _wp_args(cls, prefix, max_word, unk_id)
    args = (h._h, a.ctypes.data if a.size else None, a.size, None if off is None else off.ctypes.data, n_hay, *w[:6], match_kind)
    n = ctypes.c_uint64(0)
    _check(lib().acx_wordpiece_host(*args, 0, None, None, None, None, None, ctypes.byref(n)))  # (count only)
    t = int(n.value)
    ids, start, end = (np.zeros(t + 1, dtype=np.int64) for _ in range(3))
    first, ro = np.zeros(t + 1, dtype=np.uint8), np.zeros(rows + 1, dtype=np.int64)
    _check(lib().acx_wordpiece_host(*args, t + 1, ids.ctypes.data, start.ctypes.data, end.ctypes.data, first.ctypes.data,
                                    ro.ctypes.data, ctypes.byref(n)))
    return ids[:t], start[:t], end[:t], first[:t], ro


class DeviceRows(_Result):
    """The result of split_rows / split_rows_device (acx_rows_t): the offsets that cut nbytes of delimited data into rows --
    rows + 1 int64 words from 0 to nbytes, in HBM (on_device, on `device`) or in host memory.  `rows` is valid at once;
    offsets() copies the words out and offsets_ptr() is where they lie (both wait for the device stage)."""
    _PREFIX = "rows"
    device, rows, nbytes = _Size("device"), _Size("count"), _Size("bytes")

    def offsets_ptr(self) -> int:
        return self._address("offsets")

    def offsets(self) -> np.ndarray:
        return self._copy_out("copy", self.rows + 1, np.int64)


def split_rows(hay, delimiter: int = 10) -> DeviceRows:
    """acx_split_rows: host bytes cut at every `delimiter` byte (the delimiter ends its row), a host result"""
    h = np.frombuffer(bytes(hay), dtype=np.uint8)
    out = ctypes.c_void_p()
    _check(lib().acx_split_rows(_ptr(h), len(h), delimiter, ctypes.byref(out)))
    return DeviceRows(out.value)


def split_rows_device(d_hay: int, nbytes: int, delimiter: int = 10) -> DeviceRows:
    """acx_split_rows_device: nbytes at d_hay (HBM, any address) -> the offsets in HBM on the same device; `rows` is known
    when it returns, the offsets may still be written (their accessors wait)"""
    out = ctypes.c_void_p()
    _check(lib().acx_split_rows_device(d_hay or None, nbytes, delimiter, ctypes.byref(out)))
    return DeviceRows(out.value)


def split_rows_host(hay, delimiter: int = 10, *, count_only: bool = False):
    """acx_split_rows_host: the definition on the host, no device involved -> rows + 1 int64 offsets (count_only: the number
    of rows)"""
    h = np.frombuffer(bytes(hay), dtype=np.uint8)
    p = _ptr(h)
    n = ctypes.c_uint64()
    _check(lib().acx_split_rows_host(p, len(h), delimiter, None, 0, ctypes.byref(n)))
    if count_only:
        return int(n.value)
    out = np.zeros(n.value + 1, dtype=np.int64)
    _check(lib().acx_split_rows_host(p, len(h), delimiter, out.ctypes.data, len(out), ctypes.byref(n)))
    return out


def split_rows_into_device(d_hay: int, nbytes: int, delimiter: int, d_offsets: int, capacity: int) -> int:
    """acx_split_rows_into_device: the device stage alone -- nbytes at d_hay (any address) -> rows + 1 int64 words at d_offsets
    (8-byte aligned, `capacity` words; 0: count only); complete when it returns.  Returns the number of rows; ValueError (code
    EINVAL) when the buffer is too small -- nothing was written then"""
    n = ctypes.c_uint64()
    _check(lib().acx_split_rows_into_device(d_hay or None, nbytes, delimiter, d_offsets or None, capacity, ctypes.byref(n)))
    return int(n.value)


class DeviceSpans(_BatchPartsResult):
    """The result of Automaton.spans / spans_device (acx_spans_t): the merged spans of a search's matches as two int64
    columns of `count` words and, for a batch, n_hay + 1 row offsets -- in HBM (on_device) or in host memory.  column()
    copies one out; data_ptr() is where it lies (both wait for the stage's last kernel)."""
    _PREFIX = "spans"
    count, rows = _Size("count"), _Size("rows")
    _PARTS = {SPAN_START: ("count", 0, np.int64), SPAN_END: ("count", 0, np.int64), SPAN_ROW_OFFSETS: ("rows", 1, np.int64)}
    column = _PartsResult._copy_part

    def start(self) -> np.ndarray:
        return self.column(SPAN_START)

    def end(self) -> np.ndarray:
        return self.column(SPAN_END)

    def row_offsets(self) -> Optional[np.ndarray]:
        return self.column(SPAN_ROW_OFFSETS) if self.batch else None


def spans_host(matches, counts: Optional[Sequence[int]], gap: int = 0):
    """acx_spans_host: the merge of a match list (rows of pattern, start, end whose ends do not decrease within a row; all
    rows behind one another, counts[h] of them row h's -- None: one row) on the host, no device involved ->
    (row_offsets, start, end): len(counts) + 1 (one row: 2) int64 offsets and the spans' int64 columns.  ValueError (code
    EINVAL) when the counts do not sum to the records or gap is 2**63 or more."""
    m, c = _records(matches), _u64(counts)
    n_hay = 1 if c is None else len(c)
    ro = np.zeros(n_hay + 1, dtype=np.int64)
    start = np.zeros(len(m) + 1, dtype=np.int64)
    end = np.zeros(len(m) + 1, dtype=np.int64)
    n = ctypes.c_uint64()
    _check(lib().acx_spans_host(_ptr(m), len(m), _ptr(c, _SPARE.ctypes.data), n_hay, gap, ro.ctypes.data, start.ctypes.data,
                                end.ctypes.data, ctypes.byref(n)))
    return ro, start[:n.value], end[:n.value]


def spans_rows_device(d_records: int, n: int, d_counts: int, n_hay: int, gap: int, d_row_offsets: int, d_start: int,
                      d_end: int) -> int:
    """acx_spans_rows_device: the device stage alone -- n records of 24 bytes at d_records, n_hay counts at d_counts ->
    n_hay + 1 int64 row offsets at d_row_offsets and the spans' columns at d_start / d_end (room for n words each; only the
    first S are written); complete when it returns.  Returns S, the number of spans."""
    s = ctypes.c_uint64()
    _check(lib().acx_spans_rows_device(d_records or None, n, d_counts or None, n_hay, gap, d_row_offsets or None,
                                       d_start or None, d_end or None, ctypes.byref(s)))
    return int(s.value)


ASCII_WORD_BYTES = b"0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ_abcdefghijklmnopqrstuvwxyz"  # the default word set: [0-9A-Za-z_]


def word_set(word_bytes) -> Optional[np.ndarray]:
    """the 32 bytes acx_*words* take for a word set: None (the default, ASCII [0-9A-Za-z_]) stays None; else any bytes-like
    of the byte values that count -- any length, duplicates allowed, empty allowed.  A str is a TypeError."""
    if word_bytes is None:
        return None
    if isinstance(word_bytes, str):
        raise TypeError("word_bytes must be bytes-like, not str")
    out = np.zeros(32, dtype=np.uint8)
    for v in bytes(word_bytes):
        out[v >> 3] |= 1 << (v & 7)
    return out


def words_host(hay, offsets: Optional[Sequence[int]], matches, counts: Optional[Sequence[int]], overlapping: bool = False,
               match_kind: int = MATCH_LEFTMOST_LONGEST, word_bytes=None):
    """acx_words_host: the definition of whole-word matching on the host, no device involved.  hay: bytes-like; offsets: n + 1
    from 0 to len(hay), or None (one row); matches: rows of (pattern, start, end) -- every occurrence, as an overlapping find
    reports them -- counts[h] of them row h's (None: one row holds them all).  Returns (records, counts): the surviving
    records as a MATCH_DTYPE array and the rows' new counts.  ValueError (code EINVAL) for a bad kind, offsets that do not
    rise from 0 to len(hay) or counts that do not sum to the records."""
    h = np.frombuffer(bytes(hay), dtype=np.uint8)
    m, c, off, ws = _records(matches), _u64(counts), _u64(offsets), word_set(word_bytes)
    n_hay = (1 if c is None else len(c)) if off is None else len(off) - 1
    if c is not None and off is not None and len(c) != n_hay:
        raise ValueError("offsets needs len(counts) + 1 entries")
    out = np.zeros(len(m) + 1, dtype=MATCH_DTYPE)
    oc = np.zeros(n_hay + 1, dtype=np.uint64)
    n = ctypes.c_uint64()
    _check(lib().acx_words_host(_ptr(h), len(h), None if off is None else off.ctypes.data, n_hay, _ptr(m), len(m),
                                _ptr(c, _SPARE.ctypes.data), int(overlapping), match_kind, None if ws is None else ws.ctypes.data,
                                out.ctypes.data, oc.ctypes.data, ctypes.byref(n)))
    return out[:n.value], oc[:n_hay]


def words_rows_device(d_hay: int, nbytes: int, d_offsets: int, n_hay: int, uniform_len: int, d_records: int, n: int,
                      d_counts: int, overlapping: bool, match_kind: int, word_bytes, d_out_records: int, d_out_counts: int) -> int:
    """acx_words_rows_device: the device stage alone -- nbytes at d_hay (any address) cut by n_hay + 1 offsets at d_offsets, by
    uniform_len or not at all (one row), n records of 24 bytes at d_records in the overlapping find's order, n_hay counts at
    d_counts -> the surviving records at d_out_records (room for n) and the rows' new counts at d_out_counts; complete when
    it returns.  Returns the number of surviving records."""
    ws = word_set(word_bytes)
    k = ctypes.c_uint64()
    _check(lib().acx_words_rows_device(d_hay or None, nbytes, d_offsets or None, n_hay, uniform_len, d_records or None, n,
                                       d_counts or None, int(overlapping), match_kind, None if ws is None else ws.ctypes.data,
                                       d_out_records or None, d_out_counts or None, ctypes.byref(k)))
    return int(k.value)


class DeviceSnippets(_BatchPartsResult):
    """The result of Automaton.snippets / snippets_device (acx_snippets_t): one snippet per match -- the bytes back to back
    (uint8), count + 1 offsets, the pattern and lead columns (int64) and, for a batch, n_hay + 1 row offsets -- in HBM
    (on_device) or in host memory.  part() copies one out; data_ptr() is where it lies (both wait for the gather)."""
    _PREFIX = "snippets"
    count, rows, nbytes = _Size("count"), _Size("rows"), _Size("nbytes")
    _PARTS = {SNIP_DATA: ("nbytes", 0, np.uint8), SNIP_OFFSETS: ("count", 1, np.int64), SNIP_PATTERN: ("count", 0, np.int64),
              SNIP_LEAD: ("count", 0, np.int64), SNIP_ROW_OFFSETS: ("rows", 1, np.int64)}
    part = _PartsResult._copy_part

    def data(self) -> np.ndarray:
        return self.part(SNIP_DATA)

    def offsets(self) -> np.ndarray:
        return self.part(SNIP_OFFSETS)

    def pattern(self) -> np.ndarray:
        return self.part(SNIP_PATTERN)

    def lead(self) -> np.ndarray:
        return self.part(SNIP_LEAD)

    def row_offsets(self) -> Optional[np.ndarray]:
        return self.part(SNIP_ROW_OFFSETS) if self.batch else None

    def tolist(self) -> list:
        """the snippets as bytes objects, in order"""
        d, o = self.data().tobytes(), self.offsets()
        return [d[o[i]:o[i + 1]] for i in range(self.count)]


def snippets_host(matches, counts: Optional[Sequence[int]], hay, offsets: Optional[Sequence[int]], context: int = 0,
                  flags: int = 0, *, sizes_only: bool = False):
    """acx_snippets_host: the definition of the cut on the host, no device involved.  matches: rows of (pattern, start, end),
    all rows behind one another, counts[h] of them row h's (None: one row); hay: bytes-like; offsets: n_hay + 1 from 0 to
    len(hay), or None (one row).  Returns (data, offsets, pattern, lead, row_offsets) as uint8 / int64 arrays -- the two-call
    form: sizes with null outputs, then the fill -- or the data's size alone with sizes_only.  ValueError (code EINVAL) for a
    bad flag, a context of 2**63 or more, counts that do not sum to the records or offsets that do not rise from 0 to
    len(hay)."""
    m, c, off = _records(matches), _u64(counts), _u64(offsets)
    h = np.frombuffer(bytes(hay), dtype=np.uint8)
    n_hay = (1 if c is None else len(c)) if off is None else len(off) - 1
    args = (_ptr(m), len(m), _ptr(c, _SPARE.ctypes.data), n_hay, _ptr(h), len(h), None if off is None else off.ctypes.data,
            context, flags)
    total = ctypes.c_uint64()
    _check(lib().acx_snippets_host(*args, None, None, None, None, None, ctypes.byref(total)))
    if sizes_only:
        return int(total.value)
    data = np.zeros(total.value, dtype=np.uint8)
    o = np.zeros(len(m) + 1, dtype=np.int64)
    pat = np.zeros(len(m), dtype=np.int64)
    lead = np.zeros(len(m), dtype=np.int64)
    ro = np.zeros(n_hay + 1, dtype=np.int64)
    _check(lib().acx_snippets_host(*args, o.ctypes.data, _ptr(pat), _ptr(lead), ro.ctypes.data, _ptr(data), ctypes.byref(total)))
    return data, o, pat, lead, ro


def snippets_rows_device(d_records: int, n: int, d_counts: int, n_hay: int, d_hay: int, nbytes: int, d_offsets: int,
                         uniform_len: int, context: int, flags: int, d_out_offsets: int, d_pattern: int, d_lead: int,
                         d_row_offsets: int, d_data: int, data_capacity: int):
    """acx_snippets_rows_device: the device stage alone -- n records of 24 bytes at d_records, n_hay counts at d_counts, nbytes
    at d_hay (any address) cut by n_hay + 1 offsets at d_offsets, by uniform_len or not at all (one row) -> n + 1 offsets, n
    patterns, n leads, n_hay + 1 row offsets and the snippets' bytes at d_data (16-byte aligned, data_capacity bytes);
    complete when it returns.  Returns (code, total): code is 0 or ETOOBIG (total > data_capacity: d_data is untouched);
    every other failure raises."""
    t = ctypes.c_uint64()
    rc = lib().acx_snippets_rows_device(d_records or None, n, d_counts or None, n_hay, d_hay or None, nbytes, d_offsets or None,
                                        uniform_len, context, flags, d_out_offsets or None, d_pattern or None, d_lead or None,
                                        d_row_offsets or None, d_data or None, data_capacity, ctypes.byref(t))
    if rc != ETOOBIG:
        _check(rc)
    return rc, int(t.value)


def splice_host(hay, matches, replace_with: Sequence[bytes]) -> bytes:
    """acx_splice_host: `hay` with every match (pattern, start, end) replaced by replace_with[pattern] -- on the host,
    no device involved.  ValueError (code EINVAL) for unsorted, overlapping or out-of-range matches."""
    h = np.frombuffer(bytes(hay), dtype=np.uint8)
    m = _records(matches)
    blob, off = pack(replace_with)
    n = ctypes.c_uint64()
    args = (_ptr(h), h.size, _ptr(m), len(m), blob.ctypes.data, off.ctypes.data, len(replace_with))
    _check(lib().acx_splice_host(*args, None, ctypes.byref(n)))
    out = np.empty(int(n.value) + 1, dtype=np.uint8)
    _check(lib().acx_splice_host(*args, out.ctypes.data, ctypes.byref(n)))
    return out[:int(n.value)].tobytes()


def _take_matches(ptr: Optional[int], n: int) -> np.ndarray:
    """The library-owned host array of an acx_find* call as a numpy structured array, without a
    copy (a large result sits in pinned host memory): acx_free_matches runs when the array and
    every view of it are gone."""
    if not n:
        return np.empty(0, dtype=MATCH_DTYPE)
    buf = (ctypes.c_uint8 * (n * 24)).from_address(ptr)
    weakref.finalize(buf, lib().acx_free_matches, ptr)
    return np.frombuffer(buf, dtype=MATCH_DTYPE)


# How a stage's host form takes ONE haystack that is no batch (offsets = NULL): (a padded copy?, n_hay).  The C stages differ
# here, so the binding states it per stage and unifies nothing.
_SINGLE_ROW = (True, 1)     # filter, score, filter_scored, mask: a copy with one \0 behind it, a batch of one row -- the stage
#                             reads n_hay with offsets == NULL
_SINGLE_PADDED = (True, 0)  # spans, snippets: the same copy, n_hay = 0 -- the stage derives rows = offsets ? n_hay : 1
_SINGLE_OWN = (False, 0)    # replace, summarize, find_columns: the caller's own bytes (NULL for none), n_hay = 0 -- as find()


def _host_arg(haystacks, single=None, convention=None) -> tuple:
    """the host haystack argument (hay, len, offsets, n_hay) of a batch -- a sequence, packed -- or of one buffer by its
    stage's _SINGLE_* convention, with what must stay alive until the call is over behind it"""
    if single is None:
        blob, off = pack(haystacks)
        return blob.ctypes.data, int(off[-1]), off.ctypes.data, len(haystacks), blob, off
    padded, n_hay = convention
    if padded:
        a = np.frombuffer(bytes(single) + b"\0", dtype=np.uint8)
        return a.ctypes.data, len(single), None, n_hay, a
    a = np.ascontiguousarray(np.frombuffer(single, dtype=np.uint8) if not isinstance(single, np.ndarray) else single)
    return a.ctypes.data if a.size else None, a.size, None, n_hay, a


def _batched(d_offsets: int, uniform_len: int) -> bool:
    """a device call is a batch when its rows are cut by offsets or by a uniform length"""
    return bool(uniform_len or d_offsets)


def _rows(d_offsets: int, n_hay: int, uniform_len: int) -> int:
    """the rows of a device call: one haystack that is no batch is one row"""
    return n_hay if _batched(d_offsets, uniform_len) else 1


class Automaton(_Handle):
    """acx_automaton_t: compiled patterns + device tables."""
    _FREE = "acx_free_automaton"
    close = _Handle.free

    def __init__(self, patterns: Sequence[bytes], match_kind: int = MATCH_STANDARD,
                 implementation: int = IMPL_AUTO, kernel: Optional[int] = None, ascii_case_insensitive: bool = False):
        blob, off = pack(patterns)
        h = ctypes.c_void_p()
        flags = BUILD_ASCII_CASE_INSENSITIVE if ascii_case_insensitive else 0
        _check(lib().acx_build_ex(blob.ctypes.data, off.ctypes.data, len(patterns), match_kind,
                                  implementation, flags, ctypes.byref(h)))
        self._h = h.value
        if kernel is not None:
            self.set_kernel(kernel)

    @property
    def info(self) -> Info:
        i = Info()
        _check(lib().acx_automaton_info(self._h, ctypes.byref(i)))
        return i

    @property
    def max_pattern_len(self) -> int:
        return int(self.info.max_pattern_len)

    def set_kernel(self, kernel: int) -> None:
        _check(lib().acx_set_kernel(self._h, kernel))

    # ---- host-memory entry points.  find, find_batch and find_device are what bench.py times, a few microseconds a call:
    # they call the library directly and go through none of the frames below
    def find(self, hay, overlapping: bool = False, codepoints: bool = False) -> np.ndarray:
        a = np.frombuffer(hay, dtype=np.uint8) if not isinstance(hay, np.ndarray) else hay
        a = np.ascontiguousarray(a)
        out, n = ctypes.c_void_p(), ctypes.c_uint64()
        _check(lib().acx_find(self._h, a.ctypes.data if a.size else None, a.size,
                              int(overlapping), int(codepoints), ctypes.byref(out),
                              ctypes.byref(n)))
        return _take_matches(out.value, n.value)

    def find_tuples(self, hay, overlapping: bool = False,
                    codepoints: bool = False) -> List[Tuple[int, int, int]]:
        return [(int(p), int(s), int(e)) for (p, s, e) in self.find(hay, overlapping, codepoints)]

    def find_batch(self, haystacks: Sequence[bytes], overlapping: bool = False,
                   codepoints: bool = False) -> Tuple[np.ndarray, np.ndarray]:
        blob, off = pack(haystacks)
        out, n = ctypes.c_void_p(), ctypes.c_uint64()
        counts = np.zeros(len(haystacks), dtype=np.uint64)
        _check(lib().acx_find_batch(self._h, blob.ctypes.data, off.ctypes.data, len(haystacks),
                                    int(overlapping), int(codepoints), ctypes.byref(out),
                                    ctypes.byref(n), counts.ctypes.data))
        return _take_matches(out.value, n.value), counts

    def replicate(self, device: int) -> "Automaton":
        """the same automaton compiled again on another device (acx_replicate)"""
        h = ctypes.c_void_p()
        _check(lib().acx_replicate(self._h, device, ctypes.byref(h)))
        r = Automaton.__new__(Automaton)
        r._h = h.value
        return r

    def find_batch_multi(self, others: Sequence["Automaton"], haystacks: Sequence[bytes], overlapping: bool = False,
                         codepoints: bool = False) -> Tuple[np.ndarray, np.ndarray]:
        """acx_find_batch_multi over [self] + others: one host thread per handle, contiguous ranges of
        haystacks, identical to find_batch on one handle"""
        hs = [self] + list(others)
        arr = (ctypes.c_void_p * len(hs))(*[h._h for h in hs])
        blob, off = pack(haystacks)
        out, n = ctypes.c_void_p(), ctypes.c_uint64()
        counts = np.zeros(len(haystacks), dtype=np.uint64)
        _check(lib().acx_find_batch_multi(arr, len(hs), blob.ctypes.data, off.ctypes.data, len(haystacks),
                                          int(overlapping), int(codepoints), ctypes.byref(out), ctypes.byref(n),
                                          counts.ctypes.data))
        return _take_matches(out.value, n.value), counts

    # ---- device-resident entry point
    def find_device(self, d_ptr: int, nbytes: int, *, d_offsets: int = 0, n_hay: int = 0,
                    uniform_len: int = 0, overlapping: bool = False,
                    codepoints: bool = False) -> DeviceResult:
        out = ctypes.c_void_p()
        _check(lib().acx_find_device(self._h, d_ptr, nbytes, d_offsets or None, n_hay,
                                     uniform_len, int(overlapping), int(codepoints),
                                     ctypes.byref(out)))
        return DeviceResult(out.value, n_hay if (uniform_len or d_offsets) else 0)

    # ---- the stages behind a find.  Every one has a host form, acx_<stage>(a, hay, len, offsets, n_hay, *tail, out), and a
    # device form, acx_<stage>_device(a, d_hay, len, d_offsets, n_hay, uniform_len, *tail, out): a method below states the
    # stage, its tail and its result class, and for the host form how the stage takes ONE haystack (_SINGLE_*)
    def _host(self, stage: str, hay: tuple, tail: tuple, result, *more):
        """the host forms' frame: hay = _host_arg(...) (it keeps the haystack's memory alive until the call is over)"""
        out = ctypes.c_void_p()
        _check(getattr(lib(), "acx_" + stage)(self._h, *hay[:4], *tail, ctypes.byref(out)))
        return result(out.value, *more)

    def _device(self, stage: str, dev: tuple, tail: tuple, result, *more):
        """the device forms' frame: dev = (d_ptr, nbytes, d_offsets, n_hay, uniform_len); an address of 0 is NULL"""
        d_ptr, nbytes, d_offsets, n_hay, uniform_len = dev
        out = ctypes.c_void_p()
        _check(getattr(lib(), f"acx_{stage}_device")(self._h, d_ptr or None, nbytes, d_offsets or None, n_hay, uniform_len, *tail,
                                                     ctypes.byref(out)))
        return result(out.value, *more)

    # ---- replacement (acx_replace / acx_replace_device)
    def replace(self, hay, replace_with: Sequence[bytes]) -> bytes:
        """every non-overlapping match of `hay` replaced by replace_with[pattern]"""
        blob, off = pack(replace_with)
        r = self._host("replace", _host_arg(None, hay, _SINGLE_OWN), (blob.ctypes.data, off.ctypes.data, len(replace_with)),
                       DeviceReplaced, 1)
        try:
            return r.download()
        finally:
            r.free()

    def replace_batch(self, haystacks: Sequence[bytes], replace_with: Sequence[bytes]) -> List[bytes]:
        """[self.replace(h, replace_with) for h in haystacks] in one call"""
        blob, off = pack(replace_with)
        r = self._host("replace", _host_arg(haystacks), (blob.ctypes.data, off.ctypes.data, len(replace_with)), DeviceReplaced,
                       len(haystacks))
        try:
            whole, bounds = r.download(), r.offsets()
        finally:
            r.free()
        return [whole[int(bounds[i]):int(bounds[i + 1])] for i in range(len(haystacks))]

    def replace_device(self, d_ptr: int, nbytes: int, replace_with: Sequence[bytes], *, d_offsets: int = 0,
                       n_hay: int = 0, uniform_len: int = 0) -> DeviceReplaced:
        """the haystack in HBM searched and spliced there; the output stays in HBM"""
        blob, off = pack(replace_with)
        return self._device("replace", (d_ptr, nbytes, d_offsets, n_hay, uniform_len),
                            (blob.ctypes.data, off.ctypes.data, len(replace_with)), DeviceReplaced,
                            _rows(d_offsets, n_hay, uniform_len))

    # ---- summaries (acx_summarize / acx_summarize_device)
    def summarize(self, hay, what: int = SUM_FIRST | SUM_BY_PATTERN, overlapping: bool = False,
                  codepoints: bool = False) -> DeviceSummary:
        """is there a match, the first one, how many, how many per pattern -- without the match list"""
        return self._host("summarize", _host_arg(None, hay, _SINGLE_OWN), (int(overlapping), int(codepoints), what),
                          DeviceSummary, 1, int(self.info.n_patterns))

    def summarize_batch(self, haystacks: Sequence[bytes], what: int = SUM_FIRST | SUM_BY_PATTERN, overlapping: bool = False,
                        codepoints: bool = False) -> DeviceSummary:
        """the same per haystack (by_pattern: over the whole batch); entry i equals summarize(haystacks[i])"""
        return self._host("summarize", _host_arg(haystacks), (int(overlapping), int(codepoints), what), DeviceSummary,
                          len(haystacks), int(self.info.n_patterns))

    def summarize_device(self, d_ptr: int, nbytes: int, what: int = SUM_FIRST | SUM_BY_PATTERN, *, d_offsets: int = 0,
                         n_hay: int = 0, uniform_len: int = 0, overlapping: bool = False,
                         codepoints: bool = False) -> DeviceSummary:
        """the haystack in HBM searched and its result reduced there; the summaries stay in HBM until they are asked for"""
        return self._device("summarize", (d_ptr, nbytes, d_offsets, n_hay, uniform_len), (int(overlapping), int(codepoints), what),
                            DeviceSummary, _rows(d_offsets, n_hay, uniform_len), int(self.info.n_patterns))

    # ---- matches as columns (acx_find_columns / acx_find_columns_device)
    def find_columns(self, hay, overlapping: bool = False, codepoints: bool = False) -> DeviceColumns:
        """find()'s matches as three int64 columns in host memory"""
        return self._host("find_columns", _host_arg(None, hay, _SINGLE_OWN), (int(overlapping), int(codepoints)), DeviceColumns,
                          False)

    def find_columns_batch(self, haystacks: Sequence[bytes], overlapping: bool = False,
                           codepoints: bool = False) -> DeviceColumns:
        """find_batch()'s matches as columns in host memory, with the row offsets of the haystacks"""
        return self._host("find_columns", _host_arg(haystacks), (int(overlapping), int(codepoints)), DeviceColumns, True)

    def find_columns_device(self, d_ptr: int, nbytes: int, *, d_offsets: int = 0, n_hay: int = 0, uniform_len: int = 0,
                            overlapping: bool = False, codepoints: bool = False) -> DeviceColumns:
        """the haystack in HBM searched and its matches split into columns there; nothing but the total crosses the bus"""
        return self._device("find_columns", (d_ptr, nbytes, d_offsets, n_hay, uniform_len), (int(overlapping), int(codepoints)),
                            DeviceColumns, _batched(d_offsets, uniform_len))

    # ---- per-haystack pattern counts as a CSR matrix (acx_tally / acx_tally_device)
    def tally(self, haystacks: Sequence[bytes], overlapping: bool = False) -> DeviceTally:
        """which patterns occur in which haystack, and how often: host haystacks, a host result"""
        return self._host("tally", _host_arg(haystacks), (int(overlapping),), DeviceTally)

    def tally_device(self, d_ptr: int, nbytes: int, *, d_offsets: int = 0, n_hay: int = 0, uniform_len: int = 0,
                     overlapping: bool = False) -> DeviceTally:
        """the batch in HBM searched and reduced there; nothing but nnz crosses the bus"""
        return self._device("tally", (d_ptr, nbytes, d_offsets, n_hay, uniform_len), (int(overlapping),), DeviceTally)

    # ---- keep or drop the rows of a batch by match (acx_filter / acx_filter_device)
    def filter(self, haystacks: Optional[Sequence[bytes]], overlapping: bool = False, min_matches: int = 1, flags: int = 0, *,
               single: Optional[bytes] = None) -> DeviceFiltered:
        """the kept rows of host haystacks, a host result; single=...: one haystack that is no batch (offsets = NULL)"""
        return self._host("filter", _host_arg(haystacks, single, _SINGLE_ROW), (int(overlapping), min_matches, flags),
                          DeviceFiltered)

    def filter_device(self, d_ptr: int, nbytes: int, *, d_offsets: int = 0, n_hay: int = 0, uniform_len: int = 0,
                      overlapping: bool = False, min_matches: int = 1, flags: int = 0) -> DeviceFiltered:
        """the batch in HBM searched and compacted there; nothing but the result's two sizes crosses the bus"""
        return self._device("filter", (d_ptr, nbytes, d_offsets, n_hay, uniform_len), (int(overlapping), min_matches, flags),
                            DeviceFiltered)

    # ---- per-pattern weights: a score per row, and the row filter by score (acx_score* / acx_filter_scored*)
    def score(self, haystacks: Optional[Sequence[bytes]], weights, overlapping: bool = False, *,
              single: Optional[bytes] = None) -> DeviceScores:
        """every row's sum of weights[pattern] over its matches: host haystacks, a host result; single=...: one haystack
        that is no batch (offsets = NULL)"""
        w = _weights(weights)
        return self._host("score", _host_arg(haystacks, single, _SINGLE_ROW), (int(overlapping), w.ctypes.data, len(w)),
                          DeviceScores)

    def score_device(self, d_ptr: int, nbytes: int, weights, *, d_offsets: int = 0, n_hay: int = 0, uniform_len: int = 0,
                     overlapping: bool = False) -> DeviceScores:
        """the batch in HBM searched and scored there; the scores stay there"""
        w = _weights(weights)
        return self._device("score", (d_ptr, nbytes, d_offsets, n_hay, uniform_len), (int(overlapping), w.ctypes.data, len(w)),
                            DeviceScores)

    def filter_scored(self, haystacks: Optional[Sequence[bytes]], weights, overlapping: bool = False, min_score: int = 1,
                      flags: int = 0, *, single: Optional[bytes] = None) -> DeviceFiltered:
        """filter() with a row matched when its score is at least min_score"""
        w = _weights(weights)
        return self._host("filter_scored", _host_arg(haystacks, single, _SINGLE_ROW),
                          (int(overlapping), w.ctypes.data, len(w), min_score, flags), DeviceFiltered)

    def filter_scored_device(self, d_ptr: int, nbytes: int, weights, *, d_offsets: int = 0, n_hay: int = 0,
                             uniform_len: int = 0, overlapping: bool = False, min_score: int = 1,
                             flags: int = 0) -> DeviceFiltered:
        """filter_device() with a row matched when its score is at least min_score"""
        w = _weights(weights)
        return self._device("filter_scored", (d_ptr, nbytes, d_offsets, n_hay, uniform_len),
                            (int(overlapping), w.ctypes.data, len(w), min_score, flags), DeviceFiltered)

    # ---- cover / mask: every byte a match covers becomes `fill` (acx_mask*)
    def mask(self, haystacks: Optional[Sequence[bytes]], fill: int, overlapping: bool = False, flags: int = 0, *,
             single: Optional[bytes] = None) -> DeviceMasked:
        """host haystacks with their matches' bytes filled, a host result; single=...: one haystack that is no batch
        (offsets = NULL)"""
        return self._host("mask", _host_arg(haystacks, single, _SINGLE_ROW), (int(overlapping), fill, flags), DeviceMasked)

    def mask_device(self, d_ptr: int, nbytes: int, fill: int, *, d_offsets: int = 0, n_hay: int = 0, uniform_len: int = 0,
                    overlapping: bool = False, flags: int = 0) -> DeviceMasked:
        """the batch in HBM searched and painted there; the output stays there"""
        return self._device("mask", (d_ptr, nbytes, d_offsets, n_hay, uniform_len), (int(overlapping), fill, flags), DeviceMasked)

    # ---- merged spans: the union of the matches as start / end columns (acx_spans*)
    def spans(self, haystacks: Optional[Sequence[bytes]], overlapping: bool = False, codepoints: bool = False, gap: int = 0, *,
              single: Optional[bytes] = None) -> DeviceSpans:
        """host haystacks' merged spans, a host result; single=...: one haystack that is no batch (offsets = NULL, no row
        offsets)"""
        return self._host("spans", _host_arg(haystacks, single, _SINGLE_PADDED), (int(overlapping), int(codepoints), gap),
                          DeviceSpans, single is None)

    def spans_device(self, d_ptr: int, nbytes: int, *, d_offsets: int = 0, n_hay: int = 0, uniform_len: int = 0,
                     overlapping: bool = False, codepoints: bool = False, gap: int = 0) -> DeviceSpans:
        """the haystacks in HBM searched and their matches merged there; nothing but the number of spans crosses the bus"""
        return self._device("spans", (d_ptr, nbytes, d_offsets, n_hay, uniform_len), (int(overlapping), int(codepoints), gap),
                            DeviceSpans, _batched(d_offsets, uniform_len))

    # ---- snippets: the matched text and its context as the caller's own bytes (acx_snippets*)
    def snippets(self, haystacks: Optional[Sequence[bytes]], overlapping: bool = False, context: int = 0, flags: int = 0, *,
                 single: Optional[bytes] = None) -> DeviceSnippets:
        """host haystacks' snippets, a host result; single=...: one haystack that is no batch (offsets = NULL, no row
        offsets)"""
        return self._host("snippets", _host_arg(haystacks, single, _SINGLE_PADDED), (int(overlapping), context, flags),
                          DeviceSnippets, single is None)

    def snippets_device(self, d_ptr: int, nbytes: int, *, d_offsets: int = 0, n_hay: int = 0, uniform_len: int = 0,
                        overlapping: bool = False, context: int = 0, flags: int = 0) -> DeviceSnippets:
        """the haystacks in HBM searched and their matches cut there; nothing but the data's size crosses the bus"""
        return self._device("snippets", (d_ptr, nbytes, d_offsets, n_hay, uniform_len), (int(overlapping), context, flags),
                            DeviceSnippets, _batched(d_offsets, uniform_len))

    # ---- whole words: the occurrences whose neighbour bytes are no word bytes, resolved by a match kind (acx_find_words* /
    # acx_filter_words*; the handle must be a Standard one)
    def find_words(self, haystacks: Optional[Sequence[bytes]], overlapping: bool = False,
                   match_kind: int = MATCH_LEFTMOST_LONGEST, word_bytes=None, *, single: Optional[bytes] = None) -> DeviceColumns:
        """host haystacks' whole-word matches as columns, a host result; single=...: one haystack that is no batch"""
        ws = word_set(word_bytes)
        return self._host("find_words", _host_arg(haystacks, single, _SINGLE_OWN),
                          (int(overlapping), match_kind, None if ws is None else ws.ctypes.data), DeviceColumns, single is None)

    def find_words_device(self, d_ptr: int, nbytes: int, *, d_offsets: int = 0, n_hay: int = 0, uniform_len: int = 0,
                          overlapping: bool = False, match_kind: int = MATCH_LEFTMOST_LONGEST, word_bytes=None) -> DeviceColumns:
        """the haystacks in HBM searched, tested and resolved there; nothing but two counts crosses the bus"""
        ws = word_set(word_bytes)
        return self._device("find_words", (d_ptr, nbytes, d_offsets, n_hay, uniform_len),
                            (int(overlapping), match_kind, None if ws is None else ws.ctypes.data), DeviceColumns,
                            _batched(d_offsets, uniform_len))

    def filter_words(self, haystacks: Optional[Sequence[bytes]], overlapping: bool = False,
                     match_kind: int = MATCH_LEFTMOST_LONGEST, word_bytes=None, min_matches: int = 1, flags: int = 0, *,
                     single: Optional[bytes] = None) -> DeviceFiltered:
        """filter() with a row's matches counted by whole word"""
        ws = word_set(word_bytes)
        return self._host("filter_words", _host_arg(haystacks, single, _SINGLE_ROW),
                          (int(overlapping), match_kind, None if ws is None else ws.ctypes.data, min_matches, flags), DeviceFiltered)

    def filter_words_device(self, d_ptr: int, nbytes: int, *, d_offsets: int = 0, n_hay: int = 0, uniform_len: int = 0,
                            overlapping: bool = False, match_kind: int = MATCH_LEFTMOST_LONGEST, word_bytes=None,
                            min_matches: int = 1, flags: int = 0) -> DeviceFiltered:
        """filter_device() with a row's matches counted by whole word"""
        ws = word_set(word_bytes)
        return self._device("filter_words", (d_ptr, nbytes, d_offsets, n_hay, uniform_len),
                            (int(overlapping), match_kind, None if ws is None else ws.ctypes.data, min_matches, flags),
                            DeviceFiltered)

    # ---- token labels: the matches mapped onto token boundaries (acx_tokens*)
    def tokens(self, haystacks: Optional[Sequence[bytes]], ts, te, overlapping: bool = False, codepoints: bool = False, *,
               single: Optional[bytes] = None) -> DeviceTokenLabels:
        """host haystacks' token labels, a host result; ts, te: the tokens' global starts and ends (bytes, or characters with
        codepoints); single=...: one haystack that is no batch (offsets = NULL)"""
        s, e = _i64(ts), _i64(te)
        if len(s) != len(e):
            raise ValueError("ts and te need one entry per token each")
        return self._host("tokens", _host_arg(haystacks, single, _SINGLE_ROW),
                          (int(overlapping), int(codepoints), s.ctypes.data, e.ctypes.data, len(s)), DeviceTokenLabels)

    def tokens_device(self, d_ptr: int, nbytes: int, d_ts: int, d_te: int, n_tokens: int, *, d_offsets: int = 0, n_hay: int = 0,
                      uniform_len: int = 0, overlapping: bool = False) -> DeviceTokenLabels:
        """the batch in HBM searched and its matches mapped onto the tokens there; the columns stay there"""
        return self._device("tokens", (d_ptr, nbytes, d_offsets, n_hay, uniform_len),
                            (int(overlapping), d_ts or None, d_te or None, n_tokens), DeviceTokenLabels)

    # ---- the anchored search: which pattern begins exactly here (acx_match_at*)
    def match_at(self, haystacks: Optional[Sequence[bytes]], positions, flags: int = 0, codepoints: bool = False, *,
                 single: Optional[bytes] = None) -> DeviceMatchesAt:
        """host data -- a sequence of rows, or single=...: one haystack that is no batch (offsets = NULL) -- and host positions
        (global, in bytes or, with codepoints, characters; None with AT_ROW_STARTS), a host result"""
        pos = None if positions is None else _i64(positions)
        hay = _host_arg(haystacks, single, _SINGLE_OWN)
        out = ctypes.c_void_p()
        _check(lib().acx_match_at(self._h, *hay[:4], None if pos is None else pos.ctypes.data, 0 if pos is None else len(pos),
                                  flags, int(codepoints), ctypes.byref(out)))
        return DeviceMatchesAt(out.value)

    def match_at_device(self, d_ptr: int, nbytes: int, d_positions: int, n_pos: int, flags: int = 0, *, d_offsets: int = 0,
                        n_hay: int = 0, uniform_len: int = 0) -> DeviceMatchesAt:
        """everything in HBM; the columns stay there"""
        out = ctypes.c_void_p()
        _check(lib().acx_match_at_device(self._h, d_ptr or None, nbytes, d_offsets or None, n_hay, uniform_len,
                                         d_positions or None, n_pos, flags, ctypes.byref(out)))
        return DeviceMatchesAt(out.value)

    def match_at_into_device(self, d_ptr: int, nbytes: int, d_positions: int, n_pos: int, d_pattern: int, d_end: int,
                             flags: int = 0, *, d_offsets: int = 0, n_hay: int = 0, uniform_len: int = 0) -> None:
        """the raw form: an int64 word per anchor at d_pattern and at d_end, complete when it returns"""
        _check(lib().acx_match_at_into_device(self._h, d_ptr or None, nbytes, d_offsets or None, n_hay, uniform_len,
                                              d_positions or None, n_pos, flags, d_pattern or None, d_end or None))

    # ---- greedy segmentation by the dictionary: MaxMatch on the device (acx_segment*)
    def segment(self, haystacks: Optional[Sequence[bytes]], flags: int = 0, codepoints: bool = False, *,
                single: Optional[bytes] = None) -> DeviceSegments:
        """host data -- a sequence of rows, or single=...: one haystack that is no batch (offsets = NULL) -- a host result;
        codepoints: the boundaries in characters (implies SEG_UTF8)"""
        hay = _host_arg(haystacks, single, _SINGLE_OWN)
        out = ctypes.c_void_p()
        _check(lib().acx_segment(self._h, *hay[:4], flags, int(codepoints), ctypes.byref(out)))
        return DeviceSegments(out.value)

    def segment_device(self, d_ptr: int, nbytes: int, flags: int = 0, *, d_offsets: int = 0, n_hay: int = 0,
                       uniform_len: int = 0) -> DeviceSegments:
        """everything in HBM; the columns stay there"""
        out = ctypes.c_void_p()
        _check(lib().acx_segment_device(self._h, d_ptr or None, nbytes, d_offsets or None, n_hay, uniform_len, flags,
                                        ctypes.byref(out)))
        return DeviceSegments(out.value)

    def segment_into_device(self, d_ptr: int, nbytes: int, cap: int, d_pattern: int, d_offsets_out: int, d_row_offsets: int,
                            flags: int = 0, *, d_offsets: int = 0, n_hay: int = 0, uniform_len: int = 0) -> int:
        """the raw form: T is returned; cap, cap + 1 and rows + 1 int64 words at the three addresses are written only when
        T <= cap, and are complete when it returns"""
        n = ctypes.c_uint64(0)
        _check(lib().acx_segment_into_device(self._h, d_ptr or None, nbytes, d_offsets or None, n_hay, uniform_len, flags, cap,
                                             d_pattern or None, d_offsets_out or None, d_row_offsets or None, ctypes.byref(n)))
        return int(n.value)

    # ---- WordPiece tokenization by the dictionary on the device (acx_wordpiece*)
    def wordpiece(self, haystacks: Optional[Sequence[bytes]], cls, *, prefix=b"##", max_word: int = 100, unk_id: int = -1,
                  codepoints: bool = False, single: Optional[bytes] = None) -> DeviceWordPieces:
        """host data -- a sequence of rows, or single=...: one haystack that is no batch (offsets = NULL) -- a host result;
        cls: 256 classes (wp_classes); codepoints: start and end in characters"""
        hay = _host_arg(haystacks, single, _SINGLE_OWN)
        w = _wp_args(cls, prefix, max_word, unk_id)
        out = ctypes.c_void_p()
        _check(lib().acx_wordpiece(self._h, *hay[:4], *w[:6], int(codepoints), ctypes.byref(out)))
        return DeviceWordPieces(out.value)

    def wordpiece_device(self, d_ptr: int, nbytes: int, cls, *, prefix=b"##", max_word: int = 100, unk_id: int = -1,
                         d_offsets: int = 0, n_hay: int = 0, uniform_len: int = 0) -> DeviceWordPieces:
        """everything in HBM; the columns stay there"""
        w = _wp_args(cls, prefix, max_word, unk_id)
        out = ctypes.c_void_p()
        _check(lib().acx_wordpiece_device(self._h, d_ptr or None, nbytes, d_offsets or None, n_hay, uniform_len, *w[:6],
                                          ctypes.byref(out)))
        return DeviceWordPieces(out.value)

    def wordpiece_into_device(self, d_ptr: int, nbytes: int, cls, cap: int, d_id: int, d_start: int, d_end: int, d_first: int,
                              d_row_offsets: int, *, prefix=b"##", max_word: int = 100, unk_id: int = -1, d_offsets: int = 0,
                              n_hay: int = 0, uniform_len: int = 0) -> int:
        """the raw form: T is returned; T entries at each of the four columns and rows + 1 int64 words at d_row_offsets are
        written only when cap != 0 and T <= cap, and are complete when it returns; cap = 0: the count pass alone"""
        w = _wp_args(cls, prefix, max_word, unk_id)
        n = ctypes.c_uint64(0)
        _check(lib().acx_wordpiece_into_device(self._h, d_ptr or None, nbytes, d_offsets or None, n_hay, uniform_len, *w[:6], cap,
                                               d_id or None, d_start or None, d_end or None, d_first or None,
                                               d_row_offsets or None, ctypes.byref(n)))
        return int(n.value)

    def generate(self, d_ptr: int, nbytes: int, kind: int, seed: int,
                 stream_offset: int = 0) -> None:
        _check(lib().acx_generate_haystack(self._h, d_ptr, nbytes, kind, seed, stream_offset))

    # ---- measurement
    def profile_enable(self, on=True) -> None:
        """True / 1: time every call's scan kernel; N > 1: every N-th call; False / 0: off."""
        _check(lib().acx_profile_enable(self._h, int(on)))

    PATH_STATS = ("sparse", "hot_calls", "hot_groups", "overflow_hits", "dense_tiles", "dense_radix", "overflow_regrown", "k0", "byte_ranges", "wide_redone", "resident_launches", "in_place",
                  "replaced_on_device", "folded_on_device")

    def path_stats(self, reset: bool = True) -> dict:
        """which way this handle's calls went (acx_path_stats): {sparse, hot_calls, hot_groups, overflow_hits,
        dense_tiles, dense_radix, overflow_regrown, k0, byte_ranges, wide_redone, resident_launches, in_place,
        replaced_on_device, folded_on_device}"""
        out = (ctypes.c_uint64 * len(self.PATH_STATS))()
        _check(lib().acx_path_stats(self._h, out, int(reset)))
        return dict(zip(self.PATH_STATS, [int(v) for v in out]))

    def profile_read(self, reset: bool = True) -> Profile:
        p = Profile()
        _check(lib().acx_profile_read(self._h, ctypes.byref(p), int(reset)))
        return p
