"""What reaches C through the ctypes binding: every entry point of capi.Automaton in every form it has (single, batch,
device), the result classes and the *_host / *_rows_device helpers, run against a recorder in the library's place and
compared with literal tables.  The recorder answers every acx_* call with OK, reads the memory behind the pointers it
knows (the haystack's bytes, the offsets, the weights, the packed replacements, records and counts) while the call is
still running, and hands out fake handles and sizes.  No device and no library call is involved.

How an argument is written down here: None is a NULL pointer (the binding may spell it None or 0), "A" the automaton's
handle, "R" a result's handle, "OUT" a pointer the C function writes through, "PTR" any other non-NULL pointer, and a
decoded value (bytes, a list) a pointer whose memory was read.  Scalars are themselves."""
import ctypes

import numpy as np
import pytest

from ahocorasick_rs_amd import capi
from test_capi_abi_cpu import header_prototypes

PROTOS = header_prototypes()
A_HANDLE, R_HANDLE, D_PTR = 0xA000, 0xB000, 0xD000


def words(ptr, n, ctype=ctypes.c_uint64):
    return [int(x) for x in (ctype * n).from_address(ptr)]


def read_host_form(a):
    """(a, hay, len, offsets, n_hay, ...): the len bytes and the n_hay + 1 offsets"""
    hay, n, off, n_hay = a[1:5]
    if hay:
        a[1] = ctypes.string_at(hay, n)
    if off:
        a[3] = words(off, n_hay + 1)


def read_packed(at):
    """(blob, offsets, n) at `at`: the packed byte strings"""
    def read(a):
        blob, off, n = a[at:at + 3]
        o = words(off, n + 1)
        raw = ctypes.string_at(blob, o[-1])
        a[at], a[at + 1] = [raw[o[i]:o[i + 1]] for i in range(n)], "PTR"
    return read


def read_array(at, n_at, ctype=ctypes.c_uint64, per=1, plus=0):
    """a pointer at `at` to (a[n_at] + plus) * per words"""
    def read(a):
        if a[at]:
            a[at] = words(a[at], (a[n_at] + plus) * per, ctype)
    return read


def read_bytes(at, n_at):
    def read(a):
        if a[at]:
            a[at] = ctypes.string_at(a[at], a[n_at])
    return read


def read_find_batch(at):
    """(hay, offsets, n_hay) at `at`"""
    def read(a):
        o = words(a[at + 1], a[at + 2] + 1)
        a[at], a[at + 1] = ctypes.string_at(a[at], o[-1]), o
    return read


HOST_FORMS = ("acx_replace", "acx_summarize", "acx_find_columns", "acx_tally", "acx_filter", "acx_score", "acx_filter_scored",
              "acx_mask", "acx_spans", "acx_snippets")
READERS = {name: [read_host_form] for name in HOST_FORMS}
READERS["acx_replace"].append(read_packed(5))
READERS["acx_replace_device"] = [read_packed(6)]
READERS["acx_splice_host"] = [read_bytes(0, 1), read_array(2, 3, per=3), read_packed(4)]
for name, at in (("acx_score", 6), ("acx_filter_scored", 6), ("acx_score_device", 7), ("acx_filter_scored_device", 7)):
    READERS.setdefault(name, []).append(read_array(at, at + 1, ctypes.c_int32))
READERS["acx_find"] = [read_bytes(1, 2)]
READERS["acx_find_batch"] = [read_find_batch(1)]
READERS["acx_find_batch_multi"] = [read_array(0, 1, ctypes.c_void_p), read_find_batch(2)]
READERS["acx_build_ex"] = [read_packed(0)]
READERS["acx_compile_host_ex"] = [read_packed(0)]
for name in ("acx_summarize_host", "acx_tally_host", "acx_score_host", "acx_spans_host", "acx_snippets_host"):
    READERS[name] = [read_array(0, 1, per=3), read_array(2, 3)]  # records, counts
READERS["acx_score_host"].append(read_array(4, 5, ctypes.c_int32))
READERS["acx_snippets_host"] += [read_bytes(4, 5), read_array(6, 3, plus=1)]
READERS["acx_split_host"] = [read_array(0, 1, per=3)]
READERS["acx_filter_host"] = [read_bytes(0, 1), read_array(2, 3, plus=1), read_array(4, 3)]
READERS["acx_mask_host"] = [read_bytes(0, 1), read_array(2, 3, plus=1), read_array(4, 5, per=3), read_array(6, 3)]
READERS["acx_split_rows"] = READERS["acx_split_rows_host"] = [read_bytes(0, 1)]


class Recorder:
    """stands where the loaded library stands: every acx_* function answers OK (a size getter its size, a pointer
    getter a pointer) and the call is kept as (name, arguments as the module docstring writes them)"""

    def __init__(self, sizes=None, outs=None):
        self.calls = []
        self.sizes = sizes or {}   # what a function returns
        self.outs = outs or {}     # what a function writes through its uint64_t * arguments, in order

    def names(self):
        return [c[0] for c in self.calls]

    def only(self, name):
        got = [c[1] for c in self.calls if c[0] == name]
        assert len(got) == 1, (name, self.names())
        return got[0]

    def __getattr__(self, name):
        if not name.startswith("acx_"):
            raise AttributeError(name)
        kinds, ret = PROTOS[name]

        def call(*args):
            assert len(args) == len(kinds), (name, args)
            a = list(args)
            outs = list(self.outs.get(name, ()))
            for i, (v, k) in enumerate(zip(args, kinds)):
                if k != "ptr":
                    assert isinstance(v, (int, np.integer)) and not isinstance(v, bool), (name, i, v)
                    a[i] = int(v)
                elif v is None or (isinstance(v, int) and v == 0):
                    a[i] = None
                elif hasattr(v, "_obj"):  # ctypes.byref(x)
                    x = v._obj
                    if isinstance(x, ctypes.c_void_p):
                        x.value = A_HANDLE if name in ("acx_build_ex", "acx_replicate", "acx_compile_host_ex") else \
                            D_PTR if name == "acx_device_alloc" else R_HANDLE
                    elif isinstance(x, ctypes.c_uint64):
                        x.value = outs.pop(0) if outs else 0
                    elif isinstance(x, capi.Info):
                        x.n_patterns = 2
                    a[i] = "OUT"
                elif isinstance(v, ctypes.Array):
                    a[i] = ctypes.addressof(v)
                else:
                    assert isinstance(v, int), (name, i, v)
            for read in READERS.get(name, ()):
                read(a)
            for i, k in enumerate(kinds):
                if k == "ptr" and isinstance(a[i], int):
                    a[i] = {A_HANDLE: "A", R_HANDLE: "R"}.get(a[i], "PTR")
            self.calls.append((name, tuple(a)))
            if name == "acx_last_error":
                return b"recorded"
            if ret == "ptr":
                return self.sizes.get(name, D_PTR)
            return self.sizes.get(name, 1 if name.endswith("_on_device") else 0)
        return call


@pytest.fixture
def rec(monkeypatch):
    r = Recorder()
    monkeypatch.setattr(capi, "_lib", r)
    return r


@pytest.fixture
def automaton(rec):
    a = capi.Automaton([b"ab", b"bc"])
    assert rec.only("acx_build_ex") == ([b"ab", b"bc"], "PTR", 2, 0, -1, 0, "OUT") and a._h == A_HANDLE
    rec.calls.clear()
    yield a
    a._h = None  # (nothing to give back)


B3 = [b"", b"abc", b"xbcab"]
BATCHES = {"b3": (B3, (b"abcxbcab", 8, [0, 0, 3, 8], 3)), "empty": ([], (b"", 0, [0], 0))}
W = [3, -4]
RW = [b"X", b"YZ"]

# ---- the stages with a host / device pair: how the method is called beyond the haystack (positional, keyword), the tail
# that reaches C between n_hay (uniform_len on the device) and `out`, and the result class
STAGES = {
    "replace": (([RW], {}), ([b"X", b"YZ"], "PTR", 2)),
    "summarize": (([capi.SUM_FIRST], dict(overlapping=True, codepoints=False)), (1, 0, 1)),
    "find_columns": (([], dict(overlapping=False, codepoints=True)), (0, 1)),
    "tally": (([], dict(overlapping=True)), (1,)),
    "filter": (([], dict(overlapping=True, min_matches=2, flags=1)), (1, 2, 1)),
    "score": (([W], dict(overlapping=True)), (1, W, 2)),
    "filter_scored": (([W], dict(overlapping=True, min_score=-5, flags=1)), (1, W, 2, -5, 1)),
    "mask": (([0x2A], dict(overlapping=True, flags=1)), (1, 0x2A, 1)),
    "spans": (([], dict(overlapping=True, codepoints=True, gap=7)), (1, 1, 7)),
    "snippets": (([], dict(overlapping=True, context=9, flags=1)), (1, 9, 1)),
}
RESULT = {"replace": capi.DeviceReplaced, "summarize": capi.DeviceSummary, "find_columns": capi.DeviceColumns,
          "tally": capi.DeviceTally, "filter": capi.DeviceFiltered, "score": capi.DeviceScores,
          "filter_scored": capi.DeviceFiltered, "mask": capi.DeviceMasked, "spans": capi.DeviceSpans,
          "snippets": capi.DeviceSnippets}
# the batch form's method where it has a name of its own
BATCH_METHOD = {"replace": "replace_batch", "summarize": "summarize_batch", "find_columns": "find_columns_batch"}

# ---- the single form, per stage: what reaches C as (hay, len, offsets, n_hay) for b"abc" and for b"", and how many bytes
# behind `len` are the binding's own (the pad)
#   group A: a padded copy, a batch of one row (the C stage reads n_hay with offsets == NULL)
#   group B: a padded copy, n_hay = 0 (the C stage derives rows = offsets ? n_hay : 1)
#   group C: the caller's own bytes, NULL for none, n_hay = 0
GROUP_A = {b"abc": (b"abc\0", 3, None, 1), b"": (b"\0", 0, None, 1)}
GROUP_B = {b"abc": (b"abc\0", 3, None, 0), b"": (b"\0", 0, None, 0)}
GROUP_C = {b"abc": (b"abc", 3, None, 0), b"": (None, 0, None, 0)}
SINGLE = {"filter": GROUP_A, "score": GROUP_A, "filter_scored": GROUP_A, "mask": GROUP_A, "spans": GROUP_B,
          "snippets": GROUP_B, "replace": GROUP_C, "summarize": GROUP_C, "find_columns": GROUP_C}


def check_result(stage, r, batch, n_hay):
    """what the wrapper set on the result object"""
    assert type(r) is RESULT[stage] and r._h == R_HANDLE
    if stage == "summarize":
        assert (r.n_hay, r.n_patterns) == (n_hay, 2)
    elif stage == "replace":
        assert r.n_hay == n_hay
    elif stage in ("find_columns", "spans", "snippets"):
        assert r.batch is batch
    r._h = None  # (nothing to give back)


@pytest.mark.parametrize("which", sorted(BATCHES))
@pytest.mark.parametrize("stage", sorted(STAGES))
def test_batch_form(rec, automaton, stage, which):
    (pos, kw), tail = STAGES[stage]
    haystacks, host = BATCHES[which]
    if stage == "replace":  # the bytes come back: the recorder's output is empty, its bounds are zeros
        rec.sizes["acx_replaced_len"] = 0
        assert automaton.replace_batch(haystacks, *pos) == [b""] * len(haystacks)
        assert rec.only("acx_replace") == ("A", *host, *tail, "OUT")
        assert rec.only("acx_replaced_offsets") == ("R", "PTR") and rec.only("acx_free_replaced") == ("R",)
        assert rec.names()[-1] == "acx_free_replaced"
        return
    r = getattr(automaton, BATCH_METHOD.get(stage, stage))(haystacks, *pos, **kw)
    assert rec.only("acx_" + stage) == ("A", *host, *tail, "OUT")
    check_result(stage, r, True, len(haystacks))


@pytest.mark.parametrize("hay", [b"abc", b""])
@pytest.mark.parametrize("stage", sorted(SINGLE))
def test_single_form(monkeypatch, rec, automaton, stage, hay):
    (pos, kw), tail = STAGES[stage]
    want_hay, n, off, n_hay = SINGLE[stage][hay]
    if SINGLE[stage] is not GROUP_C:  # read the pad byte too: it is the binding's own memory
        monkeypatch.setitem(READERS, "acx_" + stage, [lambda a: a.__setitem__(1, ctypes.string_at(a[1], a[2] + 1))] +
                            READERS["acx_" + stage][1:])
    if stage == "replace":
        assert automaton.replace(hay, *pos) == b""
        assert rec.only("acx_free_replaced") == ("R",) and rec.names()[-1] == "acx_free_replaced"
    elif SINGLE[stage] is GROUP_C:
        check_result(stage, getattr(automaton, stage)(hay, *pos, **kw), False, 1)
    else:
        check_result(stage, getattr(automaton, stage)(None, *pos, single=hay, **kw), False, 1)
    assert rec.only("acx_" + stage) == ("A", want_hay, n, off, n_hay, *tail, "OUT")


def test_single_form_takes_other_buffers(rec, automaton):
    """group C reads the caller's buffer as it is: a bytearray, a uint8 array, and a contiguous copy of a strided one"""
    strided = np.frombuffer(b"aXbXcX", dtype=np.uint8)[::2]
    for hay in (bytearray(b"abc"), np.frombuffer(b"abc", dtype=np.uint8), strided):
        rec.calls.clear()
        automaton.find_columns(hay)._h = None
        assert rec.only("acx_find_columns")[1:5] == (b"abc", 3, None, 0)
    for stage in ("filter", "spans"):  # groups A and B copy
        rec.calls.clear()
        getattr(automaton, stage)(None, single=bytearray(b"abc"))._h = None
        assert rec.only("acx_" + stage)[1:4] == (b"abc", 3, None)


# ---- the device forms: (d_ptr, nbytes, keywords) -> what reaches C as (d_hay, len, d_offsets, n_hay, uniform_len), whether
# the wrapper takes the call for a batch, and its rows (`k` where it is none: 0 for find_device, 1 for the rest)
DEVICE = {
    "d_offsets": ((0x7000, 8, dict(d_offsets=0x9000, n_hay=3)), ("PTR", 8, "PTR", 3, 0), True, 3),
    "uniform_len": ((0x7000, 8, dict(n_hay=2, uniform_len=4)), ("PTR", 8, None, 2, 4), True, 2),
    "neither": ((0x7000, 8, dict(n_hay=5)), ("PTR", 8, None, 5, 0), False, None),
    "null": ((0, 0, {}), (None, 0, None, 0, 0), False, None),
}


@pytest.mark.parametrize("case", sorted(DEVICE))
@pytest.mark.parametrize("stage", sorted(STAGES))
def test_device_form(rec, automaton, stage, case):
    (pos, kw), tail = STAGES[stage]
    (d_ptr, nbytes, dkw), dev, batch, rows = DEVICE[case]
    r = getattr(automaton, stage + "_device")(d_ptr, nbytes, *pos, **dkw, **kw)
    assert rec.only(f"acx_{stage}_device") == ("A", *dev, *tail, "OUT")
    check_result(stage, r, batch, rows if batch else 1)


@pytest.mark.parametrize("case", sorted(DEVICE))
def test_find_device(rec, automaton, case):
    (d_ptr, nbytes, dkw), dev, batch, rows = DEVICE[case]
    r = automaton.find_device(d_ptr, nbytes, **dkw, overlapping=True, codepoints=False)
    assert rec.only("acx_find_device") == ("A", *dev, 1, 0, "OUT")
    assert type(r) is capi.DeviceResult and r._h == R_HANDLE and r.n_hay == (rows if batch else 0)
    r._h = None


def test_find(rec, automaton):
    strided = np.frombuffer(b"aXbXcX", dtype=np.uint8)[::2]
    for hay, want in ((b"abc", b"abc"), (b"", None), (np.frombuffer(b"abc", dtype=np.uint8), b"abc"), (strided, b"abc")):
        rec.calls.clear()
        got = automaton.find(hay, overlapping=True)
        assert rec.only("acx_find") == ("A", want, len(hay), 1, 0, "OUT", "OUT")
        assert got.dtype == capi.MATCH_DTYPE and len(got) == 0 and rec.names() == ["acx_find"]
    assert automaton.find_tuples(b"abc") == []


@pytest.mark.parametrize("which", sorted(BATCHES))
def test_find_batch(rec, automaton, which):
    haystacks, (hay, _, off, n) = BATCHES[which]
    got, counts = automaton.find_batch(haystacks, codepoints=True)
    assert rec.only("acx_find_batch") == ("A", hay, off, n, 0, 1, "OUT", "OUT", "PTR")
    assert len(got) == 0 and counts.dtype == np.uint64 and len(counts) == n
    rec.calls.clear()
    other = automaton.replicate(3)
    assert rec.only("acx_replicate") == ("A", 3, "OUT") and other._h == A_HANDLE
    got, counts = automaton.find_batch_multi([other], haystacks, overlapping=True)
    assert rec.only("acx_find_batch_multi") == ([A_HANDLE, A_HANDLE], 2, hay, off, n, 1, 0, "OUT", "OUT", "PTR")
    assert len(got) == 0 and len(counts) == n
    other._h = None


def test_the_rest_of_the_automaton(rec, automaton):
    assert automaton.info.n_patterns == 2 and rec.only("acx_automaton_info") == ("A", "OUT")
    automaton.set_kernel(capi.KERNEL_PREFILTER)
    automaton.generate(0x7000, 64, 1, 9, stream_offset=5)
    automaton.profile_enable(8)
    automaton.profile_read(reset=False)
    assert automaton.path_stats(reset=True) == dict.fromkeys(capi.Automaton.PATH_STATS, 0)
    assert [rec.only(n) for n in ("acx_set_kernel", "acx_generate_haystack", "acx_profile_enable", "acx_profile_read",
                                  "acx_path_stats")] == [("A", 2), ("A", "PTR", 64, 1, 9, 5), ("A", 8), ("A", "OUT", 0),
                                                         ("A", "PTR", 1)]
    rec.calls.clear()
    automaton.close()
    automaton.close()
    assert rec.calls == [("acx_free_automaton", ("A",))] and automaton._h is None


def test_a_failure_raises_by_its_code(rec, automaton):
    for code, exc in ((capi.EINVAL, ValueError), (capi.ETOOBIG, ValueError), (capi.ENOMEM, MemoryError),
                      (capi.EDEVICE, capi.AcxError)):
        rec.sizes["acx_tally"] = code
        with pytest.raises(exc, match="recorded") as e:
            automaton.tally(B3)
        assert getattr(e.value, "code", code) == code


# ---- the result classes: which C function every accessor calls, with which `which`, and the array it hands over.  One row
# per accessor: (accessor, arguments, the C call, the length and dtype of what comes back -- or the value itself)
def sizes_of(prefix, **sizes):
    return {f"acx_{prefix}_{k}": v for k, v in sizes.items()}


I64, U8, U64 = np.int64, np.uint8, np.uint64
RESULTS = {
    "columns": (lambda: capi.DeviceColumns(R_HANDLE, True), sizes_of("columns", count=5, rows=3), [
        ("count", None, ("acx_columns_count", ("R",)), 5), ("rows", None, ("acx_columns_rows", ("R",)), 3),
        ("on_device", None, ("acx_columns_on_device", ("R",)), True),
        ("data_ptr", (capi.COL_END,), ("acx_columns_data", ("R", 2)), D_PTR),
        ("column", (capi.COL_START,), ("acx_columns_copy", ("R", 1, "PTR")), (5, I64)),
        ("pattern", (), ("acx_columns_copy", ("R", 0, "PTR")), (5, I64)),
        ("start", (), ("acx_columns_copy", ("R", 1, "PTR")), (5, I64)),
        ("end", (), ("acx_columns_copy", ("R", 2, "PTR")), (5, I64)),
        ("row_offsets", (), ("acx_columns_copy", ("R", 3, "PTR")), (4, I64))]),
    "tally": (lambda: capi.DeviceTally(R_HANDLE), sizes_of("tally", nnz=4, rows=3), [
        ("nnz", None, ("acx_tally_nnz", ("R",)), 4), ("rows", None, ("acx_tally_rows", ("R",)), 3),
        ("on_device", None, ("acx_tally_on_device", ("R",)), True),
        ("data_ptr", (capi.TALLY_COUNT,), ("acx_tally_data", ("R", 2)), D_PTR),
        ("part", (capi.TALLY_PATTERN,), ("acx_tally_copy", ("R", 1, "PTR")), (4, I64)),
        ("row_offsets", (), ("acx_tally_copy", ("R", 0, "PTR")), (4, I64)),
        ("pattern", (), ("acx_tally_copy", ("R", 1, "PTR")), (4, I64)),
        ("count", (), ("acx_tally_copy", ("R", 2, "PTR")), (4, I64))]),
    "filtered": (lambda: capi.DeviceFiltered(R_HANDLE), sizes_of("filtered", rows=3, bytes=7), [
        ("n_rows", None, ("acx_filtered_rows", ("R",)), 3), ("nbytes", None, ("acx_filtered_bytes", ("R",)), 7),
        ("on_device", None, ("acx_filtered_on_device", ("R",)), True),
        ("data_ptr", (capi.FILT_DATA,), ("acx_filtered_data", ("R", 2)), D_PTR),
        ("part", (capi.FILT_OFFSETS,), ("acx_filtered_copy", ("R", 1, "PTR")), (4, I64)),
        ("rows", (), ("acx_filtered_copy", ("R", 0, "PTR")), (3, I64)),
        ("offsets", (), ("acx_filtered_copy", ("R", 1, "PTR")), (4, I64)),
        ("data", (), ("acx_filtered_copy", ("R", 2, "PTR")), (7, U8))]),
    "scores": (lambda: capi.DeviceScores(R_HANDLE), sizes_of("scores", rows=3), [
        ("rows", None, ("acx_scores_rows", ("R",)), 3), ("on_device", None, ("acx_scores_on_device", ("R",)), True),
        ("data_ptr", (), ("acx_scores_data", ("R",)), D_PTR),
        ("scores", (), ("acx_scores_copy", ("R", "PTR")), (3, I64))]),
    "masked": (lambda: capi.DeviceMasked(R_HANDLE), sizes_of("masked", rows=3, bytes=7), [
        ("rows", None, ("acx_masked_rows", ("R",)), 3), ("nbytes", None, ("acx_masked_bytes", ("R",)), 7),
        ("on_device", None, ("acx_masked_on_device", ("R",)), True),
        ("data_ptr", (), ("acx_masked_data", ("R",)), D_PTR), ("offsets_ptr", (), ("acx_masked_offsets", ("R",)), D_PTR),
        ("data", (), ("acx_masked_copy", ("R", "PTR")), (7, U8)),
        ("offsets", (), ("acx_masked_copy_offsets", ("R", "PTR")), (4, I64))]),
    "rows": (lambda: capi.DeviceRows(R_HANDLE), {**sizes_of("rows", count=3, bytes=7), "acx_rows_device": 2}, [
        ("rows", None, ("acx_rows_count", ("R",)), 3), ("nbytes", None, ("acx_rows_bytes", ("R",)), 7),
        ("device", None, ("acx_rows_device", ("R",)), 2), ("on_device", None, ("acx_rows_on_device", ("R",)), True),
        ("offsets_ptr", (), ("acx_rows_offsets", ("R",)), D_PTR),
        ("offsets", (), ("acx_rows_copy", ("R", "PTR")), (4, I64))]),
    "spans": (lambda: capi.DeviceSpans(R_HANDLE, True), sizes_of("spans", count=5, rows=3), [
        ("count", None, ("acx_spans_count", ("R",)), 5), ("rows", None, ("acx_spans_rows", ("R",)), 3),
        ("on_device", None, ("acx_spans_on_device", ("R",)), True),
        ("data_ptr", (capi.SPAN_END,), ("acx_spans_data", ("R", 1)), D_PTR),
        ("column", (capi.SPAN_START,), ("acx_spans_copy", ("R", 0, "PTR")), (5, I64)),
        ("start", (), ("acx_spans_copy", ("R", 0, "PTR")), (5, I64)),
        ("end", (), ("acx_spans_copy", ("R", 1, "PTR")), (5, I64)),
        ("row_offsets", (), ("acx_spans_copy", ("R", 2, "PTR")), (4, I64))]),
    "snippets": (lambda: capi.DeviceSnippets(R_HANDLE, True), sizes_of("snippets", count=5, rows=3, nbytes=7), [
        ("count", None, ("acx_snippets_count", ("R",)), 5), ("rows", None, ("acx_snippets_rows", ("R",)), 3),
        ("nbytes", None, ("acx_snippets_nbytes", ("R",)), 7), ("on_device", None, ("acx_snippets_on_device", ("R",)), True),
        ("data_ptr", (capi.SNIP_LEAD,), ("acx_snippets_data", ("R", 3)), D_PTR),
        ("part", (capi.SNIP_PATTERN,), ("acx_snippets_copy", ("R", 2, "PTR")), (5, I64)),
        ("data", (), ("acx_snippets_copy", ("R", 0, "PTR")), (7, U8)),
        ("offsets", (), ("acx_snippets_copy", ("R", 1, "PTR")), (6, I64)),
        ("pattern", (), ("acx_snippets_copy", ("R", 2, "PTR")), (5, I64)),
        ("lead", (), ("acx_snippets_copy", ("R", 3, "PTR")), (5, I64)),
        ("row_offsets", (), ("acx_snippets_copy", ("R", 4, "PTR")), (4, I64))]),
    "summary": (lambda: capi.DeviceSummary(R_HANDLE, 70, 2), {"acx_summary_total": 9}, [
        ("total", None, ("acx_summary_total", ("R",)), 9), ("on_device", None, ("acx_summary_on_device", ("R",)), True),
        ("counts", (), ("acx_summary_counts", ("R", "PTR")), (70, U64)),
        ("any_bits", (), ("acx_summary_any", ("R", "PTR")), (2, U64)),
        ("any", (), ("acx_summary_any", ("R", "PTR")), (70, np.bool_)),
        ("first", (), ("acx_summary_first", ("R", "PTR")), (70, capi.MATCH_DTYPE)),
        ("by_pattern", (), ("acx_summary_by_pattern", ("R", "PTR")), (2, U64)),
        ("device_ptr", ("first",), ("acx_summary_device_first", ("R",)), D_PTR)]),
    "result": (lambda: capi.DeviceResult(R_HANDLE, 3), {"acx_result_count": 5}, [
        ("count", None, ("acx_result_count", ("R",)), 5),
        ("device_ptr", None, ("acx_result_device_matches", ("R",)), D_PTR),
        ("matches", (), ("acx_result_copy", ("R", "PTR")), (5, capi.MATCH_DTYPE)),
        ("counts", (), ("acx_result_copy_counts", ("R", "PTR")), (3, U64))]),
    "replaced": (lambda: capi.DeviceReplaced(R_HANDLE, 3), {"acx_replaced_len": 7}, [
        ("nbytes", None, ("acx_replaced_len", ("R",)), 7),
        ("device_ptr", None, ("acx_replaced_device_bytes", ("R",)), D_PTR),
        ("offsets", (), ("acx_replaced_offsets", ("R", "PTR")), (4, U64)),
        ("download", (), ("acx_replaced_copy", ("R", "PTR")), bytes(7))]),
}
FREE = {"filtered": "acx_free_filtered", "result": "acx_free_result", "replaced": "acx_free_replaced"}


@pytest.mark.parametrize("name", sorted(RESULTS))
def test_result_accessors(rec, name):
    make, sizes, rows = RESULTS[name]
    rec.sizes.update(sizes)
    r = make()
    for accessor, args, call, want in rows:
        rec.calls.clear()
        got = getattr(r, accessor) if args is None else getattr(r, accessor)(*args)
        assert call in rec.calls, (accessor, rec.calls)
        if isinstance(want, tuple):
            assert isinstance(got, np.ndarray) and (len(got), got.dtype) == want and got.ndim == 1, (accessor, got)
        else:
            assert got == want and type(got) is type(want), (accessor, got)
    rec.calls.clear()
    r.free()
    r.free()
    del r
    assert rec.calls == [(FREE.get(name, "acx_free_" + name), ("R",))]


# an empty result: the destination of an empty part is NULL, the offsets (one word at least) keep theirs; a single form
# has no row offsets and asks for none
EMPTY = {
    "columns": (lambda: capi.DeviceColumns(R_HANDLE, False), [("pattern", ("R", 0, None)), ("row_offsets", None)]),
    "tally": (lambda: capi.DeviceTally(R_HANDLE), [("pattern", ("R", 1, None)), ("row_offsets", ("R", 0, "PTR"))]),
    "filtered": (lambda: capi.DeviceFiltered(R_HANDLE), [("rows", ("R", 0, None)), ("offsets", ("R", 1, "PTR")),
                                                         ("data", ("R", 2, None))]),
    "scores": (lambda: capi.DeviceScores(R_HANDLE), [("scores", ("R", None))]),
    "masked": (lambda: capi.DeviceMasked(R_HANDLE), [("data", ("R", None)), ("offsets", ("R", "PTR"))]),
    "rows": (lambda: capi.DeviceRows(R_HANDLE), [("offsets", ("R", "PTR"))]),
    "spans": (lambda: capi.DeviceSpans(R_HANDLE, False), [("start", ("R", 0, None)), ("row_offsets", None)]),
    "snippets": (lambda: capi.DeviceSnippets(R_HANDLE, False), [("data", ("R", 0, None)), ("offsets", ("R", 1, "PTR")),
                                                                ("lead", ("R", 3, None)), ("row_offsets", None)]),
    "summary": (lambda: capi.DeviceSummary(R_HANDLE, 0, 0), [("counts", ("R", None)), ("any_bits", ("R", None)),
                                                            ("first", ("R", None)), ("by_pattern", ("R", None))]),
    "result": (lambda: capi.DeviceResult(R_HANDLE, 0), [("matches", None), ("counts", None)]),
    "replaced": (lambda: capi.DeviceReplaced(R_HANDLE, 0), [("offsets", ("R", "PTR")), ("download", None)]),
}


@pytest.mark.parametrize("name", sorted(EMPTY))
def test_empty_result_accessors(rec, name):
    make, rows = EMPTY[name]
    r = make()
    for accessor, want in rows:
        rec.calls.clear()
        got = getattr(r, accessor)()
        copies = [c[1] for c in rec.calls if "_copy" in c[0] or c[0] in
                  ("acx_replaced_offsets", "acx_summary_counts", "acx_summary_any", "acx_summary_first", "acx_summary_by_pattern")]
        if want is None:
            assert not copies and (got is None or len(got) == 0), (accessor, rec.calls)
        else:
            assert copies == [want], (accessor, rec.calls)
    r._h = None


def test_snippets_tolist(rec):
    rec.sizes.update(sizes_of("snippets", count=2, rows=0, nbytes=0))
    r = capi.DeviceSnippets(R_HANDLE, False)
    assert r.tolist() == [b"", b""]
    r._h = None


# ---- the definitions on the host and the stages alone: the records, counts and bytes as read, NULL where nothing is
M2 = [(1, 0, 2), (0, 1, 3)]
M2W = [1, 0, 2, 0, 1, 3]


def test_summarize_host(rec):
    any_, first, hist = capi.summarize_host(M2, [1, 1, 0], 2)
    assert rec.only("acx_summarize_host") == (M2W, 2, [1, 1, 0], 3, 2, 3, "PTR", "PTR", "PTR")
    assert (len(any_), len(first), len(hist)) == (3, 3, 2) and first.dtype == capi.MATCH_DTYPE
    rec.calls.clear()
    assert capi.summarize_host([], None, 2, capi.SUM_FIRST)[2] is None
    assert rec.only("acx_summarize_host") == (None, 0, None, 1, 2, 1, "PTR", "PTR", "PTR")
    rec.calls.clear()
    capi.summarize_host([], [], 0)  # an empty batch is still a batch: its counts pointer is not NULL
    assert rec.only("acx_summarize_host") == (None, 0, [], 0, 0, 3, "PTR", "PTR", "PTR")


def test_split_host_and_device(rec):
    cols = capi.split_host(M2)
    assert rec.only("acx_split_host") == (M2W, 2, "PTR", "PTR", "PTR") and [len(c) for c in cols] == [2, 2, 2]
    rec.calls.clear()
    capi.split_host([])
    assert rec.only("acx_split_host") == (None, 0, None, None, None)
    capi.split_device(0x7000, 4, 0x7100, 0, 0x7300)
    assert rec.only("acx_split_device") == ("PTR", 4, "PTR", None, "PTR")


def test_tally_host_and_rows_device(rec):
    rec.outs["acx_tally_host"] = [1]
    ro, pat, cnt = capi.tally_host(M2, [2, 0])
    assert rec.only("acx_tally_host") == (M2W, 2, [2, 0], 2, "PTR", "PTR", "PTR", "OUT")
    assert (len(ro), len(pat), len(cnt)) == (3, 1, 1) and ro.dtype == pat.dtype == cnt.dtype == np.int64
    rec.calls.clear()
    capi.tally_host([], [])
    assert rec.only("acx_tally_host") == (None, 0, None, 0, "PTR", None, None, "OUT")
    rec.outs["acx_tally_rows_device"] = [6]
    assert capi.tally_rows_device(0x7000, 9, 0, 3, 2, 0x7100, 0x7200, 0x7300) == 6
    assert rec.only("acx_tally_rows_device") == ("PTR", 9, None, 3, 2, "PTR", "PTR", "PTR", "OUT")


def test_filter_host_and_rows_device(rec):
    rec.outs["acx_filter_host"] = [1, 2]
    rows, oo, data = capi.filter_host(b"abcxy", [0, 3, 5], [1, 0], 2, 1)
    want = (b"abcxy", 5, [0, 3, 5], 2, [1, 0], 2, 1)
    assert [c[1] for c in rec.calls] == [(*want, None, None, None, "OUT", "OUT"), (*want, "PTR", "PTR", "PTR", "OUT", "OUT")]
    assert (len(rows), len(oo), len(data)) == (1, 2, 2) and data.dtype == np.uint8
    rec.calls.clear()
    rec.outs["acx_filter_host"] = [0, 0]
    assert capi.filter_host(b"", None, [], sizes_only=True) == (0, 0)
    assert rec.only("acx_filter_host") == (None, 0, None, 0, None, 1, 0, None, None, None, "OUT", "OUT")
    with pytest.raises(ValueError):
        capi.filter_host(b"abc", [0, 3], [1, 1])
    rec.outs["acx_filter_rows_device"] = [2, 5]
    assert capi.filter_rows_device(0x7000, 8, 0, 2, 4, 0x7100, 1, 1, 0x7200, 0x7300, 0) == (2, 5)
    assert rec.only("acx_filter_rows_device") == ("PTR", 8, None, 2, 4, "PTR", 1, 1, "PTR", "PTR", None, "OUT", "OUT")


def test_score_host_and_rows_device(rec):
    out = capi.score_host(M2, [1, 1], W)
    assert rec.only("acx_score_host") == (M2W, 2, [1, 1], 2, W, 2, "PTR") and (len(out), out.dtype) == (2, np.int64)
    rec.calls.clear()
    capi.score_host([], None, [])
    assert rec.only("acx_score_host") == (None, 0, None, 1, None, 0, "PTR")
    rec.calls.clear()
    capi.score_host([], [], W)
    assert rec.only("acx_score_host") == (None, 0, [], 0, W, 2, None)
    with pytest.raises(ValueError):
        capi.score_host([], None, [1 << 31])
    capi.score_rows_device(0x7000, 3, 0x7100, 2, 0, 4, 0x7300)
    assert rec.only("acx_score_rows_device") == ("PTR", 3, "PTR", 2, None, 4, "PTR")


def test_mask_host_and_rows_device(rec):
    out = capi.mask_host(b"abcxy", [0, 3, 5], M2, [1, 1], 0x2A, capi.MASK_ZERO)
    assert rec.only("acx_mask_host") == (b"abcxy", 5, [0, 3, 5], 2, M2W, 2, [1, 1], 0x2A, 1, "PTR")
    assert (len(out), out.dtype) == (5, np.uint8)
    rec.calls.clear()
    assert len(capi.mask_host(b"", None, [], None, 0)) == 0
    assert rec.only("acx_mask_host") == (None, 0, None, 1, None, 0, None, 0, 0, "PTR")
    rec.calls.clear()
    capi.mask_host(b"", [0], [], [], 1)
    assert rec.only("acx_mask_host") == (None, 0, [0], 0, None, 0, [], 1, 0, "PTR")
    with pytest.raises(ValueError):
        capi.mask_host(b"abc", [0, 3], [], [0, 0], 1)
    capi.mask_rows_device(0x7000, 8, 0, 2, 4, 0x7100, 3, 0x7200, 7, 1, 0x7000)
    assert rec.only("acx_mask_rows_device") == ("PTR", 8, None, 2, 4, "PTR", 3, "PTR", 7, 1, "PTR")


def test_split_rows_all_four(rec):
    rec.sizes.update(sizes_of("rows", count=2, bytes=4))
    r = capi.split_rows(b"a\nb\n", 10)
    assert rec.only("acx_split_rows") == (b"a\nb\n", 4, 10, "OUT") and type(r) is capi.DeviceRows and r._h == R_HANDLE
    rec.calls.clear()
    capi.split_rows(b"")._h = None
    assert rec.only("acx_split_rows") == (None, 0, 10, "OUT")
    capi.split_rows_device(0, 0, 9)._h = None
    assert rec.only("acx_split_rows_device") == (None, 0, 9, "OUT")
    rec.outs["acx_split_rows_host"] = [2]
    off = capi.split_rows_host(b"a\nb\n")
    assert [c[1] for c in rec.calls if c[0] == "acx_split_rows_host"] == [(b"a\nb\n", 4, 10, None, 0, "OUT"),
                                                                         (b"a\nb\n", 4, 10, "PTR", 3, "OUT")]
    assert (len(off), off.dtype) == (3, np.int64)
    assert capi.split_rows_host(b"", count_only=True) == 2
    rec.outs["acx_split_rows_into_device"] = [4]
    assert capi.split_rows_into_device(0x7000, 8, 10, 0, 0) == 4
    assert rec.only("acx_split_rows_into_device") == ("PTR", 8, 10, None, 0, "OUT")
    r._h = None


def test_spans_host_and_rows_device(rec):
    rec.outs["acx_spans_host"] = [1]
    ro, start, end = capi.spans_host(M2, [2, 0], gap=4)
    assert rec.only("acx_spans_host") == (M2W, 2, [2, 0], 2, 4, "PTR", "PTR", "PTR", "OUT")
    assert (len(ro), len(start), len(end)) == (3, 1, 1) and ro.dtype == start.dtype == end.dtype == np.int64
    rec.calls.clear()
    ro, _, _ = capi.spans_host([], None)
    assert rec.only("acx_spans_host") == (None, 0, None, 1, 0, "PTR", "PTR", "PTR", "OUT") and len(ro) == 2
    rec.calls.clear()
    capi.spans_host([], [])
    assert rec.only("acx_spans_host") == (None, 0, [], 0, 0, "PTR", "PTR", "PTR", "OUT")
    rec.outs["acx_spans_rows_device"] = [3]
    assert capi.spans_rows_device(0x7000, 9, 0x7100, 3, 2, 0x7200, 0, 0x7300) == 3
    assert rec.only("acx_spans_rows_device") == ("PTR", 9, "PTR", 3, 2, "PTR", None, "PTR", "OUT")


def test_snippets_host_and_rows_device(rec):
    rec.outs["acx_snippets_host"] = [6]
    data, o, pat, lead, ro = capi.snippets_host(M2, [1, 1], b"abcxy", [0, 3, 5], context=1, flags=capi.SNIPPET_UTF8)
    want = (M2W, 2, [1, 1], 2, b"abcxy", 5, [0, 3, 5], 1, 1)
    assert [c[1] for c in rec.calls] == [(*want, None, None, None, None, None, "OUT"),
                                         (*want, "PTR", "PTR", "PTR", "PTR", "PTR", "OUT")]
    assert [(len(x), x.dtype) for x in (data, o, pat, lead, ro)] == [(6, U8), (3, I64), (2, I64), (2, I64), (3, I64)]
    rec.calls.clear()
    rec.outs["acx_snippets_host"] = [0]
    capi.snippets_host([], None, b"", None)
    want = (None, 0, None, 1, None, 0, None, 0, 0)
    assert [c[1] for c in rec.calls] == [(*want, None, None, None, None, None, "OUT"),
                                         (*want, "PTR", None, None, "PTR", None, "OUT")]
    rec.calls.clear()
    assert capi.snippets_host([], [], b"", [0], sizes_only=True) == 0
    assert rec.only("acx_snippets_host") == (None, 0, [], 0, None, 0, [0], 0, 0, None, None, None, None, None, "OUT")
    rec.outs["acx_snippets_rows_device"] = [11]
    assert capi.snippets_rows_device(0x7000, 3, 0x7100, 2, 0x7200, 8, 0, 4, 1, 1, 0x7300, 0x7400, 0x7500, 0x7600, 0, 16) == (0, 11)
    assert rec.only("acx_snippets_rows_device") == ("PTR", 3, "PTR", 2, "PTR", 8, None, 4, 1, 1, "PTR", "PTR", "PTR", "PTR",
                                                    None, 16, "OUT")
    rec.sizes["acx_snippets_rows_device"] = capi.ETOOBIG
    assert capi.snippets_rows_device(0x7000, 3, 0x7100, 2, 0x7200, 8, 0, 4, 1, 1, 0x7300, 0x7400, 0x7500, 0x7600, 0, 4) == \
        (capi.ETOOBIG, 11)


def test_splice_host(rec):
    rec.outs["acx_splice_host"] = [4]
    got = capi.splice_host(b"abcd", M2[:1], RW)
    want = (b"abcd", 4, [1, 0, 2], 1, RW, "PTR", 2)
    assert [c[1] for c in rec.calls] == [(*want, None, "OUT"), (*want, "PTR", "OUT")] and len(got) == 4
    rec.calls.clear()
    capi.splice_host(b"", [], RW)
    assert rec.calls[0][1] == (None, 0, None, 0, RW, "PTR", 2, None, "OUT")


def test_the_process_wide_functions(rec):
    rec.outs["acx_shard_range"] = [2, 5]
    assert capi.shard_range(10, 1, 3) == (2, 5) and rec.only("acx_shard_range") == (10, 1, 3, "OUT", "OUT")
    capi.set_device(2)
    assert capi.device_count() == 0 and rec.only("acx_set_device") == (2,)
    assert capi.filter_hash(b"abc") == 0 and rec.only("acx_filter_hash") == (int.from_bytes(b"abc", "little"),)
    assert capi.prefix_slot(b"abcdef", 4, 10) == 0 and rec.only("acx_prefix_slot") == (int.from_bytes(b"abcd", "little"), 4, 10)
    assert len(capi.comm_unique_id()) == 128 and rec.only("acx_comm_unique_id") == ("PTR",)
    assert capi.output_offsets([1, 2]) == [0, 0, 0] and rec.only("acx_output_offsets") == ("PTR", 2, "PTR")
    b = capi.DeviceBuffer(32)
    assert b.ptr == D_PTR and rec.only("acx_device_alloc") == ("OUT", 32)
    b.upload(np.zeros(4, dtype=np.uint64))
    assert len(b.download(8)) == 8
    assert rec.only("acx_device_upload") == ("PTR", "PTR", 32) and rec.only("acx_device_download") == ("PTR", "PTR", 8)
    b.free()
    b.free()
    assert rec.only("acx_device_free") == ("PTR",) and b.ptr is None
    c = capi.Comm.init_rank(bytes(128), 2, 1, 0)
    assert rec.only("acx_comm_init_rank") == ("PTR", 2, 1, 0, "OUT")
    c.close()
    c.close()
    assert rec.only("acx_comm_free") == ("R",)
