"""The part accessors of the post-find results (acx_columns, acx_spans, acx_tally, acx_filtered, acx_snippets by `which`;
acx_masked, acx_scores, acx_rows by name) on both routes -- acx_X (host memory in, a host block out) and acx_X_device -- at
the smallest shapes: 2 patterns; 8 bytes as one haystack, as a batch of 2 rows, a batch of no row, and 2 rows without a match.
Every valid part has an address and copies out what the host form (acx_*_host) makes of the find's records, byte for byte and
not a byte more; every refusal has its code and its text, and a valid call straight behind it still answers.  The texts are
the literal strings of the sources.  The stages' kernels at their seams are test_gpu_{columns,spans,tally,filter,snippets,
mask,score,rows}.py's."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
capi = pytest.importorskip("ahocorasick_rs_amd.capi")

OK, EINVAL = capi.OK, capi.EINVAL
NULL_TEXT = "null argument"
SINGLE_TEXT = "the single form has no row offsets"
GUARD = 0xC3
PATS = [b"ab", b"cd"]
W = np.asarray([5, -3], dtype=np.int32)
FILL = ord("*")

# (haystack, offsets or None: one haystack that is no batch)
SHAPES = {
    "single": (b"abcdefgh", None),
    "batch": (b"abcdefgh", [0, 5, 8]),
    "empty batch": (b"", [0]),
    "no match": (b"xxxxxxxx", [0, 5, 8]),
}


def call(name, *args):
    """-> (code, text): the text is read only behind a failure (a success leaves the last one)"""
    L = capi.lib()
    rc = getattr(L, name)(*args)
    return rc, ("" if rc == OK else L.acx_last_error().decode())


def ptr(arr):
    return arr.ctypes.data if arr is not None and arr.size else None


def i64(n):
    return np.zeros(max(n, 1), dtype=np.int64)


class Shape:
    """One shape: its bytes on the host and on the device, the find's records and counts (the library's own find; what the
    stages make of them is the host forms' word)."""

    def __init__(self, a, name):
        hay, off = SHAPES[name]
        self.name = name
        self.hay = np.frombuffer(hay, dtype=np.uint8)
        self.len = len(hay)
        self.batch = off is not None
        self.n_hay = len(off) - 1 if self.batch else 1
        self.off = np.asarray(off, dtype=np.uint64) if self.batch else None
        if not self.batch:
            self.m = a.find(hay)
            self.counts = np.asarray([len(self.m)], dtype=np.uint64)
        elif self.n_hay:
            self.m, self.counts = a.find_batch([hay[off[i]:off[i + 1]] for i in range(self.n_hay)])
        else:
            self.m, self.counts = np.empty(0, dtype=capi.MATCH_DTYPE), np.zeros(1, dtype=np.uint64)
        self.n = len(self.m)
        self.d_hay = capi.DeviceBuffer(16).upload(self.hay) if self.len else capi.DeviceBuffer(16)
        self.d_off = capi.DeviceBuffer(32).upload(self.off) if self.batch else None

    def host_args(self):  # hay, len, offsets, n_hay
        return ptr(self.hay), self.len, ptr(self.off), self.n_hay if self.batch else 0

    def device_args(self):  # d_hay, len, d_offsets, n_hay, uniform_len
        return self.d_hay.ptr, self.len, self.d_off.ptr if self.batch else None, self.n_hay if self.batch else 0, 0

    def free(self):
        self.d_hay.free()
        if self.d_off:
            self.d_off.free()


@pytest.fixture(scope="module")
def world():
    a = capi.Automaton(PATS, 0)
    shapes = {name: Shape(a, name) for name in SHAPES}
    yield a, shapes
    for s in shapes.values():
        s.free()
    a.close()


def make(name, a, s, device, *tail):
    """the result handle of acx_<name> (host route) or acx_<name>_device over shape s; tail: the entry's own arguments"""
    out = ctypes.c_void_p()
    if device:
        rc = call(name + "_device", a._h, *s.device_args(), *tail, ctypes.byref(out))
    else:
        rc = call(name, a._h, *s.host_args(), *tail, ctypes.byref(out))
    assert rc == (OK, "") and out.value, (name, s.name, device, rc)
    return out.value


def row_offsets(s):
    return np.concatenate([[0], np.cumsum(s.counts[:s.n_hay])]).astype(np.int64) if s.batch else None


# ---------------------------------------------------------------------------
# what the host forms make of a shape's records: a list of parts in the order of `which` (None: the single form lacks it)
# ---------------------------------------------------------------------------
def want_columns(s):
    p, b, e = i64(s.n), i64(s.n), i64(s.n)
    assert call("acx_split_host", ptr(s.m), s.n, p.ctypes.data, b.ctypes.data, e.ctypes.data) == (OK, "")
    return [p[:s.n], b[:s.n], e[:s.n], row_offsets(s)]


def want_spans(s):
    ro, b, e, k = i64(s.n_hay + 1), i64(s.n), i64(s.n), ctypes.c_uint64(99)
    assert call("acx_spans_host", ptr(s.m), s.n, s.counts.ctypes.data, s.n_hay, 0, ro.ctypes.data, b.ctypes.data, e.ctypes.data,
                ctypes.byref(k)) == (OK, "")
    return [b[:k.value], e[:k.value], ro[:s.n_hay + 1] if s.batch else None]


def want_tally(s):
    ro, p, c, nnz = i64(s.n_hay + 1), i64(s.n), i64(s.n), ctypes.c_uint64(99)
    assert call("acx_tally_host", ptr(s.m), s.n, s.counts.ctypes.data, s.n_hay, ro.ctypes.data, p.ctypes.data, c.ctypes.data,
                ctypes.byref(nnz)) == (OK, "")
    return [ro[:s.n_hay + 1], p[:nnz.value], c[:nnz.value]]


def want_filtered(s):
    rows, oo, data = i64(s.n_hay), i64(s.n_hay + 1), np.zeros(max(s.len, 1), dtype=np.uint8)
    k, nb = ctypes.c_uint64(99), ctypes.c_uint64(99)
    assert call("acx_filter_host", ptr(s.hay), s.len, ptr(s.off), s.n_hay, s.counts.ctypes.data, 1, capi.FILTER_KEEP_MATCHED,
                rows.ctypes.data, oo.ctypes.data, data.ctypes.data, ctypes.byref(k), ctypes.byref(nb)) == (OK, "")
    return [rows[:k.value], oo[:k.value + 1], data[:nb.value]]


def want_snippets(s):
    oo, p, lead, ro, data = i64(s.n + 1), i64(s.n), i64(s.n), i64(s.n_hay + 1), np.zeros(3 * 8, dtype=np.uint8)
    total = ctypes.c_uint64(99)
    assert call("acx_snippets_host", ptr(s.m), s.n, s.counts.ctypes.data, s.n_hay, ptr(s.hay), s.len, ptr(s.off), 1, 0,
                oo.ctypes.data, p.ctypes.data, lead.ctypes.data, ro.ctypes.data, data.ctypes.data, ctypes.byref(total)) == (OK, "")
    return [data[:total.value], oo[:s.n + 1], p[:s.n], lead[:s.n], ro[:s.n_hay + 1] if s.batch else None]


# name of the entry, its own arguments, the accessors' prefix, the text of a `which` out of range, the host form, the sizes
KINDS = {
    "columns": ("acx_find_columns", (0, 0), "acx_columns", "no such column", want_columns, ("count", "rows")),
    "spans": ("acx_spans", (0, 0, 0), "acx_spans", "no such column", want_spans, ("count", "rows")),
    "tally": ("acx_tally", (0,), "acx_tally", "no such part", want_tally, ("nnz", "rows")),
    "filtered": ("acx_filter", (0, 1, capi.FILTER_KEEP_MATCHED), "acx_filtered", "no such part", want_filtered, ("rows", "bytes")),
    "snippets": ("acx_snippets", (0, 1, 0), "acx_snippets", "no such part", want_snippets, ("count", "rows", "nbytes")),
}


def read_at(address, nbytes, on_device):
    """nbytes at an address a *_data accessor gave (a part, even an empty one, has an address)"""
    assert address
    if not nbytes:
        return b""
    if not on_device:
        return ctypes.string_at(address, nbytes)
    out = np.empty(nbytes, dtype=np.uint8)
    capi._check(capi.lib().acx_device_download(out.ctypes.data, address, nbytes))
    return out.tobytes()


def copied(fn, *front, nbytes):
    """-> (code, text), the bytes a *_copy wrote -- with 16 guard bytes behind them"""
    dst = np.full(nbytes + 16, GUARD, dtype=np.uint8)
    rc = call(fn, *front, dst.ctypes.data)
    assert (dst[nbytes:] == GUARD).all(), (fn, front, "the copy wrote behind the part")
    return rc, dst[:nbytes].tobytes()


def check_parts(prefix, h, want, range_text, device):
    L = capi.lib()
    data, copy = getattr(L, prefix + "_data"), prefix + "_copy"
    assert getattr(L, prefix + "_on_device")(h) == int(device)
    full = next(k for k, w in enumerate(want) if w is not None and w.nbytes)  # (every shape has a part that is not empty)

    def valid():
        assert copied(copy, h, full, nbytes=want[full].nbytes) == ((OK, ""), want[full].tobytes())

    for which, w in enumerate(want):
        if w is None:  # the single form's row offsets
            assert data(h, which) is None
            assert call(copy, h, which, np.zeros(4, np.int64).ctypes.data) == (EINVAL, SINGLE_TEXT)
            assert call(copy, h, which, None) == (EINVAL, SINGLE_TEXT)
            valid()
            continue
        address = data(h, which)
        assert address, (which, "a part, even an empty one, has an address")
        assert read_at(address, w.nbytes, device) == w.tobytes(), which
        assert copied(copy, h, which, nbytes=w.nbytes) == ((OK, ""), w.tobytes()), which
        if w.nbytes:
            assert call(copy, h, which, None) == (EINVAL, NULL_TEXT), which
            valid()
        else:
            assert call(copy, h, which, None) == (OK, ""), which
    for which in (-1, len(want)):
        assert data(h, which) is None
        assert copied(copy, h, which, nbytes=0) == ((EINVAL, range_text), b"")
        assert call(copy, h, which, None) == (EINVAL, range_text)
        valid()


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_parts_by_which(world, kind, device):
    a, shapes = world
    entry, tail, prefix, range_text, host_form, sizes = KINDS[kind]
    L = capi.lib()
    for s in shapes.values():
        want = host_form(s)
        h = make(entry, a, s, device, *tail)
        try:
            check_parts(prefix, h, want, range_text, device)
            got = {name: getattr(L, prefix + "_" + name)(h) for name in sizes}
            if kind in ("columns", "spans", "snippets"):
                assert got["count"] == len(want[0 if kind != "snippets" else 2]) and got["rows"] == (s.n_hay if s.batch else 0)
            if kind == "snippets":
                assert got["nbytes"] == want[0].nbytes
            if kind == "tally":
                assert got == {"nnz": len(want[1]), "rows": s.n_hay}
            if kind == "filtered":
                assert got == {"rows": len(want[0]), "bytes": want[2].nbytes}
        finally:
            getattr(L, "acx_free_" + prefix[4:])(h)


def test_tally_and_scores_brought_down(world, monkeypatch):
    """the host entries' device route (ACX_*_HOST_MAX is read per call): the block comes down in one copy, parts and sizes as
    on the host route"""
    a, shapes = world
    monkeypatch.setenv("ACX_TALLY_HOST_MAX", "0")
    monkeypatch.setenv("ACX_SCORE_HOST_MAX", "0")
    for s in (shapes["batch"], shapes["no match"]):
        h = make("acx_tally", a, s, False, 0)
        try:
            check_parts("acx_tally", h, want_tally(s), "no such part", False)
        finally:
            capi.lib().acx_free_tally(h)
        h = make("acx_score", a, s, False, 0, W.ctypes.data, 2)
        try:
            check_scores(h, s, False)
        finally:
            capi.lib().acx_free_scores(h)


# ---------------------------------------------------------------------------
# masked, scores, rows: the named accessors
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_masked(world, device):
    a, shapes = world
    L = capi.lib()
    for s in shapes.values():
        want = np.zeros(max(s.len, 1), dtype=np.uint8)
        assert call("acx_mask_host", ptr(s.hay), s.len, ptr(s.off), s.n_hay, ptr(s.m), s.n, s.counts.ctypes.data, FILL, 0,
                    want.ctypes.data) == (OK, "")
        want = want[:s.len]
        offsets = (s.off if s.batch else np.asarray([0, s.len])).astype(np.int64)
        h = make("acx_mask", a, s, device, 0, FILL, 0)
        try:
            assert (L.acx_masked_rows(h), L.acx_masked_bytes(h), L.acx_masked_on_device(h)) == (s.n_hay, s.len, int(device))

            def valid():
                assert copied("acx_masked_copy_offsets", h, nbytes=offsets.nbytes) == ((OK, ""), offsets.tobytes())

            assert read_at(L.acx_masked_offsets(h), offsets.nbytes, device) == offsets.tobytes()
            assert read_at(L.acx_masked_data(h), s.len, device) == want.tobytes()  # (no byte still has an address)
            valid()
            assert copied("acx_masked_copy", h, nbytes=s.len) == ((OK, ""), want.tobytes())
            assert call("acx_masked_copy", h, None) == ((EINVAL, NULL_TEXT) if s.len else (OK, ""))
            valid()
            assert call("acx_masked_copy_offsets", h, None) == (EINVAL, NULL_TEXT)
            valid()
        finally:
            L.acx_free_masked(h)


def check_scores(h, s, device):
    L = capi.lib()
    want = i64(s.n_hay)
    assert call("acx_score_host", ptr(s.m), s.n, s.counts.ctypes.data, s.n_hay, W.ctypes.data, 2, want.ctypes.data) == (OK, "")
    want = want[:s.n_hay]
    assert (L.acx_scores_rows(h), L.acx_scores_on_device(h)) == (s.n_hay, int(device))
    assert read_at(L.acx_scores_data(h), want.nbytes, device) == want.tobytes()  # (no row still has an address)
    assert copied("acx_scores_copy", h, nbytes=want.nbytes) == ((OK, ""), want.tobytes())
    assert call("acx_scores_copy", h, None) == ((EINVAL, NULL_TEXT) if s.n_hay else (OK, ""))
    assert copied("acx_scores_copy", h, nbytes=want.nbytes) == ((OK, ""), want.tobytes())


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_scores(world, device):
    a, shapes = world
    for s in shapes.values():
        h = make("acx_score", a, s, device, 0, W.ctypes.data, 2)
        try:
            check_scores(h, s, device)
        finally:
            capi.lib().acx_free_scores(h)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_rows(device):
    L = capi.lib()
    for text in (b"ab\ncd\nef", b""):
        hay = np.frombuffer(text, dtype=np.uint8)
        want, n = i64(len(text) + 1), ctypes.c_uint64(99)
        assert call("acx_split_rows_host", ptr(hay), len(text), 10, want.ctypes.data, len(want), ctypes.byref(n)) == (OK, "")
        want = want[:n.value + 1]
        d_hay = capi.DeviceBuffer(16).upload(hay) if len(text) else None
        out = ctypes.c_void_p()
        src = (d_hay.ptr if d_hay else None) if device else ptr(hay)
        assert call("acx_split_rows_device" if device else "acx_split_rows", src, len(text), 10, ctypes.byref(out)) == (OK, "")
        h = out.value
        try:
            assert (L.acx_rows_count(h), L.acx_rows_bytes(h), L.acx_rows_on_device(h)) == (n.value, len(text), int(device))
            assert read_at(L.acx_rows_offsets(h), want.nbytes, device) == want.tobytes()
            assert copied("acx_rows_copy", h, nbytes=want.nbytes) == ((OK, ""), want.tobytes())
            assert call("acx_rows_copy", h, None) == (EINVAL, NULL_TEXT)
            assert copied("acx_rows_copy", h, nbytes=want.nbytes) == ((OK, ""), want.tobytes())
        finally:
            L.acx_free_rows(h)
            if d_hay:
                d_hay.free()


# ---------------------------------------------------------------------------
# no handle
# ---------------------------------------------------------------------------
def test_null_handles(world):
    """every accessor answers 0 or null to a null handle, every copy refuses it, every free returns; the handle of a live
    result answers behind them"""
    a, shapes = world
    L = capi.lib()
    s = shapes["batch"]
    live = make("acx_find_columns", a, s, True, 0, 0)
    want = want_columns(s)
    dst = np.zeros(8, dtype=np.int64)
    try:
        for kind, (_, _, prefix, range_text, _, sizes) in KINDS.items():
            for name in sizes + ("on_device",):
                assert getattr(L, prefix + "_" + name)(None) == 0, (kind, name)
            assert getattr(L, prefix + "_data")(None, 0) is None
            assert call(prefix + "_copy", None, 0, dst.ctypes.data) == (EINVAL, range_text)
            assert copied("acx_columns_copy", live, 0, nbytes=want[0].nbytes) == ((OK, ""), want[0].tobytes())
            getattr(L, "acx_free_" + prefix[4:])(None)
        for name in ("acx_masked_rows", "acx_masked_bytes", "acx_masked_on_device", "acx_scores_rows", "acx_scores_on_device",
                     "acx_rows_count", "acx_rows_bytes", "acx_rows_on_device", "acx_rows_device"):
            assert getattr(L, name)(None) == 0, name
        for name in ("acx_masked_data", "acx_masked_offsets", "acx_scores_data", "acx_rows_offsets"):
            assert getattr(L, name)(None) is None, name
        for name in ("acx_masked_copy", "acx_masked_copy_offsets", "acx_scores_copy", "acx_rows_copy"):
            assert call(name, None, dst.ctypes.data) == (EINVAL, NULL_TEXT), name
            assert copied("acx_columns_copy", live, 3, nbytes=want[3].nbytes) == ((OK, ""), want[3].tobytes())
        for name in ("acx_free_masked", "acx_free_scores", "acx_free_rows"):
            getattr(L, name)(None)
    finally:
        L.acx_free_columns(live)
