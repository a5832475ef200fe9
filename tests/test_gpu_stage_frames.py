"""The frame of the five *_rows_device entry points (acx_score_rows_device, acx_mask_rows_device, acx_tally_rows_device,
acx_filter_rows_device, acx_split_rows_into_device) at the smallest shapes -- 2 rows, 3 records, 8 bytes, 2 patterns: the code
and the text of every refusal the entries share, a valid call straight behind each refusal (the temporaries of the failed
call are back and nothing of it is reused), and every entry's own answer to an empty call.  The texts are the literal strings
of the sources, the results a few lines of numpy.  The stages' kernels at their seams are test_gpu_{score,mask,tally,filter,
rows}.py's; tests/test_stage_frames_cpu.py has the host forms."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
capi = pytest.importorskip("ahocorasick_rs_amd.capi")

OK, EINVAL = capi.OK, capi.EINVAL
RECORDS_TEXT = "the counts do not sum to the number of records"
OFFSETS_TEXT = "offsets must rise from 0 to the batch's length"
EXCLUDE_TEXT = "offsets and uniform_len exclude one another"
UNIFORM_TEXT = "n_hay * uniform_len is not the batch's length"
GUARD = 0xC3
GUARD64 = int.from_bytes(bytes([GUARD]) * 8, "little", signed=True)

HAY = np.frombuffer(b"abcdefgh", dtype=np.uint8)
OFF = [0, 5, 8]
REC = np.asarray([[1, 0, 2], [0, 1, 3], [1, 0, 2]], dtype=np.uint64)  # (pattern, start, end in its row)
GOOD, BAD = [2, 1], [1, 1]
W = np.asarray([5, -3], dtype=np.int32)


@pytest.fixture()
def dev():
    """dev(array) -> a device buffer that holds the array's bytes; every one is freed behind the test"""
    made = []

    def up(arr, room=0):
        a = np.ascontiguousarray(arr)
        b = capi.DeviceBuffer(max(a.nbytes, room, 16))
        made.append(b)
        return b.upload(a) if a.nbytes else b

    yield up
    for b in made:
        b.free()


def guard(nbytes):
    return np.full(nbytes, GUARD, dtype=np.uint8)


def call(name, *args):
    """-> (code, text): the text is read only behind a failure (a success leaves the last one)"""
    L = capi.lib()
    rc = getattr(L, name)(*args)
    return rc, ("" if rc == OK else L.acx_last_error().decode())


def words(buf, n):
    return list(buf.download(8 * n).view(np.int64))


# ---------------------------------------------------------------------------
# score
# ---------------------------------------------------------------------------
def test_score_rows_device(dev):
    d_m, d_w, d_good, d_bad = dev(REC), dev(W), dev(np.asarray(GOOD, np.uint64)), dev(np.asarray(BAD, np.uint64))
    out = dev(guard(32))
    w = W.astype(np.int64)[REC[:, 0].astype(np.int64)]
    want = [int(w[:2].sum()), int(w[2:].sum()), GUARD64, GUARD64]
    for _ in range(2):  # a refusal, then the valid call; and once more behind a success
        assert call("acx_score_rows_device", d_m.ptr, 3, d_bad.ptr, 2, d_w.ptr, 2, out.ptr) == (EINVAL, RECORDS_TEXT)
        assert call("acx_score_rows_device", d_m.ptr, 3, d_good.ptr, 2, d_w.ptr, 2, out.ptr) == (OK, "")
        assert words(out, 4) == want
    # no row: nothing is asked of the device, not even where the scores lie
    assert call("acx_score_rows_device", None, 0, None, 0, None, 0, None) == (OK, "")
    assert call("acx_score_rows_device", d_m.ptr, 0, d_good.ptr, 0, d_w.ptr, 2, out.ptr) == (OK, "") and words(out, 4) == want
    assert call("acx_score_rows_device", d_m.ptr, 3, d_good.ptr, 0, d_w.ptr, 2, out.ptr) == (EINVAL, RECORDS_TEXT)  # records but no rows
    assert call("acx_score_rows_device", d_m.ptr, 3, d_good.ptr, 0, None, 2, None) == (EINVAL, RECORDS_TEXT)        # ... before the nulls
    assert call("acx_score_rows_device", d_m.ptr, 3, d_bad.ptr, 2, d_w.ptr, 2, None) == (EINVAL, "null argument")
    assert call("acx_score_rows_device", d_m.ptr, 3, d_bad.ptr, 2, d_w.ptr + 2, 2, out.ptr) == (EINVAL, "the weights must be 4-byte aligned")
    assert call("acx_score_rows_device", d_m.ptr, 3, d_good.ptr, 2, d_w.ptr, 2, out.ptr) == (OK, "") and words(out, 4) == want


# ---------------------------------------------------------------------------
# tally
# ---------------------------------------------------------------------------
def test_tally_rows_device(dev):
    d_m, d_good, d_bad = dev(REC), dev(np.asarray(GOOD, np.uint64)), dev(np.asarray(BAD, np.uint64))
    ro, pat, cnt = dev(guard(32)), dev(guard(32)), dev(guard(32))
    nnz = ctypes.c_uint64(99)
    args = (2, 2, ro.ptr, pat.ptr, cnt.ptr, ctypes.byref(nnz))
    want_p, want_c = np.unique(REC[:2, 0].astype(np.int64), return_counts=True)  # row 0; row 1 is one record
    for _ in range(2):
        assert call("acx_tally_rows_device", d_m.ptr, 3, d_bad.ptr, *args) == (EINVAL, RECORDS_TEXT) and nnz.value == 0
        assert call("acx_tally_rows_device", d_m.ptr, 3, d_good.ptr, *args) == (OK, "") and nnz.value == 3
        assert words(ro, 4) == [0, 2, 3, GUARD64]
        assert words(pat, 4) == list(want_p) + [int(REC[2, 0]), GUARD64] and words(cnt, 4) == list(want_c) + [1, GUARD64]
    # no row: one offset, 0, is written and waited for
    ro2 = dev(guard(16))
    nnz.value = 99
    assert call("acx_tally_rows_device", None, 0, None, 0, 2, ro2.ptr, None, None, ctypes.byref(nnz)) == (OK, "")
    assert nnz.value == 0 and words(ro2, 2) == [0, GUARD64]
    assert call("acx_tally_rows_device", d_m.ptr, 3, None, 0, 2, ro2.ptr, pat.ptr, cnt.ptr, ctypes.byref(nnz)) == (EINVAL, RECORDS_TEXT)
    assert call("acx_tally_rows_device", d_m.ptr, 3, None, 0, 1 << 25, ro2.ptr, pat.ptr, cnt.ptr, ctypes.byref(nnz)) == (
        EINVAL, "more than 2^24 patterns")                                                           # ... before "records but no rows"
    assert call("acx_tally_rows_device", d_m.ptr, 3, d_bad.ptr, 2, 2, None, pat.ptr, cnt.ptr, ctypes.byref(nnz)) == (EINVAL, "null argument")
    assert call("acx_tally_rows_device", d_m.ptr, 3, d_good.ptr, *args) == (OK, "") and nnz.value == 3 and words(ro, 3) == [0, 2, 3]


# ---------------------------------------------------------------------------
# mask
# ---------------------------------------------------------------------------
def painted(fill=ord("*")):
    want = HAY.copy()
    for (_, s, e), r in zip(REC.tolist(), np.repeat(np.arange(2), GOOD)):
        lo, n = OFF[r], OFF[r + 1] - OFF[r]
        want[lo + min(s, n):lo + min(e, n)] = fill
    return want


def test_mask_rows_device(dev):
    d_hay, d_off, d_off7 = dev(HAY), dev(np.asarray(OFF, np.uint64)), dev(np.asarray([0, 5, 7], np.uint64))
    d_m, d_good, d_bad = dev(REC), dev(np.asarray(GOOD, np.uint64)), dev(np.asarray(BAD, np.uint64))
    fill = ord("*")

    def mask(d_offsets, n_hay, uniform, d_counts, length=8, n=3, flags=0):
        out = dev(guard(24))
        rc = call("acx_mask_rows_device", d_hay.ptr, length, d_offsets, n_hay, uniform, d_m.ptr, n, d_counts, fill, flags, out.ptr + 8)
        return rc, out.download(24)

    def valid():
        rc, got = mask(d_off.ptr, 2, 0, d_good.ptr)
        assert rc == (OK, "") and np.array_equal(got[8:16], painted()) and (got[:8] == GUARD).all() and (got[16:] == GUARD).all()

    for _ in range(2):
        rc, got = mask(d_off.ptr, 2, 0, d_bad.ptr)
        assert rc == (EINVAL, RECORDS_TEXT)
        assert np.array_equal(got[8:16], HAY), "the copy runs in front of the counts' check"
        assert (got[:8] == GUARD).all() and (got[16:] == GUARD).all()
        valid()
    for what, (args, text) in {
            "offsets and a row length": ((d_off.ptr, 2, 4, d_good.ptr), EXCLUDE_TEXT),
            "rows that do not fill the batch": ((None, 2, 3, d_good.ptr), UNIFORM_TEXT),
            "offsets that end at 7": ((d_off7.ptr, 2, 0, d_good.ptr), OFFSETS_TEXT),
            "offsets and a row length, and unknown flags": ((d_off.ptr, 2, 4, d_good.ptr, 8, 3, 2), "unknown mask flags"),
            "offsets and a row length, and records but no rows": ((d_off.ptr, 0, 4, d_good.ptr), EXCLUDE_TEXT),
            "offsets that end at 7 and counts that do not sum": ((d_off7.ptr, 2, 0, d_bad.ptr), OFFSETS_TEXT),
    }.items():
        rc, got = mask(*args)
        assert rc == (EINVAL, text), what
        assert (got == GUARD).all(), (what, "a refusal in front of the stage writes nothing")
        valid()
    rc, got = mask(None, 2, 4, d_good.ptr)  # the same rows by their length
    want = painted()
    want[5:8] = HAY[5:8]
    want[4:6] = fill  # (row 1 begins at 4: its record covers bytes 4 and 5)
    assert rc == (OK, "") and np.array_equal(got[8:16], want)
    # no byte: the checks, then nothing; no rows (offsets that cut nothing) is no different
    d_off0 = dev(np.zeros(3, np.uint64))
    for args in ((d_off0.ptr, 2, 0, d_good.ptr, 0, 0), (d_off0.ptr, 0, 0, None, 0, 0), (None, 0, 0, None, 0, 0)):
        rc, got = mask(*args)
        assert rc == (OK, "") and (got == GUARD).all(), args
    assert mask(d_off0.ptr, 0, 0, d_good.ptr, 0, 3)[0] == (EINVAL, RECORDS_TEXT)  # records but no rows, in front of "no byte"
    assert mask(d_off0.ptr, 2, 4, d_good.ptr, 0, 0)[0] == (EINVAL, EXCLUDE_TEXT)
    valid()


# ---------------------------------------------------------------------------
# filter
# ---------------------------------------------------------------------------
def test_filter_rows_device(dev):
    d_hay, d_off, d_off7 = dev(HAY), dev(np.asarray(OFF, np.uint64)), dev(np.asarray([0, 5, 7], np.uint64))
    d_counts = dev(np.asarray(GOOD, np.uint64))
    k, nb = ctypes.c_uint64(99), ctypes.c_uint64(99)

    def filt(d_offsets, n_hay, uniform, length=8, min_matches=2, flags=capi.FILTER_KEEP_MATCHED):
        rows, oo, data = dev(guard(24)), dev(guard(32)), dev(guard(32))
        k.value = nb.value = 99
        rc = call("acx_filter_rows_device", d_hay.ptr, length, d_offsets, n_hay, uniform, d_counts.ptr, min_matches, flags, rows.ptr,
                  oo.ptr, data.ptr, ctypes.byref(k), ctypes.byref(nb))
        return rc, (k.value, nb.value), words(rows, 3), words(oo, 4), data.download(32)

    def valid():
        rc, sizes, rows, oo, data = filt(d_off.ptr, 2, 0)  # row 0 has its 2 matches
        assert rc == (OK, "") and sizes == (1, 5)
        assert rows == [0, GUARD64, GUARD64] and oo == [0, 5, GUARD64, GUARD64]
        assert data[:5].tobytes() == HAY[:5].tobytes() and (data[16:] == GUARD).all()

    valid()
    for what, (args, text, sizes_left) in {  # (the sizes are zeroed behind the first checks)
            "offsets and a row length": ((d_off.ptr, 2, 4), EXCLUDE_TEXT, (0, 0)),
            "rows that do not fill the batch": ((None, 2, 3), UNIFORM_TEXT, (0, 0)),
            "offsets that end at 7": ((d_off7.ptr, 2, 0), OFFSETS_TEXT, (0, 0)),
            "offsets and a row length, and unknown flags": ((d_off.ptr, 2, 4, 8, 2, 2), "unknown filter flags", (99, 99)),
            "offsets and a row length, and no threshold": ((d_off.ptr, 2, 4, 8, 0), "min_matches must be at least 1", (99, 99)),
    }.items():
        rc, sizes, rows, oo, data = filt(*args)
        assert rc == (EINVAL, text) and sizes == sizes_left, what
        assert rows == [GUARD64] * 3 and oo == [GUARD64] * 4 and (data == GUARD).all(), (what, "a refusal writes nothing")
        valid()
    rc, sizes, rows, oo, data = filt(None, 2, 4, min_matches=1)  # the same bytes as rows of 4: both have a match
    assert rc == (OK, "") and sizes == (2, 8) and rows[:2] == [0, 1] and oo[:3] == [0, 4, 8] and data[:8].tobytes() == HAY.tobytes()
    # no row: one offset, 0, is written and waited for
    d_off0 = dev(np.zeros(1, np.uint64))
    rc, sizes, rows, oo, data = filt(d_off0.ptr, 0, 0, length=0)
    assert rc == (OK, "") and sizes == (0, 0) and oo == [0, GUARD64, GUARD64, GUARD64] and rows == [GUARD64] * 3 and (data == GUARD).all()
    valid()


# ---------------------------------------------------------------------------
# split_rows
# ---------------------------------------------------------------------------
def test_split_rows_into_device(dev):
    text = np.frombuffer(b"ab\ncd\nef", dtype=np.uint8)
    want = [0, 3, 6, 8]
    d_hay = dev(text)
    n = ctypes.c_uint64(99)
    for _ in range(2):
        out = dev(guard(48))
        rc = call("acx_split_rows_into_device", d_hay.ptr, 8, 10, out.ptr + 8, 3, ctypes.byref(n))  # one word short
        assert rc[0] == EINVAL and n.value == 3 and rc[1] == "the offsets buffer holds 3 words, 4 are needed"
        assert str(len(want)) in rc[1]
        assert (out.download(48) == GUARD).all(), "a word was written although the buffer is too small"
        assert call("acx_split_rows_into_device", d_hay.ptr, 8, 10, out.ptr + 8, 4, ctypes.byref(n)) == (OK, "") and n.value == 3
        assert words(out, 6) == [GUARD64] + want + [GUARD64]
    # no byte: no row, the one word 0 -- a copy, no kernel
    out = dev(guard(24))
    n.value = 99
    assert call("acx_split_rows_into_device", None, 0, 10, out.ptr + 8, 1, ctypes.byref(n)) == (OK, "") and n.value == 0
    assert words(out, 3) == [GUARD64, 0, GUARD64]
    assert call("acx_split_rows_into_device", None, 0, 10, None, 0, ctypes.byref(n)) == (OK, "")
    assert call("acx_split_rows_into_device", None, 0, 10, out.ptr + 8, 0, ctypes.byref(n)) == (
        EINVAL, "the offsets buffer holds 0 words, 1 are needed")
    assert call("acx_split_rows_into_device", d_hay.ptr, 8, 10, None, 0, ctypes.byref(n)) == (OK, "") and n.value == 3  # count only
