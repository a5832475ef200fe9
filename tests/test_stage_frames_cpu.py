"""CPU checks of what the host forms of the post-find stages share (acx_summarize_host, acx_tally_host, acx_score_host,
acx_mask_host, acx_filter_host): for every bad argument the return code AND the text of acx_last_error(), at the smallest
shapes -- 2 rows, 3 or 4 records, 8 bytes -- and, where two rules are broken at once, which of them is reported.  The texts
are the literal strings of the sources; the results of the valid calls come from a few lines of numpy.
tests/test_gpu_stage_frames.py has the device forms."""
import ctypes

import numpy as np
import pytest

capi = pytest.importorskip("ahocorasick_rs_amd.capi")

OK, EINVAL = capi.OK, capi.EINVAL
COUNTS_TEXT = "the counts do not sum to the number of matches"
OFFSETS_TEXT = "offsets must rise from 0 to the batch's length"
NULL_TEXT = "null argument"
U64_MAX = (1 << 64) - 1
# the counts of two rows (one list has one row): which of them fit depends on the number of records alone
COUNT_LISTS = ([1, 1], [2, 2], [4, 0], [4], [0, 0], [U64_MAX, 4])
# 8 bytes cut badly
BAD_OFFSETS = ([1, 8], [0, 7], [0, 5, 4, 8])

REC = np.asarray([[1, 0, 2], [0, 1, 3], [1, 0, 1], [0, 2, 9]], dtype=np.uint64)  # (pattern, start, end in its row), 2 patterns
HAY = np.frombuffer(b"abcdefgh", dtype=np.uint8).copy()


def u64(xs):
    return np.asarray(xs, dtype=np.uint64)


def ptr(a):
    return None if a is None else a.ctypes.data


def call(name, *args):
    """-> (code, text): the text is read only behind a failure (a success leaves the last one)"""
    L = capi.lib()
    rc = getattr(L, name)(*args)
    return rc, ("" if rc == OK else L.acx_last_error().decode())


def fits(counts, n_m):
    return sum(counts) == n_m  # (Python's integers: no wrap)


# ---------------------------------------------------------------------------
# acx_summarize_host
# ---------------------------------------------------------------------------
def summarize(n_m, counts, n_hay, n_patterns=2, what=3, m=REC, bits=True, first=True, hist=True):
    c = None if counts is None else u64(counts)
    out = (np.full(2, 0xC3, np.uint64), np.zeros(4, dtype=capi.MATCH_DTYPE), np.full(4, 0xC3, np.uint64))
    rc = call("acx_summarize_host", ptr(m), n_m, ptr(c), n_hay, n_patterns, what, ptr(out[0]) if bits else None,
              ptr(out[1]) if first else None, ptr(out[2]) if hist else None)
    return rc, out


@pytest.mark.parametrize("n_m", [3, 4])
def test_summarize_host_counts(n_m):
    for counts in COUNT_LISTS:
        rc, _ = summarize(n_m, counts, len(counts))
        assert rc == ((OK, "") if fits(counts, n_m) else (EINVAL, COUNTS_TEXT)), counts


def test_summarize_host_bad_arguments_and_their_order():
    assert summarize(4, [1, 1], 2, what=4)[0] == (EINVAL, "unknown summary bits")          # ... before the counts
    assert summarize(4, [2, 2], 2, what=1 << 31)[0] == (EINVAL, "unknown summary bits")
    assert summarize(4, [1, 1], 2, m=None)[0] == (EINVAL, "null matches")                   # ... before the counts
    assert summarize(4, [1, 1], 2, m=None, what=8)[0] == (EINVAL, "unknown summary bits")   # ... and behind the bits
    assert summarize(4, [1, 1], 2, bits=False)[0] == (EINVAL, NULL_TEXT)                    # ... before the counts
    assert summarize(4, [2, 2], 2, first=False)[0] == (EINVAL, NULL_TEXT)
    assert summarize(4, [1, 1], 2, hist=False)[0] == (EINVAL, NULL_TEXT)
    assert summarize(4, [2, 2], 2, hist=False, what=1)[0] == (OK, "")                       # a part that is not asked for
    assert summarize(4, [2, 2], 2, bits=False, first=False, what=2)[0] == (OK, "")
    # the counts before the records' patterns
    assert summarize(4, [1, 1], 2, n_patterns=1)[0] == (EINVAL, COUNTS_TEXT)
    assert summarize(4, [2, 2], 2, n_patterns=1)[0] == (EINVAL, "match 0 names pattern 1 of 1")
    # null counts: ONE haystack, whatever n_hay says
    for n_hay in (0, 1, 2):
        rc, (bits, first, hist) = summarize(1, None, n_hay)
        assert rc == (OK, "") and bits[0] == 1 and first[0].tolist() == (1, 0, 2) and list(hist[:2]) == [0, 1], n_hay
        assert summarize(4, None, n_hay)[0] == (OK, "")


def test_summarize_host_valid_call():
    rc, (bits, first, hist) = summarize(4, [3, 1], 2)
    assert rc == (OK, "")
    assert bits[0] == 0b11 and bits[1] == 0xC3
    assert [f.tolist() for f in first[:2]] == [tuple(REC[0]), tuple(REC[3])]
    assert list(hist[:2]) == list(np.bincount(REC[:, 0].astype(np.int64), minlength=2)) and hist[2] == 0xC3
    rc, (bits, first, _) = summarize(4, [4, 0], 2)
    assert rc == (OK, "") and bits[0] == 0b01 and first[1].tolist() == (capi.NO_MATCH, 0, 0)


# ---------------------------------------------------------------------------
# acx_tally_host
# ---------------------------------------------------------------------------
def tally(n_m, counts, n_hay, m=REC, ro=True, outs=True, nnz=True):
    c = None if counts is None else u64(counts)
    out = (np.full(4, -7, np.int64), np.full(4, -7, np.int64), np.full(4, -7, np.int64))
    k = ctypes.c_uint64(99)
    rc = call("acx_tally_host", ptr(m), n_m, ptr(c), n_hay, ptr(out[0]) if ro else None, ptr(out[1]) if outs else None,
              ptr(out[2]) if outs else None, ctypes.byref(k) if nnz else None)
    return rc, out, k.value


@pytest.mark.parametrize("n_m", [3, 4])
def test_tally_host_counts(n_m):
    for counts in COUNT_LISTS:
        rc, _, _ = tally(n_m, counts, len(counts))
        assert rc == ((OK, "") if fits(counts, n_m) else (EINVAL, COUNTS_TEXT)), counts


def test_tally_host_bad_arguments_and_their_order():
    for n_hay in (1, 2):  # null counts with rows: a null argument, not a counts error
        assert tally(4, None, n_hay)[0] == (EINVAL, NULL_TEXT), n_hay
    assert tally(1, None, 0)[0] == (EINVAL, COUNTS_TEXT)     # no row, one record
    assert tally(0, None, 0)[0] == (OK, "")
    assert tally(4, [1, 1], 2, ro=False)[0] == (EINVAL, NULL_TEXT)   # ... before the counts
    assert tally(4, [1, 1], 2, nnz=False)[0] == (EINVAL, NULL_TEXT)
    assert tally(4, [1, 1], 2, m=None)[0] == (EINVAL, NULL_TEXT)
    assert tally(4, [2, 2], 2, outs=False)[0] == (EINVAL, NULL_TEXT)
    assert tally(0, [0, 0], 2, m=None, outs=False)[0] == (OK, "")    # no record: no place for one is needed


def test_tally_host_valid_call():
    rc, (ro, pat, cnt), nnz = tally(4, [3, 1], 2)
    assert rc == (OK, "") and nnz == 3
    want_p, want_c = np.unique(REC[:3, 0].astype(np.int64), return_counts=True)  # row 0; row 1 is one record
    assert list(ro[:3]) == [0, 2, 3] and ro[3] == -7
    assert list(pat[:3]) == list(want_p) + [int(REC[3, 0])] and list(cnt[:3]) == list(want_c) + [1]
    assert pat[3] == -7 and cnt[3] == -7


# ---------------------------------------------------------------------------
# acx_score_host
# ---------------------------------------------------------------------------
W = np.asarray([5, -3], dtype=np.int32)


def score(n_m, counts, n_hay, m=REC, w=W, n_w=2, out=True):
    c = None if counts is None else u64(counts)
    s = np.full(4, -7, np.int64)
    return call("acx_score_host", ptr(m), n_m, ptr(c), n_hay, ptr(w), n_w, ptr(s) if out else None), s


@pytest.mark.parametrize("n_m", [3, 4])
def test_score_host_counts(n_m):
    for counts in COUNT_LISTS:
        rc, _ = score(n_m, counts, len(counts))
        assert rc == ((OK, "") if fits(counts, n_m) else (EINVAL, COUNTS_TEXT)), counts


def test_score_host_bad_arguments_and_their_order():
    assert score(4, None, 2)[0] == (EINVAL, "several haystacks need counts")
    assert score(1, None, 0)[0] == (EINVAL, COUNTS_TEXT)             # no row, one record
    assert score(0, None, 0)[0] == (OK, "")
    assert score(4, None, 1)[0] == (OK, "")                          # one row holds them all
    assert score(4, None, 2, out=False)[0] == (EINVAL, NULL_TEXT)    # the null output before the missing counts
    assert score(4, [1, 1], 2, m=None)[0] == (EINVAL, NULL_TEXT)     # ... and before the counts' sum
    assert score(4, [1, 1], 2, w=None)[0] == (EINVAL, NULL_TEXT)
    assert score(4, [1, 1], 2, w=None, n_w=0)[0] == (EINVAL, COUNTS_TEXT)
    assert score(4, [2, 2], 2, w=None, n_w=0)[0] == (OK, "")         # no weight: nothing to read


def test_score_host_valid_call():
    rc, s = score(4, [3, 1], 2)
    w = W.astype(np.int64)[REC[:, 0].astype(np.int64)]
    assert rc == (OK, "") and list(s) == [int(w[:3].sum()), int(w[3:].sum()), -7, -7]
    rc, s = score(4, None, 1)
    assert rc == (OK, "") and list(s) == [int(w.sum()), -7, -7, -7]


# ---------------------------------------------------------------------------
# acx_mask_host
# ---------------------------------------------------------------------------
def mask(offsets, n_hay, n_m, counts, flags=0, hay=HAY, length=8, m=REC, dst=True, fill=ord("*")):
    o = None if offsets is None else u64(offsets)
    c = None if counts is None else u64(counts)
    out = np.full(12, 0xC3, np.uint8)
    d = None if dst is False else (ptr(out) if dst is True else dst)
    return call("acx_mask_host", ptr(hay), length, ptr(o), n_hay, ptr(m), n_m, ptr(c), fill, flags, d), out


@pytest.mark.parametrize("n_m", [3, 4])
def test_mask_host_counts(n_m):
    for counts in COUNT_LISTS:
        rows = len(counts)
        rc, _ = mask([0, 8] if rows == 1 else [0, 5, 8], rows, n_m, counts)
        assert rc == ((OK, "") if fits(counts, n_m) else (EINVAL, COUNTS_TEXT)), counts


def test_mask_host_offsets():
    for off in BAD_OFFSETS:
        rows = len(off) - 1
        assert mask(off, rows, 4, [4, 0, 0][:rows])[0] == (EINVAL, OFFSETS_TEXT), off
    assert mask(None, 2, 4, [2, 2])[0] == (EINVAL, "several haystacks need offsets")
    assert mask(None, 1, 4, [4])[0] == (OK, "")
    assert mask(None, 0, 4, [4])[0] == (OK, "")   # no offsets: ONE haystack, whatever n_hay says


def test_mask_host_bad_arguments_and_their_order():
    assert mask([0, 5, 8], 2, 4, None)[0] == (EINVAL, "several haystacks need counts")
    assert mask([0, 8], 1, 4, None)[0] == (OK, "")
    assert mask([0], 0, 1, None, length=0)[0] == (EINVAL, COUNTS_TEXT)       # no row, one record
    assert mask([0], 0, 0, None, length=0)[0] == (OK, "")
    for flags in (2, 4, 1 << 31):
        assert mask([1, 8], 1, 4, [1], flags=flags)[0] == (EINVAL, "unknown mask flags"), flags  # ... before offsets and counts
    assert mask([0, 5, 8], 2, 4, [1, 1], flags=2, m=None)[0] == (EINVAL, "unknown mask flags")   # ... and before the nulls
    assert mask([1, 8], 1, 4, [1], m=None)[0] == (EINVAL, NULL_TEXT)                             # the nulls before the offsets
    assert mask([0, 5, 8], 2, 4, [1, 1], dst=False)[0] == (EINVAL, NULL_TEXT)
    assert mask([0, 5, 8], 2, 4, [1, 1], hay=None)[0] == (EINVAL, NULL_TEXT)
    assert mask([0, 5, 8], 2, 4, [1, 1], hay=None, flags=1)[0] == (EINVAL, COUNTS_TEXT)          # the 0 / 1 mask reads no haystack
    assert mask([1, 8], 1, 4, [1], flags=1, dst=ptr(HAY))[0] == (EINVAL, "ACX_MASK_ZERO cannot be made in place")
    assert mask([0, 7], 1, 4, [1, 1])[0] == (EINVAL, OFFSETS_TEXT)                               # the offsets before the counts
    assert mask(None, 2, 4, None)[0] == (EINVAL, "several haystacks need offsets")               # ... the missing ones as well
    assert mask([0, 5, 4, 8], 3, 4, None)[0] == (EINVAL, OFFSETS_TEXT)
    rc, out = mask([0, 5, 8], 2, 4, [1, 1])                                                      # a refusal writes nothing
    assert rc == (EINVAL, COUNTS_TEXT) and (out == 0xC3).all()


@pytest.mark.parametrize("flags", [0, 1])
def test_mask_host_valid_call(flags):
    off, counts = [0, 5, 8], [2, 2]
    rc, out = mask(off, 2, 4, counts, flags=flags)
    want = np.zeros(8, np.uint8) if flags else HAY.copy()
    row = np.repeat(np.arange(2), counts)
    for (_, s, e), r in zip(REC.tolist(), row):
        lo, hi = off[r], off[r + 1]
        want[lo + min(s, hi - lo):lo + min(e, hi - lo)] = ord("*")
    assert rc == (OK, "") and np.array_equal(out[:8], want) and (out[8:] == 0xC3).all()


# ---------------------------------------------------------------------------
# acx_filter_host
# ---------------------------------------------------------------------------
def filt(offsets, n_hay, counts, min_matches=1, flags=0, hay=HAY, length=8, sizes=True, outs=True):
    o = None if offsets is None else u64(offsets)
    c = None if counts is None else u64(counts)
    out = (np.full(4, -7, np.int64), np.full(4, -7, np.int64), np.full(12, 0xC3, np.uint8))
    k, nb = ctypes.c_uint64(99), ctypes.c_uint64(99)
    rc = call("acx_filter_host", ptr(hay), length, ptr(o), n_hay, ptr(c), min_matches, flags, *[ptr(x) if outs else None for x in out],
              ctypes.byref(k) if sizes else None, ctypes.byref(nb) if sizes else None)
    return rc, out, (k.value, nb.value)


def test_filter_host_offsets():
    for off in BAD_OFFSETS:
        rows = len(off) - 1
        assert filt(off, rows, [1, 0, 1][:rows])[0] == (EINVAL, OFFSETS_TEXT), off
    assert filt(None, 2, [1, 0])[0] == (EINVAL, "several haystacks need offsets")
    assert filt(None, 1, [0])[0] == (OK, "")


def test_filter_host_bad_arguments_and_their_order():
    for flags in (2, 4, 1 << 31):
        assert filt([1, 8], 1, [1], flags=flags, min_matches=0)[0] == (EINVAL, "unknown filter flags"), flags
    assert filt([1, 8], 1, [1], min_matches=0)[0] == (EINVAL, "min_matches must be at least 1")  # ... before the offsets
    assert filt([0, 5, 8], 2, [1, 1], min_matches=0, sizes=False)[0] == (EINVAL, "min_matches must be at least 1")
    assert filt([1, 8], 1, [1], sizes=False)[0] == (EINVAL, NULL_TEXT)                           # the nulls before the offsets
    assert filt([0, 7], 1, None)[0] == (EINVAL, NULL_TEXT)
    assert filt([0, 5, 8], 2, [1, 1], hay=None)[0] == (EINVAL, NULL_TEXT)
    assert filt([0, 5, 8], 2, [1, 1], hay=None, outs=False)[0] == (OK, "")                       # sizes only: no byte is read
    assert filt([0], 0, None, length=0)[0] == (OK, "")
    rc, out, _ = filt([0, 5, 4, 8], 3, [1, 1, 1])                                                # a refusal writes nothing
    assert rc == (EINVAL, OFFSETS_TEXT) and all((x == x[0]).all() for x in out)


@pytest.mark.parametrize("flags", [0, capi.FILTER_KEEP_MATCHED])
def test_filter_host_valid_call(flags):
    off, counts = np.asarray([0, 5, 8]), np.asarray([0, 2])
    rc, (rows, oo, data), (k, nb) = filt(off, 2, counts, min_matches=2, flags=flags)
    keep = np.flatnonzero((counts >= 2) == bool(flags))
    want = b"".join(HAY.tobytes()[off[h]:off[h + 1]] for h in keep)
    assert rc == (OK, "") and (k, nb) == (len(keep), len(want))
    assert list(rows[:k]) == list(keep) and list(oo[:k + 1]) == [0, len(want)] and data[:nb].tobytes() == want
    assert (rows[k:] == -7).all() and (oo[k + 1:] == -7).all() and (data[nb:] == 0xC3).all()
    assert filt(off, 2, counts, min_matches=2, flags=flags, outs=False)[2] == (k, nb)
