"""The row cut on the device (acx_split_rows_into_device / acx_split_rows_device; split_rows -> RowOffsets): the stage alone
at the seams of its tile kernels -- lengths around the 16-byte line and around the tile, every residue of the input's address,
delimiters at the first and the last byte and on both sides of every tile seam, every byte a delimiter, the bytes an inexact
SWAR compare confuses, a tile scan of two levels -- with guard words around the output, guard bytes THAT ARE THE DELIMITER
around the input, and the input verified unwritten; the owning call; the Python function on tensors in HBM with torch as the
consumer, its offsets passed to the six tensor-taking methods of both classes, lifetime and threads.  Expected values come
from numpy (the definition restated below), never from the library; equality is exact; the kernel's sizes are read from its
header."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
capi = pytest.importorskip("ahocorasick_rs_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ahocorasick_rs_amd", "csrc")


def hip_constants(path, names):
    src = open(os.path.join(CSRC, path)).read()
    out = {}
    for n in names:
        m = re.search(r"\b%s\s*=\s*(\d+)\s*[,;]" % n, src)
        assert m, f"{n} is no longer a plain constant of {path}"
        out[n] = int(m.group(1))
    return out


_C = hip_constants("rows.hpp", ("ROWS_THREADS", "ROWS_TILE"))
THREADS, T = _C["ROWS_THREADS"], _C["ROWS_TILE"]
S = 2048  # replace_scan's items per workgroup (replace.hip RS_THREADS * RS_PER): beyond it the scan has two levels
GUARD = -0x3C3C3C3C3C3C3C3D
DELIMITERS = (0x0A, 0x00, 0xFF, 0x80)
LENGTHS = (0, 1, 15, 16, 17, T - 1, T, T + 1, 3 * T + 5)


def test_constants_are_what_the_sizes_below_assume():
    assert THREADS % 64 == 0 and T % (16 * THREADS) == 0 and T >= 256
    src = open(os.path.join(CSRC, "replace.hip")).read()
    assert re.search(r"RS_THREADS = 256, RS_PER = 8\b", src), "the scan's level size is no longer 2048"


def definition(a, d):
    """0; p + 1 for every position p with a[p] == d, ascending; len(a) if it is not empty and its last byte is not d"""
    a = np.asarray(a, dtype=np.uint8)
    cuts = np.flatnonzero(a == d).astype(np.int64) + 1
    tail = [len(a)] if len(a) and a[-1] != d else []
    return np.concatenate([np.zeros(1, np.int64), cuts, np.asarray(tail, dtype=np.int64)])


def other(d):
    return (d ^ 0x55) or 1  # a byte that is not the delimiter


def trap_alphabet(d):
    """the bytes an inexact SWAR compare confuses with d: a borrow out of a matching byte makes d ^ 1 behind it look equal"""
    return np.asarray([d, d ^ 1, d ^ 0x80, (d + 1) & 0xFF, (d - 1) & 0xFF], dtype=np.uint8)


def run_stage(hay, d, res=0, what=None):
    """split_rows_into_device on `hay` at address residue `res` modulo 16, between bytes that ARE the delimiter (a load that
    counts a byte outside the input changes the result); the output between 8 guard words on either side, exactly rows + 1
    words of capacity -> checked against the definition; the guards and the input checked unwritten"""
    hay = np.ascontiguousarray(np.asarray(hay, dtype=np.uint8))
    nb = len(hay)
    want = definition(hay, d)
    lead = 64 + res
    image = np.full(lead + nb + 48, d, dtype=np.uint8)
    image[lead:lead + nb] = hay
    d_hay = capi.DeviceBuffer(len(image) + 16).upload(image)
    out_image = np.full(8 + len(want) + 8, GUARD, dtype=np.int64)
    d_out = capi.DeviceBuffer(8 * len(out_image)).upload(out_image.view(np.uint8))
    try:
        assert d_hay.ptr % 16 == 0 and d_out.ptr % 8 == 0
        rows = capi.split_rows_into_device(d_hay.ptr + lead if nb else 0, nb, d, d_out.ptr + 64, len(want))
        got = d_out.download(8 * len(out_image)).view(np.int64)
        after = d_hay.download(len(image))
    finally:
        d_hay.free()
        d_out.free()
    assert np.array_equal(after, image), (what, "the input was written")
    assert (got[:8] == GUARD).all(), (what, res, nb, "a word before the output was written")
    assert (got[8 + len(want):] == GUARD).all(), (what, res, nb, "a word behind the output was written")
    assert rows == len(want) - 1, (what, res, nb, rows, len(want) - 1)
    mine = got[8:8 + len(want)]
    if not np.array_equal(mine, want):
        bad = int(np.flatnonzero(mine != want)[0])
        raise AssertionError((what, "delimiter", d, "residue", res, "bytes", nb, "rows", rows, "first difference at word", bad,
                              mine[max(bad - 2, 0):bad + 4].tolist(), want[max(bad - 2, 0):bad + 4].tolist()))
    return want


def seam_cases(n, res, d):
    """(name, bytes): the placements of the delimiter that each length is checked with.  A tile may be cut by position or by
    the address's 16-byte lines, so both kinds of seam get a delimiter on either side."""
    o = other(d)
    plain = np.full(n, o, dtype=np.uint8)
    yield "no delimiter", plain
    if n:
        a = plain.copy()
        a[0] = d
        yield "the first byte only", a
        a = plain.copy()
        a[-1] = d
        yield "the last byte only", a
    if n > 256:
        a = plain.copy()
        for seam in list(range(T, n + 1, T)) + [k * T - res for k in range(1, n // T + 2)]:
            for p in (seam - 1, seam):
                if 0 <= p < n:
                    a[p] = d
        yield "the last byte of every tile and the first of the next", a
    if n:
        rng = np.random.default_rng(n * 16 + res)
        yield "the SWAR trap's alphabet", trap_alphabet(d)[rng.integers(0, 5, size=n)]


@pytest.mark.parametrize("n", LENGTHS)
def test_stage_lengths_crossed_with_every_residue(n):
    for res in range(16):
        for what, hay in seam_cases(n, res, 0x0A):
            run_stage(hay, 0x0A, res, what)


@pytest.mark.parametrize("res", range(16))
def test_stage_every_byte_a_delimiter(res):
    n = 2 * T + 3
    want = run_stage(np.full(n, 0x0A, dtype=np.uint8), 0x0A, res, "every byte")
    assert len(want) == n + 1  # (rows of one byte each: 8 bytes of output per byte of input)
    run_stage(np.full(n, 0xFF, dtype=np.uint8), 0xFF, res, "every byte")


@pytest.mark.parametrize("d", DELIMITERS)
def test_stage_random_densities_and_the_swar_trap(d):
    rng = np.random.default_rng(20261019 + d)
    for n, res in ((3 * T + 5, 0), (2 * T - 7, 5), (T + 1, 15), (777, 9)):
        for p in (2, 64, 1000):
            hay = np.full(n, other(d), dtype=np.uint8)
            hay[rng.integers(0, p, size=n) == 0] = d
            run_stage(hay, d, res, ("density 1/%d" % p, n))
        # only bytes that differ from d in one bit or by one: everything an inexact compare could take for d
        hay = trap_alphabet(d)[rng.integers(0, 5, size=n)]
        run_stage(hay, d, res, ("the trap's alphabet", n))
        hay = trap_alphabet(d)[1:][rng.integers(0, 4, size=n)]
        assert len(run_stage(hay, d, res, ("the trap's alphabet without d", n))) == 2
        for at in range(16):  # d ^ 1 right behind a d at every place of a 16-byte line
            hay = np.full(48, other(d), dtype=np.uint8)
            hay[at], hay[at + 1] = d, d ^ 1
            run_stage(hay, d, res, ("d ^ 1 behind d", at))


def test_stage_a_tile_scan_of_two_levels():
    """more tiles than one workgroup of the scan takes: the tiles' bases come from the scan's second level"""
    n = (S + 1) * T
    hay = np.full(n, ord("a"), dtype=np.uint8)
    hay[999::1000] = 0x0A
    want = run_stage(hay, 0x0A, 3, "2049 tiles")
    assert len(want) == n // 1000 + 2 and (n + 3 + T - 1) // T > S


def test_stage_capacity_count_only_and_arguments():
    L = capi.lib()
    hay = np.frombuffer(b"one\ntwo\nthree\nfour", dtype=np.uint8)
    want = definition(hay, 10)
    d_hay = capi.DeviceBuffer(64).upload(np.concatenate([np.full(5, 10, np.uint8), hay, np.full(8, 10, np.uint8)]))
    out_image = np.full(16, GUARD, dtype=np.int64)
    d_out = capi.DeviceBuffer(128).upload(out_image.view(np.uint8))
    n = ctypes.c_uint64(99)
    try:
        p = d_hay.ptr + 5
        assert capi.split_rows_into_device(p, len(hay), 10, 0, 0) == len(want) - 1  # d_offsets == NULL: count only
        for capacity in (len(want) - 1, 1, 0):  # one word short, and shorter: nothing is written, the count is reported
            rc = L.acx_split_rows_into_device(p, len(hay), 10, d_out.ptr + 64, capacity, ctypes.byref(n))
            assert rc == capi.EINVAL and n.value == len(want) - 1, capacity
            assert str(len(want)) in L.acx_last_error().decode(), L.acx_last_error()
            assert (d_out.download(128).view(np.int64) == GUARD).all(), "a word was written although the buffer is too small"
        assert L.acx_split_rows_into_device(p, len(hay), 10, d_out.ptr + 64 + 4, 8, ctypes.byref(n)) == capi.EINVAL  # misaligned
        assert (d_out.download(128).view(np.int64) == GUARD).all()
        # len == 0: no rows, the one word 0, a null input allowed
        assert capi.split_rows_into_device(0, 0, 10, d_out.ptr + 64, 1) == 0
        got = d_out.download(128).view(np.int64)
        assert got[8] == 0 and (got[:8] == GUARD).all() and (got[9:] == GUARD).all()
        assert L.acx_split_rows_into_device(p, 0, 10, d_out.ptr + 64, 0, ctypes.byref(n)) == capi.EINVAL  # no room for the one word
        assert capi.split_rows_into_device(0, 0, 10, 0, 0) == 0
    finally:
        d_hay.free()
        d_out.free()


@pytest.mark.parametrize("res", [0, 7])
def test_the_owning_call(res):
    rng = np.random.default_rng(res)
    for n, d, p in ((0, 10, 1), (1, 10, 1), (40, 0, 3), (T + 9, 10, 80), (5 * T + 1, 0xFF, 2), (3 * T, 10, 1 << 30)):
        hay = np.full(n, other(d), dtype=np.uint8)
        hay[rng.integers(0, p, size=n) == 0] = d
        want = definition(hay, d)
        image = np.concatenate([np.full(16 + res, d, np.uint8), hay, np.full(32, d, np.uint8)])
        d_hay = capi.DeviceBuffer(len(image) + 16).upload(image)
        try:
            r = capi.split_rows_device(d_hay.ptr + 16 + res if n else 0, n, d)
            assert r.rows == len(want) - 1, (n, d, "the count is valid at return")
            assert r.on_device and r.nbytes == n and r.device == 0
            assert np.array_equal(r.offsets(), want), (n, d, p)
            ptr = r.offsets_ptr()
            assert ptr and ptr % 8 == 0
            again = np.zeros(len(want), dtype=np.int64)
            capi._check(capi.lib().acx_device_download(again.ctypes.data, ptr, 8 * len(want)))
            assert np.array_equal(again, want)
            assert np.array_equal(d_hay.download(len(image)), image), "the input was written"
            r.free()
        finally:
            d_hay.free()


_TENSOR_SCRIPT = r"""
import gc
import sys
import threading
import torch  # first: one process holds ONE HIP runtime, and torch must be the one to load it
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import numpy as np
import ahocorasick_rs as ar

def definition(a, d):
    a = np.asarray(a, dtype=np.uint8)
    cuts = np.flatnonzero(a == d).astype(np.int64) + 1
    tail = [len(a)] if len(a) and a[-1] != d else []
    return np.concatenate([np.zeros(1, np.int64), cuts, np.asarray(tail, dtype=np.int64)])

def host(col):
    return torch.from_dlpack(col).cpu().numpy().copy()

# a small text: a few hundred lines, empty lines (a row of one byte) among them, the last one unterminated
words = "the quick brown Fox jumps over the lazy dog and runs Far away from needle to NEEDLE".split()
rng = np.random.default_rng(7)
lines = []
for i in range(300):
    k = int(rng.integers(0, 9))
    lines.append(" ".join(words[int(j)] for j in rng.integers(0, len(words), size=k)))
text = ("\n".join(lines) + "\nthe end without a newline").encode()
assert b"\r" not in text and text.count(b"\n") == 300
data = np.frombuffer(text, dtype=np.uint8).copy()
want = definition(data, 10)
t = torch.from_numpy(data.copy()).to("cuda:0")

# split_rows on a tensor in HBM
ro = ar.split_rows(t)
assert isinstance(ro, ar.RowOffsets) and ro.device == 0 and ro.nbytes == len(text) and len(ro) == len(want) - 1 == 301
off = torch.from_dlpack(ro.offsets)
assert off.dtype == torch.int64 and off.device == t.device and tuple(off.shape) == (len(want),) and off.is_contiguous()
assert np.array_equal(off.cpu().numpy(), want) and ro.tolist() == want.tolist()
assert ro.offsets.__dlpack_device__() == (10, 0)
assert torch.equal(t.cpu(), torch.from_numpy(data)), "the input was written"
# a slice at an odd address, other delimiters, a tensor produced on another stream just before the call
for lo in (1, 3, 16, 29):
    assert np.array_equal(host(ar.split_rows(t[lo:]).offsets), definition(data[lo:], 10)), lo
assert np.array_equal(host(ar.split_rows(t, " ").offsets), definition(data, 32))
assert np.array_equal(host(ar.split_rows(t, delimiter=ord("e")).offsets), definition(data, ord("e")))
side = torch.cuda.Stream()
with torch.cuda.stream(side):
    big = torch.full((1 << 22,), 97, dtype=torch.uint8, device="cuda:0")
    big[4095::4096] = 10
    rb = ar.split_rows(big)
assert len(rb) == 1024 and torch.equal(torch.from_dlpack(rb.offsets), torch.arange(0, (1 << 22) + 1, 4096, device="cuda:0"))
# a host tensor, the empty tensor
rh = ar.split_rows(torch.from_numpy(data))
assert rh.device is None and np.array_equal(np.from_dlpack(rh.offsets), want)
re_ = ar.split_rows(torch.zeros(0, dtype=torch.uint8, device="cuda:0"))
assert len(re_) == 0 and re_.nbytes == 0 and torch.from_dlpack(re_.offsets).tolist() == [0]
for bad in (t.to(torch.int32), t[::2], t[:len(text) // 2 * 2].reshape(2, -1)):
    try:
        ar.split_rows(bad)
    except (TypeError, BufferError):
        pass
    else:
        raise AssertionError(("accepted", bad.dtype, tuple(bad.shape)))

# the six tensor-taking methods: offsets=ro.offsets gives exactly what the uploaded numpy offsets give
d_want = torch.from_numpy(want).to("cuda:0")
spats = ["needle", "fox", "the", "lazy dog", "x\n", "\nthe", "ay\nfrom", "quick", "over the", "far", "e", "runs far"]
weights = [3, -2, 1, 5, 7, -11, 13, 2, -1, 4, 1, -6]

def snap(r):
    if isinstance(r, ar.PatternCounts):
        return ("pc", r.shape, host(r.row_offsets), host(r.pattern), host(r.count))
    if isinstance(r, ar.FilteredRows):
        return ("fr", r.source_rows, len(r), r.nbytes, host(r.rows), host(r.offsets), host(r.data))
    if isinstance(r, ar.RowScores):
        return ("rs", len(r), host(r.score))
    assert isinstance(r, ar.MaskedRows)
    return ("mr", len(r), r.nbytes, host(r.offsets), host(r.data))

def same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y, (a[0], x, y)

def calls(a, star, ov):
    yield "count_by_pattern_sparse_batch", lambda o: a.count_by_pattern_sparse_batch(t, ov, offsets=o)
    yield "filter_batch", lambda o: a.filter_batch(t, ov, offsets=o)
    yield "filter_batch matched", lambda o: a.filter_batch(t, ov, keep="matched", min_matches=2, offsets=o)
    yield "score_batch", lambda o: a.score_batch(t, weights, ov, offsets=o)
    yield "filter_by_score_batch", lambda o: a.filter_by_score_batch(t, weights, ov, min_score=2, offsets=o)
    yield "mask_all_batch", lambda o: a.mask_all_batch(t, star, ov, offsets=o)
    yield "match_mask_batch", lambda o: a.match_mask_batch(t, ov, offsets=o)

handles = []
for mk, ov in ((ar.MatchKind.Standard, False), (ar.MatchKind.Standard, True), (ar.MatchKind.LeftmostLongest, False)):
    handles.append((ar.AhoCorasick(spats, matchkind=mk), "*", ov, True))
    handles.append((ar.BytesAhoCorasick([p.encode() for p in spats], matchkind=mk), b"*", ov, False))
handles.append((ar.AhoCorasick(spats, ascii_case_insensitive=True), "*", False, True))
handles.append((ar.BytesAhoCorasick([p.encode() for p in spats], ascii_case_insensitive=True), 42, False, False))
rows_b = text.splitlines(keepends=True)
assert [text[want[i]:want[i + 1]] for i in range(len(want) - 1)] == rows_b
for a, star, ov, is_str in handles:
    seen = 0
    for name, call in calls(a, star, ov):
        mine, ref = snap(call(ro.offsets)), snap(call(d_want))
        same(mine, ref)
        seen += int(mine[0] == "fr" and 0 < mine[2] < 301) + int(mine[0] == "pc" and len(mine[3]) > 0)
    assert seen >= 2, "the text does not exercise the methods"
    # filter_batch: also what the list of lines gives, and the kept rows are lines again
    fr = a.filter_batch(t, ov, offsets=ro.offsets)
    fl = a.filter_batch([r.decode() for r in rows_b] if is_str else rows_b, ov)
    assert fr.tolist() == fl.tolist() and np.array_equal(host(fr.rows), np.from_dlpack(fl.rows))
    assert np.array_equal(host(fr.offsets), np.from_dlpack(fl.offsets)) and np.array_equal(host(fr.data), np.from_dlpack(fl.data))
    kept = bytes(host(fr.data))
    assert kept.splitlines(keepends=True) == [rows_b[i] for i in host(fr.rows)]
    assert np.array_equal(host(ar.split_rows(torch.from_dlpack(fr.data)).offsets), host(fr.offsets))  # a newline-delimited file again
# a pattern that ends with the newline matches at the end of its row, one that spans two rows never does
b = ar.BytesAhoCorasick([b"x\n", b"\nthe"])
pc = b.count_by_pattern_sparse_batch(t, offsets=ro.offsets)
assert set(host(pc.pattern).tolist()) <= {0} and int(host(pc.count).sum()) == text.count(b"x\n")
# the host forms plug in the same way
hb = ar.BytesAhoCorasick([p.encode() for p in spats])
same(snap(hb.filter_batch(data, offsets=ar.split_rows(data).offsets)), snap(hb.filter_batch(rows_b)))

# lifetime: the tensor keeps the offsets alive after the RowOffsets object and its input are gone
t2 = t.clone()
ro2 = ar.split_rows(t2)
x = torch.from_dlpack(ro2.offsets)
unused = ro2.offsets.__dlpack__()
del ro2, unused, t2
gc.collect()
for k in range(6):  # (other results come and go where the words would be if they had been given back)
    keep = ar.split_rows(torch.full((len(text),), 10, dtype=torch.uint8, device="cuda:0"))
    del keep
gc.collect()
torch.cuda.synchronize()
assert np.array_equal(x.cpu().numpy(), want)
del x
gc.collect()

# four threads, each splits and filters its own tensor
errors = []
def run(i):
    try:
        mine = data[i * 37:].copy()
        tt = torch.from_numpy(mine.copy()).to("cuda:0")
        w = definition(mine, 10)
        ref = snap(hb.filter_batch(tt, offsets=torch.from_numpy(w).to("cuda:0")))
        for k in range(3):
            r = ar.split_rows(tt)
            assert np.array_equal(host(r.offsets), w), (i, k)
            same(snap(hb.filter_batch(tt, offsets=r.offsets)), ref)
    except BaseException as e:
        errors.append((i, repr(e)))
threads = [threading.Thread(target=run, args=(i,)) for i in range(4)]
for th in threads:
    th.start()
for th in threads:
    th.join()
assert not errors, errors
assert torch.equal(t.cpu(), torch.from_numpy(data))
print("OK")
"""


def test_tensors_in_and_offsets_into_the_batch_methods():
    """split_rows on tensors in HBM; torch.from_dlpack of the offsets on the tensor's device; offsets=ro.offsets into the six
    tensor-taking methods of both classes (Standard, overlapping, LeftmostLongest, case-insensitive) against the uploaded numpy
    offsets and, for filter_batch, against the list of lines; lifetime; threads.  In a process of its own: torch has to be the
    first to load the HIP runtime."""
    pytest.importorskip("torch")
    p = subprocess.run([sys.executable, "-c", _TENSOR_SCRIPT, ROOT, os.path.join(ROOT, "tests")], capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
