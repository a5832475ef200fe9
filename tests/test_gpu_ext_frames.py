"""The frame of the extension's entry points (csrc/pymodule.cpp) at the smallest shapes -- three byte patterns on the 8 bytes
b"xabcbabc", two str patterns on the 5 characters "aébab", batches of two rows: every kind of haystack a method takes gives the
same value and says where it lies; the type and the literal text of every refusal the methods share, on every method that takes
the argument, with a valid call straight behind each refusal; and which of two bad arguments a call names.  Every refusal is an
argument check on the host in front of any launch.  The expected values are a few literals worked out from the patterns by hand;
the searches at their seams are the other test_gpu_*.py's.  In a process of its own, once for the module: torch has to be the
first to load the HIP runtime."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_SCRIPT = r"""
import json
import sys
import traceback
import torch  # first: one process holds ONE HIP runtime, and torch must be the one to load it
sys.path[:0] = [sys.argv[1]]
import numpy as np
import ahocorasick_rs as ar

HAY = b"xabcbabc"
BP = [b"ab", b"bc", b"b"]
SP = ["ab", "é"]
KINDS = (ar.MatchKind.Standard, ar.MatchKind.LeftmostLongest)
B = [ar.BytesAhoCorasick(BP, matchkind=k) for k in KINDS]  # built once
S = [ar.AhoCorasick(SP, matchkind=k) for k in KINDS]
M = [(0, 1, 3), (2, 4, 5), (0, 5, 7)]  # both match kinds: "ab" begins first wherever "b" or "bc" could
M_OV = [(0, 1, 3), (2, 2, 3), (1, 2, 4), (2, 4, 5), (0, 5, 7), (2, 6, 7), (1, 6, 8)]  # Standard, overlapping: every occurrence
REP = [b"1", b"22", b""]


def value(r):
    return r.tolist() if hasattr(r, "tolist") else r


def words(col):
    return np.from_dlpack(col).tolist()


def haystacks(data=HAY):
    a = np.frombuffer(data, dtype=np.uint8).copy()
    return {"bytes": data, "bytearray": bytearray(data), "memoryview": memoryview(data), "numpy": a,
            "torch host": torch.from_numpy(a.copy()), "cuda:0": torch.from_numpy(a.copy()).to("cuda:0")}


# ---------------------------------------------------------------------------
# haystack kinds
# ---------------------------------------------------------------------------
def haystack_kinds():
    single = {  # method: (the arguments behind the haystack, the keywords, the value -- through tolist() where there is one)
        "find_matches_as_indexes": ((), {}, M),
        "replace_all": ((REP,), {}, b"x1c1c"),
        "is_match": ((), {}, True),
        "find_first": ((), {}, (0, 1, 3)),
        "count_matches": ((), {}, 3),
        "count_by_pattern": ((), {}, [2, 0, 1]),
        "find_matches_as_columns": ((), {}, M),
        "cover_spans": ((), {}, [(1, 3), (4, 7)]),
        "find_matches_as_snippets": ((), {"context": 1}, [b"xabc", b"cba", b"babc"]),
    }
    overlapping = {  # the Standard object alone
        "find_matches_as_indexes": ((True,), {}, M_OV),
        "count_matches": ((True,), {}, 7),
        "count_by_pattern": ((True,), {}, [2, 2, 3]),
        "find_matches_as_columns": ((True,), {}, M_OV),
        "cover_spans": ((True,), {"gap": 0}, [(1, 8)]),
        "find_matches_as_snippets": ((True,), {}, [b"ab", b"b", b"bc", b"b", b"ab", b"b", b"bc"]),
    }
    for b, table in ((B[0], single), (B[1], single), (B[0], overlapping)):
        for name, (args, kw, want) in table.items():
            for kind, h in haystacks().items():
                r = getattr(b, name)(h, *args, **kw)
                assert value(r) == want, (name, kind, value(r))
                if hasattr(r, "tolist"):
                    assert r.device == (0 if kind == "cuda:0" else None), (name, kind, r.device)
    assert value(B[0].cover_spans(HAY, gap=1)) == [(1, 7)]
    for kind, h in haystacks(b"ab\ncd\nef").items():
        r = ar.split_rows(h)
        assert r.tolist() == [0, 3, 6, 8] and r.device == (0 if kind == "cuda:0" else None), (kind, r.tolist(), r.device)
    # the str class: code-point offsets in the columns, the spans and find_first; byte offsets in the snippets
    for s in S:
        for hay, m, spans, snips, offs, lead in (
                ("abxab", [(0, 0, 2), (0, 3, 5)], [(0, 2), (3, 5)], ["abxa", "bxab"], [0, 4, 8], [0, 2]),
                ("aébab", [(1, 1, 2), (0, 3, 5)], [(1, 2), (3, 5)], ["aéba", "bab"], [0, 5, 8], [1, 1])):
            assert s.find_matches_as_indexes(hay) == m and s.find_first(hay) == m[0], hay
            assert s.find_matches_as_strings(hay) == [SP[p] for p, _, _ in m], hay
            c = s.find_matches_as_columns(hay)
            assert c.tolist() == m and c.device is None and words(c.start) == [x[1] for x in m], hay
            assert s.cover_spans(hay).tolist() == spans and s.cover_spans(hay).device is None, hay
            sn = s.find_matches_as_snippets(hay, context=2)
            assert sn.tolist() == snips and words(sn.offsets) == offs and words(sn.lead) == lead, (hay, sn.tolist())
            assert words(sn.pattern) == [x[0] for x in m] and sn.device is None and sn.nbytes == offs[-1], hay
            assert s.find_matches_as_snippets(hay).tolist() == s.find_matches_as_strings(hay), hay
            assert s.is_match(hay) is True and s.count_matches(hay) == 2 and s.count_by_pattern(hay) == [[x[0] for x in m].count(p) for p in (0, 1)], hay
        assert s.replace_all("aébab", ["1", "22"]) == "a22b1"


# ---------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------
# method: the keywords it takes -- o: overlapping, b: a batch, r: offsets / row_length (ONE tensor of rows), g: gap, c: context,
# m: min_matches, s: min_score, f: fill, w: weights, p: replace_with, t: a single haystack that may be a __dlpack__ tensor
# (the bytes class)
METHODS = {
    "find_matches_as_indexes": "ot", "find_matches_as_strings": "o", "find_matches_as_indexes_batch": "ob",
    "replace_all": "pt", "replace_all_batch": "pb",
    "is_match": "t", "find_first": "t", "count_matches": "ot", "count_by_pattern": "ot",
    "is_match_batch": "b", "find_first_batch": "b", "count_matches_batch": "ob", "count_by_pattern_batch": "ob",
    "find_matches_as_columns": "ot", "find_matches_as_columns_batch": "ob",
    "count_by_pattern_sparse_batch": "obr", "filter_batch": "obrm", "score_batch": "wobr", "filter_by_score_batch": "wobrs",
    "mask_all": "fo", "match_mask": "o", "mask_all_batch": "fobr", "match_mask_batch": "obr",
    "cover_spans": "otg", "cover_spans_batch": "obrg", "find_matches_as_snippets": "otc", "find_matches_as_snippets_batch": "obrc",
}
NAMED = ("replace_all_batch", "is_match_batch", "find_first_batch", "count_matches_batch", "count_by_pattern_batch")
BOOL_TEXT = "argument 'overlapping': 'int' object cannot be converted to 'PyBool'"
NOT_BYTES = "a bytes-like object is required, not '%s'"
NOT_STR = "argument 'haystack': '%s' object cannot be converted to 'PyString'"
ONE_DIM = "Only one-dimensional sequences are supported"
NOT_U8 = "buffer contents are not compatible with u8"
NOT_CONTIGUOUS = "Must be a contiguous sequence of bytes"
ROW_LENGTH = "row_length must be positive and divide the tensor's length"
ONE_OF = "a tensor of haystacks needs exactly one of offsets and row_length"
NO_CUTS = "offsets / row_length cut ONE __dlpack__ tensor into rows: a sequence of haystacks takes neither"


def refuses(exc, text, f, *args, **kw):
    try:
        f(*args, **kw)
    except Exception as e:
        assert type(e) is exc and str(e) == text, (f.__name__, args, kw, repr(e), "wanted", exc.__name__, text)
    else:
        raise AssertionError(("not refused", f.__name__, args, kw))


class Frame:
    # one automaton object: its methods with valid arguments, and what they return for them
    def __init__(self, o):
        self.o = o
        self.utf8 = isinstance(o, ar.AhoCorasick)
        self.methods = {n: k for n, k in METHODS.items() if hasattr(o, n)}
        self.hay = "aébab" if self.utf8 else HAY
        self.hays = ["aébab", "abxab"] if self.utf8 else [b"xabc", b"babc"]
        self.bad = b"ab" if self.utf8 else "ab"  # the other class's haystack
        self.bad_text = NOT_STR % "bytes" if self.utf8 else NOT_BYTES % "str"
        self.lead = {"w": [3, -1] if self.utf8 else [3, -1, 2], "f": "*" if self.utf8 else 42, "p": ["1", "22"] if self.utf8 else REP}
        self.good = {n: value(self.call(n)) for n in self.methods}

    def args(self, name, hay=None):
        keys = self.methods[name]
        return [self.hays if "b" in keys else self.hay] if hay is None else [hay], [self.lead[k] for k in "wfp" if k in keys]

    def call(self, name, hay=None, **kw):
        h, lead = self.args(name, hay)
        return getattr(self.o, name)(*h, *lead, **kw)

    def refuses(self, exc, text, name, hay=None, lead=None, **kw):
        # the refusal, then the valid call: it gives what it gave before
        h, good_lead = self.args(name, hay)
        refuses(exc, text, getattr(self.o, name), *h, *(good_lead if lead is None else lead), **kw)
        assert value(self.call(name)) == self.good[name], (name, "the valid call behind the refusal")

    def bad_haystack_text(self, name):
        if self.utf8 and "b" in self.methods[name] and name not in NAMED:
            return "'bytes' object cannot be converted to 'PyString'"
        return self.bad_text


def tensors():
    # (what, tensor, the refusal) on the host and on the device
    for where in ("cpu", "cuda:0"):
        t = torch.arange(16, dtype=torch.uint8).to(where)
        yield "2-D " + where, t[:8].reshape(2, 4), TypeError, ONE_DIM
        yield "int32 " + where, torch.zeros(8, dtype=torch.int32).to(where), BufferError, NOT_U8
        yield "strided " + where, t[::2], TypeError, NOT_CONTIGUOUS


def refusals():
    rows = np.frombuffer(HAY, dtype=np.uint8).copy()
    for o in B + S:
        f = Frame(o)
        for name, keys in f.methods.items():
            batch = "b" in keys
            bad = [f.bad] * 2 if batch else f.bad
            f.refuses(TypeError, f.bad_haystack_text(name), name, bad)  # a str for the bytes class, bytes for the str class
            if "o" in keys:
                f.refuses(TypeError, BOOL_TEXT, name, overlapping=1)
            for key, word in (("g", "gap"), ("c", "context")):
                if key in keys:
                    for v, exc, text in ((True, TypeError, "argument '%s': 'bool' object cannot be converted to 'PyInt'" % word),
                                         (-1, ValueError, "%s must be in range(2**63)" % word),
                                         (2 ** 63, ValueError, "%s must be in range(2**63)" % word),
                                         (1.0, TypeError, "argument '%s': 'float' object cannot be converted to 'PyInt'" % word)):
                        f.refuses(exc, text, name, **{word: v})
                    assert value(f.call(name, **{word: 2 ** 63 - 1})) is not None
            if "m" in keys:
                f.refuses(ValueError, "min_matches must be at least 1", name, min_matches=0)
                f.refuses(TypeError, "argument 'min_matches': 'bool' object cannot be converted to 'PyInt'", name, min_matches=True)
            if "s" in keys:
                f.refuses(ValueError, "min_score must fit an int64", name, min_score=2 ** 63)
                assert value(f.call(name, min_score=-2 ** 63)) is not None
            if "f" in keys and f.utf8:
                f.refuses(ValueError, "fill must be one ASCII character", name, lead=["é"])
                f.refuses(ValueError, "fill must be one ASCII character", name, lead=["ab"])
                f.refuses(TypeError, "argument 'fill': 'int' object cannot be converted to 'PyString'", name, lead=[256])
            elif "f" in keys:
                f.refuses(ValueError, "fill must be in range(256)", name, lead=[256])
                f.refuses(ValueError, "fill must be in range(256)", name, lead=[-1])
                f.refuses(ValueError, "fill must be in range(256)", name, lead=[2 ** 64])
                f.refuses(ValueError, "fill must be one byte", name, lead=[b"ab"])
                f.refuses(TypeError, "argument 'fill': an int in range(256) or a one-byte buffer is needed, not 'bool'", name, lead=[True])
            if "r" in keys:
                for where in ("cpu", "cuda:0"):
                    t = torch.from_numpy(rows.copy()).to(where)
                    cuts = torch.tensor([0, 4, 8], dtype=torch.int64).to(where)
                    by_length = value(f.call(name, t, row_length=4))
                    assert value(f.call(name, t, offsets=cuts)) == by_length, (name, where)
                    if not f.utf8:
                        assert by_length == f.good[name], (name, where)
                    f.refuses(TypeError, "argument 'row_length': 'bool' object cannot be converted to 'PyInt'", name, t, row_length=True)
                    f.refuses(ValueError, ROW_LENGTH, name, t, row_length=0)
                    f.refuses(ValueError, ROW_LENGTH, name, t, row_length=-4)
                    f.refuses(ValueError, ROW_LENGTH, name, t, row_length=3)
                    f.refuses(TypeError, ONE_OF, name, t)
                    f.refuses(TypeError, ONE_OF, name, t, offsets=cuts, row_length=4)
                    f.refuses(TypeError, NO_CUTS, name, offsets=cuts)
                    f.refuses(TypeError, NO_CUTS, name, row_length=4)
                for what, t, exc, text in tensors():
                    f.refuses(exc, text, name, t, row_length=4)
            if "t" in keys and not f.utf8:
                for what, t, exc, text in tensors():
                    f.refuses(exc, text, name, t)
            if not batch and not f.utf8:  # the same three through the buffer protocol
                a = np.arange(16, dtype=np.uint8)
                f.refuses(TypeError, ONE_DIM, name, a[:8].reshape(2, 4))
                f.refuses(BufferError, NOT_U8, name, np.zeros(8, dtype=np.int32))
                f.refuses(TypeError, NOT_CONTIGUOUS, name, a[::2])
            if not batch and ("t" not in keys or f.utf8):  # no tensor here: mask_all and match_mask, and the str class
                for where in ("cpu", "cuda:0"):
                    t = torch.from_numpy(rows.copy()).to(where)
                    f.refuses(TypeError, NOT_STR % "Tensor" if f.utf8 else NOT_BYTES % "Tensor", name, t)
    for what, t, exc, text in tensors():
        refuses(exc, text, ar.split_rows, t)
        assert ar.split_rows(b"ab\ncd\nef").tolist() == [0, 3, 6, 8]
    refuses(TypeError, NOT_BYTES % "str", ar.split_rows, "ab\n")
    refuses(ValueError, "delimiter must be in range(256)", ar.split_rows, b"ab\n", 256)


# ---------------------------------------------------------------------------
# the order of refusals
# ---------------------------------------------------------------------------
def order_of_refusals():
    for o in B + S:
        f = Frame(o)
        for name, keys in f.methods.items():
            bad = [f.bad] * 2 if "b" in keys else f.bad
            if "o" in keys:  # overlapping in front of the haystack
                f.refuses(TypeError, BOOL_TEXT, name, bad, overlapping=1)
            for key, word in (("g", "gap"), ("c", "context")):  # ... and so are gap and context; overlapping in front of them
                if key in keys:
                    f.refuses(ValueError, "%s must be in range(2**63)" % word, name, bad, **{word: -1})
                    f.refuses(TypeError, BOOL_TEXT, name, overlapping=1, **{word: -1})
            if "m" in keys:
                f.refuses(ValueError, "min_matches must be at least 1", name, bad, min_matches=0)
            if "s" in keys:
                f.refuses(ValueError, "min_score must fit an int64", name, bad, min_score=2 ** 63)
            if "f" in keys:
                f.refuses(ValueError, "fill must be one ASCII character" if f.utf8 else "fill must be one byte", name, bad,
                          lead=["ab" if f.utf8 else b"ab"])
            if "r" in keys:  # the tensor in front of how it is cut
                f.refuses(BufferError, NOT_U8, name, torch.zeros(8, dtype=torch.int32), row_length=0)
                f.refuses(TypeError, ONE_OF, name, torch.zeros(8, dtype=torch.int32))
            if "p" in keys:  # the haystack in front of replace_with
                item = "argument 'replace_with': 'int' object cannot be converted to 'PyString'" if f.utf8 else NOT_BYTES % "int"
                f.refuses(TypeError, f.bad_haystack_text(name), name, bad, lead=[[1]])
                f.refuses(TypeError, item, name, lead=[[1]])
                if not f.utf8 and "t" in keys:
                    for what, t, exc, text in tensors():
                        f.refuses(exc, text, name, t, lead=[[1]])
                    f.refuses(TypeError, item, name, torch.zeros(8, dtype=torch.uint8).to("cuda:0"), lead=[[1]])


report = {}
for section in (haystack_kinds, refusals, order_of_refusals):
    try:
        section()
        report[section.__name__] = None
    except Exception:
        report[section.__name__] = traceback.format_exc()
print("REPORT " + json.dumps(report))
"""


@pytest.fixture(scope="module")
def report():
    pytest.importorskip("torch")
    p = subprocess.run([sys.executable, "-c", _SCRIPT, ROOT], capture_output=True, text=True, timeout=300)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("REPORT ")]
    assert p.returncode == 0 and lines, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    return json.loads(lines[-1][len("REPORT "):])


def test_haystack_kinds(report):
    """bytes, bytearray, memoryview, a numpy array, a host tensor and a tensor in HBM give one value and say where it lies, on
    every single-haystack method of BytesAhoCorasick and on split_rows; AhoCorasick's code-point and byte offsets"""
    assert report["haystack_kinds"] is None, report["haystack_kinds"]


def test_refusals(report):
    """the type and text of every argument refusal on every method that takes the argument, a valid call behind each"""
    assert report["refusals"] is None, report["refusals"]


def test_order_of_refusals(report):
    """a call with two bad arguments names the one that is checked first"""
    assert report["order_of_refusals"] is None, report["order_of_refusals"]
