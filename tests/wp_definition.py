"""The WordPiece definition of wp.hpp restated in plain Python -- the dictionary against the current position with startswith,
no trie -- and the generator of the seeded fuzz.  tests/test_wp_cpu.py and tests/test_gpu_wp.py take their expected values
from here, never from the library.

Inputs: patterns P_i (the vocabulary as a vocab.txt lists it), a continuation prefix C, the data cut into rows, a class per
byte VALUE (WORD, SPACE, ALONE), M = max_word_bytes, unk_id.  A folding handle compares pattern bytes folded (ASCII letters
only); the classes see the raw byte.
Words of a row [b, L): every ALONE byte is a word; every maximal run of WORD bytes inside the row is a word.
Pieces of a word [ws, we): longer than M -> ONE piece (unk_id, ws, we).  Else p = ws; at p == ws the candidates are all (i, e)
with h[p:e] == P_i, e <= we; at p > ws those with P_i = C + x, x not empty, h[p:e] == x, e <= we.  Standard picks the smallest
e then i, LeftmostFirst the smallest i, LeftmostLongest the largest e then the smallest i.  No candidate: the WHOLE word is ONE
piece (unk_id, ws, we).  Result: id, start, end (global), first (1 on a word's first piece), row_offsets (rows + 1)."""
import numpy as np

WORD, SPACE, ALONE = 0, 1, 2
STD, LF, LL = 0, 1, 2
KEY = {STD: lambda c: (c[1], c[0]), LF: lambda c: c[0], LL: lambda c: (-c[1], c[0])}
WHITESPACE = b" \t\n\r\x0b\x0c"
PUNCTUATION = bytes(list(range(33, 48)) + list(range(58, 65)) + list(range(91, 97)) + list(range(123, 127)))


def classes(separators=WHITESPACE, isolated=b""):
    cls = np.zeros(256, dtype=np.uint8)
    cls[list(bytes(separators))] = SPACE
    cls[list(bytes(isolated))] = ALONE
    return cls


def words_of(raw, cls, b, L):
    """the words [ws, we) of the row [b, L) (a long run of separators is skipped in one step: the next byte that is none)"""
    p = b
    while p < L:
        c = cls[raw[p]]
        if c == SPACE:
            p += 1
            if p + 64 < L and cls[raw[p]] == SPACE:
                rest = np.flatnonzero(cls[np.frombuffer(raw, dtype=np.uint8, count=min(L - p, 1 << 16), offset=p)] != SPACE)
                p = p + int(rest[0]) if len(rest) else min(L, p + (1 << 16))
            continue
        we = p + 1
        while c == WORD and we < L and cls[raw[we]] == WORD:
            we += 1
        yield p, we
        p = we


def definition(patterns, hay, kind, cls, *, prefix=b"##", M=100, unk=-1, offsets=None, fold=False):
    """(id, start, end, first, row_offsets) by the loop of the definition"""
    raw = bytes(hay)
    h = raw.lower() if fold else raw
    P = [bytes(x).lower() if fold else bytes(x) for x in patterns]
    C = bytes(prefix).lower() if fold else bytes(prefix)
    whole = list(enumerate(P))
    cont = [(i, x[len(C):]) for i, x in enumerate(P) if x.startswith(C) and len(x) > len(C)]
    off = [0, len(raw)] if offsets is None else [int(x) for x in offsets]
    out, ro = [], []
    for r in range(len(off) - 1):
        ro.append(len(out))
        for ws, we in words_of(raw, cls, off[r], off[r + 1]):
            pieces, p = [], ws
            while p < we and we - ws <= M:
                cand = [(i, p + len(x)) for i, x in (whole if p == ws else cont) if h.startswith(x, p, we)]
                if not cand:
                    break
                i, e = min(cand, key=KEY[kind])
                pieces.append((i, p, e, int(p == ws)))
                p = e
            out += pieces if p == we and we - ws <= M else [(unk, ws, we, 1)]
    ro.append(len(out))
    col = lambda k, t: np.asarray([x[k] for x in out], dtype=t).reshape(-1)
    return col(0, np.int64), col(1, np.int64), col(2, np.int64), col(3, np.uint8), np.asarray(ro, dtype=np.int64)


def fuzz_case(seed, size=400):
    """One seeded case: dict(patterns, hay, kind, cls, prefix, M, offsets, fold).  Every case holds the word "ef" (e and
    C + f are entries, and nothing else has an e or an f: two pieces under every kind), a word with a "d" (no entry has one:
    a failed step) and a run of more than M word bytes."""
    rng = np.random.default_rng(1000 + seed)
    prefix = (b"##", b"##", b"", b"@", b"##")[seed % 5]
    fold = seed % 4 == 1
    M = int(rng.integers(4, 13))
    word = lambda lo, hi: rng.choice(list(b"abc"), size=int(rng.integers(lo, hi))).astype(np.uint8).tobytes()
    patterns = [word(1, 4) for _ in range(int(rng.integers(2, 7)))] + [prefix + word(1, 3) for _ in range(int(rng.integers(2, 7)))]
    patterns += [b"e", prefix + b"f"]
    if seed % 3 == 0:
        patterns.append(prefix)  # an entry equal to C itself (an empty one cannot be compiled)
    patterns = [x for x in patterns if x]
    order = rng.permutation(len(patterns))
    patterns = [patterns[k] for k in order]
    text = []
    while sum(len(x) + 1 for x in text) < size:
        k = int(rng.integers(0, 10))
        text.append(b"," if k == 0 else b"" if k == 1 else word(1, 2 * M) if k == 2 else word(1, 6) + (b"#" if k == 3 else b""))
    text += [b"ef", b"ab" + b"d", b"a" * (M + 1 + int(rng.integers(0, 3)))]
    text = [text[k] for k in rng.permutation(len(text))]
    hay = b"".join(x + (b" ", b"\n", b"  ", b",")[int(rng.integers(0, 4))] for x in text)
    if fold:
        a = np.frombuffer(hay, dtype=np.uint8).copy()
        up = (rng.random(len(a)) < 0.3) & (a >= 97) & (a <= 122)
        a[up] -= 32
        hay = a.tobytes()
    offsets = None
    if seed % 3:
        cuts = sorted(int(x) for x in rng.integers(0, len(hay) + 1, size=int(rng.integers(1, 8))))
        low = hay.lower()
        kept = [(low.find(w), low.find(w) + len(w)) for w in (b"ef", b"abd", b"a" * (M + 1))]  # no row start inside these three
        cuts = [c for c in cuts if not any(s < c < e + 2 for s, e in kept)] or [0]
        offsets = [0] + cuts + ([cuts[-1]] * 2 if seed % 2 else []) + [len(hay)]
    return dict(patterns=patterns, hay=hay, kind=(STD, LF, LL)[seed % 3], cls=classes(b" \n", b","), prefix=prefix, M=M,
                offsets=offsets, fold=fold)


def fuzz_shows_all_three(case, want):
    """does the Python loop's result `want` hold a multi-piece word, a word unknown by a failed step and one unknown by length"""
    ids, start, end, first, ro = want
    multi = bool(np.any(first == 0))
    unk = ids == -1
    by_step = bool(np.any(unk & (end - start <= case["M"])))
    by_length = bool(np.any(unk & (end - start > case["M"])))
    return multi, by_step, by_length
