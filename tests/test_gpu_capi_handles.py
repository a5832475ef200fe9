"""Every result class of the ctypes binding gives its handle back exactly once: free() and then the object going away,
and free() twice -- `_h` is None afterwards and no C call follows the first free.  What a recorder in the library's place
(test_capi_calls_cpu.py) cannot reach: the real handles of the host and the device routes."""
import gc

import numpy as np
import pytest

from ahocorasick_rs_amd import capi

pytestmark = pytest.mark.gpu

PATTERNS = [b"ab", b"bc"]
BATCH = [b"", b"abc", b"xbcab"]
LINES = b"abc\nxbcab\n"


class Spy:
    """the loaded library with every call's name written down"""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        fn = getattr(self.real, name)

        def call(*args):
            self.calls.append(name)
            return fn(*args)
        return call


@pytest.fixture
def spy(monkeypatch):
    s = Spy(capi.lib())
    monkeypatch.setattr(capi, "_lib", s)
    return s


@pytest.fixture(scope="module")
def staged():
    """the automaton, and the batch and the delimited text in HBM: (a, d_hay, nbytes, d_offsets, n_hay, d_lines)"""
    capi.set_device(0)
    a = capi.Automaton(PATTERNS)
    blob, off = capi.pack(BATCH)
    nbytes = int(off[-1])
    d_hay = capi.DeviceBuffer(64).upload(blob[:nbytes])
    d_off = capi.DeviceBuffer(64).upload(off)
    d_lines = capi.DeviceBuffer(64).upload(np.frombuffer(LINES, dtype=np.uint8))
    yield a, d_hay.ptr, nbytes, d_off.ptr, len(BATCH), d_lines.ptr
    for x in (d_hay, d_off, d_lines, a):
        x.free()


def dev(s):
    return (s[1], s[2]), dict(d_offsets=s[3], n_hay=s[4])


# class -> its free function and the routes that make one: host first (where there is one), then device
ROUTES = {
    capi.DeviceResult: ("acx_free_result", [lambda s: s[0].find_device(*dev(s)[0], **dev(s)[1])]),
    capi.DeviceReplaced: ("acx_free_replaced", [lambda s: s[0].replace_device(*dev(s)[0], [b"X", b"YZ"], **dev(s)[1])]),
    capi.DeviceSummary: ("acx_free_summary", [lambda s: s[0].summarize_batch(BATCH),
                                              lambda s: s[0].summarize_device(*dev(s)[0], **dev(s)[1])]),
    capi.DeviceColumns: ("acx_free_columns", [lambda s: s[0].find_columns_batch(BATCH),
                                              lambda s: s[0].find_columns_device(*dev(s)[0], **dev(s)[1])]),
    capi.DeviceTally: ("acx_free_tally", [lambda s: s[0].tally(BATCH), lambda s: s[0].tally_device(*dev(s)[0], **dev(s)[1])]),
    capi.DeviceFiltered: ("acx_free_filtered", [lambda s: s[0].filter(BATCH),
                                                lambda s: s[0].filter_device(*dev(s)[0], **dev(s)[1]),
                                                lambda s: s[0].filter_scored(BATCH, [1, 2]),
                                                lambda s: s[0].filter_scored_device(*dev(s)[0], [1, 2], **dev(s)[1])]),
    capi.DeviceScores: ("acx_free_scores", [lambda s: s[0].score(BATCH, [1, 2]),
                                            lambda s: s[0].score_device(*dev(s)[0], [1, 2], **dev(s)[1])]),
    capi.DeviceMasked: ("acx_free_masked", [lambda s: s[0].mask(BATCH, 0x2A),
                                            lambda s: s[0].mask_device(*dev(s)[0], 0x2A, **dev(s)[1])]),
    capi.DeviceRows: ("acx_free_rows", [lambda s: capi.split_rows(LINES), lambda s: capi.split_rows_device(s[5], len(LINES))]),
    capi.DeviceSpans: ("acx_free_spans", [lambda s: s[0].spans(BATCH), lambda s: s[0].spans_device(*dev(s)[0], **dev(s)[1])]),
    capi.DeviceSnippets: ("acx_free_snippets", [lambda s: s[0].snippets(BATCH),
                                                lambda s: s[0].snippets_device(*dev(s)[0], **dev(s)[1])]),
}


@pytest.mark.parametrize("cls", sorted(ROUTES, key=lambda c: c.__name__), ids=lambda c: c.__name__)
def test_a_result_is_freed_exactly_once(spy, staged, cls):
    free, routes = ROUTES[cls]
    for make in routes:
        for twice in (False, True):
            r = make(staged)
            assert type(r) is cls and r._h
            spy.calls.clear()
            r.free()
            assert r._h is None and spy.calls == [free]
            if twice:
                r.free()
            del r
            gc.collect()
            assert spy.calls == [free]
