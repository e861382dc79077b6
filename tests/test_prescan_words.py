"""The walker's reading of a pre-lock scan table (fx_common.h: fx_prescan_valid_hops, fx_prescan_entry), through
fxrx_debug_prescan_words: first hitting chunk, packing, fall-back position, hops covered.  No GPU."""
import ctypes as C

import pytest

HOP, CHUNK, NONE = 256, 16, 0xFFFFFFFF


def _entry(fx, words, K, start, stop, n):
    a = (C.c_uint32 * max(1, len(words)))(*words)
    out = (C.c_int64 * 3)()
    r = fx.lib().fxrx_debug_prescan_words(a, len(words), K, start, stop, n, C.byref(out))
    assert r in (0, 1), r
    return r == 1, int(out[0]), int(out[1]), int(out[2])


def _valid(start, stop, n, K):
    """hops h < K with start + 256 h < stop and start + 256 h + 256 <= n, counted one by one"""
    k = 0
    while k < K and start + HOP * k < stop and start + HOP * k + HOP <= n:
        k += 1
    return k


@pytest.mark.parametrize("start,stop,n,K", [
    (4096, 8192, 100_000, 128),          # K longer than the segment: 16 hops
    (4096, 8192, 100_000, 4),            # K shorter
    (4096, 8193, 100_000, 128),          # one sample into a 17th hop
    (4096, 100_000, 4096 + 5 * HOP - 1, 64),     # the data ends one sample short of the fifth hop's new half
    (4096, 100_000, 4096 + 5 * HOP, 64),
    (4096, 100_000, 4096 + 255, 64),     # not one whole hop of data
    (4096, 100_000, 4000, 64),           # a segment that starts behind the data
    (20_000, 40_000, 1 << 40, 0),        # no hops asked for
    ((1 << 33) + 7, (1 << 33) + 7 + 70_000, 1 << 34, 80),    # beyond 32 bits
])
def test_hops_covered_and_fall_back(fx, start, stop, n, K):
    hops = _valid(start, stop, n, K)
    nw = (K + CHUNK - 1) // CHUNK
    took, p, scanned, got = _entry(fx, [NONE] * nw, K, start, stop, n)
    assert got == hops
    assert not took and p == start + HOP * hops and scanned == hops


def test_first_hitting_chunk_and_packing(fx):
    start, stop, n, K = 50_000, 90_000, 1_000_000, 80
    for words, hop, lag in (
        ([5 << 16 | 300, NONE, NONE, NONE, NONE], 5, 300),
        ([0 << 16 | 256, NONE, NONE, NONE, NONE], 0, 256),                    # hop 0: the candidate starts at `start`
        ([NONE, NONE, 47 << 16 | 0, 48 << 16 | 100, NONE], 47, 0),            # the lowest chunk with a hit wins, lag 0
        ([NONE, NONE, NONE, NONE, 79 << 16 | 355], 79, 355),                  # last hop, largest accepted lag
        ([NONE, 16 << 16 | 0xFFFE, NONE, NONE, NONE], 16, 0xFFFE),            # all 16 bits of the lag field
    ):
        took, p, scanned, hops = _entry(fx, words, K, start, stop, n)
        assert took and hops == 80
        assert p == start + HOP * hop - HOP + lag, (words, p)
        assert scanned == hop + 1
    took, p, scanned, hops = _entry(fx, [], 0, start, stop, n)
    assert not took and p == start and scanned == 0 and hops == 0
