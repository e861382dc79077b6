"""Aligned windows in detector mode (`-m gpu`): with want_framesyms every detection of the batched API carries the 512 samples
x[start, start + 512) of its stream, cut on the GPU by fx_detwin_kernel (csrc/fx_detwin.hip) -- what liquid's
qdetector_cccf_execute returns.  The checker is the input array itself: exact equality, zeros below the stream's zero-floor."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

THR = 0.45
EST = ("stream", "start", "cfo_bin", "rxy", "tau", "gamma", "dphi", "phi")


def _ref(x, s):
    """x[s, s + 512) with (0, 0) below index 0"""
    w = np.zeros(512, np.complex64)
    lo = max(s, 0)
    w[lo - s:] = x[lo:s + 512]
    return w


def _check(got, xs, base=0):
    """every result of `got` has the window of its stream's array (positions relative to `base`)"""
    for g in got:
        assert g["num_framesyms"] == 512 and g["framesyms"] is not None and g["framesyms"].dtype == np.complex64
        assert np.array_equal(g["framesyms"], _ref(xs[g["stream"]], g["start"] - base)), (g["stream"], g["start"])


def _key(g):
    return tuple(g[k] for k in EST)


@pytest.fixture(scope="module")
def stream(fx):
    # (the first frame begins 8 samples in front of the array: its aligned window starts below index 0)
    return np.ascontiguousarray(fx.synth_stream(150_008, stream_id=501, payload_len=40)[0][8:])


@pytest.fixture(scope="module")
def whole(fx, stream):
    """the one-block run: the reference of the tests below (never modified)"""
    ctx = fx.RxContext(1, mode=fx.MODE_DETECTOR, threshold=THR, want_framesyms=True)
    got = ctx.process([stream])
    ctx.close()
    return got


def test_one_block_windows_equal_the_input(fx, stream, whole):
    """fails without the feature: detector mode returned a NULL pointer and num_framesyms = 0"""
    assert 12 <= len(whole) <= 400
    _check(whole, [stream])
    assert min(g["start"] for g in whole) < 0                      # ... and the samples below index 0 are zeros (_ref)
    ctx = fx.RxContext(1, mode=fx.MODE_DETECTOR, threshold=THR)    # want_framesyms = 0: same detections, no windows
    plain = ctx.process([stream])
    ctx.close()
    assert [_key(g) for g in plain] == [_key(g) for g in whole]
    assert all(g["framesyms"] is None and g["num_framesyms"] == 0 for g in plain)


@pytest.mark.parametrize("delta", [1, 255, 256, 511, -1])
def test_window_across_a_block_cut(fx, stream, whole, delta):
    s = whole[len(whole) // 2]["start"]
    cut = s + delta
    ctx = fx.RxContext(1, mode=fx.MODE_DETECTOR, threshold=THR, want_framesyms=True)
    got = ctx.process([np.ascontiguousarray(stream[:cut])])
    _check(got, [stream])                                          # (while they are valid: before the next block)
    got2 = ctx.process([np.ascontiguousarray(stream[cut:])])
    _check(got2, [stream])
    ctx.close()
    got += got2
    assert [_key(g) for g in got] == [_key(g) for g in whole]
    assert all(np.array_equal(a["framesyms"], b["framesyms"]) for a, b in zip(got, whole))
    assert any(g["start"] == s for g in got2)                      # the detection was reported by the block behind the cut


def test_windows_after_a_reset_mid_stream(fx, stream, whole):
    a = whole[len(whole) // 3]["start"] + 8                        # the reset falls 8 samples into a frame's aligned window
    ctx = fx.RxContext(1, mode=fx.MODE_DETECTOR, threshold=THR, want_framesyms=True)
    _check(ctx.process([np.ascontiguousarray(stream[:a])]), [stream])
    ctx.reset()
    rest = np.ascontiguousarray(stream[a:])
    got = ctx.process([rest])
    ctx.close()
    assert len(got) >= 4 and min(g["start"] for g in got) < 0 <= max(g["start"] for g in got) < len(rest)   # positions restart at 0
    _check(got, [rest])                                            # zeros, not stream[a - 8:a], below the new index 0


def test_ragged_streams_with_blocks_in_flight(fx, stream):
    xs = [stream[:141_000], np.ascontiguousarray(fx.synth_stream(120_000, stream_id=502, payload_len=64)[0]),
          np.ascontiguousarray(fx.synth_stream(97_531, stream_id=503, payload_len=24)[0]), np.zeros(0, np.complex64)]
    nb = 5
    cuts = [[(len(x) * k) // nb + (37 * k * (i + 1)) % 301 if 0 < k < nb else (len(x) if k else 0) for k in range(nb + 1)] for i, x in enumerate(xs)]
    blocks = [[np.ascontiguousarray(x[c[k]:c[k + 1]]) for x, c in zip(xs, cuts)] for k in range(nb)]
    ctx = fx.RxContext(4, mode=fx.MODE_DETECTOR, threshold=THR, want_framesyms=True)
    ctx.set_depth(3)
    for k in range(3):
        ctx.submit(blocks[k])
    got = []
    for k in range(nb):
        n = ctx.collect_raw()
        if k + 3 < nb:
            ctx.submit(blocks[k + 3])                              # a submit in between does not touch the collected block's windows
        res = ctx.results(n)
        _check(res, xs)
        got += res
    ctx.close()
    for i, x in enumerate(xs[:3]):
        one = fx.RxContext(1, mode=fx.MODE_DETECTOR, threshold=THR)
        want = [g["start"] for g in one.process([x])]
        one.close()
        assert [g["start"] for g in got if g["stream"] == i] == want and len(want) >= 8
    assert not [g for g in got if g["stream"] == 3]


def test_dense_detections_beyond_the_reserved_slots(fx, monkeypatch):
    """more detections than window slots were reserved: the rest is cut when the block is collected, from the block's input; windows
    that start in the carried tail -- gone by then -- are cut with the chain (stream 1's first record lies beyond a reservation of 1)"""
    x = fx.synth_stream(60_000, stream_id=313177, mod=28, fec0=18, fec1=7, payload_len=7, gap=300, snr_db=30.0)[0]
    thr = 0.35
    ref = fx.RxContext(2, mode=fx.MODE_DETECTOR, threshold=thr)
    want = [_key(g) for g in ref.process([x, x])]
    ref.close()
    assert len(want) > 2 * (len(x) // 600)
    cut = want[len(want) // 4][1] + 100                            # a window of both streams reaches 100 samples into the tail
    late = {}
    for reserve in (1, 1_000_000):
        monkeypatch.setenv("FXRX_DETWIN_RESERVE", str(reserve))
        ctx = fx.RxContext(2, mode=fx.MODE_DETECTOR, threshold=thr, want_framesyms=True)
        got = []
        for lo, hi in ((0, cut), (cut, len(x))):
            blk = np.ascontiguousarray(x[lo:hi])
            res = ctx.process([blk, blk])
            _check(res, [x, x])
            got += res
        late[reserve] = ctx.timing()["late_windows"]
        ctx.close()
        assert sorted(_key(g) for g in got) == sorted(want)
        assert any(g["stream"] == 1 and g["start"] == cut - 100 for g in got)
    assert late[1] > 0 and late[1_000_000] == 0


def test_input_sources(fx, stream, whole):
    import torch
    x = stream[:100_001]
    n_want = len([g for g in whole if g["start"] + 512 <= len(x)])
    pinned = torch.from_numpy(x.copy()).pin_memory()
    for src in (torch.from_numpy(x.copy()).cuda(), pinned, x.copy()):
        ctx = fx.RxContext(1, mode=fx.MODE_DETECTOR, threshold=THR, want_framesyms=True)
        if isinstance(src, np.ndarray) or src.is_cuda:
            got = ctx.process([src])
        else:
            got = ctx.results(ctx.process_raw([src.data_ptr()], [src.numel()], False))
        ctx.close()
        _check(got, [x])
        assert [_key(g) for g in got[:n_want]] == [_key(g) for g in whole[:n_want]] and n_want >= 8
    q = np.clip(np.rint(x.view(np.float32).reshape(-1, 2) * 8192.0), -32768, 32767).astype(np.int16)
    xf = fx.rx.iq_convert(q)
    ctx = fx.RxContext(1, mode=fx.MODE_DETECTOR, threshold=THR, want_framesyms=True)
    got = ctx.process([q])
    ctx.close()
    assert len(got) >= 8
    _check(got, [xf])
