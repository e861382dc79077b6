"""The drop-in boundary without a flush (`-m gpu`): qdetector_cccf_execute per sample on a ring of page-locked buffers, its windows
cut on the GPU (no host history), and flexframesync_execute with streaming delivery (fxrx_sync_set_streaming), fed the way
the reference's lib/frame_detector_cc_impl.cc:76-82 and lib/flex_rx_impl.cc:212-215 feed them."""
import ctypes as C
import time
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

THR = 0.45


def _detector_feed(fx, x, block, fail_at=None, cap=4096):
    """the reference's per-sample loop (csrc/blocks/dropin_feed.cpp: dropin_feed_detector) -> [(tau, gamma, dphi, phi, window)], stats"""
    F = fx._ffi.feed_lib()
    est = np.zeros((cap, 4), np.float32); wins = np.zeros((cap, 512), np.complex64)
    st = fx._ffi.DropinDetStats()
    x = np.ascontiguousarray(x, np.complex64)
    assert F.dropin_feed_detector(x.ctypes.data, len(x), block, (1 << 64) - 1 if fail_at is None else fail_at, C.c_float(THR),
                                  est.ctypes.data, wins.ctypes.data, cap, C.byref(st)) == 0
    assert st.detections <= cap
    return [(tuple(est[i]), wins[i]) for i in range(st.detections)], st


@pytest.fixture(scope="module")
def det_stream(fx):
    return np.ascontiguousarray(fx.synth_stream(150_000, stream_id=511, payload_len=60)[0])


@pytest.fixture(scope="module")
def batched(fx, det_stream):
    ctx = fx.RxContext(1, mode=fx.MODE_DETECTOR, threshold=THR, want_framesyms=True)
    got = ctx.process([det_stream])
    ctx.close()
    return got


def _win(x, s):
    w = np.zeros(512, np.complex64)
    lo = max(s, 0)
    w[lo - s:] = x[lo:s + 512]
    return w


def test_qdetector_per_sample_equals_the_batched_detector(fx, det_stream, batched):
    """block length 8192: windows straddle the ring's buffers; nothing is kept on the host to cut them from"""
    got, st = _detector_feed(fx, det_stream, 8192)
    assert st.errors == 0 and len(batched) >= 20
    assert len(got) == len(batched)
    for (e, w), b in zip(got, batched):
        assert e == (np.float32(b["tau"]), np.float32(b["gamma"]), np.float32(b["dphi"]), np.float32(b["phi"]))
        assert np.array_equal(w, _win(det_stream, b["start"]))
    assert any(b["start"] // 8192 != (b["start"] + 511) // 8192 for b in batched)      # some window did straddle two buffers


def _locate(x, w, floor):
    """the position p at which w is the input as a detector that started (or restarted freshly reset) at sample `floor` saw it:
    w == x[p:p + 512] with everything below `floor` read as (0, 0), as the batched interface defines a window that begins below its
    stream's zero-floor (noise makes p unique); or None"""
    z = int(np.argmax(w != 0)) if w.any() else 512               # leading zeros: only a window that begins below the floor has any
    if z == 0:
        for p in np.flatnonzero(x[:len(x) - 511] == w[0]):
            if np.array_equal(x[p:p + 512], w):
                return int(p)
        return None
    p = floor - z
    return p if z < 512 and np.array_equal(w[z:], x[floor:p + 512]) else None


def test_qdetector_drops_a_failed_block_and_never_feeds_it_twice(fx, det_stream, batched):
    """An injected collect failure: with 8192-sample blocks and one block in flight, the collect that fails is that of the block
    [65536, 73728) (the one before it is collected at the latest 1024 samples after it filled).  That block is dropped, the detector
    restarts freshly reset at 73728.  The interface reports no positions (and the context's restart behind the gap anyway): a detection
    is located by its window, which must be the input at that position in the samples handed to the handle.  A preamble that lies
    across 73728 can still fire in the restarted detector, on the part behind the restart: its window begins below the restart, and
    there reads zeros (never the dropped samples), exactly as a window that begins below sample 0 does."""
    block, lo, hi = 8192, 65536, 73728
    x = det_stream
    got, st = _detector_feed(fx, x, block, fail_at=70_000)
    assert st.errors == 1
    true_pos = [b["start"] for b in batched]
    pos = []
    for e, w in got:
        p = _locate(x, w, hi)
        if p is None:
            p = _locate(x, w, 0)                                       # (the stream's very first detection may begin below sample 0)
        assert p is not None, "a returned window is not the input at any position"
        pos.append(p)
    assert all(a < b for a, b in zip(pos, pos[1:]))                # distinct, in order: nothing was fed twice
    # What the drop can touch is [lo - 512, hi + 512).  Below: a detection is reported by the block that holds the end of its window, so
    # one whose window reaches into the dropped block (start > lo - 512) goes with it.  Above: the restarted detector can fire on the
    # part of a preamble that lies across hi; such a window begins below hi and the detector moves on to its end, below hi + 512, and
    # searches from there as the uninterrupted one does -- a preamble that begins at or behind hi + 512 is seen whole and undisturbed.
    # Everywhere else every detection is a true one with the true estimates, and every true detection is there.
    z0, z1 = lo - 512, hi + 512
    assert all(hi - 512 < p for p in pos if z0 <= p < z1)          # nothing is reported from the dropped block; only across or behind hi
    assert [p for p in pos if not z0 <= p < z1] == [p for p in true_pos if not z0 <= p < z1]
    assert pos[-1] == true_pos[-1] and pos[0] == true_pos[0]       # detections before and behind the gap arrive
    inside = [p for p in true_pos if lo <= p and p + 512 <= hi]
    assert inside and not set(inside) & set(pos)                   # the dropped block's detections are gone
    est = {b["start"]: (np.float32(b["tau"]), np.float32(b["gamma"]), np.float32(b["dphi"]), np.float32(b["phi"])) for b in batched}
    for p, (e, w) in zip(pos, got):
        if not z0 <= p < z1:
            assert e == est[p]


def _sync_handle(fx, got):
    L = fx.lib()

    def cb(hd, hv, pl, n, pv, st, ud):
        syms = np.frombuffer(C.string_at(st.framesyms, 8 * st.num_framesyms), np.complex64) if st.num_framesyms else np.zeros(0, np.complex64)
        got.append((bytes(hd[:20]), hv, pv, C.string_at(pl, n) if n else b"", (st.evm, st.rssi, st.cfo, st.mod_scheme, st.mod_bps, st.check, st.fec0, st.fec1), syms.tobytes()))
        return 0
    cbf = fx._ffi.FRAMESYNC_CALLBACK(cb)
    q = L.flexframesync_create(cbf, None)
    assert q
    return q, cbf


def _feed_256(L, q, x):
    for i in range(0, len(x) - len(x) % 256, 256):
        blk = x[i:i + 256]
        L.flexframesync_execute(q, blk.ctypes.data, 256)


def test_streaming_delivers_every_frame_without_a_flush(fx):
    L = fx.lib()
    x, inj = fx.synth_stream(500_000, stream_id=512, payload_len=150)
    x = np.ascontiguousarray(x[:len(x) - len(x) % 256])
    zeros = np.zeros(256, np.complex64)
    # control: streaming off, default block length: nothing arrives before the flush
    ref = []
    q, keep = _sync_handle(fx, ref)
    _feed_256(L, q, x)
    assert ref == []
    L.fxrx_sync_flush(q)
    while L.fxrx_sync_pending(q):
        L.flexframesync_execute(q, None, 0)
    L.flexframesync_destroy(q)
    assert [r[3] for r in ref] == [pl for _, pl in inj] and all(r[1] and r[2] for r in ref)
    # streaming on: no flush anywhere
    got = []
    q, keep2 = _sync_handle(fx, got)
    L.fxrx_sync_set_streaming(q, 8192)
    _feed_256(L, q, x)
    extra, t0 = 0, time.monotonic()
    while len(got) < len(ref) and extra < 4_000_000 and time.monotonic() - t0 < 10.0:      # (a guard against hanging, not a latency claim)
        L.flexframesync_execute(q, zeros.ctypes.data, 256)
        extra += 256
    assert L.fxrx_sync_errors(q) == 0
    L.flexframesync_destroy(q)
    assert len(got) == len(ref) == len(inj)
    assert got == ref                                              # header, verdicts, payload, stats and symbols bit for bit, in order


def test_set_block_and_back_with_frames_pending(fx):
    L = fx.lib()
    x, inj = fx.synth_stream(300_000, stream_id=513, payload_len=150)
    x = np.ascontiguousarray(x[:len(x) - len(x) % 256])
    got = []
    q, keep = _sync_handle(fx, got)
    L.fxrx_sync_set_block(q, 1 << 16)
    third = (len(x) // 3) // 256 * 256
    _feed_256(L, q, x[:third])
    L.fxrx_sync_flush(q)
    assert L.fxrx_sync_pending(q) > 0
    L.fxrx_sync_set_block(q, 12_288)                               # with frames pending: they are kept, the stream continues
    assert L.fxrx_sync_pending(q) > 0
    _feed_256(L, q, x[third:2 * third])
    L.fxrx_sync_set_block(q, 1 << 16)                              # ... and back
    _feed_256(L, q, x[2 * third:])
    L.fxrx_sync_flush(q)
    while L.fxrx_sync_pending(q):
        L.flexframesync_execute(q, None, 0)
    assert L.fxrx_sync_errors(q) == 0
    L.flexframesync_destroy(q)
    assert [g[3] for g in got] == [pl for _, pl in inj] and all(g[1] and g[2] for g in got)


def test_qdetector_set_block_and_back_with_detections_pending(fx, det_stream):
    """the detector's block length changed with detections pending, per sample from here: 4096 -> 1024 at sample 20 000, back at 30 000"""
    L = fx.lib()
    x = np.ascontiguousarray(det_stream[:40_000])
    ctx = fx.RxContext(1, mode=fx.MODE_DETECTOR, threshold=THR, want_framesyms=True)
    want = ctx.process([x])
    ctx.close()
    ms = L.msequence_create(7, 0x0089, 1)
    pn = np.array([(1 if L.msequence_advance(ms) else -1) + 1j * (1 if L.msequence_advance(ms) else -1) for _ in range(64)]) * np.sqrt(0.5)
    L.msequence_destroy(ms)
    q = L.qdetector_cccf_create_linear(pn.astype(np.complex64).ctypes.data, 64, 7, 2, 7, C.c_float(0.3))
    assert q
    L.qdetector_cccf_set_threshold(q, THR)
    L.fxrx_qdet_set_block(q, 4096)
    got = []

    def call(re, im):
        p = L.qdetector_cccf_execute(q, fx._ffi.FxComplex(re, im))
        if p:
            e = tuple(np.float32(getattr(L, "qdetector_cccf_get_" + n)(q)) for n in ("tau", "gamma", "dphi", "phi"))
            got.append((e, np.frombuffer(C.cast(p, C.POINTER(C.c_float * 1024)).contents, np.complex64).copy()))
    xs = x.view(np.float32).reshape(-1, 2).tolist()
    for i, (re, im) in enumerate(xs):
        if i == 20_000:
            # A detection leaves with the call after its block was collected, and a block is collected at most block / 8 + 1024
            # samples after it filled: the detections of the blocks up to 16 384 are gone by now, none would be pending.  The flush
            # (as in test_set_block_and_back_with_frames_pending) runs the 3616 samples queued, which hold two preambles, so that the
            # ring is changed with detections pending.  A ring changed with samples queued (and whatever is in flight then), left to
            # fxrx_qdet_set_block's own flush, is the change at 30 000 (784 samples queued, no flush from here).
            L.fxrx_qdet_flush(q)
            assert L.fxrx_qdet_pending(q) > 0
            L.fxrx_qdet_set_block(q, 1024)                         # with detections pending: they are kept, the stream continues
            assert L.fxrx_qdet_pending(q) > 0
        if i == 30_000:
            L.fxrx_qdet_set_block(q, 4096)                         # ... and back
        call(re, im)
    L.fxrx_qdet_flush(q)
    while L.fxrx_qdet_pending(q):
        call(0.0, 0.0)
    assert L.fxrx_qdet_errors(q) == 0
    L.qdetector_cccf_destroy(q)
    assert len(want) >= 15 and len(got) == len(want)
    for (e, w), b in zip(got, want):
        assert e == (np.float32(b["tau"]), np.float32(b["gamma"]), np.float32(b["dphi"]), np.float32(b["phi"]))
        assert np.array_equal(w, _win(x, b["start"]))


def test_sync_setters_refuse_without_their_prerequisites(fx):
    """no samples fed: a refusal returns -1 and makes no new context; with the prerequisites on, in order, each setter returns 0"""
    L = fx.lib()
    q, keep = _sync_handle(fx, [])
    ctx = L.fxrx_sync_context(q)
    assert ctx
    needy = [(L.fxrx_sync_set_soft_chain, 1), (L.fxrx_sync_set_soft_rs, 1), (L.fxrx_sync_set_soft_rs_fmax, 5), (L.fxrx_sync_set_soft_rs_chain, 1)]
    for f, v in needy:
        ctx = L.fxrx_sync_context(q)
        assert f(q, v) == -1 and L.fxrx_sync_context(q) == ctx
        assert f(q, 0) == 0                                        # turning an option off is always taken, whatever else is off
    ctx = L.fxrx_sync_context(q)
    L.fxrx_sync_set_soft(q, 1)
    assert L.fxrx_sync_context(q) != ctx
    ctx = L.fxrx_sync_context(q)
    assert L.fxrx_sync_set_soft_rs_fmax(q, 5) == -1 and L.fxrx_sync_set_soft_rs_chain(q, 1) == -1       # soft_rs is still off
    assert L.fxrx_sync_set_soft_chain(q, 1) == -1 and L.fxrx_sync_context(q) == ctx                     # soft_block is still off
    assert L.fxrx_sync_set_soft_rs(q, 1) == 0 and L.fxrx_sync_set_soft_rs_fmax(q, 5) == 0 and L.fxrx_sync_set_soft_rs_chain(q, 1) == 0
    assert L.fxrx_sync_set_soft_block(q, 1) == 0 and L.fxrx_sync_set_soft_chain(q, 1) == 0
    ctx = L.fxrx_sync_context(q)
    for v in (4, 35, -1):
        assert L.fxrx_sync_set_soft_rs_fmax(q, v) == -1 and L.fxrx_sync_context(q) == ctx
    for f, _ in reversed(needy):
        assert f(q, 0) == 0
    assert L.fxrx_sync_set_soft_block(q, 0) == 0
    assert L.fxrx_sync_errors(q) == 0
    L.flexframesync_destroy(q)
