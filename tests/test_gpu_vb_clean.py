"""The batch Viterbi path's codeword check (fx_vbpre_kernel, gr-liquiddsp_amd/csrc/fx_vbclean.h): a rate-1/2 frame whose coded
bits are, as received, the encoding of a message with a zero tail is decoded by inverting the code, and its trellis is skipped.
The decisions must stay exactly the Viterbi decoder's: every case here is compared field for field with the same IQ decoded
with the check off (FXRX_VB_CLEAN=0) and against the CPU oracle; the vb_clean counter says how many frames took the short cut."""
import numpy as np
import pytest

from parity_util import oracle_frames, compare_frames

CONV_V27 = 11
PUNCTURED = (15, 16, 17, 18, 19, 20)
BATCH_FEC1 = (1, 4, 5, 6, 7, 8, 9, 10)          # outer codes that keep a frame on the batch Viterbi path (not convolutional, not RS)


def _same(a, b):
    assert len(a) == len(b), (len(a), len(b))
    for fa, fb in zip(a, b):
        assert fa.keys() == fb.keys()
        for k in fa:
            va, vb = fa[k], fb[k]
            if isinstance(va, np.ndarray) or isinstance(vb, np.ndarray):
                assert va is not None and vb is not None and np.array_equal(va, vb), k
            else:
                assert va == vb or (va != va and vb != vb), (k, va, vb)


def _run(fx, monkeypatch, xs, clean, **kw):
    monkeypatch.setenv("FXRX_VB_CLEAN", "1" if clean else "0")
    ctx = fx.RxContext(len(xs), want_framesyms=True, **kw)
    got = ctx.process(xs)
    tm = ctx.timing()
    ctx.close()
    return got, tm


def _n_r12(frames, max_len=None):
    return sum(1 for g in frames if g["header_valid"] and g["fec0"] == CONV_V27 and g["fec1"] in BATCH_FEC1
               and (max_len is None or len(g["payload"]) <= max_len))


@pytest.mark.gpu
def test_config2_stream_decodes_without_trellis(fx, oracle, monkeypatch):
    """bench.py's headline stream (PSK4 r1/2, 1024-B payloads, Es/N0 = 20 dB): every batch-path frame is a codeword as
    received; the frames are those of the check-off run and every payload is the injected one."""
    x, injected = fx.synth_stream(20_000_000, stream_id=0)
    on, tm_on = _run(fx, monkeypatch, [x], True)
    off, tm_off = _run(fx, monkeypatch, [x], False)
    _same(on, off)
    n = _n_r12(on)
    assert n == len(injected) and all(g["payload_valid"] and g["payload"] == pl for g, (_, pl) in zip(on, injected))
    assert tm_off["vb_clean"] == 0
    assert tm_on["vb_clean"] >= 0.99 * n, (tm_on["vb_clean"], n)
    assert tm_on["vb_fallbacks"] == 0
    # the oracle on a leading piece of the same stream
    xp = x[:3_000_000]
    gp, tp = _run(fx, monkeypatch, [xp], True)
    assert tp["vb_clean"] > 0
    compare_frames(oracle_frames(oracle, xp), gp)


@pytest.mark.gpu
def test_snr_sweep_mixes_clean_and_trellis_frames(fx, oracle, monkeypatch):
    """Rate-1/2 PSK4 streams at 5 ... 14 dB (raw bit error rates from ~1e-2 down to ~1e-7): some frames carry raw bit errors
    (trellis path), others none (short cut); both kinds in one block, identical to the check-off run and to the oracle."""
    snrs = [5.0, 7.0, 9.0, 10.0, 11.0, 12.0, 14.0]
    xs = [fx.synth_stream(300_000, stream_id=1200 + i, mod=2, fec0=CONV_V27, payload_len=[300, 64, 64, 100, 200, 500, 1024][i], snr_db=s)[0]
          for i, s in enumerate(snrs)]
    on, tm_on = _run(fx, monkeypatch, xs, True)
    off, tm_off = _run(fx, monkeypatch, xs, False)
    _same(on, off)
    n = _n_r12(on)
    print("r1/2 frames", n, "clean", tm_on["vb_clean"], "repairs", tm_on["vb_repairs"], "fallbacks", tm_on["vb_fallbacks"])
    assert tm_off["vb_clean"] == 0
    assert 0 < tm_on["vb_clean"] < n
    for s, x in enumerate(xs):
        compare_frames(oracle_frames(oracle, x), [g for g in on if g["stream"] == s])


@pytest.mark.gpu
def test_punctured_and_outer_codes(fx, oracle, monkeypatch):
    """Streams mixing rate 1/2 with the punctured codes (which keep the trellis) and with block codes as the outer code (fec1:
    the check runs on the inner code's bits after the outer decoder): punctured frames never count as clean, nor do packets
    too long for the front part's LDS buffer (they keep the trellis too)."""
    cases = [(2, CONV_V27, 1, 300), (2, CONV_V27, 1, 3000), (27, 15, 1, 200), (2, CONV_V27, 4, 120), (3, 17, 1, 90), (2, CONV_V27, 7, 64), (28, 20, 5, 150),
             (1, CONV_V27, 10, 33), (2, 19, 1, 400), (27, CONV_V27, 27, 100), (2, 16, 6, 50), (29, 18, 1, 250)]
    xs = [fx.synth_stream(150_000, stream_id=1300 + i, mod=m, fec0=f0, fec1=f1, payload_len=pl, snr_db=25.0)[0]
          for i, (m, f0, f1, pl) in enumerate(cases)]
    on, tm_on = _run(fx, monkeypatch, xs, True)
    off, _ = _run(fx, monkeypatch, xs, False)
    _same(on, off)
    n = _n_r12(on, max_len=2000)
    assert n > 0 and _n_r12(on) > n and sum(1 for g in on if g["header_valid"] and g["fec0"] in PUNCTURED) > 0
    assert 0.99 * n <= tm_on["vb_clean"] <= n, (tm_on["vb_clean"], n)
    for s, x in enumerate(xs):
        compare_frames(oracle_frames(oracle, x), [g for g in on if g["stream"] == s])
    # punctured codes alone: nothing is clean
    xp = [x for x, (m, f0, f1, pl) in zip(xs, cases) if f0 in PUNCTURED]
    gp, tp = _run(fx, monkeypatch, xp, True)
    assert len(gp) > 0 and tp["vb_clean"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("dbg", [0, 1, 2])
def test_blocks_in_flight_on_continuing_streams(fx, oracle, monkeypatch, dbg):
    """Continuing streams cut into blocks, three in flight, clean and trellis frames mixed (14 and 4 dB), with the test switches
    that force wrong traceback guesses (FXRX_VB_DEBUG 1) and unrepaired hand-overs (2): check on, check off and the oracle
    agree."""
    xa = fx.synth_stream(900_000, stream_id=1400, payload_len=500, snr_db=14.0)[0]
    xb = fx.synth_stream(900_000, stream_id=1401, payload_len=800, snr_db=4.0)[0]
    monkeypatch.setenv("FXRX_VB_DEBUG", str(dbg))
    res = {}
    for clean in (True, False):
        monkeypatch.setenv("FXRX_VB_CLEAN", "1" if clean else "0")
        ctx = fx.RxContext(2, want_framesyms=True)
        ctx.set_depth(3)
        got, inflight, n_clean = [], 0, 0
        for i in range(0, len(xa), 100_000):
            if inflight == 3:
                got += ctx.results(ctx.collect_raw()); inflight -= 1; n_clean += ctx.timing()["vb_clean"]
            ba, bb = xa[i:i + 100_000], xb[i:i + 100_000]
            ctx.submit_raw([ba.ctypes.data, bb.ctypes.data], [len(ba), len(bb)], False); inflight += 1
        while inflight:
            got += ctx.results(ctx.collect_raw()); inflight -= 1; n_clean += ctx.timing()["vb_clean"]
        ctx.close()
        res[clean] = (got, n_clean)
    _same(res[True][0], res[False][0])
    assert res[False][1] == 0 and 0 < res[True][1] < _n_r12(res[True][0])
    for s, x in enumerate((xa, xb)):
        compare_frames(oracle_frames(oracle, x), [g for g in res[True][0] if g["stream"] == s])
