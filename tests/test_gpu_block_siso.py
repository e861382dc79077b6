"""Soft values carried through fec1's block decoder into fec0's Viterbi decoder (fxrx_config.soft_chain) on the GPU (`-m gpu`).

The oracle has no such decoder; the checker is the numpy reference of tests/ref_block_siso.py.
  (1) fxrx_debug_block_siso -- the decode kernel's own soft-output block decoders on crafted packets -- against the reference, every
      value, >= 20 000 codewords per code, lengths 1, 2, 3, 7, 8, 9, 63 and those with 64, 65 (Hamming(7,4) / (8,4): 66) and 129
      codewords: the boundaries of the kernel's rounds of 64 lanes.
  (2) Whole frames at low SNR with want_framesyms: payload and payload_valid of every frame equal ref_block_siso.packet_decode_chain
      on the frame's own soft_bits; QAM16, all seven codes over V27 and over one punctured code each, payloads of 1 .. 300 bytes.  Floors
      per code: >= 20 frames differ from the soft_block-only run; SECDED codes: >= 5 frames hold a block without any Chase candidate
      (Golay cannot have one, tests/test_block_siso.py; the Hamming codes have no candidates).
  (3) At 20 dB, and for every pair the stage rule does not cover, every field of every frame equals the soft_block run.
  (4) Results do not depend on segmentation, depth or cuts of the stream.
  (5) The drop-in with fxrx_sync_set_soft_chain delivers the batched context's frames; the setter without soft_block returns -1.
  (6) Gain, Hamming codes: at the point the CPU model chose, soft_chain yields more valid payloads than soft_block alone on the same
      IQ, by at least half the model's difference.  The model has no synchroniser: all of its 200 frames reach the payload decoder.
      The receiver at these SNRs finds few frames and decodes few headers, and a frame without a header reaches the payload decoder
      in neither run; so the model's difference is taken as a share of the frames with a valid header.  The model's Es/N0 is per
      symbol; synth_stream's snr_db is per sample of a unit-power signal at 2 samples a symbol, 3 dB less.  Golay and SECDED:
      parity with the reference only; their counts are printed by (2).

The CPU model (siso_cases.model_counts: PSK4, fec0 = V27, 64-byte payloads, CRC-24, 200 frames a point, AWGN at Es/N0 through
ref_decode's soft demapper; valid payloads soft_block -> soft_chain):
    Es/N0     Hamming(7,4)   Hamming(12,8)   Golay(24,12)   SECDED(72,64)
    -1 dB       0 ->   0       0 ->   0        0 ->   0       0 ->   0
     0 dB       1 ->  32       0 ->   1        2 ->  42       0 ->   0
     1 dB      43 -> 165       1 ->  83      121 -> 194       0 ->   0
     2 dB     162 -> 200      80 -> 190      197 -> 200       0 ->   0
     3 dB     200 -> 200     186 -> 199      200 -> 200      13 ->  64
     4 dB     200 -> 200     200 -> 200      200 -> 200     106 -> 177
     5 dB     200 -> 200     200 -> 200      200 -> 200     186 -> 199
     6 dB     200 -> 200     200 -> 200      200 -> 200     200 -> 200
The points of (6) are those of the largest difference: Hamming(7,4) at 1 dB (122 of 200), Hamming(12,8) at 2 dB (110 of 200):
synth_stream's snr_db = -2 dB and -1 dB.

Measured on an MI355X, valid payloads soft_block -> soft_chain of the frames with a valid header: PSK4 Hamming(12,8) / V27 at
snr_db -1: 2 -> 20 of 29 (399 sent), at 0: 95 -> 111 of 119; QAM16 at 5 dB (100 000 samples): Hamming(7,4) 25 -> 39 of 54,
Hamming(12,8) 18 -> 39 of 59, Golay 39 -> 41 of 50; QAM16 at 7 dB: SECDED(72,64) 16 -> 39 of 67."""
import ctypes as C

import numpy as np
import pytest

import ref_decode as R
import ref_block_soft as B
import ref_block_siso as S
import siso_cases as K

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------- (1) the decoders themselves
@pytest.mark.parametrize("fs", B.SOFT_BLOCK)
def test_debug_block_siso_matches_the_reference(fx, fs):
    L = fx.lib()
    rng = np.random.RandomState(700 + fs)
    total = 0
    for n in K.lengths(fs):
        count = max(2 * K.KINDS, 2400 // K.ncw(fs, n))
        _, soft = K.crafted(rng, fs, n, count)
        soft = np.ascontiguousarray(soft)
        got = np.zeros((count, 8 * n), np.uint8)
        assert L.fxrx_debug_block_siso(fs, n, count, soft.ctypes.data, got.ctypes.data) == 0, L.fxrx_last_error()
        want = S.block_decode_siso(fs, soft, n)
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert len(bad) == 0, "n=%d: %d of %d packets differ, first #%d (kind %d): got %s want %s" % (
            n, len(bad), count, bad[0], bad[0] % K.KINDS, got[bad[0]][:24], want[bad[0]][:24])
        total += count * K.ncw(fs, n)
    assert total >= 20_000


# ---------------------------------------------------------------------------------------------------- traffic
def _key(f):
    return tuple((k, f[k].tobytes() if isinstance(f[k], np.ndarray) else f[k]) for k in sorted(f))


def _run(fx, xs, depth=1, cuts=1, **kw):
    ctx = fx.RxContext(len(xs), want_framesyms=True, soft_decision=True, soft_block=True, **kw)
    ctx.set_depth(depth)
    got, inflight, keep = [], 0, []
    bounds = [[len(x) * k // cuts for k in range(cuts + 1)] for x in xs]
    for k in range(cuts):
        parts = [np.ascontiguousarray(x[b[k]:b[k + 1]]) for x, b in zip(xs, bounds)]
        keep.append(parts)
        if inflight == depth:
            got += ctx.results(ctx.collect_raw()); inflight -= 1
        ctx.submit_raw([q.ctypes.data for q in parts], [len(q) for q in parts], False); inflight += 1
    while inflight:
        got += ctx.results(ctx.collect_raw()); inflight -= 1
    ctx.close()
    return sorted(got, key=lambda f: (f["stream"], f["start"]))


def _chain_batch(frames, n, check, fec0, fec1, info):
    """ref_block_siso.packet_decode_chain on many frames of one shape, the Viterbi stage batched"""
    k, l0, l1 = R.packet_dims(n, check, fec0, fec1)
    vals = []
    for f in frames:
        v = R.interleave_soft(np.asarray(f["soft_bits"], np.uint8)[:8 * l1], l1, decode=True)
        fi = {}
        vals.append(R.interleave_soft(S.block_decode_siso(fec1, v, l0, fi)[0], l0, decode=True))
        info.append(fi.get("no_candidate", 0))
    dec = R.viterbi(fec0, np.array(vals), k, 255)[0]
    return [R._finish(np.asarray(d, np.uint8), n, check) for d in dec]


# per code: (fec0, payload_len, snr_db) of its three streams: V27 at 64 bytes, V27 at a length with a tail, one punctured code
PUNCT = {R.FEC_H74: R.FEC_V27P23, R.FEC_H84: R.FEC_V27P78, R.FEC_H128: R.FEC_V27P23, R.FEC_GOLAY: R.FEC_V27P78, R.FEC_SD22: R.FEC_V27P23,
         R.FEC_SD39: R.FEC_V27P78, R.FEC_SD72: R.FEC_V27P23}
TAIL = {R.FEC_H74: 1, R.FEC_H84: 2, R.FEC_H128: 3, R.FEC_GOLAY: 300, R.FEC_SD22: 5, R.FEC_SD39: 131, R.FEC_SD72: 300}
# QAM16: its payload fails several dB above the SNR at which frames are still found and their (QPSK) headers decode, so that most frames
# reach the payload decoder and many of them sit at its limit.  (With PSK4 over V27 detection and header give out first.)
SNR_V27 = {R.FEC_H74: 5.0, R.FEC_H84: 4.0, R.FEC_H128: 5.0, R.FEC_GOLAY: 4.0, R.FEC_SD22: 5.0, R.FEC_SD39: 6.0, R.FEC_SD72: 6.5}
SNR_UP = {R.FEC_V27P23: 2.0, R.FEC_V27P78: 4.5}


def _low_streams(fx, fec1):
    spec = [(R.FEC_V27, 64, SNR_V27[fec1]), (R.FEC_V27, TAIL[fec1], SNR_V27[fec1]), (PUNCT[fec1], 37, SNR_V27[fec1] + SNR_UP[PUNCT[fec1]])]
    xs = [fx.synth_stream(100_000, stream_id=7100 + 10 * fec1 + i, mod=R.QAM16, fec0=f0, fec1=fec1, payload_len=n, snr_db=snr)[0]
          for i, (f0, n, snr) in enumerate(spec)]
    return spec, xs


@pytest.mark.parametrize("fec1", B.SOFT_BLOCK)
def test_low_snr_frames_follow_the_reference_chain(fx, fec1):
    spec, xs = _low_streams(fx, fec1)
    on = _run(fx, xs, soft_chain=True, soft_header=True)
    off = {(f["stream"], f["start"]): f for f in _run(fx, xs, soft_header=True)}
    groups = {}
    for f in on:
        if f["header_valid"]:
            groups.setdefault((f["stream"], len(f["payload"]), f["check"], f["fec0"], f["fec1"]), []).append(f)
    checked = differ = nocand = valid = 0
    for (stream, n, check, f0, f1), frames in groups.items():
        if (f0, f1, n) != (spec[stream][0], fec1, spec[stream][1]):          # a header that decoded to other properties: one by one
            want = [S.packet_decode_chain(f["soft_bits"], n, check, f0, f1) for f in frames]
            info = [0] * len(frames)
        else:
            info = []
            want = _chain_batch(frames, n, check, f0, f1, info)
        for f, w, nc in zip(frames, want, info):
            assert (f["payload"], f["payload_valid"]) == w, (stream, f["start"])
            o = off.get((f["stream"], f["start"]))
            differ += o is None or (o["payload"], o["payload_valid"]) != (f["payload"], f["payload_valid"])
            nocand += nc > 0
            valid += f["payload_valid"]
            checked += 1
    print("fec1 %d: %d frames checked, %d valid, %d differ from soft_block alone, %d with a block without candidates" % (fec1, checked, valid, differ, nocand))
    assert checked == sum(f["header_valid"] for f in on) and checked > 40 and 0 < valid < checked
    assert differ >= 20
    if fec1 in R.SECDED:
        assert nocand >= 5


INNER = (R.FEC_NONE, R.FEC_V27, R.FEC_V27P23, R.FEC_V27P34, R.FEC_V27P78)
OUTER = (R.FEC_NONE, R.FEC_GOLAY, R.FEC_RS, R.FEC_H74, R.FEC_H84, R.FEC_H128, R.FEC_SD22, R.FEC_SD39, R.FEC_SD72)


def test_soft_chain_at_20db_and_outside_the_rule_changes_nothing(fx):
    """20 dB: every inner x outer pair (covered ones included).  Low SNR: pairs the rule does not cover -- fec1 none, convolutional,
    Reed-Solomon, a block fec0 behind a block fec1"""
    cases = [(R.PSK4 if i % 2 else R.QAM16, f0, f1, 20.0) for i, (f0, f1) in enumerate((a, b) for a in INNER for b in OUTER)]
    cases += [(R.PSK4, R.FEC_V27, R.FEC_NONE, 1.0), (R.PSK4, R.FEC_H128, R.FEC_NONE, 4.0), (R.PSK4, R.FEC_NONE, R.FEC_V27, 1.0),
              (R.PSK4, R.FEC_V27, R.FEC_V27P23, 2.0), (R.PSK4, R.FEC_V27, R.FEC_RS, 2.0), (R.PSK4, R.FEC_RS, R.FEC_GOLAY, 3.0),
              (R.PSK4, R.FEC_H74, R.FEC_GOLAY, 3.0), (R.PSK4, R.FEC_SD72, R.FEC_H128, 4.0), (R.PSK4, R.FEC_NONE, R.FEC_SD39, 4.0)]
    xs = []
    for i, (m, f0, f1, snr) in enumerate(cases):
        xs.append(fx.synth_stream(50_000, stream_id=7500 + i, mod=m, fec0=f0, fec1=f1, payload_len=60 + i % 37, snr_db=snr)[0])
    off, on = _run(fx, xs, segment_len=16384), _run(fx, xs, segment_len=16384, soft_chain=True)
    assert [_key(f) for f in off] == [_key(f) for f in on]
    clean = [f for f in on if cases[f["stream"]][3] == 20.0]
    assert all(f["payload_valid"] for f in clean)
    assert {(f["fec0"], f["fec1"]) for f in clean} == {(f0, f1) for _, f0, f1, snr in cases if snr == 20.0}
    low = [f for f in on if cases[f["stream"]][3] < 20.0 and f["header_valid"]]
    assert len(low) > 50 and 0 < sum(f["payload_valid"] for f in low) < len(low)


def test_results_do_not_depend_on_how_the_input_is_fed(fx):
    xs = _low_streams(fx, R.FEC_H128)[1] + _low_streams(fx, R.FEC_SD72)[1][:1]
    ref = _run(fx, xs, soft_chain=True, soft_header=True)
    assert sum(f["header_valid"] for f in ref) > 60
    for seg, depth, cuts in ((4096, 1, 1), (0, 4, 1), (0, 1, 3), (4096, 4, 3)):
        got = _run(fx, xs, depth, cuts, soft_chain=True, soft_header=True, segment_len=seg)
        assert [_key(f) for f in got] == [_key(f) for f in ref], (seg, depth, cuts)
    # a frame lies across a cut of the three-block feed
    cutpos = [len(xs[0]) * k // 3 for k in (1, 2)]
    assert any(f["start"] < c < f["start"] + 2 * f["num_framesyms"] for f in ref for c in cutpos)


# ---------------------------------------------------------------------------------------------------- (5) the drop-in
def test_dropin_soft_chain_matches_the_batched_context(fx):
    L = fx.lib()
    x = _low_streams(fx, R.FEC_GOLAY)[1][0]
    got = []
    cbf = fx._ffi.FRAMESYNC_CALLBACK(lambda hd, hv, pl, n, pv, st, ud: got.append(
        (C.string_at(hd, 20), hv, pv, C.string_at(pl, n) if (pl and n) else b"")) or 0)
    q = L.flexframesync_create(cbf, None)
    assert q
    try:
        assert L.flexframesync_decode_payload_soft(q, 1) == 0
        assert L.fxrx_sync_set_soft_chain(q, 1) == -1                 # without soft_block: refused, the setting stays off
        assert L.fxrx_sync_set_soft_chain(q, 0) == 0
        assert L.fxrx_sync_set_soft_block(q, 1) == 0
        L.fxrx_sync_set_threshold(q, 0.0)
        xx = np.ascontiguousarray(np.concatenate([x, np.zeros(256 - len(x) % 256, np.complex64)]))
        feed = lambda: [L.flexframesync_execute(q, xx[i:i + 256].ctypes.data, 256) for i in range(0, len(xx), 256)]
        def drain():
            L.fxrx_sync_flush(q)
            while L.fxrx_sync_pending(q):
                L.flexframesync_execute(q, None, 0)
        feed(); drain()
        refused, got[:] = list(got), []
        assert L.fxrx_sync_set_soft_chain(q, 1) == 0
        feed(); drain()
    finally:
        L.flexframesync_destroy(q)
    pick = lambda fr: [(f["header"], f["header_valid"], f["payload_valid"], f["payload"]) for f in fr]
    assert refused == pick(_run(fx, [xx]))                           # the refused setter left soft_block's results
    want = pick(_run(fx, [xx], soft_chain=True))
    assert got == want and len(got) > 10 and got != refused


# ---------------------------------------------------------------------------------------------------- (6) gain
# (fec1, the model's Es/N0, its valid payloads of 200 with soft_block, with soft_chain, samples): the module's table
# (at snr_db -2 about one header in 400 decodes: a long stream, for a count of frames that can show the margin)
GAIN = [(R.FEC_H74, 1.0, 43, 165, 24_000_000), (R.FEC_H128, 2.0, 80, 190, 1_000_000)]
SAMPLES_PER_SYMBOL_DB = 10.0 * np.log10(2.0)


def test_soft_chain_gains_over_soft_block(fx):
    xs = [fx.synth_stream(ns, stream_id=7800 + i, mod=R.PSK4, fec0=R.FEC_V27, fec1=f1, payload_len=64, snr_db=round(esn0 - SAMPLES_PER_SYMBOL_DB))[0]
          for i, (f1, esn0, _, _, ns) in enumerate(GAIN)]
    counts, headers = {}, {}
    for sc in (False, True):
        ctx = fx.RxContext(len(xs), soft_decision=True, soft_block=True, soft_chain=sc, soft_header=True)
        for f in ctx.process(xs):
            counts[(f["stream"], sc)] = counts.get((f["stream"], sc), 0) + f["payload_valid"]
            headers[(f["stream"], sc)] = headers.get((f["stream"], sc), 0) + f["header_valid"]
        ctx.close()
    print("valid payloads soft_block / soft_chain:", counts, "valid headers:", headers)
    for i, (f1, esn0, m_sb, m_sc, _) in enumerate(GAIN):
        off, on, hv = counts.get((i, False), 0), counts.get((i, True), 0), headers.get((i, True), 0)
        assert headers.get((i, False), 0) == hv and hv >= 15
        assert on - off >= 0.5 * (m_sc - m_sb) / 200.0 * hv, (f1, esn0, off, on, hv)
