"""Soft-decision Reed-Solomon decoding (fxrx_config.soft_rs) on the GPU (`-m gpu`).  The oracle has no such decoder; the checker is the
numpy reference of tests/ref_rs_soft.py.
  (1) fxrx_debug_rs_soft -- the decode kernel's rs_decode_soft_wave -- against the reference, bytes and chosen f, bit for bit: every
      crafted block of tests/rs_soft_cases.py and seeded noisy packets at a noise level where about half decode, at n = 1, 223, 224
      and 446 message bytes (N = 33, N = 255, two blocks of N = 144, two blocks of N = 255).
  (2) Whole frames at low SNR with want_framesyms: payload and payload_valid of every frame with a valid header equal
      ref_rs_soft.packet_decode_soft_rs on the frame's own soft_bits -- Reed-Solomon alone and over V27, PSK4 and QAM16 -- for the
      three soft_block / soft_chain levels; some frames are valid only with soft_rs.
  (3) Frames without a Reed-Solomon stage in a mixed batch are, field for field, those of the soft_rs = 0 run.
  (4) Results do not depend on segmentation (4096-sample segments), depth or cuts of the stream (a cut makes frames turn up
      unannounced: late decodes).
  (5) The drop-in setter's return values.
  (6) The crafted noise-free frames of tests/rs_soft_cases.py (PSK4, CRC-32, 64 bytes, fec1 = Reed-Solomon, fec0 none and V27, 24
      bytes of the block with one bit on the wrong side at a small amplitude; tests/test_rs_soft.py proves on the CPU what they
      are): payload_valid = 0 with soft_decision alone, 1 with soft_rs and the payload the sent one.  Behind a block without
      Reed-Solomon frames the frame turns up unannounced and is decoded at collect (late_stats: 'Reed-Solomon frames without a
      launch'); fed once more it goes through the launch; both give the frame of the fresh context."""
import numpy as np
import pytest

import ref_decode as R
import ref_rs_soft as S
import rs_soft_cases as K

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------- (1) the decoder itself
COUNT = {1: 700, 223: 400, 224: 300, 446: 200}        # noisy packets per size: 2100 blocks in all (the reference takes seconds for them)


@pytest.mark.parametrize("n", K.SIZES)
def test_debug_rs_soft_matches_the_reference(fx, n):
    L = fx.lib()
    nb, dl = R.rs_dims(n)
    soft, want, want_f = K.packet_reference(n, COUNT[n], 4100 + n)
    got, got_f = np.zeros((len(soft), n), np.uint8), np.full((len(soft), nb), 77, np.uint8)
    assert L.fxrx_debug_rs_soft(n, len(soft), soft.ctypes.data, got.ctypes.data, got_f.ctypes.data) == 0, L.fxrx_last_error()
    bad = np.nonzero((got != want).any(axis=1) | (got_f != want_f).any(axis=1))[0]
    assert len(bad) == 0, "n=%d: %d of %d packets differ, first #%d: f got %s want %s" % (n, len(bad), len(soft), bad[0], got_f[bad[0]], want_f[bad[0]])
    noisy = want_f[len(K.case_packets(n)):]
    print("n=%d: %d packets, hard decoder's candidate wins %d of %d noisy blocks" % (n, len(soft), int((noisy == 0).sum()), noisy.size))
    assert 0.2 < (noisy == 0).mean() < 0.9


# ---------------------------------------------------------------------------------------------------- traffic
def _key(f):
    return tuple((k, f[k].tobytes() if isinstance(f[k], np.ndarray) else f[k]) for k in sorted(f))


def _run(fx, xs, depth=1, cuts=1, **kw):
    ctx = fx.RxContext(len(xs), want_framesyms=True, soft_decision=True, **kw)
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


# (mod, fec0, fec1, payload_len, snr_db): Reed-Solomon next to the channel -- fec1, or fec0 when fec1 is none --, near its limit
RS_SPEC = [(R.PSK4, R.FEC_NONE, R.FEC_RS, 64, 3.5), (R.PSK4, R.FEC_NONE, R.FEC_RS, 300, 4.5), (R.QAM16, R.FEC_NONE, R.FEC_RS, 64, 10.5),
           (R.PSK4, R.FEC_V27, R.FEC_RS, 64, 3.5), (R.QAM16, R.FEC_V27, R.FEC_RS, 230, 10.5), (R.PSK4, R.FEC_RS, R.FEC_NONE, 64, 4.0)]
OTHER_SPEC = [(R.PSK4, R.FEC_V27, R.FEC_GOLAY, 64, 1.0), (R.QAM16, R.FEC_V27, R.FEC_H128, 64, 6.0), (R.PSK4, R.FEC_NONE, R.FEC_SD72, 64, 4.0),
              (R.PSK4, R.FEC_V27, R.FEC_NONE, 64, 0.0), (R.PSK4, R.FEC_RS, R.FEC_GOLAY, 64, 3.0), (R.PSK4, R.FEC_NONE, R.FEC_NONE, 64, 6.0)]


def _streams(fx, spec, base, ns=60_000):
    return [fx.synth_stream(ns, stream_id=base + i, mod=m, fec0=f0, fec1=f1, payload_len=n, snr_db=snr)[0] for i, (m, f0, f1, n, snr) in enumerate(spec)]


def _reference(frames, soft_rs):
    """ref_rs_soft.packet_decode_soft_rs (soft_rs off: ref_decode.packet_decode_soft) of every frame's soft_bits, the frames of one
    shape as one batch: (payload, valid) per frame"""
    out, groups = [None] * len(frames), {}
    for i, f in enumerate(frames):
        groups.setdefault((len(f["payload"]), f["check"], f["fec0"], f["fec1"]), []).append(i)
    hard = lambda s: np.packbits((np.asarray(s) > 127).astype(np.uint8), axis=-1)
    for (n, check, fec0, fec1), idx in groups.items():
        k, l0, l1 = R.packet_dims(n, check, fec0, fec1)
        stage0 = fec1 == R.FEC_NONE
        if not (fec1 == R.FEC_RS or (stage0 and fec0 == R.FEC_RS)):
            for i in idx:
                out[i] = R.packet_decode_soft(frames[i]["soft_bits"], n, check, fec0, fec1)
            continue
        nout = k if stage0 else l0
        nb, dl = R.rs_dims(nout)
        v = np.stack([R.interleave_soft(np.asarray(frames[i]["soft_bits"], np.uint8)[:8 * l1], l1, decode=True) for i in idx])
        if stage0:
            v = np.stack([R.interleave_soft(x, l0, decode=True) for x in v])
        v = v[:, :8 * nb * (dl + 32)].reshape(-1, 8 * (dl + 32))
        if soft_rs:
            blocks = S.rs_decode_soft_blocks(v)[0]
        else:
            # (the f = 0 candidate, batched: tests/test_rs_soft.py shows that it is ref_decode.rs_decode_block's result)
            blocks = S.rs_decode_erasures_batch(hard(v), np.zeros((len(v), 0), np.int64))[0]
        dec = blocks[:, :dl].reshape(len(idx), nb * dl)[:, :nout]
        if not stage0:
            in0 = np.stack([R.interleave(d, decode=True) for d in dec])
            dec = R.viterbi(fec0, np.unpackbits(in0, axis=1).astype(np.int64), k, 1)[0] if fec0 in R.CONV else np.stack([R.fec_decode(fec0, x, k) for x in in0])
        for i, d in zip(idx, dec):
            out[i] = R._finish(np.asarray(d, np.uint8), n, check)
    return out


@pytest.fixture(scope="module")
def rs_streams(fx):
    return _streams(fx, RS_SPEC, 9100)


@pytest.mark.parametrize("level", [dict(), dict(soft_block=True), dict(soft_block=True, soft_chain=True)], ids=["soft", "soft_block", "soft_chain"])
def test_low_snr_frames_follow_the_reference(fx, rs_streams, level):
    on = _run(fx, rs_streams, soft_rs=True, soft_header=True, **level)
    off = {(f["stream"], f["start"]): f for f in _run(fx, rs_streams, soft_header=True, **level)}
    checked = valid = valid_off = only_on = only_off = 0
    frames = [f for f in on if f["header_valid"]]
    offs = [off[(f["stream"], f["start"])] for f in frames]
    for f, want, o, want_off in zip(frames, _reference(frames, True), offs, _reference(offs, False)):
        assert (f["payload"], f["payload_valid"]) == want, (f["stream"], f["start"])
        assert (o["payload"], o["payload_valid"]) == want_off, (o["stream"], o["start"])
        checked += 1; valid += f["payload_valid"]; valid_off += o["payload_valid"]
        only_on += f["payload_valid"] and not o["payload_valid"]; only_off += o["payload_valid"] and not f["payload_valid"]
    print("%d frames checked: valid %d with soft_rs, %d without; %d only with, %d only without" % (checked, valid, valid_off, only_on, only_off))
    assert checked == sum(f["header_valid"] for f in on) and checked > 60 and 0 < valid < checked
    assert only_on > 0                                   # the option decodes frames that are lost without it


def test_frames_without_reed_solomon_are_those_of_soft_rs_off(fx, rs_streams):
    xs = rs_streams[:2] + _streams(fx, OTHER_SPEC, 9200)
    for level in (dict(), dict(soft_block=True), dict(soft_block=True, soft_chain=True)):
        off, on = _run(fx, xs, segment_len=16384, **level), _run(fx, xs, segment_len=16384, soft_rs=True, **level)
        soft_stage = lambda f: f["fec1"] == R.FEC_RS or (f["fec1"] == R.FEC_NONE and f["fec0"] == R.FEC_RS)
        plain = lambda fr: [_key(f) for f in fr if not (f["header_valid"] and soft_stage(f))]
        assert plain(off) == plain(on) and len(plain(on)) > 60
        assert [_key(f) for f in off] != [_key(f) for f in on]


def test_results_do_not_depend_on_how_the_input_is_fed(fx, rs_streams):
    ref = _run(fx, rs_streams, soft_rs=True, soft_header=True)
    assert sum(f["header_valid"] for f in ref) > 60
    for seg, depth, cuts in ((4096, 1, 1), (0, 4, 1), (0, 1, 3), (4096, 4, 3)):
        got = _run(fx, rs_streams, depth, cuts, soft_rs=True, soft_header=True, segment_len=seg)
        assert [_key(f) for f in got] == [_key(f) for f in ref], (seg, depth, cuts)
    cutpos = [len(rs_streams[0]) * k // 3 for k in (1, 2)]
    assert any(f["start"] < c < f["start"] + 2 * f["num_framesyms"] for f in ref for c in cutpos)


# ---------------------------------------------------------------------------------------------------- (6) the crafted frames
@pytest.mark.parametrize("fec0", [R.FEC_NONE, R.FEC_V27], ids=["rs_alone", "rs_over_v27"])
def test_crafted_frame_is_lost_hard_and_decoded_with_soft_rs(fx, fec0):
    c, x = K.frame_case(fec0), K.frame_stream(fec0)
    other = fx.synth_stream(20_000, stream_id=9300, payload_len=64)[0]          # (PSK4, V27, no outer code, 20 dB)
    for level in (dict(), dict(soft_block=True), dict(soft_block=True, soft_chain=True)):
        off = _run(fx, [x], **level)
        assert len(off) == 1 and off[0]["header_valid"] and (off[0]["fec0"], off[0]["fec1"]) == (fec0, R.FEC_RS)
        assert off[0]["payload_valid"] == 0 and off[0]["payload"] != c["payload"]
        ctx = fx.RxContext(1, want_framesyms=True, soft_decision=True, soft_rs=True, **level)
        first = ctx.process([x])
        assert len(first) == 1 and first[0]["payload_valid"] == 1 and first[0]["payload"] == c["payload"]
        # a block without Reed-Solomon frames, then the frame: it turns up unannounced and is decoded at collect; once more: by the launch
        ctx.reset()
        plain = ctx.process([other])
        more_rs = ctx.LATE_REASONS.index("more_rs")
        late0 = ctx.late_stats()[more_rs]
        late = ctx.process([x])
        late1 = ctx.late_stats()[more_rs]
        again = ctx.process([x])
        late2 = ctx.late_stats()[more_rs]
        ctx.close()
        assert len(plain) > 3 and all(f["payload_valid"] and f["fec1"] != R.FEC_RS for f in plain)
        assert (late1 - late0, late2 - late1) == (1, 0)
        pick = lambda fr: [(f["header"], f["header_valid"], f["payload_valid"], f["payload"], np.asarray(f["soft_bits"]).tobytes()) for f in fr]
        assert pick(late) == pick(first) == pick(again)
        v = R.interleave_soft(np.asarray(first[0]["soft_bits"], np.uint8)[:8 * c["dims"][2]], c["dims"][2], decode=True)
        assert (S.hard_bytes(v) == c["word"]).all()                  # the receiver demapped the crafted word


# ---------------------------------------------------------------------------------------------------- (5) the drop-in
def test_dropin_setter_return_values(fx):
    L = fx.lib()
    cbf = fx._ffi.FRAMESYNC_CALLBACK(lambda hd, hv, pl, n, pv, st, ud: 0)
    q = L.flexframesync_create(cbf, None)
    assert q
    try:
        assert L.fxrx_sync_set_soft_rs(q, 1) == -1                    # soft payload decoding is off: refused, the setting stays off
        assert L.fxrx_sync_set_soft_rs(q, 0) == 0
        assert L.flexframesync_decode_payload_soft(q, 1) == 0
        assert L.fxrx_sync_set_soft_rs(q, 1) == 0
        assert L.fxrx_sync_set_soft_rs(q, 0) == 0
    finally:
        L.flexframesync_destroy(q)
