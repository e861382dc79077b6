"""The bound on f and the soft hand-over of soft-decision Reed-Solomon decoding (fxrx_config.soft_rs_fmax, soft_rs_chain) on the GPU
(`-m gpu`).  The checker is the numpy reference of tests/ref_rs_chain.py.
  (1) fxrx_debug_rs_chain -- the decode kernel's rs_decode_soft_wave -- against the reference in every byte, soft value and chosen f:
      the crafted blocks and packets of tests/rs_chain_cases.py and its seeded noisy packets, at n = 1, 223, 224, 225 and 446 message
      bytes, for fmax 0, 2, 16, 30, 32 and both output forms; chain = 0 at fmax = 32 is fxrx_debug_rs_soft.
  (2) Whole frames with want_framesyms, Reed-Solomon over V27 and over punctured rates, PSK4 and QAM16, 64 and 300 bytes (three
      Reed-Solomon blocks), inside the waterfall and at 20 dB: payload and payload_valid of every frame with a valid header equal
      ref_rs_chain.packet_decode_rs_chain on the frame's own soft_bits.  Floors from the reference on those soft values: blocks given
      up on, blocks accepted at f > 0, frames whose payload differs between soft_rs_chain on and off.
  (3) Identities on that traffic: the new fields at their defaults change no field of any frame; fmax = 0 without the chain gives the
      payloads of soft_rs = 0; fmax = 32 with the chain those without it; frames of other code pairs are untouched by the chain;
      segmentation and depth do not matter.
  (4) A block of Reed-Solomon-over-V27 frames behind a block without any is decoded at collect and gives the frames of the launch.
  (5) The drop-in setters: return values, and 256-sample calls give the batched result."""
import ctypes as C

import numpy as np
import pytest

import ref_decode as R
import ref_rs_chain as RC
import ref_rs_soft as S
import rs_chain_cases as K

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------- (1) the decoder itself
def _debug(L, n, soft, fmax, chain):
    nb = R.rs_dims(n)[0]
    got, got_f = np.full((len(soft), 8 * n if chain else n), 0x5a, np.uint8), np.full((len(soft), nb), 77, np.uint8)
    assert L.fxrx_debug_rs_chain(n, len(soft), fmax, chain, soft.ctypes.data, got.ctypes.data, got_f.ctypes.data) == 0, L.fxrx_last_error()
    return got, got_f


@pytest.mark.parametrize("n", K.SIZES)
def test_debug_rs_chain_matches_the_reference(fx, n):
    L = fx.lib()
    soft, _, ncraft = K.packet_set(n)
    for fmax in K.FMAX:
        hard, so, chosen = K.packet_reference(n, fmax)
        for chain, want in ((0, hard), (1, so)):
            got, got_f = _debug(L, n, soft, fmax, chain)
            bad = np.nonzero((got != want).any(axis=1) | (got_f != chosen).any(axis=1))[0]
            assert len(bad) == 0, "n=%d fmax=%d chain=%d: %d of %d packets differ, first #%d: f got %s want %s" % (
                n, fmax, chain, len(bad), len(soft), bad[0], got_f[bad[0]], chosen[bad[0]])
        noisy = chosen[ncraft:]
        print("n=%d fmax=%d: %d packets; noisy blocks given up on %d of %d, accepted at f > 0 %d" % (
            n, fmax, len(soft), int((noisy == RC.NO_F).sum()), noisy.size, int(((noisy != RC.NO_F) & (noisy > 0)).sum())))
    acc, gone = K.noisy_shares(n)
    assert acc >= 0.1 and gone >= 0.1


@pytest.mark.parametrize("n", K.SIZES)
def test_hard_form_without_a_bound_is_debug_rs_soft(fx, n):
    L = fx.lib()
    soft = K.packet_set(n)[0]
    nb = R.rs_dims(n)[0]
    got, got_f = _debug(L, n, soft, 32, 0)
    want, want_f = np.zeros((len(soft), n), np.uint8), np.full((len(soft), nb), 77, np.uint8)
    assert L.fxrx_debug_rs_soft(n, len(soft), soft.ctypes.data, want.ctypes.data, want_f.ctypes.data) == 0, L.fxrx_last_error()
    assert (got == want).all() and (got_f == want_f).all() and (got_f != RC.NO_F).all()


# ---------------------------------------------------------------------------------------------------- traffic
def _key(f):
    return tuple((k, f[k].tobytes() if isinstance(f[k], np.ndarray) else f[k]) for k in sorted(f))


def _run(fx, xs, depth=1, **kw):
    ctx = fx.RxContext(len(xs), want_framesyms=True, soft_decision=True, **kw)
    ctx.set_depth(depth)
    got = ctx.process(xs)
    ctx.close()
    return sorted(got, key=lambda f: (f["stream"], f["start"]))


# (mod, fec0, fec1, payload_len, snr_db): Reed-Solomon in front of a convolutional code, inside the waterfall that
# profiles/soft_rs_sensitivity.txt records (PSK4 2 - 4 dB, QAM16 8 - 10 dB), a little above it (where blocks are near the decoder's
# radius: accepted at f > 0), and a 20 dB control
RSV_SPEC = [(R.PSK4, R.FEC_V27, R.FEC_RS, 64, 3.0), (R.PSK4, R.FEC_V27, R.FEC_RS, 300, 4.0), (R.QAM16, R.FEC_V27, R.FEC_RS, 64, 9.0),
            (R.QAM16, R.FEC_V27P34, R.FEC_RS, 300, 10.0), (R.PSK4, R.FEC_V27P23, R.FEC_RS, 64, 3.75), (R.QAM16, R.FEC_V27, R.FEC_RS, 64, 10.0),
            (R.PSK4, R.FEC_V27, R.FEC_RS, 300, 20.0)]
OTHER_SPEC = [(R.PSK4, R.FEC_V27, R.FEC_GOLAY, 64, 1.0), (R.QAM16, R.FEC_V27, R.FEC_H128, 64, 6.0), (R.PSK4, R.FEC_NONE, R.FEC_SD72, 64, 4.0),
              (R.PSK4, R.FEC_V27, R.FEC_NONE, 64, 2.0), (R.PSK4, R.FEC_RS, R.FEC_GOLAY, 64, 3.0), (R.PSK4, R.FEC_NONE, R.FEC_RS, 64, 3.5),
              (R.PSK4, R.FEC_RS, R.FEC_NONE, 64, 4.0), (R.PSK4, R.FEC_NONE, R.FEC_NONE, 64, 6.0)]
LEVELS = [dict(), dict(soft_block=True), dict(soft_block=True, soft_chain=True)]


def _streams(fx, spec, base, ns=60_000):
    return [fx.synth_stream(ns, stream_id=base + i, mod=m, fec0=f0, fec1=f1, payload_len=n, snr_db=snr)[0] for i, (m, f0, f1, n, snr) in enumerate(spec)]


@pytest.fixture(scope="module")
def rsv_streams(fx):
    return _streams(fx, RSV_SPEC, 9500)


_TRACES = {}


def _group_trace(key, v):
    """ref_rs_soft's 17 trials on a group's blocks, once per set of soft values (they do not depend on the decoder's options)"""
    k = (key, hash(v.tobytes()))
    if k not in _TRACES:
        tr = {}
        S.rs_decode_soft_blocks(v, tr)
        _TRACES[k] = tr
    return _TRACES[k]


def _reference(frames, fmax, chain, stats=None):
    """ref_rs_chain.packet_decode_rs_chain of every frame's soft_bits -- (payload, valid) per frame --, the frames of one shape as one
    batch (test_rs_chain.py ties the batched steps to the per-packet functions).  Frames must be Reed-Solomon over a convolutional
    code.  stats (a dict) counts blocks: 'given_up', 'accepted_f_gt_0', 'blocks'."""
    out, groups = [None] * len(frames), {}
    for i, f in enumerate(frames):
        assert f["fec1"] == R.FEC_RS and f["fec0"] in R.CONV
        groups.setdefault((len(f["payload"]), f["check"], f["fec0"]), []).append(i)
    for (n, check, fec0), idx in groups.items():
        k, l0, l1 = R.packet_dims(n, check, fec0, R.FEC_RS)
        nb, dl = R.rs_dims(l0)
        v = np.stack([R.interleave_soft(np.asarray(frames[i]["soft_bits"], np.uint8)[:8 * l1], l1, decode=True) for i in idx])
        v = np.ascontiguousarray(v[:, :8 * nb * (dl + 32)].reshape(-1, 8 * (dl + 32)))
        blocks, chosen = RC.bounded_from_trace(_group_trace((n, check, fec0), v), fmax)
        if stats is not None:
            stats["blocks"] = stats.get("blocks", 0) + len(chosen)
            stats["given_up"] = stats.get("given_up", 0) + int((chosen == RC.NO_F).sum())
            stats["accepted_f_gt_0"] = stats.get("accepted_f_gt_0", 0) + int(((chosen != RC.NO_F) & (chosen > 0)).sum())
        if chain:
            so = RC.blocks_soft_out(v, blocks, chosen)[:, :8 * dl].reshape(len(idx), 8 * nb * dl)[:, :8 * l0]
            v0 = np.stack([R.interleave_soft(x, l0, decode=True) for x in so])
            dec = R.viterbi(fec0, v0.astype(np.int64), k, 255)[0]
        else:
            b1 = blocks[:, :dl].reshape(len(idx), nb * dl)[:, :l0]
            in0 = np.stack([R.interleave(d, decode=True) for d in b1])
            dec = R.viterbi(fec0, np.unpackbits(in0, axis=1).astype(np.int64), k, 1)[0]
        for i, d in zip(idx, dec):
            out[i] = R._finish(np.asarray(d, np.uint8), n, check)
    return out


def test_batched_reference_is_the_per_packet_reference(fx, rsv_streams):
    frames = [f for f in _run(fx, rsv_streams[:2], soft_rs=True, soft_header=True) if f["header_valid"]][::9]
    for fmax, chain in ((16, True), (0, False)):
        for f, w in zip(frames, _reference(frames, fmax, chain)):
            assert RC.packet_decode_rs_chain(f["soft_bits"], len(f["payload"]), f["check"], f["fec0"], f["fec1"], fmax, chain) == w


@pytest.mark.parametrize("fmax,chain", [(16, True), (0, True), (24, True), (16, False), (32, True)], ids=["f16_chain", "f0_chain", "f24_chain", "f16", "f32_chain"])
def test_low_snr_frames_follow_the_reference(fx, rsv_streams, fmax, chain):
    on = _run(fx, rsv_streams, soft_rs=True, soft_rs_fmax=fmax, soft_rs_chain=chain, soft_header=True)
    frames = [f for f in on if f["header_valid"]]
    stats = {}
    want = _reference(frames, fmax, chain, stats)
    other = _reference(frames, fmax, not chain)
    valid = differ = 0
    for f, w, o in zip(frames, want, other):
        assert (f["payload"], f["payload_valid"]) == w, (f["stream"], f["start"])
        valid += f["payload_valid"]; differ += w[0] != o[0]
    print("fmax %d chain %d: %d frames, %d valid; blocks %s; payload differs from chain %s in %d frames" % (fmax, chain, len(frames), valid, stats, "off" if chain else "on", differ))
    assert len(frames) > 60 and 0 < valid < len(frames)
    assert {len(f["payload"]) for f in frames} == {64, 300}
    if fmax < 32:
        # the traffic is not trivial: blocks given up on, blocks won by erasures, and frames that the hand-over changes
        assert stats["given_up"] > 0 and differ > 0
    if fmax >= 16:
        assert stats["accepted_f_gt_0"] > 0
    if fmax == 32:
        assert stats["given_up"] == 0 and differ == 0


def test_identities_on_that_traffic(fx, rsv_streams):
    for level in LEVELS:
        base = _run(fx, rsv_streams, soft_rs=True, soft_header=True, **level)
        again = _run(fx, rsv_streams, soft_rs=True, soft_rs_fmax=None, soft_rs_chain=False, soft_header=True, **level)
        assert [_key(f) for f in again] == [_key(f) for f in base] and len(base) > 60          # the defaults: every field of every frame
    pay = lambda fr: [(f["stream"], f["start"], f["header_valid"], f["payload_valid"], f["payload"]) for f in fr]
    hard = _run(fx, rsv_streams, soft_header=True)
    assert pay(_run(fx, rsv_streams, soft_rs=True, soft_rs_fmax=0, soft_header=True)) == pay(hard)
    assert pay(_run(fx, rsv_streams, soft_rs=True, soft_rs_fmax=32, soft_rs_chain=True, soft_header=True)) == pay(_run(fx, rsv_streams, soft_rs=True, soft_header=True))
    assert pay(hard) != pay(_run(fx, rsv_streams, soft_rs=True, soft_rs_fmax=0, soft_rs_chain=True, soft_header=True))


def test_other_code_pairs_are_untouched_by_the_chain(fx, rsv_streams):
    xs = rsv_streams[:2] + _streams(fx, OTHER_SPEC, 9600)
    acts = lambda f: f["header_valid"] and f["fec1"] == R.FEC_RS and f["fec0"] in R.CONV
    for level in LEVELS:
        off = _run(fx, xs, segment_len=16384, soft_header=True, soft_rs=True, soft_rs_fmax=16, **level)
        on = _run(fx, xs, segment_len=16384, soft_header=True, soft_rs=True, soft_rs_fmax=16, soft_rs_chain=True, **level)
        plain = lambda fr: [_key(f) for f in fr if not acts(f)]
        assert plain(off) == plain(on) and len(plain(on)) > 80
        assert {(f["fec0"], f["fec1"]) for f in on if f["header_valid"] and not acts(f)} >= {(f0, f1) for _, f0, f1, _, _ in OTHER_SPEC}
        assert [_key(f) for f in off] != [_key(f) for f in on]


def test_results_do_not_depend_on_how_the_input_is_fed(fx, rsv_streams):
    kw = dict(soft_rs=True, soft_rs_fmax=16, soft_rs_chain=True, soft_header=True)
    ref = _run(fx, rsv_streams, **kw)
    assert sum(f["header_valid"] for f in ref) > 60
    for seg, depth in ((4096, 1), (0, 4), (4096, 4)):
        got = _run(fx, rsv_streams, depth, segment_len=seg, **kw)
        assert [_key(f) for f in got] == [_key(f) for f in ref], (seg, depth)


# ---------------------------------------------------------------------------------------------------- (4) the late path
def test_unannounced_reed_solomon_block_is_decoded_at_collect_the_same_way(fx, rsv_streams):
    x = rsv_streams[1]                                             # PSK4, Reed-Solomon over V27, 300 bytes, 4 dB
    other = fx.synth_stream(20_000, stream_id=9700, payload_len=64)[0]          # (PSK4, V27, no outer code, 20 dB)
    kw = dict(want_framesyms=True, soft_decision=True, soft_header=True, soft_rs=True, soft_rs_fmax=16, soft_rs_chain=True)
    ctx = fx.RxContext(1, **kw)
    first = ctx.process([x])
    ctx.close()
    # (a fresh context: the Reed-Solomon launch fades out only over many blocks without such frames, and x holds a dozen)
    ctx = fx.RxContext(1, **kw)
    plain = ctx.process([other])
    more_rs = ctx.LATE_REASONS.index("more_rs")
    late0 = ctx.late_stats()[more_rs]
    late = ctx.process([x])
    late1 = ctx.late_stats()[more_rs]
    ctx.close()
    assert len(plain) > 3 and all(f["fec1"] != R.FEC_RS for f in plain)
    assert late1 - late0 == 1
    pick = lambda fr: [(f["header"], f["header_valid"], f["payload_valid"], f["payload"], np.asarray(f["soft_bits"]).tobytes()) for f in fr]
    assert pick(late) == pick(first) and len(first) > 5
    frames = [f for f in late if f["header_valid"]]
    stats = {}
    for f, w in zip(frames, _reference(frames, 16, True, stats)):
        assert (f["payload"], f["payload_valid"]) == w
    assert stats["given_up"] > 0                                                 # blocks of it were handed on as soft values


# ---------------------------------------------------------------------------------------------------- (5) the drop-in
def test_dropin_setters(fx, rsv_streams):
    L = fx.lib()
    pad = lambda x: np.ascontiguousarray(np.concatenate([x, np.zeros(256 - len(x) % 256, np.complex64)]))
    xx = pad(np.concatenate([rsv_streams[0], rsv_streams[1], rsv_streams[4]]))
    got = []
    cbf = fx._ffi.FRAMESYNC_CALLBACK(lambda hd, hv, pl, n, pv, st, ud: got.append(
        (C.string_at(hd, 20), hv, pv, C.string_at(pl, n) if (pl and n) else b"")) or 0)
    q = L.flexframesync_create(cbf, None)
    assert q

    def feed(x):
        got[:] = []
        for i in range(0, len(x), 256):
            L.flexframesync_execute(q, x[i:i + 256].ctypes.data, 256)
        L.fxrx_sync_flush(q)
        while L.fxrx_sync_pending(q):
            L.flexframesync_execute(q, None, 0)
        return list(got)
    try:
        assert L.flexframesync_decode_payload_soft(q, 1) == 0
        L.fxrx_sync_set_threshold(q, 0.0)
        assert L.fxrx_sync_set_soft_rs_chain(q, 1) == -1              # soft_rs is off: refused, nothing changes
        assert L.fxrx_sync_set_soft_rs_fmax(q, 17) == -1
        assert L.fxrx_sync_set_soft_rs_chain(q, 0) == 0 and L.fxrx_sync_set_soft_rs_fmax(q, 0) == 0
        plain = feed(xx)
        assert L.fxrx_sync_set_soft_rs(q, 1) == 0
        assert L.fxrx_sync_set_soft_rs_fmax(q, 16) == -1              # 16 is the odd bound 15 plus one: refused
        assert L.fxrx_sync_set_soft_rs_fmax(q, 35) == -1
        unbounded = feed(xx)
        assert L.fxrx_sync_set_soft_rs_fmax(q, 17) == 0               # fmax = 16
        assert L.fxrx_sync_set_soft_rs_chain(q, 1) == 0
        on = feed(xx)
    finally:
        L.flexframesync_destroy(q)

    def batched(**kw):
        ctx = fx.RxContext(1, want_framesyms=True, soft_decision=True, **kw)
        fr = ctx.process([xx])
        ctx.close()
        return [(f["header"], f["header_valid"], f["payload_valid"], f["payload"]) for f in fr]
    assert plain == batched() and len(plain) > 40                     # the refused calls changed nothing
    assert unbounded == batched(soft_rs=True)
    assert on == batched(soft_rs=True, soft_rs_fmax=16, soft_rs_chain=True)
    assert on != unbounded and on != plain and on != batched(soft_rs=True, soft_rs_fmax=16)
