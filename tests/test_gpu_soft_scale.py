"""The soft payload options at full frame length, in bulk, and through the drop-in, on the GPU (`-m gpu`).  The checkers are the
numpy references of tests/ref_block_soft.py, ref_block_siso.py and ref_rs_soft.py; the cases are those of tests/soft_scale_cases.py,
which tests/test_soft_scale.py shows on the CPU to be what they are named.

  (a) fxrx_debug_block_decode(soft = 1), fxrx_debug_block_siso and fxrx_debug_rs_soft on every case, bit for bit: bytes, soft outputs,
      chosen f.  Lengths are a stage's sizes for a 65535-byte payload with CRC-32: up to 262 160 codewords in 4097 rounds of 64
      lanes, 588 Reed-Solomon blocks in one wave.
  (b) Whole 65535-byte frames, one per stream, CRC-32, want_framesyms and soft_decision on, at every level of soft_block, soft_chain
      and soft_rs: payload and payload_valid equal the reference decode of the frame's own soft_bits; with the options that let the
      stage next to the channel decode from soft values, they equal the sent payload.  A Reed-Solomon frame that meets the
      coverage condition (a block won by a candidate with f > 0: the hard decoder fails there) is not valid without soft_rs
      unless a Viterbi decoder behind it repairs it, so at the levels without soft_rs such a frame is held to the reference only.  The coverage conditions of
      tests/test_soft_scale.py are asserted on the frames' own soft_bits.
  (c) Reed-Solomon frames in bulk under soft_rs: 0 .. 16 payload bytes, more than 4 x 64 of them in a context's first block, so that
      waves of the soft_rs instance take several frames each with the GF tables kept in LDS; the same block again on the same
      context, its grid taken from the block before.
  (d) The drop-in with fxrx_sync_set_soft_rs, fed in 256-sample calls, delivers the batched soft_rs context's frames.
  (e) equalizer, soft_header, soft_block, soft_chain and soft_rs together over sc16 and sc8 input: field for field the float path
      on fxrx_iq_convert_host's output, payloads by the references.

SNRs of (b) and (c), and what the references counted on an MI355X: FULL and BULK_SNR below."""
import ctypes as C
import time

import numpy as np
import pytest

import ref_decode as R
import ref_block_soft as B
import ref_block_siso as S
import ref_rs_soft as RS
import ref_ingest as ri
import rs_soft_cases as RK
import soft_scale_cases as K
from test_ingest import quantised
from test_gpu_ingest import same, run_int, run_float, make_ctx
from test_gpu_rs_soft import RS_SPEC, _streams, _key

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------- (a) the decoders at scale
@pytest.mark.parametrize("c", K.BLOCK_CASES, ids=K.case_id)
def test_block_decoders_at_full_length_match_the_reference(fx, c):
    fs, n = c
    L = fx.lib()
    t0 = time.time()
    ref = K.block_reference(fs, n)
    t1 = time.time()
    soft = ref["soft"]
    got = np.zeros((K.PACKETS, n), np.uint8)
    assert L.fxrx_debug_block_decode(fs, 1, n, K.PACKETS, soft.ctypes.data, got.ctypes.data) == 0, L.fxrx_last_error()
    got_siso = np.zeros((K.PACKETS, 8 * n), np.uint8)
    assert L.fxrx_debug_block_siso(fs, n, K.PACKETS, soft.ctypes.data, got_siso.ctypes.data) == 0, L.fxrx_last_error()
    print("%s: reference %.1f s, GPU calls %.1f s" % (K.case_id(c), t1 - t0, time.time() - t1))
    for p in range(K.PACKETS):
        bad = K.lanes_that_differ(fs, got[p], ref["dec"][p])[0]
        assert len(bad) == 0, "packet %d: %d codewords differ, first #%d (round %d)" % (p, len(bad), bad[0], bad[0] // K.LANES)
        bad = np.nonzero(got_siso[p] != ref["siso"][p])[0]
        assert len(bad) == 0, "packet %d: %d soft outputs differ, first in codeword #%d" % (p, len(bad), bad[0] // K.message_bits(fs))


@pytest.mark.parametrize("n", K.RS_CASES)
def test_rs_soft_at_full_length_matches_the_reference(fx, n):
    L = fx.lib()
    nb, dl = R.rs_dims(n)
    t0 = time.time()
    ref = K.rs_reference(n)
    t1 = time.time()
    got, got_f = np.zeros((K.PACKETS, n), np.uint8), np.full((K.PACKETS, nb), 77, np.uint8)
    assert L.fxrx_debug_rs_soft(n, K.PACKETS, ref["soft"].ctypes.data, got.ctypes.data, got_f.ctypes.data) == 0, L.fxrx_last_error()
    print("n=%d: reference %.1f s, GPU call %.1f s" % (n, t1 - t0, time.time() - t1))
    for p in range(K.PACKETS):
        bad = np.nonzero(got_f[p] != ref["f"][p])[0]
        assert len(bad) == 0, "packet %d: f differs in %d of %d blocks, first #%d: got %d want %d" % (p, len(bad), nb, bad[0], got_f[p][bad[0]], ref["f"][p][bad[0]])
        bad = np.nonzero(got[p] != ref["dec"][p])[0]
        assert len(bad) == 0, "packet %d: %d bytes differ, first in block #%d" % (p, len(bad), bad[0] // dl)


# ---------------------------------------------------------------------------------------------------- (b) whole frames
# (mod, fec0, fec1, snr_db, synth_stream's stream_id: payload and noise).  Hamming(12,8) behind V27 is 1.5 x 2 x 65539 bytes: QAM64 keeps
# it under 0.6 Msamples.  Block codes: from the SNR of the code's low-SNR test (tests/test_gpu_block_soft.LOW, test_gpu_block_siso.SNR_V27,
# moved to the modulation), raised in steps of 0.25 / 0.5 dB until the frame was valid at every level: Golay 8.5 -> 9.0, Hamming(12,8)
# 12.25 -> 12.5 (soft_chain alone decodes it from 12.0), SECDED(72,64) 8.75 -> 9.0.  Reed-Solomon: from test_gpu_rs_soft.RS_SPEC's 10.5 dB.
# With 294 blocks a frame the window between "valid with soft_rs" and "no block needs f > 0 any more" is 0.2 dB wide, so it was
# searched in steps of 0.1 dB over three noise seeds a pair for a frame that is valid with soft_rs and has a block won by f > 0 in
# every third.  Measured on an MI355X (blocks won by f > 0 per third; histogram of f / 2):
#   (none, RS) 12.0 dB (2, 1, 2), f: 289 x 0, 3 x 2, 2 x 4;  (V27, RS) 12.0 dB (4, 3, 2), f: 579 x 0 and 9 blocks at f = 2 .. 28;
#   (RS, none) 12.5 dB (2, 1, 1), f: 290 x 0, one each at 2, 4, 8, 18.  Without soft_rs the two pairs with nothing behind the
#   Reed-Solomon stage are invalid; behind (V27, RS) the Viterbi decoder repairs what the hard Reed-Solomon decoder leaves.
# Block codes, codewords on which soft and hard decoding differ (first round, last round, rounds between the 129th codeword and the
# last round): Golay 252 of 43 693 (1, 1, 249); Hamming(12,8) 15 905 of 131 080 (8, 1, 15 884); SECDED(72,64) 9496 of 16 385 blocks
# (39, 1, 9385).  A valid Golay frame without an inner code has few such codewords (every one must come out right), and SECDED's last
# round is one block: their noise seeds are the first of 240 and of 14 tried with which the frame is valid and the condition holds.
FULL = [(R.QAM16, R.FEC_NONE, R.FEC_GOLAY, 9.0),
        (R.QAM64, R.FEC_V27, R.FEC_H128, 12.5),
        (R.QAM16, R.FEC_V27, R.FEC_SD72, 9.0),
        (R.QAM16, R.FEC_NONE, R.FEC_RS, 12.0),
        (R.QAM16, R.FEC_V27, R.FEC_RS, 12.0),
        (R.QAM16, R.FEC_RS, R.FEC_NONE, 12.5)]
FULL_IDS = (10194, 9701, 9772, 9718, 9723, 9725)
LEVELS = {"soft_block": dict(), "soft_chain": dict(soft_chain=True), "soft_block+soft_rs": dict(soft_rs=True),
          "soft_chain+soft_rs": dict(soft_chain=True, soft_rs=True)}


def _rs_pair(f0, f1):
    return f1 == R.FEC_RS or (f1 == R.FEC_NONE and f0 == R.FEC_RS)


def _rule(f0, f1, level):
    """which reference a level's result of a (fec0, fec1) frame follows"""
    if _rs_pair(f0, f1):
        return "rs" if LEVELS[level].get("soft_rs") else "hard_rs"
    return "chain" if LEVELS[level].get("soft_chain") and S.chained(f0, f1) else "block"


def full_streams(fx, spec, ids=None):
    xs, sent = [], []
    for i, (m, f0, f1, snr) in enumerate(spec):
        sid = FULL_IDS[i] if ids is None else ids[i]
        g = fx.FrameGen(m, f0, f1, K.CHECK)
        n = len(g.frame(np.zeros(K.PAYLOAD, np.uint8)))
        g.close()
        x, fr = fx.synth_stream(n + 2000, stream_id=sid, mod=m, fec0=f0, fec1=f1, check=K.CHECK, payload_len=K.PAYLOAD, snr_db=snr, lead=500)
        assert len(fr) == 1 and n < 620_000
        xs.append(x); sent.append(fr[0][1])
    return xs, sent


def run_level(fx, xs, **kw):
    ctx = fx.RxContext(len(xs), want_framesyms=True, soft_decision=True, soft_block=True, **kw)
    got = sorted(ctx.process(xs), key=lambda f: (f["stream"], f["start"]))
    ctx.close()
    return got


def stage_reference(f0, f1, soft_bits):
    """one full-length frame's soft_bits through the stage next to the channel, by every rule that applies to the pair: {rule: (b0
    bytes or None, fec0's Viterbi input or None)}, and the coverage the references report.  As ref_block_soft.packet_decode,
    ref_block_siso.packet_decode_chain and ref_rs_soft.packet_decode_soft_rs stage by stage, so that the costly stages run once
    and the Viterbi decoder runs on every frame of the module at once (hard decisions as 0 / 255: the same decisions and ties)."""
    k, l0, l1 = R.packet_dims(K.PAYLOAD, K.CHECK, f0, f1)
    v = R.interleave_soft(np.asarray(soft_bits, np.uint8)[:8 * l1], l1, decode=True)
    out, cov = {}, {}

    def behind(d1):                          # fec1's hard output -> fec0
        in0 = R.interleave(np.asarray(d1, np.uint8), decode=True)
        return (None, np.unpackbits(in0).astype(np.int64) * 255) if f0 in R.CONV else (R.fec_decode(f0, in0, k), None)

    if _rs_pair(f0, f1):
        stage0 = f1 == R.FEC_NONE
        vv = R.interleave_soft(v, l0, decode=True) if stage0 else v
        nout = k if stage0 else l0
        nb, dl = R.rs_dims(nout)
        blocks = vv[:8 * nb * (dl + 32)].reshape(nb, 8 * (dl + 32))
        soft_dec, f = RS.rs_decode_soft_blocks(blocks)
        # (the f = 0 candidate, batched: tests/test_rs_soft.py shows that it is ref_decode.rs_decode_block's result)
        hard_dec = RS.rs_decode_erasures_batch(RS.hard_bytes(blocks), np.zeros((nb, 0), np.int64))[0]
        for rule, dec in (("rs", soft_dec), ("hard_rs", hard_dec)):
            d = dec[:, :dl].ravel()[:nout]
            out[rule] = (d, None) if stage0 else behind(d)
        cov = dict(blocks=nb, dirty=K.rs_coverage(f, R.rs_syndromes(RS.hard_bytes(blocks)).any(axis=1))[0],
                   thirds=K.rs_coverage(f, np.ones(nb, bool))[1], f_hist=np.bincount(f // 2, minlength=17).tolist())
    else:
        d1 = B.block_decode_soft(f1, v, l0)[0]
        out["block"] = behind(d1)
        if S.chained(f0, f1):
            out["chain"] = (None, R.interleave_soft(S.block_decode_siso(f1, v, l0)[0], l0, decode=True).astype(np.int64))
        lanes = K.lanes_that_differ(f1, d1, K.hard_decode(f1, v[None], l0)[0])[0]
        cov = dict(codewords=K.SK.ncw(f1, l0), differ=len(lanes), rounds=K.round_coverage(f1, l0, lanes))
    return out, cov


def finish_references(staged):
    """{(stream, rule): (b0, Viterbi input)} -> {(stream, rule): (payload, valid)}; one Viterbi run for all that need it"""
    todo = [key for key, (b0, vin) in staged.items() if b0 is None]
    k = K.PAYLOAD + R.crc_len(K.CHECK)
    dec = {}
    if todo:
        by_code = {}
        for key in todo:
            by_code.setdefault(key[2], []).append(key)
        for f0, keys in by_code.items():
            for key, d in zip(keys, R.viterbi(f0, np.stack([staged[key][1] for key in keys]), k, 255)[0]):
                dec[key] = d
    return {key[:2]: R._finish(np.asarray(dec[key] if b0 is None else b0, np.uint8), K.PAYLOAD, K.CHECK) for key, (b0, vin) in staged.items()}


@pytest.fixture(scope="module")
def full(fx):
    """the six frames at the four levels, and the references of their soft_bits, once"""
    t0 = time.time()
    xs, sent = full_streams(fx, FULL)
    got = {level: run_level(fx, xs, **kw) for level, kw in LEVELS.items()}
    t1 = time.time()
    first = got["soft_block"]
    assert [f["stream"] for f in first] == list(range(len(FULL))) and all(f["header_valid"] for f in first)
    staged, cov = {}, {}
    for f, (m, f0, f1, snr) in zip(first, FULL):
        assert (f["fec0"], f["fec1"], f["check"], len(f["payload"])) == (f0, f1, K.CHECK, K.PAYLOAD)
        out, cov[f["stream"]] = stage_reference(f0, f1, f["soft_bits"])
        for rule, r in out.items():
            staged[(f["stream"], rule, f0)] = r
    want = finish_references(staged)
    print("\nfull-length frames: synthesis and GPU %.1f s, references %.1f s" % (t1 - t0, time.time() - t1))
    for i, (m, f0, f1, snr) in enumerate(FULL):
        print("  stream %d mod %d fec0 %d fec1 %d at %.2f dB: %s; valid %s" % (
            i, m, f0, f1, snr, cov[i], {level: got[level][i]["payload_valid"] for level in LEVELS if len(got[level]) == len(FULL)}))
    return dict(got=got, want=want, cov=cov, sent=sent)


@pytest.mark.parametrize("level", list(LEVELS))
@pytest.mark.parametrize("i", range(len(FULL)), ids=["fec0_%d_fec1_%d" % (f0, f1) for _, f0, f1, _ in FULL])
def test_full_length_frame_follows_the_reference(full, i, level):
    m, f0, f1, snr = FULL[i]
    frames = full["got"][level]
    assert [f["stream"] for f in frames] == list(range(len(FULL)))
    f, first = frames[i], full["got"]["soft_block"][i]
    # the options change the decoders, not what they are given
    assert f["header_valid"] and f["header"] == first["header"] and np.array_equal(f["soft_bits"], first["soft_bits"])
    rule = _rule(f0, f1, level)
    assert (f["payload"], f["payload_valid"]) == full["want"][(i, rule)], (rule, f["payload_valid"], full["want"][(i, rule)][1])
    if rule != "hard_rs":
        assert f["payload_valid"] == 1 and f["payload"] == full["sent"][i]
    elif f0 not in R.CONV:
        assert f["payload_valid"] == 0                              # a block needs f > 0 and nothing behind it repairs the frame


@pytest.mark.parametrize("i", range(len(FULL)), ids=["fec0_%d_fec1_%d" % (f0, f1) for _, f0, f1, _ in FULL])
def test_full_length_frame_made_the_soft_decoder_work(full, i):
    m, f0, f1, snr = FULL[i]
    cov = full["cov"][i]
    if _rs_pair(f0, f1):
        assert cov["blocks"] == (588 if f1 == R.FEC_RS and f0 == R.FEC_V27 else 294)
        assert cov["dirty"] >= 0.5 and min(cov["thirds"]) >= 1, cov
    else:
        assert cov["codewords"] > 129 and min(cov["rounds"]) >= 1, cov


# ---------------------------------------------------------------------------------------------------- (c) Reed-Solomon frames in bulk
BULK_SNR = 7.5                      # (MI355X: 389 frames, all headers valid, 274 payloads valid, f > 0 wins in 54 %)  QAM16, Reed-Solomon alone, 36 .. 52 coded bytes of which 16 wrong ones are the hard decoder's limit
BULK_LENGTHS = tuple(range(17))
BULK_SAMPLES = 20_000


def bulk_streams(fx, snr, base=9800):
    return [fx.synth_stream(BULK_SAMPLES, stream_id=base + n, mod=R.QAM16, fec0=R.FEC_NONE, fec1=R.FEC_RS, check=K.CHECK, payload_len=n, snr_db=snr, gap=64)[0]
            for n in BULK_LENGTHS]


def bulk_reference(frames):
    """per frame: (payload, valid) by ref_rs_soft, the frames of one length as one batch, and whether a block of it was won by f > 0"""
    out, soft_won, groups = [None] * len(frames), [False] * len(frames), {}
    for j, f in enumerate(frames):
        groups.setdefault((len(f["payload"]), f["check"], f["fec0"], f["fec1"]), []).append(j)
    for (n, check, f0, f1), idx in groups.items():
        if (f0, f1) != (R.FEC_NONE, R.FEC_RS):                       # a header that decoded to other properties
            for j in idx:
                out[j] = RS.packet_decode_soft_rs(frames[j]["soft_bits"], n, check, f0, f1)
            continue
        k, l0, l1 = R.packet_dims(n, check, f0, f1)
        nb, dl = R.rs_dims(l0)
        v = np.stack([R.interleave_soft(np.asarray(frames[j]["soft_bits"], np.uint8)[:8 * l1], l1, decode=True) for j in idx])
        blocks, f = RS.rs_decode_soft_blocks(v[:, :8 * nb * (dl + 32)].reshape(-1, 8 * (dl + 32)))
        dec = blocks[:, :dl].reshape(len(idx), nb * dl)[:, :l0]
        for j, d, fj in zip(idx, dec, f.reshape(len(idx), nb)):
            out[j] = R._finish(R.interleave(d, decode=True), n, check)
            soft_won[j] = bool((fj > 0).any())
    return out, soft_won


def test_rs_frames_in_bulk_follow_the_reference(fx):
    xs = bulk_streams(fx, BULK_SNR)
    pick = lambda fr: [_key(f) for f in sorted(fr, key=lambda f: (f["stream"], f["start"]))]
    ctx = fx.RxContext(len(xs), want_framesyms=True, soft_decision=True, soft_block=True, soft_rs=True)
    first = ctx.process(xs)
    stats = ctx.late_stats()
    n_rs, late0 = stats[8], stats[:6]
    ctx.reset()
    again = ctx.process(xs)                                           # the grid comes from the block before
    stats = ctx.late_stats()
    ctx.close()
    frames = [f for f in first if f["header_valid"]]
    rs_frames = [f for f in frames if (f["fec0"], f["fec1"]) == (R.FEC_NONE, R.FEC_RS)]
    # more Reed-Solomon frames than 4 x 64 in the list of a first block: launched at 64 waves, every wave takes four or more
    assert n_rs >= 256 and len(rs_frames) >= 256, (n_rs, len(rs_frames))
    assert {len(f["payload"]) for f in rs_frames} >= set(BULK_LENGTHS)
    want, soft_won = bulk_reference(frames)
    for f, w in zip(frames, want):
        assert (f["payload"], f["payload_valid"]) == w, (f["stream"], f["start"])
    share = np.mean(soft_won)
    valid = sum(f["payload_valid"] for f in frames)
    print("%d frames with a valid header, Reed-Solomon list %d long; %d valid; a candidate with f > 0 wins in %.0f %%" % (len(frames), n_rs, valid, 100 * share))
    assert 0.25 < share < 0.75 and 0 < valid < len(frames)
    assert pick(again) == pick(first) and stats[8] == n_rs
    assert stats[:6] == late0                                         # nothing was left to collect
    assert all(v == 0 for v in late0[1:])


# ---------------------------------------------------------------------------------------------------- (d) the drop-in
def test_dropin_soft_rs_matches_the_batched_context(fx):
    L = fx.lib()
    cases = [RK.frame_case(R.FEC_NONE), RK.frame_case(R.FEC_V27)]
    crafted = np.concatenate([RK.frame_stream(R.FEC_NONE), RK.frame_stream(R.FEC_V27)])
    pad = lambda x: np.ascontiguousarray(np.concatenate([x, np.zeros(256 - len(x) % 256, np.complex64)]))
    crafted = pad(crafted)
    xx = pad(np.concatenate(_streams(fx, RS_SPEC, 9100) + [crafted]))
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
        assert L.fxrx_sync_set_soft_rs(q, 1) == 0
        L.fxrx_sync_set_threshold(q, 0.0)
        on = feed(xx)
        assert L.fxrx_sync_set_soft_rs(q, 0) == 0
        off = feed(crafted)
    finally:
        L.flexframesync_destroy(q)

    def batched(x, **kw):
        ctx = fx.RxContext(1, want_framesyms=True, soft_decision=True, **kw)
        fr = ctx.process([x])
        ctx.close()
        return [(f["header"], f["header_valid"], f["payload_valid"], f["payload"]) for f in fr]
    want = batched(xx, soft_rs=True)
    assert on == want and len(on) > 60
    assert on != batched(xx)                                          # the option shows in these streams
    assert [(g[1], g[2], g[3]) for g in on[-2:]] == [(1, 1, c["payload"]) for c in cases]
    assert off == batched(crafted) and [(g[1], g[2]) for g in off] == [(1, 0), (1, 0)]


# ---------------------------------------------------------------------------------------------------- (e) options together
# (mod, fec0, fec1, payload_len, snr_db): every code family behind the options, at the SNRs of the options' own low-SNR tests
TOGETHER = [(R.PSK4, R.FEC_V27, R.FEC_GOLAY, 64, 1.0), (R.QAM16, R.FEC_V27, R.FEC_H128, 61, 5.0), (R.QAM16, R.FEC_V27P23, R.FEC_SD72, 37, 8.5),
            (R.PSK4, R.FEC_NONE, R.FEC_H74, 63, 4.0), (R.PSK4, R.FEC_SD39, R.FEC_NONE, 58, 5.0), (R.PSK4, R.FEC_V27P78, R.FEC_NONE, 70, 5.0),
            (R.PSK4, R.FEC_NONE, R.FEC_RS, 64, 3.5), (R.QAM16, R.FEC_V27, R.FEC_RS, 230, 10.5), (R.PSK4, R.FEC_RS, R.FEC_NONE, 64, 4.0),
            (R.PSK4, R.FEC_RS, R.FEC_GOLAY, 64, 3.0)]
ALL_ON = dict(equalizer=True, soft_decision=True, soft_header=True, soft_block=True, soft_chain=True, soft_rs=True)


@pytest.fixture(scope="module")
def together_streams(fx):
    return [fx.synth_stream(60_000, stream_id=9900 + i, mod=m, fec0=f0, fec1=f1, payload_len=n, snr_db=snr)[0] for i, (m, f0, f1, n, snr) in enumerate(TOGETHER)]


@pytest.mark.parametrize("fmt,where", [(ri.IQ_SC16, "pinned_kernel"), (ri.IQ_SC8, "device")], ids=["sc16", "sc8"])
def test_every_option_on_over_integer_iq(fx, together_streams, fmt, where):
    qs = [quantised(x, fmt)[0] for x in together_streams]
    ref_ctx = fx.RxContext(len(qs), want_framesyms=True, **ALL_ON)
    ctx = make_ctx(fx, where, len(qs), want_framesyms=True, **ALL_ON)
    ref = run_float(fx, ref_ctx, qs)
    got = run_int(fx, ctx, qs, fmt, where)
    ctx.close(); ref_ctx.close()
    same(got, ref, "every option on")
    frames = [f for f in got if f["header_valid"]]
    valid = 0
    for f in frames:
        n, f0, f1 = len(f["payload"]), f["fec0"], f["fec1"]
        want = RS.packet_decode_soft_rs(f["soft_bits"], n, f["check"], f0, f1) if _rs_pair(f0, f1) else S.packet_decode_chain(f["soft_bits"], n, f["check"], f0, f1)
        assert (f["payload"], f["payload_valid"]) == want, (f["stream"], f["start"])
        valid += f["payload_valid"]
    print("%d frames with a valid header, %d valid" % (len(frames), valid))
    assert {(f["fec0"], f["fec1"]) for f in frames if f["payload_valid"]} >= {(f0, f1) for _, f0, f1, _, _ in TOGETHER}
    assert len(frames) > 100 and 0 < valid < len(frames)
