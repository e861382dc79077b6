"""Soft-input block decoding (fxrx_config.soft_block) on the GPU (`-m gpu`).

The oracle has no such decoder; the checker is the numpy reference of tests/ref_block_soft.py.
  (a) fxrx_debug_block_decode -- the decode kernel's own __device__ block decoders, soft and hard, on crafted packets -- against the
      reference bit for bit, >= 100 000 codewords per code: 0 / 255 words with errors, near-codeword noise, all-127 / 128 ties,
      uniform noise, lengths that leave partial groups and short last blocks.
  (b) At 20 dB the frames are identical with the option on and off: every inner x outer pair of the reference's menu, block-code
      fec0 under fec1 NONE, Reed-Solomon fec0 under Golay.
  (c) At 1-5 dB, with want_framesyms, every frame's payload and payload_valid equal the reference chain run on its soft_bits, and
      the results do not depend on segmentation.
  (d) Valid payloads rise with the option on (Hamming(7,4), Hamming(12,8), Golay, SECDED(72,64)).
  (e) The drop-in, fed in 256-sample calls after fxrx_sync_set_soft_block(q, 1), delivers the batched context's frames."""
import ctypes as C

import numpy as np
import pytest

import ref_decode as R
import ref_block_soft as B

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------- (a) the decoders themselves
def _gpu(L, fs, soft, n, data):
    data = np.ascontiguousarray(data, np.uint8)
    out = np.zeros((len(data), n), np.uint8)
    assert L.fxrx_debug_block_decode(fs, 1 if soft else 0, n, len(data), data.ctypes.data, out.ctypes.data) == 0, L.fxrx_last_error()
    return out


def _ncw(fs, n):
    if fs == R.FEC_H84:
        return 2 * n
    if fs in R.SECDED:
        return -(-n // R.SECDED[fs][0])
    return R._packed_dims(fs, n)[2]


def _crafted(rng, fs, n, count):
    """count packets of n bytes: soft values (count, 8 el) of five kinds, cycled"""
    msg = rng.randint(0, 256, (count, n)).astype(np.uint8)
    bits = np.unpackbits(np.stack([R.fec_encode(fs, m) for m in msg]), axis=1).astype(np.int64)
    kind = np.arange(count) % 5
    s = np.empty(bits.shape, np.int64)
    flip = (rng.rand(*bits.shape) < rng.choice([0.0, 0.02, 0.06, 0.12], (count, 1))).astype(np.int64)
    hard = (bits ^ flip) * 255                                                   # 0: 0 / 255 with bit errors
    near = np.where(bits == 1, 255 - rng.randint(0, 200, bits.shape), rng.randint(0, 200, bits.shape))
    near = np.where(rng.rand(*bits.shape) < 0.04, 255 - near, near)              # 1: near-codeword noise
    ties = rng.randint(127, 129, bits.shape)                                     # 2: all 127 / 128
    unif = rng.randint(0, 256, bits.shape)                                       # 3: uniform noise
    mild = np.clip(bits * 255 + rng.randint(-140, 141, bits.shape), 0, 255)     # 4: noise around the codeword
    for k, v in enumerate((hard, near, ties, unif, mild)):
        s[kind == k] = v[kind == k]
    return msg, s.astype(np.uint8)


@pytest.mark.parametrize("fs", B.SOFT_BLOCK)
def test_debug_block_decode_matches_the_reference(fx, fs):
    L = fx.lib()
    rng = np.random.RandomState(900 + fs)
    lengths = (1, 2, 3, 4, 5, 7, 11, 64, 100, 301)
    total, differ = 0, 0
    for n in lengths:
        count = max(10, 14000 // _ncw(fs, n))
        msg, soft = _crafted(rng, fs, n, count)
        got = _gpu(L, fs, True, n, soft)
        want = B.block_decode_soft(fs, soft, n)
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert len(bad) == 0, "n=%d: %d of %d packets differ, first #%d (kind %d)" % (n, len(bad), count, bad[0], bad[0] % 5)
        enc = np.packbits((soft > 127).astype(np.uint8), axis=1)
        hgot = _gpu(L, fs, False, n, enc)
        assert (hgot == B.block_decode_hard(fs, enc, n)).all(), n
        total += count * _ncw(fs, n)
        differ += int((got != hgot).any(axis=1).sum())
    assert total >= 100_000
    assert differ > 100                      # the soft decoder did decide differently from the hard one, often


# ---------------------------------------------------------------------------------------------------- traffic
INNER = (R.FEC_NONE, R.FEC_V27, R.FEC_V27P23, R.FEC_V27P45, R.FEC_V27P56, R.FEC_V27P67, R.FEC_V27P78)
OUTER = (R.FEC_NONE, R.FEC_GOLAY, R.FEC_RS, R.FEC_H74, R.FEC_H128, R.FEC_SD22, R.FEC_SD39, R.FEC_SD72)


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


def test_soft_block_at_20db_changes_nothing(fx):
    cases = [(R.PSK4 if i % 2 else R.QAM16, f0, f1) for i, (f0, f1) in enumerate((a, b) for a in INNER for b in OUTER)]
    cases += [(R.PSK8, f0, R.FEC_NONE) for f0 in R.BLOCK] + [(R.QAM16, R.FEC_RS, R.FEC_GOLAY)]
    xs, inj = [], []
    for i, (m, f0, f1) in enumerate(cases):
        x, fr = fx.synth_stream(60_000, stream_id=5100 + i, mod=m, fec0=f0, fec1=f1, payload_len=60 + i % 37, snr_db=20.0)
        xs.append(x); inj.append(fr)
    off, on = _run(fx, xs, segment_len=16384), _run(fx, xs, segment_len=16384, soft_block=True)
    assert len(on) == sum(len(f) for f in inj) and all(f["payload_valid"] for f in on)
    assert [_key(f) for f in off] == [_key(f) for f in on]
    assert {(f["fec0"], f["fec1"]) for f in on} == {(f0, f1) for _, f0, f1 in cases}


# (mod, fec0, fec1, payload_len, snr_db): each block decoder working at its limit
LOW = [(R.PSK4, R.FEC_NONE, R.FEC_H74, 61, 4.0), (R.PSK4, R.FEC_NONE, R.FEC_H128, 62, 4.0), (R.PSK4, R.FEC_NONE, R.FEC_GOLAY, 63, 3.0),
       (R.PSK4, R.FEC_NONE, R.FEC_SD72, 65, 5.0), (R.PSK4, R.FEC_V27, R.FEC_GOLAY, 64, 1.0), (R.PSK4, R.FEC_V27, R.FEC_SD22, 60, 2.0),
       (R.PSK4, R.FEC_RS, R.FEC_GOLAY, 70, 3.0), (R.PSK4, R.FEC_H84, R.FEC_NONE, 59, 4.0), (R.PSK4, R.FEC_SD39, R.FEC_NONE, 58, 5.0),
       (R.QAM16, R.FEC_NONE, R.FEC_H128, 57, 5.0)]


@pytest.fixture(scope="module")
def low_traffic(fx):
    xs = []
    for i, (m, f0, f1, n, snr) in enumerate(LOW):
        x, _ = fx.synth_stream(240_000, stream_id=6100 + i, mod=m, fec0=f0, fec1=f1, payload_len=n, snr_db=snr)
        xs.append(x)
    return xs


def test_low_snr_frames_follow_the_reference_and_segmentation(fx, low_traffic):
    ref = _run(fx, low_traffic, soft_block=True, soft_header=True)
    checked, valid = 0, 0
    for f in ref:
        if not f["header_valid"]:
            continue
        m, f0, f1, n, _ = LOW[f["stream"]]
        assert (f["fec0"], f["fec1"], len(f["payload"])) == (f0, f1, n)
        assert (f["payload"], f["payload_valid"]) == B.packet_decode(f["soft_bits"], n, f["check"], f0, f1), f["stream"]
        checked += 1
        valid += f["payload_valid"]
    assert checked > 100 and 0 < valid < checked, (checked, valid)
    for seg, depth, cuts in ((4096, 1, 1), (0, 3, 5)):
        got = _run(fx, low_traffic, depth, cuts, soft_block=True, soft_header=True, segment_len=seg)
        assert [_key(f) for f in got] == [_key(f) for f in ref], (seg, depth, cuts)


# valid payloads with the option off -> on, PSK4, no inner code.  Measured on an MI355X (400 000 samples a stream, soft header on):
# Hamming(7,4) at 5 dB 190 -> 216, Hamming(12,8) at 5 dB 200 -> 235, SECDED(72,64) at 6 dB 232 -> 268; Golay at 2 dB: about 37 -> 68 of
# 82 in profiles/soft_block_sensitivity.txt.  Floor: 3 more, and 5 % more, valid payloads with the option on
GAIN = [(R.FEC_H74, 5.0), (R.FEC_H128, 5.0), (R.FEC_GOLAY, 2.0), (R.FEC_SD72, 6.0)]


def test_soft_block_gains(fx):
    xs = []
    for i, (f1, snr) in enumerate(GAIN):
        x, _ = fx.synth_stream(400_000, stream_id=6600 + i, mod=R.PSK4, fec0=R.FEC_NONE, fec1=f1, payload_len=64, snr_db=snr)
        xs.append(x)
    counts = {}
    for sb in (False, True):
        for f in _run(fx, xs, soft_block=sb, soft_header=True):
            counts.setdefault((GAIN[f["stream"]][0], sb), 0)
            counts[(GAIN[f["stream"]][0], sb)] += f["payload_valid"]
    print("valid payloads off / on:", counts)
    for f1, _ in GAIN:
        off, on = counts.get((f1, False), 0), counts.get((f1, True), 0)
        assert on >= off + max(3, off // 20), (f1, counts)


# ---------------------------------------------------------------------------------------------------- (e) the drop-in
def test_dropin_soft_block_matches_the_batched_context(fx, low_traffic, monkeypatch):
    L = fx.lib()
    x = low_traffic[2]
    got = []
    cbf = fx._ffi.FRAMESYNC_CALLBACK(lambda hd, hv, pl, n, pv, st, ud: got.append(
        (C.string_at(hd, 20), hv, pv, C.string_at(pl, n) if (pl and n) else b"")) or 0)
    q = L.flexframesync_create(cbf, None)
    assert q
    try:
        assert L.flexframesync_decode_payload_soft(q, 1) == 0
        assert L.fxrx_sync_set_soft_block(q, 1) == 0
        monkeypatch.setenv("FXRX_DEVICE", "4096")                    # a re-creation that fails: -1 and the setting stays on
        assert L.fxrx_sync_set_soft_block(q, 0) == -1
        monkeypatch.delenv("FXRX_DEVICE")
        L.fxrx_sync_set_threshold(q, 0.0)
        xx = np.ascontiguousarray(np.concatenate([x, np.zeros(256 - len(x) % 256, np.complex64)]))
        for i in range(0, len(xx), 256):
            L.flexframesync_execute(q, xx[i:i + 256].ctypes.data, 256)
        L.fxrx_sync_flush(q)
        while L.fxrx_sync_pending(q):
            L.flexframesync_execute(q, None, 0)
    finally:
        L.flexframesync_destroy(q)
    pick = lambda fr: [(f["header"], f["header_valid"], f["payload_valid"], f["payload"]) for f in fr]
    want = pick(_run(fx, [xx], soft_block=True))
    assert got == want and len(got) > 10
    assert sum(g[2] for g in got) >= sum(f[2] for f in pick(_run(fx, [xx])))
