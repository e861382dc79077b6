"""Soft-decision frame header decoding (fxrx_config.soft_header) on the GPU (`-m gpu`).

The oracle has no soft header decoder; the checker is the plain numpy reference of tests/ref_header_soft.py.
  (a) fxrx_debug_header_decode -- the walker's own __device__ header decoder on crafted input -- against the reference, bit for
      bit, bytes and CRC verdict, on > 100 000 headers; the hard decoder likewise.
  (b) At 20 dB the soft-header walkers return exactly the frames of the default ones (several codes, three streams, depth 3 with
      continuing blocks, the equaliser on).
  (c) At 1-3 dB the results do not depend on segmentation or on how the input is cut into blocks, every accepted header is
      the transmitted one, and the soft header accepts clearly more headers than the hard one.
  (d) The drop-in, fed in 256-sample calls after flexframesync_decode_header_soft(q, 1), delivers the batched soft-header
      context's frames; a setter whose context cannot be re-created returns -1 and leaves the setting as it was."""
import ctypes as C
import os

import numpy as np
import pytest

import ref_decode as R
import ref_header_soft as H

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------- (a) the decoder itself
def _gpu_decode(L, soft, data):
    data = np.ascontiguousarray(data, np.uint8)
    n = len(data)
    out = np.zeros((n, 20), np.uint8)
    valid = (C.c_int * n)()
    assert L.fxrx_debug_header_decode(1 if soft else 0, data.ctypes.data, n, out.ctypes.data, valid) == 0, L.fxrx_last_error()
    return out, np.frombuffer(valid, np.int32).astype(np.int64)


def _noisy_soft(rng, enc, spread, flip=0.0):
    """0 / 255 per coded bit of enc (N, 54), moved towards the middle by up to `spread`, a fraction `flip` of them mirrored"""
    bits = np.unpackbits(enc, axis=1).astype(np.int64)
    s = np.where(bits == 1, 255 - rng.randint(0, spread + 1, bits.shape), rng.randint(0, spread + 1, bits.shape))
    m = rng.rand(*bits.shape) < flip
    s[m] = 255 - s[m]
    return s.astype(np.uint8)


def _crafted(rng):
    cases = {}
    hdr = rng.randint(0, 256, (28000, 20)).astype(np.uint8)
    tr, cw0 = {}, []
    enc = np.empty((len(hdr), 54), np.uint8)
    for i, h in enumerate(hdr):
        enc[i] = H.header_encode(h, tr)
        cw0.append(tr["cw0"])
    cw0 = np.array(cw0)
    cases["clean"] = (hdr[:4000], H.hard_as_soft(enc[:4000]))
    cases["clean_noisy"] = (hdr[4000:16000], _noisy_soft(rng, enc[4000:16000], 120))
    # 1-3 bit errors in every SECDED(72,64) block of the coded header, then the channel code on top
    e = cw0[16000:28000].copy()
    for i in range(len(e)):
        for blk in range(3):
            for b in rng.choice(72, rng.randint(1, 4), replace=False):
                e[i, 9 * blk + b // 8] ^= 0x80 >> (b % 8)
    enc_e = np.stack([H.header_encode_from_cw0(c) for c in e])
    cases["secded_errors"] = (hdr[16000:28000], _noisy_soft(rng, enc_e, 60))
    # channel noise: soft values spread over the whole range, some bits mirrored
    hn = rng.randint(0, 256, (44000, 20)).astype(np.uint8)
    en = np.stack([H.header_encode(h) for h in hn])
    cases["noisy"] = (hn[:30000], _noisy_soft(rng, en[:30000], 150, flip=0.01))
    # erasures: most values within a few steps of 127, the sign still mostly right
    bits = np.unpackbits(en[30000:], axis=1).astype(np.int64)
    s = 127 + np.where(bits == 1, 1, -1) * rng.randint(0, 6, bits.shape) + rng.randint(-3, 4, bits.shape)
    keep = rng.rand(*bits.shape) < 0.5
    s[keep] = np.where(bits == 1, 255, 0)[keep]
    cases["erasures"] = (hn[30000:], np.clip(s, 0, 255).astype(np.uint8))
    # exact ties in one Hamming word in ten: the true codeword a and a random one b at distance 4 cost the same
    tab = R.code_table(R.FEC_H84)[2]
    ht = rng.randint(0, 256, (8000, 20)).astype(np.uint8)
    et = np.stack([H.header_encode(h) for h in ht])
    # work on the de-interleaved words (what the Hamming stage sees) and put them back in channel order
    p54 = R._ilv_perm(54, True)
    inv = np.argsort(p54)
    words = H.hard_as_soft(et)[:, p54].astype(np.int64).reshape(-1, 8)
    dist4 = [[b for b in range(16) if bin(int(tab[a]) ^ int(tab[b])).count("1") == 4] for a in range(16)]
    for i in np.nonzero(rng.rand(len(words)) < 0.1)[0]:
        w = words[i]                                                 # (a view: the row is changed in place)
        ca = 0
        for k in range(8):
            ca = (ca << 1) | (1 if w[k] > 127 else 0)
        a = int(np.nonzero(tab == ca)[0][0])
        cb = int(tab[rng.choice(dist4[a])])
        diff = [k for k in range(8) if ((ca ^ cb) >> (7 - k)) & 1]
        c1, c3 = rng.randint(0, 256, 2)
        for k, c in zip(diff, (c1, 255 - c1, c3, 255 - c3)):
            w[k] = 255 - c if (ca >> (7 - k)) & 1 else c
    cases["ties"] = (ht, words.reshape(-1, 432)[:, inv].astype(np.uint8))
    # received words as hard decisions (0 / 255): codewords with bit errors and random words
    hh = rng.randint(0, 256, (20000, 20)).astype(np.uint8)
    eh = np.stack([H.header_encode(h) for h in hh])
    fl = rng.rand(*eh.shape[:1], 432) < rng.choice([0.0, 0.01, 0.03, 0.08], (len(eh), 1))
    eh = np.packbits(np.unpackbits(eh, axis=1) ^ fl.astype(np.uint8), axis=1)
    eh[16000:] = rng.randint(0, 256, (4000, 54))
    cases["hard_as_soft"] = (hh, H.hard_as_soft(eh))
    return cases


def test_debug_header_decode_matches_the_reference(fx):
    L = fx.lib()
    rng = np.random.RandomState(20261016)
    cases = _crafted(rng)
    total, tallies = 0, {}
    for name, (hdr, soft) in cases.items():
        got, ok = _gpu_decode(L, True, soft)
        want, wok = H.decode_soft(soft)
        bad = np.nonzero((got != want).any(axis=1) | (ok != wok))[0]
        assert len(bad) == 0, "%s: %d of %d headers differ, first #%d gpu %s/%d ref %s/%d" % (
            name, len(bad), len(soft), bad[0], got[bad[0]].tobytes().hex(), ok[bad[0]], want[bad[0]].tobytes().hex(), wok[bad[0]])
        # hard mode on the same channel's hard decisions
        enc = np.packbits((soft > 127).astype(np.uint8), axis=1)
        hgot, hok = _gpu_decode(L, False, enc)
        hwant, hwok = H.decode_hard(enc)
        assert (hgot == hwant).all() and (hok == hwok).all(), name
        if name == "hard_as_soft":                                   # soft decoding of 0 / 255 is hard decoding
            assert (got == hgot).all() and (ok == hok).all()
        tallies[name] = (len(soft), int(ok.sum()), int((ok.astype(bool) & (got == hdr).all(axis=1)).sum()), int(hok.sum()))
        total += len(soft)
    assert total >= 100_000
    # the traffic is not kind: every case has failures somewhere between clean and hopeless, and the soft decoder does better
    n, v, right, hv = tallies["clean"]
    assert v == right == n
    for name in ("secded_errors", "noisy", "erasures", "hard_as_soft"):
        n, v, right, hv = tallies[name]
        assert 0 < v < n, (name, tallies[name])
    n, v, right, hv = tallies["erasures"]
    assert v > hv, tallies["erasures"]


# ---------------------------------------------------------------------------------------------------- traffic with user headers
def _traffic(fx, n_frames, snr_db, seed, mod=2, fec0=11, fec1=1, check=5, payload_len=64, cfo=0.01, gap=256, lead=1000):
    """frames with random 14-byte user headers and payloads, back to back; CFO, random phase, AWGN with sigma^2 =
    10^(-snr/10) per complex sample as in synth_stream.  Returns (x, [(start, header14, payload)])"""
    rng = np.random.RandomState(seed)
    g = fx.FrameGen(mod, fec0, fec1, check)
    parts, sent, p = [np.zeros(lead, np.complex64)], [], lead
    for _ in range(n_frames):
        hd = rng.randint(0, 256, 14).astype(np.uint8)
        pl = rng.randint(0, 256, payload_len).astype(np.uint8)
        fr = g.frame(pl, header=hd, dt=rng.uniform(-0.5, 0.5))
        parts += [fr, np.zeros(gap, np.complex64)]
        sent.append((p, hd.tobytes(), pl.tobytes()))
        p += len(fr) + gap
    g.close()
    x = np.concatenate(parts + [np.zeros(4000, np.complex64)])
    n = np.arange(len(x), dtype=np.float64)
    x = (x * np.exp(1j * (cfo * n + rng.uniform(-np.pi, np.pi)))).astype(np.complex64)
    sigma = np.sqrt(0.5 * 10.0 ** (-snr_db / 10.0))
    x += (np.float32(sigma) * rng.standard_normal(2 * len(x)).astype(np.float32)).view(np.complex64)
    return x, sent


def _key(f):
    return tuple((k, f[k].tobytes() if isinstance(f[k], np.ndarray) else f[k]) for k in sorted(f) if k != "soft_bits")


def _run(fx, xs, depth=1, cuts=1, **kw):
    ctx = fx.RxContext(len(xs), **kw)
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


STREAMS = [(2, 11, 1, 5, 64), (27, 15, 1, 5, 120), (3, 16, 1, 6, 90)]     # (mod, fec0, fec1, check, payload_len)


@pytest.mark.parametrize("equalizer", [False, True])
def test_soft_header_at_20db_changes_nothing(fx, equalizer):
    xs, sent = [], []
    for i, (m, f0, f1, ck, n) in enumerate(STREAMS):
        x, s = _traffic(fx, 40, 20.0, 100 + i, mod=m, fec0=f0, fec1=f1, check=ck, payload_len=n)
        xs.append(x); sent.append(s)
    for depth, cuts in ((1, 1), (3, 5)):
        kw = dict(want_framesyms=True, equalizer=equalizer, segment_len=8192)
        hard = _run(fx, xs, depth, cuts, **kw)
        soft = _run(fx, xs, depth, cuts, soft_header=True, **kw)
        assert len(hard) == len(soft) == sum(len(s) for s in sent)
        assert all(f["header_valid"] and f["payload_valid"] for f in soft)
        assert [_key(f) for f in hard] == [_key(f) for f in soft]


# measured on an MI355X (PSK4, V27, CRC-24, 64-byte payloads, 80 frames per SNR, CFO 0.01, seeds 7000 + SNR): headers accepted,
# hard / soft -- 1 dB: 7 / 59, 2 dB: 26 / 72, 3 dB: 51 / 79; in all 84 / 210 (2.5 times).  Floor: 1.8 times + 5.
LOW_SNR = (1.0, 2.0, 3.0)
SOFT_GAIN_FLOOR = 1.8


def _accepted(frames, sent):
    starts = np.array([s[0] for s in sent])
    ok = []
    for f in frames:
        if not f["header_valid"]:
            continue
        j = int(np.argmin(np.abs(starts - f["start"])))
        assert abs(int(starts[j]) - f["start"]) < 64, f["start"]
        assert f["header"][:14] == sent[j][1], "accepted header differs from the transmitted one at %d" % f["start"]
        assert (f["mod_scheme"], f["fec0"], f["fec1"], f["check"]) == (2, 11, 1, 5)
        ok.append(j)
    assert len(ok) == len(set(ok))
    return len(ok)


@pytest.fixture(scope="module")
def low_snr_traffic(fx):
    return {snr: _traffic(fx, 80, snr, 7000 + int(snr)) for snr in LOW_SNR}


def test_soft_header_low_snr_segmentation_and_gain(fx, low_snr_traffic):
    counts = {}
    for snr, (x, sent) in low_snr_traffic.items():
        ref = _run(fx, [x], soft_header=True)
        for seg, depth, cuts in ((4096, 1, 1), (1 << 24, 1, 1), (0, 3, 7), (4096, 2, 3)):
            got = _run(fx, [x], depth, cuts, soft_header=True, segment_len=seg)
            assert [_key(f) for f in got] == [_key(f) for f in ref], (snr, seg, depth, cuts)
        hard = _run(fx, [x])
        counts[snr] = (_accepted(hard, sent), _accepted(ref, sent))
    print("accepted headers hard / soft:", counts)
    for snr, (h, s) in counts.items():
        assert s >= h, (snr, counts)
    h, s = sum(c[0] for c in counts.values()), sum(c[1] for c in counts.values())
    assert s >= SOFT_GAIN_FLOOR * h + 5, counts


def test_soft_header_repair_walks_of_the_chain_kernel(fx, low_snr_traffic, monkeypatch):
    """FXRX_CHAIN_SLOW=1 sends the block through the general path of the full-size chain kernel, whose repair walks must decode
    headers softly like the segments' walkers did (fx_launch_chain's `sh`): same frames as the one-segment run, and it did walk.
    Measured on an MI355X at segment_len=4096: 40 walk jobs, repairs 18, 80 frames (2048 and 1024 give the same counts)."""
    x, _ = low_snr_traffic[2.0]
    ref = _run(fx, [x], soft_header=True)
    monkeypatch.setenv("FXRX_CHAIN_SLOW", "1")
    ctx = fx.RxContext(1, soft_header=True, segment_len=4096)
    got = sorted(ctx.process([x]), key=lambda f: (f["stream"], f["start"]))
    tm = ctx.timing()
    ctx.close()
    print("repairs", tm["repairs"], "walk jobs", tm["walk_jobs"], "frames", len(got))
    assert [_key(f) for f in got] == [_key(f) for f in ref]
    assert tm["repairs"] > 0, "no repair walk ran: the chain kernel's soft-header walker was not exercised"


# ---------------------------------------------------------------------------------------------------- (d) the drop-in
def test_dropin_soft_header_matches_the_batched_context(fx, low_snr_traffic, monkeypatch):
    L = fx.lib()
    x, sent = low_snr_traffic[2.0]
    got = []
    cbf = fx._ffi.FRAMESYNC_CALLBACK(lambda hd, hv, pl, n, pv, st, ud: got.append(
        (C.string_at(hd, 20), hv, pv, C.string_at(pl, n) if (pl and n) else b"")) or 0)
    q = L.flexframesync_create(cbf, None)
    assert q
    try:
        assert L.flexframesync_decode_header_soft(q, 1) == 0
        # a re-creation that fails (no such device): -1, counted, and the soft header stays on
        monkeypatch.setenv("FXRX_DEVICE", "4096")
        assert L.flexframesync_decode_header_soft(q, 0) == -1
        assert L.flexframesync_decode_payload_soft(q, 1) == -1
        assert L.fxrx_sync_errors(q) == 2
        monkeypatch.delenv("FXRX_DEVICE")
        L.fxrx_sync_set_threshold(q, 0.0)                           # re-created from the handle's settings
        assert L.fxrx_sync_errors(q) == 2
        xx = np.ascontiguousarray(np.concatenate([x, np.zeros(256 - len(x) % 256, np.complex64)]))
        for i in range(0, len(xx), 256):
            L.flexframesync_execute(q, xx[i:i + 256].ctypes.data, 256)
        L.fxrx_sync_flush(q)
        while L.fxrx_sync_pending(q):
            L.flexframesync_execute(q, None, 0)
    finally:
        L.flexframesync_destroy(q)
    want = [(f["header"], f["header_valid"], f["payload_valid"], f["payload"]) for f in _run(fx, [xx], soft_header=True)]
    hard = [(f["header"], f["header_valid"], f["payload_valid"], f["payload"]) for f in _run(fx, [xx])]
    assert got == want
    assert sum(g[1] for g in got) > sum(h[1] for h in hard)      # the soft header was in force, not the hard one
