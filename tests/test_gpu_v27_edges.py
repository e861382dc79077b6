"""The edges of the two Viterbi decoders' chunked traceback and of the wave-per-frame decoder's chunked forward pass, against
the plain numpy reference of tests/ref_decode.py, compared exactly as tests/test_gpu_ref_decode.py compares them.

Frames: PSK4, CRC-24, one stream per K = 7 rate (1/2 .. 7/8), message lengths k = payload + 3 with Tn = 8 k + 6 trellis steps at
  * k = 9 .. 16: every residue of Tn mod 64 (and, k = 9 .. 14, of Tn mod 6);
  * k = 511, 512: 63.9 and 64.03 chunks of 64 steps, either side of one chunk per lane;
  * k = 2047, 2048: either side of 256 chunks, one pass of four chains by 64 lanes of the wave-per-frame traceback.
Decoders: the wave-per-frame one (FXRX_BATCH_VITERBI=0; hard and soft decisions) and the batch path with every end-state guess
forced to state 0 (FXRX_VB_DEBUG=1) at FXRX_VB_BLK=128, where the whole-wave retrace enters blocks from true states other than 0.

Channel: one SNR per rate; the noise of every frame has its own seed (SEEDS), chosen on the CPU -- `python tests/test_gpu_v27_edges.py`
prints the table -- from the oracle's symbols, which equal the GPU's, so that in every frame the hard decisions carry at least one
coded-bit error, the reference's Viterbi corrects them all, and no symbol lies within TIE of a decision boundary: no frame is
excluded.  No counter counts retraces; the test counts, from the decoded messages, the block ends at which the true path is not in
state 0 -- there the forced guess was wrong and fx_vbfinish_kernel had to trace the block again."""
import sys

import numpy as np
import pytest

import ref_decode as R
import test_gpu_ref_decode as D

pytestmark = pytest.mark.gpu

KS = list(range(9, 17)) + [511, 512, 2047, 2048]
SNR_DB = {R.FEC_V27: 3.0, R.FEC_V27P23: 4.5, R.FEC_V27P34: 5.5, R.FEC_V27P45: 6.5, R.FEC_V27P56: 7.0, R.FEC_V27P67: 7.3, R.FEC_V27P78: 7.6}
LEAD, GAP, TAIL = 500, 256, 2000
BLK = 128
# noise seed of frame KS[j] of the stream of rate R.CONV[i]
SEEDS = [
    [1000001, 1001000, 1002005, 1003000, 1004000, 1005000, 1006001, 1007003, 1008002, 1009000, 1010000, 1011001],
    [2000000, 2001000, 2002000, 2003000, 2004000, 2005000, 2006000, 2007000, 2008000, 2009000, 2010002, 2011004],
    [3000001, 3001000, 3002005, 3003002, 3004002, 3005000, 3006003, 3007001, 3008000, 3009000, 3010000, 3011000],
    [4000004, 4001004, 4002002, 4003002, 4004002, 4005002, 4006002, 4007000, 4008000, 4009000, 4010000, 4011000],
    [5000003, 5001006, 5002014, 5003003, 5004004, 5005003, 5006011, 5007022, 5008000, 5009000, 5010000, 5011000],
    [6000062, 6001010, 6002003, 6003001, 6004000, 6005008, 6006004, 6007034, 6008000, 6009000, 6010000, 6011000],
    [7000027, 7001012, 7002001, 7003051, 7004017, 7005009, 7006011, 7007011, 7008000, 7009000, 7010000, 7011000],
]


def build_stream(fx, ri, seeds):
    """the stream of rate R.CONV[ri]: (iq, [(start, payload bytes)]); frame j and the gap behind it carry the noise of seeds[j]"""
    fs = R.CONV[ri]
    prng, crng = np.random.RandomState(0x5EED + 7000 + ri), np.random.RandomState(0xC0FFEE + 7000 + ri)
    cfo, phase, delay = crng.uniform(-0.05, 0.05), crng.uniform(-np.pi, np.pi), crng.uniform(-0.5, 0.5)
    g = fx.FrameGen(R.PSK4, fs, R.FEC_NONE, R.CRC_24)
    sig, noise, frames = [np.zeros(LEAD, np.complex64)], [crng.standard_normal(2 * LEAD)], []
    p = LEAD
    for k, seed in zip(KS, seeds):
        pl = prng.randint(0, 256, k - 3).astype(np.uint8)
        fr = g.frame(pl, dt=delay)
        frames.append((p, pl.tobytes()))
        sig += [fr, np.zeros(GAP, np.complex64)]
        noise.append(np.random.RandomState(seed).standard_normal(2 * (len(fr) + GAP)))
        p += len(fr) + GAP
    g.close()
    sig.append(np.zeros(TAIL, np.complex64))
    noise.append(crng.standard_normal(2 * TAIL))
    x = np.concatenate(sig)
    x *= np.exp(1j * (cfo * np.arange(len(x), dtype=np.float64) + phase)).astype(np.complex64)
    sigma = np.sqrt(0.5 * 10.0 ** (-SNR_DB[fs] / 10.0))
    x += np.float32(sigma) * np.concatenate(noise).astype(np.float32).view(np.complex64)
    return x, frames


def message_bytes(payload, check=R.CRC_24):
    """what fec0 encodes: payload + CRC, scrambled"""
    msg = np.frombuffer(payload, np.uint8)
    cl, key = R.crc_len(check), R.crc_key(check, msg)
    return R.scramble(np.concatenate([msg, np.array([(key >> (8 * (cl - 1 - i))) & 0xff for i in range(cl)], np.uint8)]))


def corrected_errors(ref, payload):
    """coded-bit errors of the hard decisions that the reference's Viterbi corrected: 0 unless it decoded the true payload"""
    tr = {}
    R.packet_encode(np.frombuffer(payload, np.uint8), ref.check, ref.fec0, ref.fec1, tr)
    wrong = int(R.bits_of(ref.trace["in0"] ^ tr["cw0"]).sum())
    return wrong if ref.valid and ref.payload == payload else 0


def forced_retraces(payload, blk=BLK):
    """block ends of the frame's trellis (steps b blk < Tn) at which the encoder is not in state 0: its last six message bits"""
    bits = R.bits_of(message_bytes(payload))
    tn = len(bits) + 6
    return sum(1 for t in range(blk, tn, blk) if bits[t - 6:t].any())


def _frame_of(frames_by_start, p):
    return next((g for s, g in frames_by_start if abs(s - p) < 400), None)


@pytest.fixture(scope="module")
def streams(fx):
    assert SEEDS is not None and len(SEEDS) == len(R.CONV) and all(len(s) == len(KS) for s in SEEDS)
    built = [build_stream(fx, ri, SEEDS[ri]) for ri in range(len(R.CONV))]
    return [b[0] for b in built], [b[1] for b in built]


def _frames(got, inj):
    """every injected frame's record, in order, as (record, payload); all of them must be there with a valid header"""
    out = []
    for s, fr in enumerate(inj):
        mine = [(g["start"], g) for g in got if g["stream"] == s and g["header_valid"]]
        for (p, pl), k in zip(fr, KS):
            g = _frame_of(mine, p)
            assert g is not None and len(g["payload"]) == k - 3 and g["fec0"] == R.CONV[s], (s, k, p)
            out.append((g, pl))
    assert len(out) == sum(bool(g["header_valid"]) for g in got) == len(R.CONV) * len(KS)
    return out


@pytest.fixture(scope="module")
def reference(fx, streams):
    """the wave-per-frame hard-decision run, and the reference's view of each of its frames"""
    mp = pytest.MonkeyPatch()
    got, tm = D._run(fx, mp, streams[0], dict(FXRX_BATCH_VITERBI=0))
    mp.undo()
    return got, tm, {(g["stream"], g["start"]): D.Ref(g) for g in got}


def test_wave_per_frame_hard(streams, reference):
    got, tm, refs = reference
    pairs = _frames(got, streams[1])
    fixed = [corrected_errors(refs[(g["stream"], g["start"])], pl) for g, pl in pairs]
    print("\ncorrected coded-bit errors per frame:", fixed)
    assert min(fixed) >= 1, "a frame without a corrected error: %s" % fixed
    assert D._compare_hard(got, refs) == (len(pairs), 0)
    assert all(g["payload_valid"] and g["payload"] == pl for g, pl in pairs)
    assert tm["vb_blocks"] == 0


def test_wave_per_frame_soft(fx, monkeypatch, streams, reference):
    got, tm = D._run(fx, monkeypatch, streams[0], dict(FXRX_BATCH_VITERBI=0), soft=True)
    _frames(got, streams[1])
    assert D._compare_soft(got, reference[2])[:2] == (len(got), 0)
    assert tm["vb_blocks"] == 0


def test_batch_path_with_forced_wrong_guesses(fx, monkeypatch, streams, reference):
    got, tm = D._run(fx, monkeypatch, streams[0], dict(FXRX_VB_DEBUG=1, FXRX_VB_BLK=BLK))
    pairs = _frames(got, streams[1])
    assert D._compare_hard(got, reference[2]) == (len(pairs), 0)
    retraces = [forced_retraces(g["payload"]) for g, _ in pairs]
    print("\nblocks traced again per frame:", retraces, "timing", {k: tm[k] for k in ("vb_blocks", "vb_repairs", "vb_fallbacks")})
    assert tm["vb_blocks"] > 0
    assert all(r > 0 for r, (g, _) in zip(retraces, pairs) if len(g["payload"]) + 3 >= 511), retraces


def choose_seeds():
    """CPU only: the oracle's symbols of every frame, seeds bumped until every frame passes the docstring's conditions"""
    import importlib
    import os
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import oracle_ffi as o
    from parity_util import oracle_frames
    fx = importlib.import_module("gr-liquiddsp_amd")
    table = []
    for ri in range(len(R.CONV)):
        seeds = [1000000 * (ri + 1) + 1000 * j for j in range(len(KS))]
        for _ in range(200):
            x, frames = build_stream(fx, ri, seeds)
            of = [(f.info["start"], f) for f in oracle_frames(o, x) if f.header_valid]
            bad = []
            for j, (p, pl) in enumerate(frames):
                f = _frame_of(of, p)
                ok = f is not None and len(f.payload) == len(pl)
                if ok:
                    r = D.Ref(dict(payload=f.payload, check=f.check, fec0=f.fec0, fec1=f.fec1, mod_scheme=f.mod_scheme, framesyms=f.framesyms))
                    margin = R.demap_hard(r.ms, r.syms)[1].min()
                    ok = margin > 10 * D.TIE[R.PSK4] and corrected_errors(r, pl) >= 1
                if not ok:
                    bad.append(j)
            if not bad:
                break
            for j in bad:
                seeds[j] += 1
        assert not bad, (ri, bad)
        print("    %s," % seeds, flush=True)
        table.append(seeds)
    return table


if __name__ == "__main__":
    choose_seeds()
