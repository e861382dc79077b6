"""Soft-output block decoding (fxrx_config.soft_chain) without a GPU: the numpy reference of tests/ref_block_siso.py against an
independent exhaustive search, against ref_block_soft's decisions, the two identities of the rule, and the new entry points and
config checks of libfxrx.so.

Floors stated here: the no-competitor rule (a message bit on which every Chase candidate agrees: L = 255) is hit by >= 100 words
of every Chase code, the no-candidate rule (none of the 16 patterns decodes) by >= 100 words of every SECDED code.  Golay(24,12)
cannot have a word without a candidate: its covering radius is 4 and all its codewords have even weight, so a hard word at
distance 4 from the code moves to an odd distance <= 3 when Chase flips a single position (pattern 1) and then decodes; the test
asserts that the count is 0."""
import ctypes as C

import numpy as np
import pytest

import ref_decode as R
import ref_block_soft as B
import ref_block_siso as S
import siso_cases as K


def _pack(o):
    return np.packbits((np.asarray(o) > 127).astype(np.uint8), axis=-1)


def _margins_exhaustive(fs, s):
    """the max-log-MAP rule spelled out in plain integers for one word: (decisions, margins)"""
    k, n, tab = R.code_table(fs)
    costs = []
    for d in range(1 << k):
        c = int(tab[d])
        costs.append(sum((255 - int(s[b])) if (c >> (n - 1 - b)) & 1 else int(s[b]) for b in range(n)))
    d = min(range(1 << k), key=lambda m: (costs[m], m))
    dec = [(d >> (k - 1 - i)) & 1 for i in range(k)]
    L = [min(costs[m] for m in range(1 << k) if ((m >> (k - 1 - i)) & 1) != dec[i]) - costs[d] for i in range(k)]
    return dec, L


def _rule(d, L):
    return min(255, max(128, (255 + L + 1) >> 1)) if d else max(0, min(127, (255 - L) >> 1))


def _tie_words(rng, fs, count):
    """soft words on which two codewords cost the same (test_block_soft's construction)"""
    k, n, tab = R.code_table(fs)
    out = []
    while len(out) < count:
        a, b = rng.randint(0, 1 << k, 2)
        ca, cb = int(tab[a]), int(tab[b])
        diff = [q for q in range(n) if ((ca ^ cb) >> (n - 1 - q)) & 1]
        if len(diff) % 2 or a == b:
            continue
        s = np.array([255 * ((ca >> (n - 1 - q)) & 1) for q in range(n)])
        for q0, q1 in zip(diff[0::2], diff[1::2]):
            c = rng.randint(0, 256)
            for q, v in ((q0, c), (q1, 255 - c)):
                s[q] = 255 - v if (ca >> (n - 1 - q)) & 1 else v
        out.append(s)
    return out


@pytest.mark.parametrize("fs", B.ML_CODES)
def test_ml_margins_match_an_exhaustive_search(fs):
    rng = np.random.RandomState(40 + fs)
    k, n, tab = R.code_table(fs)
    few = fs == R.FEC_H128
    words = [rng.randint(0, 256, n) for _ in range(60 if few else 600)]
    words += [np.full(n, v) for v in (0, 1, 126, 127, 128, 129, 254, 255)]
    words += [rng.choice([0, 255], n) for _ in range(30 if few else 300)] + [rng.choice([127, 128], n) for _ in range(20 if few else 200)]
    words += _tie_words(rng, fs, 60 if few else 600)
    for dist in range(0, 5):                                          # 0 / 255 words at distance 0 .. 4 of a codeword
        for _ in range(8 if few else 40):
            w = R.bits_of_words(np.array([int(tab[rng.randint(1 << k)])]), n) * 255
            w[rng.choice(n, dist, replace=False)] ^= 255
            words.append(w)
    W = np.array(words)
    got = S.ml_siso(fs, W)
    ties = 0
    for w, g in zip(W, got):
        dec, L = _margins_exhaustive(fs, w)
        assert list(g) == [_rule(d, l) for d, l in zip(dec, L)], w
        ties += 0 in L
    assert ties >= (30 if few else 200)                               # margins of 0: the tie rule decided the bit
    assert (_pack(got)[:, 0] >> (8 - k) == B.ml(fs, W)[0]).all()


@pytest.mark.parametrize("fs", B.SOFT_BLOCK)
def test_hard_decisions_of_the_outputs_are_the_soft_block_decoder(fs):
    """every crafted kind, every length of the GPU test (tails, short last blocks, 64 / 65 / 129 codewords), and lengths 1 .. 26"""
    rng = np.random.RandomState(60 + fs)
    info = {}
    for n in sorted(set(K.lengths(fs)) | set(range(1, 27))):
        count = max(K.KINDS, 1500 // K.ncw(fs, n))
        _, soft = K.crafted(rng, fs, n, count)
        o = S.block_decode_siso(fs, soft, n, info)
        assert o.shape == (count, 8 * n)
        assert (_pack(o) == B.block_decode_soft(fs, soft, n)).all(), n
    if fs in B.CHASE_CODES:
        print(fs, info)
        assert info["no_competitor"] >= 100 and info["words"] > 20000
        if fs == R.FEC_GOLAY:
            assert info["no_candidate"] == 0                          # (see the module's docstring)
        else:
            assert info["no_candidate"] >= 100


@pytest.mark.parametrize("fs", B.CHASE_CODES)
def test_chase_rules_on_explicit_candidates(fs):
    """the margins against a plain loop over the candidate list, word by word: no competitor -> 0 / 255, no candidate -> 64 / 192"""
    rng = np.random.RandomState(80 + fs)
    n = 24 if fs == R.FEC_GOLAY else 3 * R.SECDED[fs][0] + 1           # SECDED: a short last block of one byte
    _, soft = K.crafted(rng, fs, n, 210)
    el = R.fec_enc_len(fs, n)
    got = S.block_decode_siso(fs, soft, n)
    if fs == R.FEC_GOLAY:
        words, nb = soft[:, :8 * el].reshape(-1, 24).astype(np.int64), None
        cands = S.chase_candidates(words, np.ones(words.shape, bool), B.golay_hard, lambda d: B.codeword_bits(fs)[d])
        bits_of = lambda d: R.bits_of_words(np.asarray(d), 12).reshape(-1, 12)
        per = 12
    else:
        nd = R.SECDED[fs][0]
        pad = np.zeros((len(soft), 4 * 8 * (nd + 1)), np.int64)
        pad[:, :8 * el] = soft
        words, nb = pad.reshape(-1, 8 * (nd + 1)), np.tile([nd, nd, nd, 1], len(soft))
        valid = np.arange(8 + 8 * nd)[None, :] < (8 + 8 * nb)[:, None]
        cands = S.chase_candidates(words, valid, lambda y: B.secded_hard(fs, y, nb), lambda d: B.secded_encode_bits(fs, d))
        bits_of = lambda d: np.unpackbits(np.asarray(d, np.uint8), axis=1)
        per = 8 * nd
    ok, cost, outs, fallback = cands
    bits = [bits_of(o) for o in outs]
    fb = bits_of(fallback)
    want = np.zeros((len(words), per), np.int64)
    seen = {"none": 0, "alone": 0}
    for w in range(len(words)):
        live = [p for p in range(16) if ok[p, w]]
        if not live:
            want[w] = np.where(fb[w] == 1, 192, 64)
            seen["none"] += 1
            continue
        win = min(live, key=lambda p: (cost[p, w], p))
        for i in range(per):
            d = bits[win][w, i]
            rivals = [cost[p, w] for p in live if bits[p][w, i] != d]
            seen["alone"] += not rivals
            want[w, i] = _rule(d, min(rivals) - cost[win, w] if rivals else 255)
            if not rivals:
                assert want[w, i] == 255 * d
    want = want.reshape(len(soft), -1)
    if fs != R.FEC_GOLAY:                                              # drop the short block's absent bytes
        nd = R.SECDED[fs][0]
        want = want[:, :8 * n]
    assert (got == want[:, :8 * n]).all()
    # (this word-by-word loop is slow, so its floors are small; the floors of 100 are asserted on the vectorised reference above)
    assert seen["alone"] >= 100 and (fs == R.FEC_GOLAY or seen["none"] >= 5), seen


def test_soft_viterbi_on_saturated_values_is_the_hard_viterbi():
    """the premise of the first identity: on 0 / 255 values every metric of ref_decode.viterbi is 255 times the hard one, so
    decisions and ties are the same"""
    rng = np.random.RandomState(5)
    for fs in R.CONV:
        bits = rng.randint(0, 2, (12, 8 * R.fec_enc_len(fs, 40)))
        bits[::2] = np.unpackbits(R.fec_encode(fs, rng.randint(0, 256, 40).astype(np.uint8)))[None] ^ (rng.rand(6, bits.shape[1]) < 0.05)
        a, ma = R.viterbi(fs, bits, 40, 1)
        b, mb = R.viterbi(fs, bits * 255, 40, 255)
        assert (a == b).all() and (mb == 255 * ma).all()


@pytest.mark.parametrize("fec1", B.SOFT_BLOCK)
def test_identity_saturated_outputs_give_the_soft_block_result(fec1):
    """clean 0 / 255 channel values with a few bit errors: where every soft output saturates, the chain is soft_block's"""
    rng = np.random.RandomState(90 + fec1)
    hit = 0
    for trial in range(24):
        fec0 = (R.FEC_V27, R.FEC_V27P23, R.FEC_V27P78)[trial % 3]
        n = (1, 2, 17, 40)[trial % 4]
        msg = rng.randint(0, 256, n).astype(np.uint8)
        soft = np.unpackbits(R.packet_encode(msg, R.CRC_16, fec0, fec1)).astype(np.int64) * 255
        soft ^= 255 * (rng.rand(len(soft)) < (0.0, 0.004, 0.01)[trial % 3])
        k, l0, l1 = R.packet_dims(n, R.CRC_16, fec0, fec1)
        o = S.block_decode_siso(fec1, R.interleave_soft(soft.astype(np.uint8), l1, decode=True), l0)[0]
        if np.isin(o, (0, 255)).all():
            hit += 1
            assert S.packet_decode_chain(soft, n, R.CRC_16, fec0, fec1) == B.packet_decode(soft, n, R.CRC_16, fec0, fec1)
    assert hit >= 8


def test_identity_pairs_outside_the_rule_are_soft_block():
    rng = np.random.RandomState(13)
    pairs = [(R.FEC_NONE, R.FEC_H128), (R.FEC_SD39, R.FEC_NONE), (R.FEC_RS, R.FEC_GOLAY), (R.FEC_NONE, R.FEC_RS), (R.FEC_H74, R.FEC_GOLAY),
             (R.FEC_V27, R.FEC_NONE), (R.FEC_V27, R.FEC_V27P23), (R.FEC_V27, R.FEC_RS), (R.FEC_GOLAY, R.FEC_SD72), (R.FEC_NONE, R.FEC_NONE)]
    for fec0, fec1 in pairs:
        assert not S.chained(fec0, fec1)
        msg = rng.randint(0, 256, 33).astype(np.uint8)
        soft = np.unpackbits(R.packet_encode(msg, R.CRC_24, fec0, fec1)).astype(np.int64) * 255
        noisy = np.clip(soft + rng.randint(-150, 151, soft.shape), 0, 255)
        assert S.packet_decode_chain(noisy, 33, R.CRC_24, fec0, fec1) == B.packet_decode(noisy, 33, R.CRC_24, fec0, fec1)
    for fec1 in B.SOFT_BLOCK:                                         # and the covered ones decode a mildly noisy packet
        assert S.chained(R.FEC_V27P34, fec1)
        msg = rng.randint(0, 256, 33).astype(np.uint8)
        soft = np.unpackbits(R.packet_encode(msg, R.CRC_24, R.FEC_V27P34, fec1)).astype(np.int64) * 255
        noisy = np.clip(soft + rng.randint(-100, 101, soft.shape), 0, 255)
        assert S.packet_decode_chain(noisy, 33, R.CRC_24, R.FEC_V27P34, fec1) == (msg.tobytes(), 1)


def test_model_of_the_gain_at_the_gpu_tests_points():
    """the CPU model (siso_cases.model_counts; its whole table is in tests/test_gpu_block_siso.py's docstring) at the points the
    GPU gain test uses, with fewer frames: the chain decodes clearly more packets than soft_block alone"""
    for fec1, snr in ((R.FEC_H74, 1.0), (R.FEC_H128, 2.0)):
        sb, sc = K.model_counts(fec1, snr, frames=40)
        print(fec1, snr, sb, sc)
        assert sc >= sb + 8


# ---------------------------------------------------------------------------------------------------- the library (these fail without the feature)
def test_library_exports_the_soft_chain_entry_points(fx):
    L = fx.lib()
    for name in ("fxrx_debug_block_siso", "fxrx_sync_set_soft_chain"):
        assert hasattr(L, name) and name in fx._ffi.EXPORTS
    assert hasattr(L, "fx_launch_blksiso")
    # the field follows soft_block: _ffi.ConfigChain is _ffi.Config (which ends there) with soft_chain appended
    F = fx._ffi
    assert issubclass(F.ConfigChain, F.Config) and [n for n, _ in F.ConfigChain._fields_] == ["soft_chain"]
    assert F.ConfigChain.soft_chain.offset == F.Config.soft_block.offset + C.sizeof(C.c_int) == C.sizeof(F.Config)
    assert C.sizeof(F.ConfigChain) == C.sizeof(F.Config) + C.sizeof(C.c_int)
    assert L.fxrx_sync_set_soft_chain(None, 1) == -1
    buf = (C.c_ubyte * 64)()
    assert L.fxrx_debug_block_siso(R.FEC_RS, 4, 1, buf, buf) == -1     # bad arguments are refused before any device is looked for
    assert L.fxrx_debug_block_siso(R.FEC_V27, 4, 1, buf, buf) == -1
    assert L.fxrx_debug_block_siso(R.FEC_GOLAY, 0, 1, buf, buf) == -1
    assert L.fxrx_debug_block_siso(R.FEC_GOLAY, 4, 1, None, buf) == -1


@pytest.mark.parametrize("mode,soft,sb", [(0, 1, 0), (0, 0, 0), (1, 1, 1)], ids=["no_soft_block", "no_soft_decision", "detector"])
def test_soft_chain_needs_soft_block_and_flex_rx(fx, mode, soft, sb):
    L = fx.lib()
    cfg = fx._ffi.ConfigChain(0, mode, 1, 0.0, 0, 0, 0, soft, 0, sb, 1)
    assert not L.fxrx_create(cfg)
    assert b"soft_chain" in L.fxrx_last_error() or b"soft_block" in L.fxrx_last_error()
    if not sb:
        assert b"soft_chain" in L.fxrx_last_error()
