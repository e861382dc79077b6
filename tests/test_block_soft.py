"""Soft-input block decoding (fxrx_config.soft_block) without a GPU: the numpy reference of tests/ref_block_soft.py against brute
force and against ref_decode's hard decoders, and the new entry points and config checks of libfxrx.so."""
import ctypes as C
import itertools

import numpy as np
import pytest

import ref_decode as R
import ref_block_soft as B


def _exhaustive(fs, s):
    """the ML rule spelled out: the cost of every message in plain integers, first minimum"""
    k, n, tab = R.code_table(fs)
    best, arg = None, None
    for d in range(1 << k):
        c = int(tab[d])
        cost = sum((255 - int(s[b])) if (c >> (n - 1 - b)) & 1 else int(s[b]) for b in range(n))
        if best is None or cost < best:
            best, arg = cost, d
    return arg, best


def _ties(rng, fs, count):
    """soft words on which two codewords a, b cost the same: shared bits at 0 / 255, the differing ones in pairs summing to 255"""
    k, n, tab = R.code_table(fs)
    out = []
    while len(out) < count:
        a, b = rng.randint(0, 1 << k, 2)
        ca, cb = int(tab[a]), int(tab[b])
        diff = [q for q in range(n) if ((ca ^ cb) >> (n - 1 - q)) & 1]
        if len(diff) % 2:
            continue
        s = np.array([255 * ((ca >> (n - 1 - q)) & 1) for q in range(n)])
        for q0, q1 in zip(diff[0::2], diff[1::2]):
            c = rng.randint(0, 256)
            for q, v in ((q0, c), (q1, 255 - c)):
                s[q] = 255 - v if (ca >> (n - 1 - q)) & 1 else v
        out.append(s)
    return out


@pytest.mark.parametrize("fs", B.ML_CODES)
def test_ml_stage_matches_exhaustive_search_with_ties(fs):
    rng = np.random.RandomState(fs)
    n = R.code_table(fs)[1]
    words = [rng.randint(0, 256, n) for _ in range(400 if fs == R.FEC_H128 else 1500)]
    words += [np.full(n, v) for v in (0, 1, 126, 127, 128, 129, 254, 255)]
    words += _ties(rng, fs, 300 if fs == R.FEC_H128 else 1000)
    W = np.array(words)
    d, c = B.ml(fs, W)
    k, _, tab = R.code_table(fs)
    n_tied = 0
    for w, gd, gc in zip(W, d, c):
        assert (gd, gc) == _exhaustive(fs, w), w
        costs = B.cost_of(B.codeword_bits(fs), np.broadcast_to(w, (1 << k, n)))
        n_tied += int((costs == gc).sum() > 1)
    assert n_tied >= (60 if fs == R.FEC_H128 else 250)                 # the tie rule was exercised


@pytest.mark.parametrize("fs", B.ML_CODES)
def test_ml_on_hard_values_is_the_hard_decoder_for_every_word(fs):
    n = R.code_table(fs)[1]
    r = np.arange(1 << n)
    d, cost = B.ml(fs, R.bits_of_words(r, n).reshape(-1, n) * 255)
    hd, dist = R.nearest_codeword(fs, r)
    assert (d == hd).all() and (cost == 255 * dist).all()


def _golay_words(rng, n_cw, weights):
    tab = R.code_table(R.FEC_GOLAY)[2]
    d = rng.randint(0, 4096, n_cw)
    cw = tab[d]
    for i, w in enumerate(weights):
        for b in rng.choice(24, w, replace=False):
            cw[i] ^= 1 << b
    return d, cw


def test_golay_chase_on_hard_values_is_the_hard_decoder_where_it_succeeds():
    rng = np.random.RandomState(2)
    # every single and double error pattern on random codewords, random triples, and weight-4 (detected) patterns
    pats = [()] + [(i,) for i in range(24)] + list(itertools.combinations(range(24), 2))
    pats += [tuple(rng.choice(24, 3, replace=False)) for _ in range(3000)] + [tuple(rng.choice(24, 4, replace=False)) for _ in range(3000)]
    tab = R.code_table(R.FEC_GOLAY)[2]
    d = rng.randint(0, 4096, len(pats))
    r = np.array([int(tab[x]) ^ sum(1 << b for b in p) for x, p in zip(d, pats)], np.int64)
    bits = R.bits_of_words(r, 24).reshape(-1, 24)
    hd, hok = B.golay_hard(bits)
    nd, dist = R.nearest_codeword(R.FEC_GOLAY, r)
    assert (hd == nd).all() and (hok == (dist <= 3)).all()
    sd, win = B.golay_chase(bits.astype(np.int64) * 255)
    assert hok.sum() > 3000 and (~hok).sum() > 2000
    assert (sd[hok] == hd[hok]).all() and (win[hok] == 0).all()
    assert (sd[hok] == d[hok]).all()


@pytest.mark.parametrize("fs", (R.FEC_SD22, R.FEC_SD39, R.FEC_SD72))
def test_secded_chase_on_hard_values_is_the_hard_decoder_where_it_succeeds(fs):
    rng = np.random.RandomState(fs)
    nd = R.SECDED[fs][0]
    P = 8 + 8 * nd
    rows, nbs = [], []
    for nb in range(1, nd + 1):
        for trial in range(300):
            data = np.zeros(nd, np.uint8)
            data[:nb] = rng.randint(0, 256, nb)
            bits = B.secded_encode_bits(fs, data[None])[0]
            T = 8 + 8 * nb
            for b in rng.choice(T, trial % 4, replace=False):          # 0-3 errors among the transmitted positions
                bits[b] ^= 1
            rows.append(bits)
            nbs.append(nb)
    bits, nbs = np.array(rows), np.array(nbs)
    hd, hok = B.secded_hard(fs, bits, nbs)
    # the same verdicts and data as ref_decode.fec_decode, block by block
    for i in range(0, len(bits), 7):
        nb = nbs[i]
        enc = np.packbits(bits[i])[:1 + nb]
        assert (R.fec_decode(fs, enc, nb) == hd[i, :nb]).all()
    sd, win = B.secded_chase(fs, bits.astype(np.int64) * 255, nbs)
    assert hok.sum() > len(bits) // 2 and (~hok).sum() > 50
    # where the hard decoder's codeword is within distance 1 of the received word, Chase returns it (pattern 0).  In a short last
    # block a syndrome can match the column of an absent data bit: the re-encoded output then differs from the received word in
    # the parity bits only (3 or 5 of them), and Chase may find a cheaper codeword -- never a costlier one
    valid = np.arange(P)[None, :] < (8 + 8 * nbs)[:, None]
    hc = B.cost_of(B.secded_encode_bits(fs, hd), bits * 255, valid)
    sc = B.cost_of(B.secded_encode_bits(fs, sd), bits * 255, valid)
    near = hok & (hc <= 255)
    assert near.sum() > len(bits) // 3 and (nbs[near] == nd).sum() > 100
    assert (sd[near] == hd[near]).all() and (win[near] == 0).all()
    assert (sc[hok] <= hc[hok]).all()


@pytest.mark.parametrize("fs", B.CHASE_CODES)
def test_chase_never_costs_more_than_the_hard_decoder(fs):
    rng = np.random.RandomState(100 + fs)
    N = 4000
    if fs == R.FEC_GOLAY:
        d, cw = _golay_words(rng, N, rng.randint(0, 5, N))
        clean = R.bits_of_words(cw, 24).reshape(N, 24).astype(np.int64) * 255
        soft = np.clip(clean + np.where(clean > 0, -1, 1) * rng.randint(0, 200, clean.shape), 0, 255)
        hd, hok = B.golay_hard((soft > 127).astype(np.uint8))
        sd, _ = B.golay_chase(soft)
        enc = lambda m: B.codeword_bits(fs)[m]
        valid = np.ones(soft.shape, bool)
    else:
        nd = R.SECDED[fs][0]
        nbs = rng.randint(1, nd + 1, N)
        data = rng.randint(0, 256, (N, nd)).astype(np.uint8)
        data[np.arange(nd)[None, :] >= nbs[:, None]] = 0
        clean = B.secded_encode_bits(fs, data).astype(np.int64) * 255
        valid = np.arange(8 + 8 * nd)[None, :] < (8 + 8 * nbs)[:, None]
        soft = np.where(valid, np.clip(clean + np.where(clean > 0, -1, 1) * rng.randint(0, 200, clean.shape), 0, 255), 0)
        hd, hok = B.secded_hard(fs, (soft > 127).astype(np.uint8), nbs)
        sd, _ = B.secded_chase(fs, soft, nbs)
        enc = lambda m: B.secded_encode_bits(fs, m)
    hc, sc = B.cost_of(enc(hd), soft, valid), B.cost_of(enc(sd), soft, valid)
    assert (sc[hok] <= hc[hok]).all()
    assert (sc[hok] < hc[hok]).sum() > 20                              # and often less


@pytest.mark.parametrize("fs", B.SOFT_BLOCK)
def test_packet_lengths_tails_and_short_blocks(fs):
    """every length 1..40 (Golay / Hamming tails, short last SECDED blocks): clean and mildly noisy soft values decode to the
    message; on 0 / 255 values the ML codes are the hard decoder"""
    rng = np.random.RandomState(7 + fs)
    for n in range(1, 41):
        msg = rng.randint(0, 256, (6, n)).astype(np.uint8)
        enc = np.stack([R.fec_encode(fs, m) for m in msg])
        assert enc.shape[1] == R.fec_enc_len(fs, n)
        soft = np.unpackbits(enc, axis=1).astype(np.int64) * 255
        assert (B.block_decode_soft(fs, soft, n) == msg).all(), n
        noisy = np.clip(soft + rng.randint(-120, 121, soft.shape), 0, 255)
        assert (B.block_decode_soft(fs, noisy, n) == msg).all(), n
        flips = (rng.rand(*soft.shape) < 0.04).astype(np.uint8)
        e = np.packbits(np.unpackbits(enc, axis=1) ^ flips, axis=1)
        if fs in B.ML_CODES:
            assert (B.block_decode_soft(fs, np.unpackbits(e, axis=1) * 255, n) == B.block_decode_hard(fs, e, n)).all()


def test_packet_chain_stage_rule():
    """the chain: block fec1 decoded soft, fec0 behind it hard; fec1 NONE: fec0 soft; Reed-Solomon hard either way"""
    rng = np.random.RandomState(12)
    for fec0, fec1 in ((R.FEC_V27, R.FEC_GOLAY), (R.FEC_NONE, R.FEC_H128), (R.FEC_SD39, R.FEC_NONE), (R.FEC_RS, R.FEC_GOLAY),
                       (R.FEC_NONE, R.FEC_RS), (R.FEC_V27P23, R.FEC_SD72), (R.FEC_H74, R.FEC_NONE)):
        msg = rng.randint(0, 256, 37).astype(np.uint8)
        pkt = R.packet_encode(msg, R.CRC_24, fec0, fec1)
        soft = np.unpackbits(pkt).astype(np.int64) * 255
        assert B.packet_decode(soft, 37, R.CRC_24, fec0, fec1) == (msg.tobytes(), 1)
        noisy = np.clip(soft + rng.randint(-100, 101, soft.shape), 0, 255)
        assert B.packet_decode(noisy, 37, R.CRC_24, fec0, fec1) == (msg.tobytes(), 1)
        if fec1 not in B.SOFT_BLOCK and fec0 not in B.SOFT_BLOCK:     # nothing for the option to do: the soft chain as it was
            assert B.packet_decode(noisy, 37, R.CRC_24, fec0, fec1) == R.packet_decode_soft(noisy.astype(np.uint8), 37, R.CRC_24, fec0, fec1)


def test_library_exports_the_soft_block_entry_points(fx):
    L = fx.lib()
    for name in ("fxrx_debug_block_decode", "fxrx_sync_set_soft_block"):
        assert hasattr(L, name) and name in fx._ffi.EXPORTS
    names = [n for n, _ in fx._ffi.Config._fields_]
    assert names[-1] == "soft_block" and names.index("soft_block") == names.index("soft_header") + 1
    assert L.fxrx_sync_set_soft_block(None, 1) == -1
    # bad arguments are refused before any device is looked for
    buf = (C.c_ubyte * 64)()
    assert L.fxrx_debug_block_decode(R.FEC_RS, 1, 4, 1, buf, buf) == -1
    assert L.fxrx_debug_block_decode(R.FEC_V27, 0, 4, 1, buf, buf) == -1
    assert L.fxrx_debug_block_decode(R.FEC_GOLAY, 1, 0, 1, buf, buf) == -1


@pytest.mark.parametrize("mode,soft", [(0, 0), (1, 1), (1, 0)], ids=["no_soft_decision", "detector", "detector_no_soft"])
def test_soft_block_needs_soft_decision_and_flex_rx(fx, mode, soft):
    L = fx.lib()
    cfg = fx._ffi.Config(0, mode, 1, 0.0, 0, 0, 0, soft, 0, 1)
    assert not L.fxrx_create(cfg)
    assert b"soft_block" in L.fxrx_last_error()
