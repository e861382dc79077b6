"""Plain numpy reference of soft-input block decoding (fxrx_config.soft_block), independent of the kernels and of the oracle (the
oracle has no such decoder).  Built on tests/ref_decode.py: its encoder tables, hard decoders, SECDED columns and interleaver.

Soft values are bytes, 0 = surely 0 ... 255 = surely 1, taken after the stage's de-interleaver in codeword bit order (the order in
which the hard decoder reads its bits).  The cost of codeword c is sum_b (c_b ? 255 - s_b : s_b).
  * Hamming(7,4), (8,4), (12,8): exhaustive maximum likelihood, ties to the smallest message.
  * Golay(24,12), SECDED(22,16) / (39,32) / (72,64): Chase-4.  The test positions are the four transmitted positions with the
    smallest (|2 s_b - 255|, b); the hard word is y_b = s_b > 127 (positions a short last SECDED block does not transmit are 0).
    For p = 0..15, test position j of y is flipped where bit j of p is set and the hard decoder runs on the result; if it
    succeeds, the candidate is the re-encoding of its output, costed over the transmitted positions.  The cheapest candidate's
    data win, ties to the smallest p; with no candidate at all the output is the hard decoder's on y.  Success: Golay -- a
    codeword within distance 3 (ref_decode.nearest_codeword's rule); SECDED -- a syndrome of 0, of weight 1, or equal to a data
    column.  A SECDED codeword's bits are its parity byte's 8 bits, then the data bits, MSB first.
These rules are the project's, not liquid's fec_decode_soft.  Reed-Solomon keeps hard decisions."""
import functools
import itertools

import numpy as np

import ref_decode as R

ML_CODES = (R.FEC_H74, R.FEC_H84, R.FEC_H128)
CHASE_CODES = (R.FEC_GOLAY, R.FEC_SD22, R.FEC_SD39, R.FEC_SD72)
SOFT_BLOCK = ML_CODES + CHASE_CODES


@functools.lru_cache(None)
def codeword_bits(fs):
    """(2^k, n) bits of every codeword, MSB first"""
    k, n, tab = R.code_table(fs)
    return R.bits_of_words(tab, n).reshape(1 << k, n)


def ml(fs, soft):
    """(N, n) soft values -> (messages (N,), costs (N,)): brute force over all 2^k codewords, ties to the smallest message"""
    cb = codeword_bits(fs).astype(bool)
    soft = np.asarray(soft, np.int32).reshape(-1, cb.shape[1])
    step = max(1, (1 << 22) // cb.size)
    data, cost = np.empty(len(soft), np.int64), np.empty(len(soft), np.int64)
    for a in range(0, len(soft), step):
        s = soft[a:a + step, None, :]
        c = np.where(cb[None], 255 - s, s).sum(axis=2)
        data[a:a + step] = c.argmin(axis=1)                  # argmin keeps the first minimum
        cost[a:a + step] = c.min(axis=1)
    return data, cost


def cost_of(bits, soft, valid=None):
    """sum over the (valid) positions of (c_b ? 255 - s_b : s_b), row-wise"""
    s = np.asarray(soft, np.int64)
    c = np.where(np.asarray(bits) != 0, 255 - s, s)
    return (c if valid is None else np.where(valid, c, 0)).sum(axis=-1)


# ---------------------------------------------------------------------------------------------------- hard decoders on bit rows
@functools.lru_cache(None)
def _golay_leaders():
    """syndrome -> the error pattern of weight <= 3 with that syndrome, -1 where there is none (min distance 8: all distinct)"""
    tab = R.code_table(R.FEC_GOLAY)[2]
    pats = [0] + [sum(1 << i for i in c) for w in (1, 2, 3) for c in itertools.combinations(range(24), w)]
    pats = np.array(pats, np.int64)
    syn = (tab[pats >> 12] ^ pats) & 0xfff
    assert len(np.unique(syn)) == len(pats) == 2325
    lead = np.full(4096, -1, np.int64)
    lead[syn] = pats
    return lead


def golay_hard(bits):
    """(N, 24) received bits -> (messages (N,), success (N,)): the codeword within distance 3, else the data part as received"""
    tab = R.code_table(R.FEC_GOLAY)[2]
    r = R.words_of(np.asarray(bits).ravel(), 24)
    e = _golay_leaders()[(tab[r >> 12] ^ r) & 0xfff]
    ok = e >= 0
    return np.where(ok, (r ^ np.where(ok, e, 0)) >> 12, r >> 12), ok


def secded_hard(fs, bits, nb):
    """(N, 8 + 8 nd) bits (parity byte, data) and data bytes transmitted (N,) -> (data (N, nd) with absent bytes 0, success (N,));
    ref_decode.fec_decode's rule: syndrome 0 clean, weight 1 a parity bit, a data column that bit flipped, else as received"""
    nd = R.SECDED[fs][0]
    bits = np.asarray(bits, np.uint8)
    par = np.packbits(bits[:, :8], axis=1)[:, 0].astype(np.int64)
    db = bits[:, 8:].copy()
    s = par ^ R._secded_parity(fs, np.packbits(db, axis=1))
    col = s[:, None] == R.secded_columns(fs)[None, :]
    bi, bj = np.nonzero(col)
    db[bi, bj] ^= 1
    d = np.packbits(db, axis=1)
    d[np.arange(nd)[None, :] >= np.asarray(nb)[:, None]] = 0
    return d, (s == 0) | (R.popcount(s) == 1) | col.any(axis=1)


def secded_encode_bits(fs, data):
    """(N, nd) data bytes -> (N, 8 + 8 nd) codeword bits"""
    data = np.asarray(data, np.uint8)
    par = R._secded_parity(fs, data).astype(np.uint8)
    return np.concatenate([np.unpackbits(par[:, None], axis=1), np.unpackbits(data, axis=1)], axis=1)


# ---------------------------------------------------------------------------------------------------- Chase-4
def chase(soft, valid, hard, encode):
    """soft (N, P), valid (N, P) the transmitted positions; hard(y bits) -> (outputs, success); encode(outputs) -> (N, P) bits.
    Returns (outputs of the winners, index of the winning pattern or -1 when nothing succeeded)."""
    soft = np.where(valid, np.asarray(soft, np.int64), 0)
    N, P = soft.shape
    key = np.where(valid, np.abs(2 * soft - 255) * 128 + np.arange(P)[None, :], 1 << 40)
    test = np.argsort(key, axis=1, kind="stable")[:, :4]
    y = (soft > 127).astype(np.uint8)
    best_out, _ = hard(y)
    best_out = best_out.copy()
    best_key = np.full(N, np.iinfo(np.int64).max)
    win = np.full(N, -1)
    rows = np.arange(N)
    for p in range(16):
        yp = y.copy()
        for j in range(4):
            if (p >> j) & 1:
                yp[rows, test[:, j]] ^= 1
        out, ok = hard(yp)
        k = cost_of(encode(out), soft, valid) * 16 + p
        take = ok & (k < best_key)
        best_key[take], best_out[take], win[take] = k[take], out[take], p
    return best_out, win


def golay_chase(soft):
    """(N, 24) soft values -> (messages (N,), winning pattern (N,))"""
    soft = np.asarray(soft, np.int64).reshape(-1, 24)
    return chase(soft, np.ones(soft.shape, bool), golay_hard, lambda d: codeword_bits(R.FEC_GOLAY)[d])


def secded_chase(fs, soft, nb):
    """(N, 8 + 8 nd) soft values of SECDED blocks with nb (N,) data bytes transmitted -> (data (N, nd), winning pattern (N,))"""
    nd = R.SECDED[fs][0]
    nb = np.asarray(nb, np.int64)
    valid = np.arange(8 + 8 * nd)[None, :] < (8 + 8 * nb)[:, None]
    return chase(soft, valid, lambda y: secded_hard(fs, y, nb), lambda d: secded_encode_bits(fs, d))


# ---------------------------------------------------------------------------------------------------- one stage, many packets
def block_decode_soft(fs, soft, n):
    """(M, >= 8 fec_enc_len(fs, n)) soft values of M packets in codeword bit order -> (M, n) decoded bytes"""
    soft = np.asarray(soft, np.int64)
    soft = soft.reshape(1, -1) if soft.ndim == 1 else soft
    M, el = len(soft), R.fec_enc_len(fs, n)
    soft = soft[:, :8 * el]
    if fs == R.FEC_H84:
        d = ml(fs, soft[:, :16 * n].reshape(-1, 8))[0].reshape(M, 2 * n)
        return ((d[:, 0::2] << 4) | d[:, 1::2]).astype(np.uint8)
    if fs in (R.FEC_H74, R.FEC_H128, R.FEC_GOLAY):
        k, w, nb, _ = R._packed_dims(fs, n)
        words = soft[:, :nb * w].reshape(M * nb, w)
        d = golay_chase(words)[0] if fs == R.FEC_GOLAY else ml(fs, words)[0]
        bits = R.bits_of_words(d, k).reshape(M, nb * k)[:, :8 * n]
        return np.packbits(bits, axis=1)
    if fs in R.SECDED:
        nd = R.SECDED[fs][0]
        full, part = divmod(n, nd)
        nblk = full + (1 if part else 0)
        pad = np.zeros((M, nblk * 8 * (nd + 1)), np.int64)
        pad[:, :8 * el] = soft
        nbv = np.full(nblk, nd)
        if part:
            nbv[-1] = part
        d = secded_chase(fs, pad.reshape(M * nblk, 8 * (nd + 1)), np.tile(nbv, M))[0]
        return d.reshape(M, nblk * nd)[:, :n]
    raise ValueError(fs)


def block_decode_hard(fs, enc, n):
    """(M, fec_enc_len(fs, n)) coded bytes -> (M, n): ref_decode.fec_decode packet by packet"""
    enc = np.asarray(enc, np.uint8)
    enc = enc.reshape(1, -1) if enc.ndim == 1 else enc
    return np.stack([R.fec_decode(fs, e, n) for e in enc])


# ---------------------------------------------------------------------------------------------------- packet chain
def packet_decode(soft, n, check, fec0, fec1):
    """soft values (8 l1, channel order) -> (payload bytes, valid) under the stage rule of fxrx_config.soft_block: the stage nearest
    the channel (fec1, and fec0 too when fec1 is NONE) decodes from soft values -- the Viterbi decoder for a convolutional code,
    the decoders above for a block code, hard decisions for Reed-Solomon; every other stage takes hard decisions (value > 127)."""
    k, l0, l1 = R.packet_dims(n, check, fec0, fec1)
    v = R.interleave_soft(np.asarray(soft, np.uint8)[:8 * l1], l1, decode=True)
    hard = lambda s: np.packbits((np.asarray(s) > 127).astype(np.uint8))

    def stage(fs, vals, m):
        if fs in R.CONV:
            return R.viterbi(fs, vals[None], m, 255)[0][0]
        if fs in SOFT_BLOCK:
            return block_decode_soft(fs, vals, m)[0]
        return R.fec_decode(fs, hard(vals), m)

    if fec1 == R.FEC_NONE:
        b0 = stage(fec0, R.interleave_soft(v, l0, decode=True), k)
    else:
        b0 = R.fec_decode(fec0, R.interleave(stage(fec1, v, l0), decode=True), k)
    return R._finish(np.asarray(b0, np.uint8), n, check)
