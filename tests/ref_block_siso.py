"""Plain numpy reference of soft-output block decoding (fxrx_config.soft_chain), independent of the kernels and of the oracle (the
oracle has no such decoder).  Built on tests/ref_decode.py and tests/ref_block_soft.py; brute force throughout: every codeword's
cost for the maximum-likelihood codes, an explicit list of the sixteen Chase candidates for Golay and SECDED.

The rule (this project's, not liquid's; integers only).  s_b: soft value of codeword position b, 0 = surely 0 ... 255 = surely 1.
C(c) = sum_b (c_b ? 255 - s_b : s_b).  d: the message ref_block_soft.block_decode_soft returns (same ties).  L_i >= 0: the margin
of message bit i.  Output, one value per message bit in the order of the output bytes, MSB first:
    o_i = min(255, max(128, (255 + L_i + 1) >> 1))  if d_i = 1,        o_i = max(0, min(127, (255 - L_i) >> 1))  if d_i = 0.
  * Hamming(7,4), (8,4), (12,8): L_i = min{C(c) : m_i != d_i} - C(d) over all codewords.
  * Golay, SECDED (Chase-4): the candidates are the successful re-encodings of the 16 patterns; L_i = min{C(c) : c a candidate, its
    m_i != d_i} - C(d); no such candidate: L_i = 255; no candidate at all (d is the hard decoder's output on the hard word):
    o_i = d_i ? 192 : 64 (NO_CANDIDATE).
  * Positions a short last block does not transmit, and padding bits past 8 n, are not emitted.
Stage rule of the packet chain: fec1 one of these codes and fec0 convolutional -> fec1 emits 8 l0 soft values, the soft
de-interleaver, the soft-input Viterbi; every other pair is ref_block_soft.packet_decode."""
import numpy as np

import ref_decode as R
import ref_block_soft as B

NO_CANDIDATE = (64, 192)                      # output of a message bit 0 / 1 that no Chase candidate backs
BIG = 1 << 40


def soft_out(d, L):
    """decisions d (0 / 1) and margins L >= 0 -> soft outputs"""
    d, L = np.asarray(d, np.int64), np.asarray(L, np.int64)
    one = np.minimum(255, np.maximum(128, (255 + L + 1) >> 1))
    zero = np.maximum(0, np.minimum(127, (255 - L) >> 1))
    return np.where(d == 1, one, zero).astype(np.uint8)


def ml_siso(fs, soft):
    """(N, n) soft values -> (N, k) soft outputs: every codeword's cost, the margins by exhaustive search"""
    k, n, _ = R.code_table(fs)
    cb = B.codeword_bits(fs).astype(bool)                                           # (2^k, n)
    mb = R.bits_of_words(np.arange(1 << k), k).reshape(1 << k, k).astype(bool)      # message bits, MSB first
    soft = np.asarray(soft, np.int64).reshape(-1, n)
    out = np.empty((len(soft), k), np.uint8)
    step = max(1, (1 << 21) // cb.size)
    for a in range(0, len(soft), step):
        s = soft[a:a + step, None, :]
        c = np.where(cb[None], 255 - s, s).sum(axis=2)                              # (N, 2^k)
        d = c.argmin(axis=1)                                                        # first minimum: the smallest message
        cd = c[np.arange(len(c)), d]
        db = mb[d]                                                                  # (N, k)
        other = mb[None, :, :] != db[:, None, :]                                    # (N, 2^k, k): codewords with m_i != d_i
        L = np.where(other, c[:, :, None], BIG).min(axis=1) - cd[:, None]
        out[a:a + step] = soft_out(db, L)
    return out


def chase_candidates(soft, valid, hard, encode):
    """ref_block_soft.chase's sixteen trials, every one kept: (ok (16, N), cost (16, N), outputs [16] as the hard decoder returns
    them, the hard decoder's output on the hard word)"""
    soft = np.where(valid, np.asarray(soft, np.int64), 0)
    N, P = soft.shape
    key = np.where(valid, np.abs(2 * soft - 255) * 128 + np.arange(P)[None, :], BIG)
    test = np.argsort(key, axis=1, kind="stable")[:, :4]
    y = (soft > 127).astype(np.uint8)
    rows = np.arange(N)
    oks, costs, outs = [], [], []
    for p in range(16):
        yp = y.copy()
        for j in range(4):
            if (p >> j) & 1:
                yp[rows, test[:, j]] ^= 1
        out, ok = hard(yp)
        oks.append(ok)
        costs.append(B.cost_of(encode(out), soft, valid))
        outs.append(out)
    return np.array(oks), np.array(costs), outs, hard(y)[0]


def chase_siso(cands, to_bits, info=None):
    """candidates -> (N, message bits) soft outputs.  info (a dict) counts 'words', 'no_candidate' words and 'no_competitor' bits."""
    ok, cost, outs, fallback = cands
    bits = np.stack([to_bits(o) for o in outs]).astype(np.int64)                    # (16, N, K)
    N = ok.shape[1]
    key = np.where(ok, cost * 16 + np.arange(16)[:, None], BIG)
    win = key.argmin(axis=0)                                                        # cheapest, ties to the smallest pattern
    some = ok.any(axis=0)
    d = np.where(some[:, None], bits[win, np.arange(N)], to_bits(fallback))
    cd = cost[win, np.arange(N)]
    rival = ok[:, :, None] & (bits != d[None])                                      # candidates whose m_i != d_i
    best = np.where(rival, cost[:, :, None], BIG).min(axis=0)
    L = np.where(rival.any(axis=0), best - cd[:, None], 255)
    out = np.where(some[:, None], soft_out(d, L), np.where(d == 1, NO_CANDIDATE[1], NO_CANDIDATE[0])).astype(np.uint8)
    if info is not None:
        info["words"] = info.get("words", 0) + N
        info["no_candidate"] = info.get("no_candidate", 0) + int((~some).sum())
        info["no_competitor"] = info.get("no_competitor", 0) + int((~rival.any(axis=0))[some].sum())
    return out


CHUNK = 4096                                  # rows at a time (memory)


def golay_siso(soft, info=None):
    soft = np.asarray(soft, np.int64).reshape(-1, 24)
    if len(soft) > CHUNK:
        return np.concatenate([golay_siso(soft[a:a + CHUNK], info) for a in range(0, len(soft), CHUNK)])
    cands = chase_candidates(soft, np.ones(soft.shape, bool), B.golay_hard, lambda d: B.codeword_bits(R.FEC_GOLAY)[d])
    return chase_siso(cands, lambda d: R.bits_of_words(np.asarray(d), 12).reshape(-1, 12), info)


def secded_siso(fs, soft, nb, info=None):
    """(N, 8 + 8 nd) soft values, nb (N,) data bytes transmitted -> (N, 8 nd) soft outputs (those of absent bytes are meaningless)"""
    nd = R.SECDED[fs][0]
    nb = np.asarray(nb, np.int64)
    if len(nb) > CHUNK:
        return np.concatenate([secded_siso(fs, soft[a:a + CHUNK], nb[a:a + CHUNK], info) for a in range(0, len(nb), CHUNK)])
    valid = np.arange(8 + 8 * nd)[None, :] < (8 + 8 * nb)[:, None]
    cands = chase_candidates(soft, valid, lambda y: B.secded_hard(fs, y, nb), lambda d: B.secded_encode_bits(fs, d))
    return chase_siso(cands, lambda d: np.unpackbits(np.asarray(d, np.uint8), axis=1), info)


def block_decode_siso(fs, soft, n, info=None):
    """(M, >= 8 fec_enc_len(fs, n)) soft values of M packets in codeword bit order -> (M, 8 n) soft values of the message bits"""
    soft = np.asarray(soft, np.int64)
    soft = soft.reshape(1, -1) if soft.ndim == 1 else soft
    M, el = len(soft), R.fec_enc_len(fs, n)
    soft = soft[:, :8 * el]
    if fs == R.FEC_H84:
        return ml_siso(fs, soft[:, :16 * n].reshape(-1, 8)).reshape(M, 8 * n)
    if fs in (R.FEC_H74, R.FEC_H128, R.FEC_GOLAY):
        k, w, nb, _ = R._packed_dims(fs, n)
        words = soft[:, :nb * w].reshape(M * nb, w)
        o = golay_siso(words, info) if fs == R.FEC_GOLAY else ml_siso(fs, words)
        return o.reshape(M, nb * k)[:, :8 * n]
    if fs in R.SECDED:
        nd = R.SECDED[fs][0]
        full, part = divmod(n, nd)
        nblk = full + (1 if part else 0)
        pad = np.zeros((M, nblk * 8 * (nd + 1)), np.int64)
        pad[:, :8 * el] = soft
        nbv = np.full(nblk, nd)
        if part:
            nbv[-1] = part
        o = secded_siso(fs, pad.reshape(M * nblk, 8 * (nd + 1)), np.tile(nbv, M), info)
        return o.reshape(M, nblk * 8 * nd)[:, :8 * n]
    raise ValueError(fs)


def chained(fec0, fec1):
    """the pairs the stage rule covers"""
    return fec1 in B.SOFT_BLOCK and fec0 in R.CONV


def packet_decode_chain(soft, n, check, fec0, fec1, info=None):
    """soft values (8 l1, channel order) -> (payload bytes, valid) under the stage rule of fxrx_config.soft_chain"""
    if not chained(fec0, fec1):
        return B.packet_decode(soft, n, check, fec0, fec1)
    k, l0, l1 = R.packet_dims(n, check, fec0, fec1)
    v = R.interleave_soft(np.asarray(soft, np.uint8)[:8 * l1], l1, decode=True)
    o = block_decode_siso(fec1, v, l0, info)[0]
    v0 = R.interleave_soft(o, l0, decode=True)
    return R._finish(np.asarray(R.viterbi(fec0, v0[None], k, 255)[0][0], np.uint8), n, check)
