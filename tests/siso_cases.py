"""Crafted inputs of the soft-output block decoders (tests/test_block_siso.py, tests/test_gpu_block_siso.py): packets of soft values in
codeword bit order, of seven kinds, cycled packet by packet."""
import numpy as np

import ref_decode as R
import ref_block_soft as B
import ref_block_siso as S

KINDS = 7
LENGTHS = (1, 2, 3, 7, 8, 9, 63)


def ncw(fs, n):
    """codewords (SECDED: blocks) of a packet of n bytes: one lane's work each in the kernel"""
    if fs == R.FEC_H84:
        return 2 * n
    if fs in R.SECDED:
        return -(-n // R.SECDED[fs][0])
    return R._packed_dims(fs, n)[2]


def n_for_groups(fs, groups):
    """the smallest packet length with at least that many codewords"""
    n = 1
    while ncw(fs, n) < groups:
        n += 1
    return n                                  # (Hamming(7,4) / (8,4) have two codewords a byte: 66 for 65)


def lengths(fs):
    """the issue's lengths, and those with 64, 65 and 129 codewords (round boundaries of the kernel's 64-lane rounds)"""
    return tuple(sorted(set(LENGTHS + tuple(n_for_groups(fs, g) for g in (64, 65, 129)))))


def crafted(rng, fs, n, count):
    """count packets of n message bytes -> (messages (count, n), soft values (count, 8 fec_enc_len))"""
    msg = rng.randint(0, 256, (count, n)).astype(np.uint8)
    bits = np.unpackbits(np.stack([R.fec_encode(fs, m) for m in msg]), axis=1).astype(np.int64)
    kind = np.arange(count) % KINDS
    shape = bits.shape
    flip = (rng.rand(*shape) < rng.choice([0.0, 0.02, 0.06, 0.12, 0.25], (count, 1))).astype(np.int64)
    hard = (bits ^ flip) * 255                                                   # 0: 0 / 255 with 0 .. many bit errors
    near = np.where(bits == 1, 255 - rng.randint(0, 200, shape), rng.randint(0, 200, shape))
    near = np.where(rng.rand(*shape) < 0.04, 255 - near, near)                   # 1: near-codeword noise
    ties = rng.randint(127, 129, shape)                                          # 2: all 127 / 128
    unif = rng.randint(0, 256, shape)                                            # 3: uniform noise
    mild = np.clip(bits * 255 + rng.randint(-140, 141, shape), 0, 255)          # 4: noise around the codeword
    edge = np.where(rng.rand(*shape) < 0.1, rng.randint(126, 130, shape), (bits ^ (rng.rand(*shape) < 0.03)) * 255)   # 5: erasures
    sat = np.where(bits == 1, 255 - rng.randint(0, 3, shape), rng.randint(0, 3, shape))
    sat = np.where(rng.rand(*shape) < 0.05, 255 - sat, sat)                      # 6: values 0 .. 2 / 253 .. 255 with bit errors
    s = np.empty(shape, np.int64)
    for k, v in enumerate((hard, near, ties, unif, mild, edge, sat)):
        s[kind == k] = v[kind == k]
    return msg, s.astype(np.uint8)


# ---------------------------------------------------------------------------------------------------- the CPU model of the gain
def model_counts(fec1, snr_db, frames=200, n=64, seed=0, fec0=R.FEC_V27, ms=R.PSK4, check=R.CRC_24):
    """valid payloads of `frames` random n-byte packets, fec0 behind fec1, over AWGN at Es/N0 = snr_db through ref_decode's soft
    demapper: (with soft_block alone, with soft_chain).  Both chains see the same soft values."""
    rng = np.random.RandomState(seed * 1000 + fec1 * 31 + int(round(snr_db * 10)) + 500)
    k, l0, l1 = R.packet_dims(n, check, fec0, fec1)
    pts, lab = R.constellation(ms)
    point_of = np.empty(len(pts), np.complex128)
    point_of[lab] = pts
    bps, nsym = R.bps(ms), R.num_symbols(ms, l1)
    sigma = np.sqrt(0.5 * 10.0 ** (-snr_db / 10.0))
    msgs, hard_in, soft_in = [], [], []
    for _ in range(frames):
        msg = rng.randint(0, 256, n).astype(np.uint8)
        pkt = R.packet_encode(msg, check, fec0, fec1)
        bits = np.zeros(nsym * bps, np.uint8)
        bits[:8 * l1] = np.unpackbits(pkt)
        r = point_of[R.words_of(bits, bps)] + sigma * (rng.randn(nsym) + 1j * rng.randn(nsym))
        soft = R.soft_to_channel(R.demap_soft(ms, r), l1)
        v = R.interleave_soft(soft, l1, decode=True)
        hard_in.append(np.unpackbits(R.interleave(B.block_decode_soft(fec1, v, l0)[0], decode=True)))
        soft_in.append(R.interleave_soft(S.block_decode_siso(fec1, v, l0)[0], l0, decode=True))
        msgs.append(msg)
    out = []
    for vals, vmax in ((np.array(hard_in), 1), (np.array(soft_in), 255)):
        dec = R.viterbi(fec0, vals, k, vmax)[0]
        out.append(sum(R._finish(d, n, check) == (m.tobytes(), 1) for d, m in zip(dec, msgs)))
    return tuple(out)
