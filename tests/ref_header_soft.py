"""Plain numpy reference of soft-decision frame header decoding (fxrx_config.soft_header), independent of both the kernels and
the oracle (the oracle has no soft header decoder).

The header is 20 bytes + CRC-32, SECDED(72,64), then Hamming(8,4) next to the channel: 54 coded bytes, 432 coded bits.  The soft
chain takes one soft value per coded bit in channel order (0 = surely 0 ... 255 = surely 1), undoes the outer interleaver as a
bit permutation, and decodes every 8 values to the Hamming(8,4) message d that minimises
    sum_b (bit b of codeword(d) ? 255 - s_b : s_b)          (bit b = bit 7 - b of the codeword byte)
found by brute force over all 16 codewords, ties to the smallest d.  Everything behind that stage -- inner interleaver, SECDED,
de-whitening, CRC -- is tests/ref_decode.py's, applied to many headers at once."""
import numpy as np

import ref_decode as R

HDR_DEC = 20                       # header bytes (14 user + 6 protocol)
HDR_K = HDR_DEC + 4                # + CRC-32
HDR_E0 = 27                        # after SECDED(72,64)
HDR_ENC = 54                       # after Hamming(8,4)
HDR_SOFT = 8 * HDR_ENC             # soft values per header
CHECK, FEC0, FEC1 = R.CRC_32, R.FEC_SD72, R.FEC_H84


def h84_codeword_bits():
    """(16, 8) bits of the 16 Hamming(8,4) codewords, MSB first"""
    return R.bits_of_words(R.code_table(R.FEC_H84)[2], 8).reshape(16, 8)


def h84_ml(soft, chunk=1 << 16):
    """(N, 8) soft values -> (data words (N,), costs (N,)): the maximum-likelihood message of every word by brute force over the
    16 codewords; ties go to the smallest message (argmin keeps the first)."""
    soft = np.asarray(soft, np.int32).reshape(-1, 8)
    cb = h84_codeword_bits().astype(bool)
    data, cost = np.empty(len(soft), np.int64), np.empty(len(soft), np.int64)
    for a in range(0, len(soft), chunk):
        s = soft[a:a + chunk, None, :]
        c = np.where(cb[None], 255 - s, s).sum(axis=2)           # (n, 16)
        data[a:a + chunk] = c.argmin(axis=1)
        cost[a:a + chunk] = c.min(axis=1)
    return data, cost


def header_encode(hdr20, trace=None):
    """20 header bytes -> the 54 channel bytes (ref_decode.packet_encode with the header's CRC and codes)"""
    return R.packet_encode(np.asarray(hdr20, np.uint8), CHECK, FEC0, FEC1, trace)


def header_encode_from_cw0(cw0):
    """the channel bytes of a header whose SECDED codeword (27 bytes, before the inner interleaver) is cw0 -- cw0 may carry errors"""
    return R.interleave(R.fec_encode(FEC1, R.interleave(np.asarray(cw0, np.uint8))))


def crc32_rows(msg):
    """ref_decode.crc_key(CRC_32, row) of every row of msg (N, n), the same register arithmetic vectorised over the rows"""
    w, poly = R.CRC_SPEC[R.CRC_32]
    top, mask = 1 << (w - 1), (1 << w) - 1
    msg = np.asarray(msg, np.uint8)
    reg = np.full(len(msg), mask, np.int64)
    for j in range(msg.shape[1]):
        byte = msg[:, j].astype(np.int64)
        for k in range(8):
            fb = ((reg & top) != 0) ^ (((byte >> k) & 1) != 0)
            reg = ((reg << 1) & mask) ^ np.where(fb, poly, 0)
    out = np.zeros(len(msg), np.int64)
    for k in range(w):
        out |= ((reg >> k) & 1) << (w - 1 - k)
    return out ^ mask


def _back(b1):
    """(N, 27) Hamming-decoded bytes -> (headers (N, 20) uint8, valid (N,) int): inner de-interleave, SECDED(72,64),
    de-whitening, CRC-32.  27 = 3 whole SECDED blocks, so the headers' blocks decode as one run."""
    b1 = np.asarray(b1, np.uint8)
    N = len(b1)
    p27 = R._ilv_perm(HDR_E0, True)
    in0 = np.packbits(np.unpackbits(b1, axis=1)[:, p27], axis=1)
    b0 = R.fec_decode(FEC0, in0.ravel(), HDR_K * N).reshape(N, HDR_K)
    b0 = b0 ^ np.resize(R.SCRAMBLE_MASK, HDR_K)[None, :]
    key = (b0[:, 20].astype(np.int64) << 24) | (b0[:, 21].astype(np.int64) << 16) | (b0[:, 22].astype(np.int64) << 8) | b0[:, 23]
    return b0[:, :HDR_DEC].copy(), (crc32_rows(b0[:, :HDR_DEC]) == key).astype(np.int64)


def decode_soft(soft):
    """(N, 432) soft values in channel order -> (headers (N, 20), valid (N,))"""
    soft = np.asarray(soft, np.uint8).reshape(-1, HDR_SOFT)
    v = soft[:, R._ilv_perm(HDR_ENC, True)]                        # interleave_soft(..., decode=True), row-wise
    d = h84_ml(v.reshape(-1, 8))[0].reshape(-1, HDR_ENC)
    return _back(((d[:, 0::2] << 4) | d[:, 1::2]).astype(np.uint8))


def decode_hard(enc):
    """(N, 54) received bytes -> (headers (N, 20), valid (N,)): hard Hamming(8,4) (ref_decode.nearest_codeword)"""
    enc = np.asarray(enc, np.uint8).reshape(-1, HDR_ENC)
    in1 = np.packbits(np.unpackbits(enc, axis=1)[:, R._ilv_perm(HDR_ENC, True)], axis=1)
    d = R.nearest_codeword(R.FEC_H84, in1.ravel().astype(np.int64))[0].reshape(-1, HDR_ENC)
    return _back(((d[:, 0::2] << 4) | d[:, 1::2]).astype(np.uint8))


def hard_as_soft(enc):
    """(N, 54) bytes -> (N, 432) soft values 0 / 255"""
    return (np.unpackbits(np.asarray(enc, np.uint8).reshape(-1, HDR_ENC), axis=1) * 255).astype(np.uint8)
