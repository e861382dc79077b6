"""Plain numpy reference of the receive side's packet chain: carrier-recovered symbols (or per-bit soft values) to payload
bytes and the CRC verdict.  Test infrastructure only.

Every piece is written from its definition, not from the oracle (oracle/fxref_*.c) or the product (gr-liquiddsp_amd/):
constellations from their formulas, nearest-point decisions in float64, the interleaver as a bit permutation, CRCs bit by
bit in the non-reflected form, block codes by brute force over all codewords, SECDED by its parity-check matrix, Reed-Solomon
by Peterson-Gorenstein-Zierler (linear algebra over GF(2^8), no Berlekamp-Massey, no Forney) and the convolutional codes by
a plain int64 Viterbi.  It shares conventions with the two implementations -- which are the specification -- and no code.

Conventions (the project's):
  * bits are MSB first everywhere: in a byte, in a symbol's label, in a block code's word;
  * packet: payload + CRC (big-endian) -> scramble -> fec0 -> interleave -> fec1 -> interleave -> symbols; the receive side
    undoes it in reverse;
  * ties that a decoder must break are broken by the project's rules, stated where they are applied.
"""
import functools
import math

import numpy as np

# ---------------------------------------------------------------------------------------------------- enums (fxref.h)
CRC_NONE, CRC_CHECKSUM, CRC_8, CRC_16, CRC_24, CRC_32 = 1, 2, 3, 4, 5, 6
FEC_NONE, FEC_H74, FEC_H84, FEC_H128, FEC_GOLAY, FEC_SD22, FEC_SD39, FEC_SD72 = 1, 4, 5, 6, 7, 8, 9, 10
FEC_V27, FEC_V27P23, FEC_V27P34, FEC_V27P45, FEC_V27P56, FEC_V27P67, FEC_V27P78 = 11, 15, 16, 17, 18, 19, 20
FEC_RS = 27
CONV = (FEC_V27, FEC_V27P23, FEC_V27P34, FEC_V27P45, FEC_V27P56, FEC_V27P67, FEC_V27P78)
BLOCK = (FEC_H74, FEC_H84, FEC_H128, FEC_GOLAY, FEC_SD22, FEC_SD39, FEC_SD72)
ALL_FEC = (FEC_NONE,) + BLOCK + CONV + (FEC_RS,)
PSK2, PSK4, PSK8, PSK16, DPSK2, DPSK4, DPSK8, ASK4, QAM16, QAM32, QAM64, QPSK = 1, 2, 3, 4, 9, 10, 11, 18, 27, 28, 29, 40
PAYLOAD_MODS = (PSK2, PSK4, PSK8, PSK16, DPSK2, DPSK4, DPSK8, ASK4, QAM16, QAM32, QAM64)
DPSK = (DPSK2, DPSK4, DPSK8)

POP16 = np.array([bin(i).count("1") for i in range(1 << 16)], np.int64)


def popcount(x):
    x = np.asarray(x, np.int64)
    return POP16[x & 0xffff] + POP16[(x >> 16) & 0xffff] + POP16[(x >> 32) & 0xffff]


def gray(i):
    return i ^ (i >> 1)


def bits_of(b):
    """bytes -> bits, MSB first"""
    return np.unpackbits(np.asarray(b, np.uint8))


def bytes_of(bits, nbytes=None):
    """bits (MSB first) -> bytes, zero padded to nbytes"""
    bits = np.asarray(bits, np.uint8)
    nbytes = (len(bits) + 7) // 8 if nbytes is None else nbytes
    out = np.zeros(8 * nbytes, np.uint8)
    out[:min(len(bits), 8 * nbytes)] = bits[:8 * nbytes]
    return np.packbits(out)


def words_of(bits, w):
    """bit array (length multiple of w) -> integers of w bits, MSB first"""
    b = np.asarray(bits, np.int64).reshape(-1, w)
    return (b << np.arange(w - 1, -1, -1, dtype=np.int64)).sum(axis=1)


def bits_of_words(v, w):
    v = np.asarray(v, np.int64)
    return ((v[:, None] >> np.arange(w - 1, -1, -1, dtype=np.int64)) & 1).astype(np.uint8).ravel()


# ---------------------------------------------------------------------------------------------------- constellations
def bps(ms):
    return {PSK2: 1, DPSK2: 1, PSK4: 2, DPSK4: 2, ASK4: 2, QPSK: 2, PSK8: 3, DPSK8: 3, PSK16: 4, QAM16: 4, QAM32: 5,
            QAM64: 6}[ms]


@functools.lru_cache(None)
def constellation(ms):
    """(points complex128, labels) of a scheme, from the formulas of fxref_modem.c's header / fxref.h:
    PSK-M: phase index i at exp(2 pi j i / M), label gray(i); DPSK shares the points (its labels are differences, see
    demap_hard); ASK4: level i at (2 i - 3) / sqrt(5), label gray(i);
    QAM: 2^mi x 2^mq rectangle (QAM16 4x4, QAM32 8x4, QAM64 8x8), levels (2 i - (L - 1)) alpha, alpha = 1/sqrt(10),
    1/sqrt(26), 1/sqrt(42) (unit mean energy), label gray(i_I) << mq | gray(i_Q);
    QPSK (header): label bit 0 = (re < 0), bit 1 = (im < 0) -- the imaginary axis is the label's MSB."""
    k = bps(ms)
    M = 1 << k
    if ms in (PSK2, PSK4, PSK8, PSK16) + DPSK:
        i = np.arange(M)
        return np.exp(2j * np.pi * i / M), gray(i)
    if ms == ASK4:
        i = np.arange(4)
        return (2.0 * i - 3.0) / math.sqrt(5.0) + 0j, gray(i)
    if ms == QPSK:
        lab = np.arange(4)
        s = 1 / math.sqrt(2.0)
        return np.where(lab & 1, -s, s) + 1j * np.where(lab & 2, -s, s), lab
    mi, mq = {QAM16: (2, 2), QAM32: (3, 2), QAM64: (3, 3)}[ms]
    Li, Lq = 1 << mi, 1 << mq
    ii, iq = np.meshgrid(np.arange(Li), np.arange(Lq), indexing="ij")
    lev_i, lev_q = 2.0 * ii - (Li - 1), 2.0 * iq - (Lq - 1)
    alpha = 1.0 / math.sqrt((lev_i ** 2 + lev_q ** 2).mean())
    return (alpha * (lev_i + 1j * lev_q)).ravel(), ((gray(ii) << mq) | gray(iq)).ravel()


def demap_hard(ms, r):
    """Nearest-point decisions in float64.  Returns (labels, margin): margin = distance to the runner-up point minus the
    distance to the nearest one (for PSK the runner-up is the neighbouring sector's point).
    DPSK: label = gray((i_k - i_{k-1}) mod M) of the phase indices; the payload's first symbol is differenced against phase
    index 0 (both implementations reset the differential state to 0 at the start of every payload)."""
    pts, lab = constellation(ms)
    r = np.asarray(r, np.complex128)
    d = np.abs(r[:, None] - pts[None, :])
    o = np.argsort(d, axis=1, kind="stable")[:, :2]
    idx = o[:, 0]
    margin = np.take_along_axis(d, o[:, 1:2], 1)[:, 0] - np.take_along_axis(d, o[:, 0:1], 1)[:, 0]
    if ms in DPSK:
        M = len(pts)
        prev = np.concatenate([[0], idx[:-1]])
        return gray((idx - prev) % M), margin
    return lab[idx], margin


def demap_soft(ms, r, hard_labels=None):
    """Per-bit soft bytes (nsym, bps), MSB of the label first: clamp(rint(127 + 16 gamma (d0 - d1)), 0, 255), gamma = 1.2 M,
    d0 / d1 the squared distance to the nearest point whose label has a 0 / a 1 at that bit (float64).  DPSK: the hard
    label's bits as 0 / 255."""
    k = bps(ms)
    r = np.asarray(r, np.complex128)
    if ms in DPSK:
        lab = demap_hard(ms, r)[0] if hard_labels is None else np.asarray(hard_labels)
        return (bits_of_words(lab, k).reshape(-1, k) * 255).astype(np.uint8)
    pts, lab = constellation(ms)
    d2 = np.abs(r[:, None] - pts[None, :]) ** 2
    out = np.empty((len(r), k), np.uint8)
    for b in range(k):
        one = ((lab >> (k - 1 - b)) & 1).astype(bool)
        d0, d1 = d2[:, ~one].min(axis=1), d2[:, one].min(axis=1)
        out[:, b] = np.clip(np.rint(127.0 + 16.0 * 1.2 * (1 << k) * (d0 - d1)), 0, 255)
    return out


def symbols_to_bytes(ms, labels, nbytes):
    """labels -> channel bytes: bps bits per symbol, MSB first, cut to 8 nbytes bits (the last symbol's pad bits dropped)"""
    return bytes_of(bits_of_words(labels, bps(ms))[:8 * nbytes], nbytes)


def soft_to_channel(soft_sym, nbytes):
    """(nsym, bps) soft bytes -> the 8 nbytes soft values of the coded bits in channel order (pad bits dropped)"""
    v = np.zeros(8 * nbytes, np.uint8)
    s = np.asarray(soft_sym).ravel()[:8 * nbytes]
    v[:len(s)] = s
    return v


def num_symbols(ms, nbytes):
    return (8 * nbytes + bps(ms) - 1) // bps(ms)


# ---------------------------------------------------------------------------------------------------- interleaver, scrambler
def _ilv_dims(n):
    M = 1 + math.isqrt(n)                   # floor(sqrt(n)) exactly (the implementations' float sqrt agrees far beyond any packet)
    N = n // M
    while n >= M * N:
        N += 1
    return M, N


def _ilv_partners(n, M, N):
    """the odd-byte partner j of every even byte 2i in one pass: a walk j = m N + c down the columns of an M x N grid,
    starting at column n // 3 and wrapping, that skips cells outside [0, n / 2)"""
    n2, c, m, out = n // 2, n // 3, 0, []
    for _ in range(n2):
        while True:
            j = m * N + c
            m += 1
            if m == M:
                m, c = 0, (c + 1) % N
            if j < n2:
                break
        out.append(j)
    return np.array(out, np.int64)


@functools.lru_cache(64)
def _ilv_perm(n, decode):
    """bit permutation of the depth-4 interleaver on n bytes: result[p] = index of the input bit that lands at bit p.
    Four passes exchange, between byte 2i and byte 2j+1, the bits under the masks ff, 0f, 55, 33 (partners from grids of N,
    N+2, N+4, N+8 columns); deinterleaving runs the same passes in reverse order (each pass is an involution)."""
    x = np.arange(8 * n, dtype=np.int64).reshape(n, 8)
    M, N = _ilv_dims(n)
    passes = [(N, 0xff), (N + 2, 0x0f), (N + 4, 0x55), (N + 8, 0x33)]
    sel_of = lambda mask: np.array([(mask >> (7 - k)) & 1 for k in range(8)], bool)
    for cols, mask in (passes[::-1] if decode else passes):
        if n < 2:
            continue
        j = _ilv_partners(n, M, cols)
        a, b, sel = 2 * np.arange(len(j)), 2 * j + 1, sel_of(mask)
        xa, xb = x[a], x[b]
        xa[:, sel], xb[:, sel] = x[b][:, sel], x[a][:, sel]
        x[a], x[b] = xa, xb
    return x.ravel()


def interleave(buf, decode=False):
    buf = np.asarray(buf, np.uint8)
    return bytes_of(bits_of(buf)[_ilv_perm(len(buf), decode)], len(buf))


def interleave_soft(soft, n, decode=False):
    """the same permutation on 8 n per-bit soft values"""
    return np.asarray(soft, np.uint8)[_ilv_perm(n, decode)]


SCRAMBLE_MASK = np.array([0xb4, 0x6a, 0x8b, 0xc5], np.uint8)


def scramble(buf):
    buf = np.asarray(buf, np.uint8)
    return buf ^ np.resize(SCRAMBLE_MASK, len(buf))


# ---------------------------------------------------------------------------------------------------- CRCs
CRC_SPEC = {CRC_8: (8, 0x07), CRC_16: (16, 0x8005), CRC_24: (24, 0x5D6DCB), CRC_32: (32, 0x04C11DB7)}


def crc_len(check):
    return {CRC_NONE: 0, CRC_CHECKSUM: 1, CRC_8: 1, CRC_16: 2, CRC_24: 3, CRC_32: 4}[check]


def crc_key(check, msg):
    """Checksum: two's complement of the byte sum mod 256.  CRC-w: reflected input and output, register preset to all ones,
    result inverted -- computed here in the non-reflected form: each byte's bits enter LSB first into a register shifted
    MSB first with the polynomial as written, the final register is bit-reversed.  (CRC-32 is the common CRC-32, CRC-16 is
    CRC-16/USB.)"""
    msg = bytes(bytearray(np.asarray(msg, np.uint8)))
    if check == CRC_NONE:
        return 0
    if check == CRC_CHECKSUM:
        return (-sum(msg)) & 0xff
    w, poly = CRC_SPEC[check]
    top, mask, reg = 1 << (w - 1), (1 << w) - 1, (1 << w) - 1
    for byte in msg:
        for k in range(8):
            fb = ((reg & top) != 0) ^ ((byte >> k) & 1)
            reg = (reg << 1) & mask
            if fb:
                reg ^= poly
    out = 0
    for k in range(w):
        if reg & (1 << k):
            out |= 1 << (w - 1 - k)
    return out ^ mask


# ---------------------------------------------------------------------------------------------------- block codes
def _positional_hamming(n):
    """positional Hamming code on positions 1..n: parity bits at the powers of two, data bits (MSB first) at the others;
    parity bit 2^p = xor of the data positions with bit p set.  Codeword bits MSB first in position order.  Returns the
    encoder table over all data words."""
    data_pos = [q for q in range(1, n + 1) if q & (q - 1)]
    k = len(data_pos)
    d = np.arange(1 << k, dtype=np.int64)
    bits = {q: (d >> (k - 1 - i)) & 1 for i, q in enumerate(data_pos)}
    p = 1
    while p <= n:
        bits[p] = np.zeros_like(d)
        for q in data_pos:
            if q & p:
                bits[p] = bits[p] ^ bits[q]
        p <<= 1
    return sum(bits[q] << (n - q) for q in range(1, n + 1))


def _golay_table():
    """extended Golay(24,12): systematic cyclic (23,12) with g(x) = x^11 + x^10 + x^6 + x^5 + x^4 + x^2 + 1 (0xC75) --
    12 data bits, then the remainder of d(x) x^11 mod g(x) -- and an even overall parity bit last"""
    d = np.arange(4096, dtype=np.int64)
    rem = d << 11
    for i in range(22, 10, -1):
        rem = np.where((rem >> i) & 1, rem ^ (0xC75 << (i - 11)), rem)
    cw23 = (d << 11) | rem
    return (cw23 << 1) | (popcount(cw23) & 1)


@functools.lru_cache(None)
def code_table(fs):
    """(k, n, encoder table over all 2^k data words)"""
    if fs == FEC_H74:
        return 4, 7, _positional_hamming(7)
    if fs == FEC_H84:
        t = _positional_hamming(7)
        return 4, 8, (t << 1) | (popcount(t) & 1)
    if fs == FEC_H128:
        return 8, 12, _positional_hamming(12)
    if fs == FEC_GOLAY:
        return 12, 24, _golay_table()
    raise ValueError(fs)


def nearest_codeword(fs, r):
    """brute-force nearest codeword over all 2^k.  Ties (Hamming(8,4), (12,8)) go to the lowest data word -- the project's rule.
    Golay: the unique codeword within distance 3; a word at distance 4 from every codeword (the extended code corrects 3) is
    left as received (its data part returned) -- also the project's rule.  Returns (data words, distance)."""
    k, n, tab = code_table(fs)
    r = np.asarray(r, np.int64)
    data, dist = np.empty(len(r), np.int64), np.empty(len(r), np.int64)
    step = max(1, (1 << 21) // len(tab))
    for a in range(0, len(r), step):
        dd = popcount(r[a:a + step, None] ^ tab[None, :])
        data[a:a + step] = dd.argmin(axis=1)
        dist[a:a + step] = dd.min(axis=1)
    if fs == FEC_GOLAY:
        far = dist > 3
        data[far] = r[far] >> 12
    return data, dist


def _packed_dims(fs, n):
    k, w, _ = code_table(fs)
    nb = (8 * n + k - 1) // k
    return k, w, nb, (nb * w + 7) // 8


SECDED = {FEC_SD22: (2, 6), FEC_SD39: (4, 7), FEC_SD72: (8, 8)}     # data bytes per block, parity bits


@functools.lru_cache(None)
def secded_columns(fs):
    """Hsiao parity-check columns of the data bits (MSB of the first data byte first): odd-weight r-bit words in increasing
    order -- (22,16): the first 16 of weight 3 in 6 bits; (39,32): the first 32 of weight 3 in 7 bits; (72,64): all 56 of
    weight 3 in 8 bits, then the first 8 of weight 5.  The parity bits' own columns are the unit vectors; the block is the
    parity byte (r bits, right-aligned) followed by the data bytes."""
    nd, r = SECDED[fs]
    w = np.arange(1, 1 << r)
    cols = list(w[popcount(w) == 3])
    if fs == FEC_SD72:
        cols += list(w[popcount(w) == 5])
    return np.array(cols[:8 * nd], np.int64)


def _secded_parity(fs, data_blocks):
    cols = secded_columns(fs)
    b = np.unpackbits(np.asarray(data_blocks, np.uint8), axis=1).astype(bool)
    return np.bitwise_xor.reduce(np.where(b, cols[None, :], 0), axis=1)


# ---------------------------------------------------------------------------------------------------- Reed-Solomon RS(255,223)
# GF(2^8) with p(x) = x^8 + x^4 + x^3 + x^2 + 1 (0x11d), alpha = x; generator g(x) = prod (x - alpha^i), i = 1..32; a block is
# dl data bytes and 32 parity bytes, byte 0 the highest-order coefficient.  A message of n bytes is cut into nb = ceil(n / 223)
# blocks (at least one) of dl = ceil(n / nb) bytes, the last one zero padded (the shortening of rs_dims).
GF_EXP = [0] * 512
GF_LOG = [0] * 256
_x = 1
for _i in range(255):
    GF_EXP[_i], GF_LOG[_x] = _x, _i
    _x <<= 1
    if _x & 0x100:
        _x ^= 0x11d
for _i in range(255, 512):
    GF_EXP[_i] = GF_EXP[_i - 255]
EXP_NP, LOG_NP = np.array(GF_EXP, np.int64), np.array(GF_LOG, np.int64)


def gmul(a, b):
    return GF_EXP[GF_LOG[a] + GF_LOG[b]] if a and b else 0


def ginv(a):
    return GF_EXP[255 - GF_LOG[a]]


def gmul_np(a, b):
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    return np.where((a != 0) & (b != 0), EXP_NP[(LOG_NP[a] + LOG_NP[b]) % 255], 0)


RS_GEN = [1]                                        # coefficient list, index = power
for _i in range(1, 33):
    _g = [0] * (len(RS_GEN) + 1)
    for _j, _c in enumerate(RS_GEN):
        _g[_j + 1] ^= _c
        _g[_j] ^= gmul(_c, GF_EXP[_i])
    RS_GEN = _g


def rs_dims(n):
    nb = max(1, (n + 222) // 223)
    return nb, (n + nb - 1) // nb


def rs_encode_blocks(d):
    """systematic: parity = d(x) x^32 mod g(x), by long division one data byte at a time; d is (blocks, dl)"""
    d = np.asarray(d, np.int64)
    g = np.array(RS_GEN[::-1][1:], np.int64)         # g_31 .. g_0 (g is monic)
    rem = np.zeros((d.shape[0], 32), np.int64)       # rem[:, 0] is the x^31 coefficient
    for i in range(d.shape[1]):
        fb = d[:, i] ^ rem[:, 0]
        rem = np.concatenate([rem[:, 1:], np.zeros((d.shape[0], 1), np.int64)], axis=1) ^ gmul_np(fb[:, None], g[None, :])
    return np.concatenate([d, rem], axis=1).astype(np.uint8)


def rs_syndromes(blocks):
    """S_i = r(alpha^i), i = 1..32, for (blocks, N) bytes"""
    blocks = np.asarray(blocks, np.int64)
    N = blocks.shape[1]
    e = (np.arange(1, 33)[:, None] * (N - 1 - np.arange(N))[None, :]) % 255
    return np.bitwise_xor.reduce(gmul_np(blocks[:, None, :], EXP_NP[e][None]), axis=2)


def _gf_eliminate(M, ncols):
    """Gauss-Jordan over GF(2^8) on the first ncols columns of the rows M (in place); returns the pivot columns"""
    piv, row = [], 0
    for c in range(ncols):
        p = next((r for r in range(row, len(M)) if M[r][c]), None)
        if p is None:
            continue
        M[row], M[p] = M[p], M[row]
        iv = ginv(M[row][c])
        M[row] = [gmul(v, iv) for v in M[row]]
        for r in range(len(M)):
            if r != row and M[r][c]:
                f = M[r][c]
                M[r] = [v ^ gmul(f, w) for v, w in zip(M[r], M[row])]
        piv.append(c)
        row += 1
    return piv


def _gf_solve(A, b):
    n = len(A)
    M = [list(A[i]) + [b[i]] for i in range(n)]
    return [M[i][n] for i in range(n)] if len(_gf_eliminate(M, n)) == n else None


def rs_decode_block(r):
    """Bounded-distance decoding (radius 16) by Peterson-Gorenstein-Zierler: the number of errors nu is the rank of the
    16 x 16 syndrome matrix [S_{i+j+1}]; the locator's coefficients solve the nu x nu system
    S_{i+nu} = sum_j Lambda_j S_{i+nu-j}; the positions are the roots of Lambda among the block's locators X_j = alpha^(N-1-j)
    (exhaustive); the values solve the Vandermonde system S_i = sum_k Y_k X_k^i.  The result is accepted only if it is a
    codeword within 16 of the input; otherwise the input is returned unchanged.  Returns (block, corrected bytes, -1 for a
    give-up)."""
    r = np.asarray(r, np.uint8)
    N = len(r)
    S = [0] + [int(v) for v in rs_syndromes(r[None])[0]]        # S[1..32]
    if not any(S):
        return r.copy(), 0
    nu = len(_gf_eliminate([[S[i + j + 1] for j in range(16)] for i in range(16)], 16))
    lam = _gf_solve([[S[i + j + 1] for j in range(nu)] for i in range(nu)], [S[i + nu + 1] for i in range(nu)])
    if lam is None:
        return r.copy(), -1
    lam = np.array([1] + lam[::-1], np.int64)       # Lambda_0 = 1, Lambda_1 .. Lambda_nu
    e = np.arange(N)
    xinv_log = (255 - (N - 1 - e) % 255) % 255
    val = np.bitwise_xor.reduce(gmul_np(lam[None, :], EXP_NP[(xinv_log[:, None] * np.arange(len(lam))[None, :]) % 255]), axis=1)
    pos = [int(j) for j in np.nonzero(val == 0)[0]]
    if len(pos) != nu:
        return r.copy(), -1
    X = [GF_EXP[(N - 1 - j) % 255] for j in pos]
    Y = _gf_solve([[GF_EXP[(GF_LOG[x] * i) % 255] for x in X] for i in range(1, nu + 1)], [S[i] for i in range(1, nu + 1)])
    if Y is None:
        return r.copy(), -1
    c = r.copy()
    for j, y in zip(pos, Y):
        c[j] ^= y
    if rs_syndromes(c[None]).any() or int((c != r).sum()) > 16:
        return r.copy(), -1
    return c, int((c != r).sum())


# ---------------------------------------------------------------------------------------------------- convolutional codes
# K = 7, generators 0x6d and 0x4f on the register (newest bit = bit 0); 6 zero tail bits; puncturing per period: at each
# step, output A then B where the pattern has a 1.
CONV_POLYS = (0x6d, 0x4f)
PUNCTURE = {FEC_V27: ([1], [1]), FEC_V27P23: ([1, 1], [1, 0]), FEC_V27P34: ([1, 1, 0], [1, 0, 1]),
            FEC_V27P45: ([1, 1, 1, 1], [1, 0, 0, 0]), FEC_V27P56: ([1, 1, 0, 1, 0], [1, 0, 1, 0, 1]),
            FEC_V27P67: ([1, 1, 1, 0, 1, 0], [1, 0, 0, 1, 0, 1]), FEC_V27P78: ([1, 1, 1, 1, 0, 1, 0], [1, 0, 0, 0, 1, 0, 1])}


def _conv_mask(fs, steps):
    a, b = PUNCTURE[fs]
    c = np.arange(steps) % len(a)
    return np.stack([np.array(a)[c], np.array(b)[c]], axis=1).astype(bool)      # (steps, 2)


def conv_encode_bits(fs, msg):
    u = np.concatenate([bits_of(msg), np.zeros(6, np.uint8)]).astype(np.uint8)
    n = len(u)
    up = np.concatenate([np.zeros(6, np.uint8), u])
    out = np.zeros((n, 2), np.uint8)
    for g, poly in enumerate(CONV_POLYS):
        for k in range(7):
            if poly >> k & 1:
                out[:, g] ^= up[6 - k:6 - k + n]
    return out[_conv_mask(fs, n)]


_S = np.arange(64)
_P0, _P1 = _S >> 1, (_S >> 1) | 32                  # predecessors of state s: MSB 0 / MSB 1
_OUT = [np.array([bin(reg & p).count("1") & 1 for reg in range(128)]) for p in CONV_POLYS]
_C0 = 2 * _OUT[0][_S] + _OUT[1][_S]                 # the branch p0 -> s holds register s
_C1 = 2 * _OUT[0][_S | 64] + _OUT[1][_S | 64]       # the branch p1 -> s holds register s | 64


def viterbi(fs, vals, dec_len, vmax, spread=None):
    """Maximum-likelihood decoding of F frames of equal length at once.  vals: (F, coded bits) in [0, vmax] (hard: 0/1 with
    vmax 1; soft: 0..255 with vmax 255); expecting bit e costs e ? vmax - v : v, punctured positions cost 0.  int64 path
    metrics without normalisation; start in state 0, traceback from state 0 after 8 dec_len + 6 steps.  A tie between the two
    branches into a state goes to the predecessor whose MSB is 0.  Returns (messages (F, dec_len) uint8, final metrics (F,)).
    spread (a list) gets max(pm) - min(pm) of frame 0 after every step (meaningless before step 6: states not yet reached
    from the start state hold 2^40)."""
    vals = np.atleast_2d(np.asarray(vals, np.int64))
    F, n = vals.shape[0], 8 * dec_len + 6
    mask = _conv_mask(fs, n)
    assert vals.shape[1] >= int(mask.sum())
    pm = np.full((F, 64), 1 << 40, np.int64)
    pm[:, 0] = 0
    dec = np.zeros((n, F, 64), bool)
    pos = 0
    for t0 in range(0, n, 8192):
        m = mask[t0:t0 + 8192]
        cnt = int(m.sum())
        v = np.zeros((F, len(m), 2), np.int64)
        v[:, m] = vals[:, pos:pos + cnt]
        pos += cnt
        c0 = np.where(m[None], v, 0)                        # cost of expecting 0
        c1 = np.where(m[None], vmax - v, 0)                 # cost of expecting 1
        bm = np.stack([c0[..., 0] + c0[..., 1], c0[..., 0] + c1[..., 1], c1[..., 0] + c0[..., 1], c1[..., 0] + c1[..., 1]],
                      axis=2)                               # (F, steps, 2 a + b)
        b0 = np.ascontiguousarray(bm[:, :, _C0].transpose(1, 0, 2))
        b1 = np.ascontiguousarray(bm[:, :, _C1].transpose(1, 0, 2))
        for t in range(len(m)):
            m0 = pm[:, _P0] + b0[t]
            m1 = pm[:, _P1] + b1[t]
            d = m1 < m0
            pm = np.where(d, m1, m0)
            dec[t0 + t] = d
            if spread is not None:
                spread.append(int(pm[0].max() - pm[0].min()))
    bits = np.zeros((F, n), np.uint8)
    s = np.zeros(F, np.int64)
    fr = np.arange(F)
    for t in range(n - 1, -1, -1):
        bits[:, t] = s & 1
        s = (s >> 1) | (dec[t, fr, s].astype(np.int64) << 5)
    return np.packbits(bits[:, :8 * dec_len], axis=1), pm[:, 0]


def conv_metric(fs, msg, vals, vmax):
    """path metric of msg's codeword against received values (the costs of viterbi())"""
    c = conv_encode_bits(fs, msg).astype(np.int64)
    v = np.asarray(vals, np.int64)[:len(c)]
    return int(np.where(c == 1, vmax - v, v).sum())


# ---------------------------------------------------------------------------------------------------- FEC dispatch
def fec_enc_len(fs, n):
    if fs == FEC_NONE:
        return n
    if fs in CONV:
        return (int(_conv_mask(fs, 8 * n + 6).sum()) + 7) // 8
    if fs in (FEC_H74, FEC_H128, FEC_GOLAY):
        return _packed_dims(fs, n)[3]
    if fs == FEC_H84:
        return 2 * n
    if fs in SECDED:
        nd = SECDED[fs][0]
        return (n // nd) * (nd + 1) + (n % nd + 1 if n % nd else 0)
    if fs == FEC_RS:
        nb, dl = rs_dims(n)
        return nb * (dl + 32)
    raise ValueError(fs)


def secded_blocks(fs, enc, n):
    """the coded bytes cut into (blocks, nd + 1) SECDED blocks; the partial last block's absent data bytes are zeros"""
    nd = SECDED[fs][0]
    full, part = divmod(n, nd)
    blk = np.zeros((full + (1 if part else 0), nd + 1), np.uint8)
    blk.ravel()[:full * (nd + 1)] = enc[:full * (nd + 1)]
    if part:
        blk[full, :part + 1] = enc[full * (nd + 1):full * (nd + 1) + part + 1]
    return blk


def fec_encode(fs, msg):
    msg = np.asarray(msg, np.uint8)
    n = len(msg)
    el = fec_enc_len(fs, n)
    if fs == FEC_NONE:
        return msg.copy()
    if fs in CONV:
        return bytes_of(conv_encode_bits(fs, msg), el)
    if fs in (FEC_H74, FEC_H128, FEC_GOLAY):
        k, w, nb, _ = _packed_dims(fs, n)
        bits = np.zeros(nb * k, np.uint8)
        bits[:8 * n] = bits_of(msg)
        return bytes_of(bits_of_words(code_table(fs)[2][words_of(bits, k)], w), el)
    if fs == FEC_H84:
        tab = code_table(fs)[2]
        return np.stack([tab[msg >> 4], tab[msg & 15]], axis=1).ravel().astype(np.uint8)
    if fs in SECDED:
        nd = SECDED[fs][0]
        d = np.zeros(((n + nd - 1) // nd, nd), np.uint8)
        d.ravel()[:n] = msg
        blocks = np.concatenate([_secded_parity(fs, d)[:, None].astype(np.uint8), d], axis=1)
        keep = np.ones(blocks.shape, bool)
        if n % nd:
            keep[-1, n % nd + 1:] = False
        return blocks[keep]
    if fs == FEC_RS:
        nb, dl = rs_dims(n)
        d = np.zeros((nb, dl), np.uint8)
        d.ravel()[:n] = msg
        return rs_encode_blocks(d).ravel()
    raise ValueError(fs)


def fec_decode(fs, enc, n, stats=None):
    """hard-decision decoding of enc (fec_enc_len(fs, n) bytes) to n bytes.  stats (a dict) collects what the decoder saw:
    conv -> 'metric'; RS -> 'rs_fixed' (corrected bytes per block, -1 = give-up); block codes -> 'dist' per codeword."""
    enc = np.asarray(enc, np.uint8)
    stats = {} if stats is None else stats
    if fs == FEC_NONE:
        return enc[:n].copy()
    if fs in CONV:
        out, metric = viterbi(fs, bits_of(enc)[None], n, 1)
        stats["metric"] = int(metric[0])
        return out[0]
    if fs in (FEC_H74, FEC_H128, FEC_GOLAY):
        k, w, nb, _ = _packed_dims(fs, n)
        data, stats["dist"] = nearest_codeword(fs, words_of(bits_of(enc)[:nb * w], w))
        return bytes_of(bits_of_words(data, k)[:8 * n], n)
    if fs == FEC_H84:
        data, stats["dist"] = nearest_codeword(fs, enc[:2 * n].astype(np.int64))
        return ((data[0::2] << 4) | data[1::2]).astype(np.uint8)
    if fs in SECDED:
        blk = secded_blocks(fs, enc, n)
        d = blk[:, 1:]
        s = blk[:, 0].astype(np.int64) ^ _secded_parity(fs, d)
        # syndrome 0: clean; weight 1: a parity bit took the hit; a data bit's column: flip that bit; anything else is a
        # detected (double) error and the data stay as received
        bi, bj = np.nonzero(s[:, None] == secded_columns(fs)[None, :])
        db = np.unpackbits(d, axis=1)
        db[bi, bj] ^= 1
        return np.packbits(db, axis=1).ravel()[:n]
    if fs == FEC_RS:
        nb, dl = rs_dims(n)
        out, fixed = [], []
        for b in enc[:nb * (dl + 32)].reshape(nb, dl + 32):
            c, f = rs_decode_block(b)
            out.append(c[:dl])
            fixed.append(f)
        stats["rs_fixed"] = fixed
        return np.concatenate(out)[:n]
    raise ValueError(fs)


# ---------------------------------------------------------------------------------------------------- packet chain
def packet_dims(n, check, fec0, fec1):
    k = n + crc_len(check)
    l0 = fec_enc_len(fec0, k)
    return k, l0, fec_enc_len(fec1, l0)


def packet_encode(msg, check, fec0, fec1, trace=None):
    """payload -> channel bytes.  trace (a dict) gets each stage's codeword before its interleaver: 'cw0' (fec0's output,
    l0 bytes) and 'cw1' (fec1's output, l1 bytes)."""
    msg = np.asarray(msg, np.uint8)
    cl = crc_len(check)
    key = crc_key(check, msg)
    b = scramble(np.concatenate([msg, np.array([(key >> (8 * (cl - 1 - i))) & 0xff for i in range(cl)], np.uint8)]))
    cw0 = fec_encode(fec0, b)
    cw1 = fec_encode(fec1, interleave(cw0))
    if trace is not None:
        trace.update(cw0=cw0, cw1=cw1)
    return interleave(cw1)


def _finish(b0, n, check):
    b0 = scramble(b0)
    key = 0
    for i in range(crc_len(check)):
        key = (key << 8) | int(b0[n + i])
    return b0[:n].tobytes(), int(crc_key(check, b0[:n]) == key)


def packet_decode(pkt, n, check, fec0, fec1, trace=None):
    """hard decisions: deinterleave (l1) -> fec1 -> deinterleave (l0) -> fec0 -> descramble -> CRC.  Returns (payload bytes,
    valid).  trace gets each decoder's input ('in1', 'in0'), fec1's output ('out1') and the decoders' statistics ('st1',
    'st0')."""
    k, l0, l1 = packet_dims(n, check, fec0, fec1)
    st1, st0 = {}, {}
    in1 = interleave(np.asarray(pkt, np.uint8)[:l1], decode=True)
    out1 = fec_decode(fec1, in1, l0, st1)
    in0 = interleave(out1, decode=True)
    b0 = fec_decode(fec0, in0, k, st0)
    if trace is not None:
        trace.update(in1=in1, out1=out1, in0=in0, st1=st1, st0=st0)
    return _finish(b0, n, check)


def packet_decode_soft(soft, n, check, fec0, fec1):
    """soft values (8 l1, channel order).  The stage rule of fxr_packet_decode_soft: a convolutional stage decodes from soft
    values as long as no stage before it made hard decisions -- the stage nearest the channel (fec1), and fec0 too when fec1
    is NONE; every other stage takes hard decisions (value > 127)."""
    k, l0, l1 = packet_dims(n, check, fec0, fec1)
    v = interleave_soft(np.asarray(soft, np.uint8)[:8 * l1], l1, decode=True)
    hard = lambda s: np.packbits((np.asarray(s) > 127).astype(np.uint8))
    if fec1 == FEC_NONE:
        v0 = interleave_soft(v, l0, decode=True)
        b0 = viterbi(fec0, v0[None], k, 255)[0][0] if fec0 in CONV else fec_decode(fec0, hard(v0), k)
    else:
        b1 = viterbi(fec1, v[None], l0, 255)[0][0] if fec1 in CONV else fec_decode(fec1, hard(v), l0)
        b0 = fec_decode(fec0, interleave(b1, decode=True), k)
    return _finish(b0, n, check)
