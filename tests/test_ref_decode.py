"""The numpy reference of the decode stage (tests/ref_decode.py) pinned against the CPU oracle and the product's host
generator, at the edges where decoders go wrong: every error pattern a block code must correct and the first ones it must not,
Reed-Solomon at 0..24 byte errors per block, maximum-likelihood Viterbi at 0-15 % channel errors, decision regions over the
whole plane.  No GPU.  The GPU decode path is compared with the same reference in test_gpu_ref_decode.py."""
import ctypes as C
import itertools

import numpy as np
import pytest

import ref_decode as R

LENGTHS = list(range(0, 301)) + [446, 447, 1000]


@pytest.fixture(scope="module")
def L(oracle):
    L = oracle.lib()
    L.fxr_packet_decode_soft.restype = C.c_int
    L.fxr_packet_decode_soft.argtypes = [C.c_uint, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.fxr_scramble.argtypes = [C.c_void_p, C.c_uint]
    return L


def o_encode(L, fs, msg):
    msg = np.ascontiguousarray(msg, np.uint8)
    el = L.fxr_fec_enc_len(fs, len(msg))
    out = np.zeros(el + 8, np.uint8)
    L.fxr_fec_encode(fs, len(msg), msg.ctypes.data, out.ctypes.data)
    return out[:el]


def o_decode(L, fs, enc, n):
    enc = np.ascontiguousarray(np.concatenate([enc, np.zeros(8, np.uint8)]), np.uint8)
    out = np.zeros(n + 8, np.uint8)
    L.fxr_fec_decode(fs, n, enc.ctypes.data, out.ctypes.data)
    return out[:n]


# ---------------------------------------------------------------------------------------------------- encoders
@pytest.mark.parametrize("fs", R.ALL_FEC)
def test_encoders_match_oracle(L, fs):
    rng = np.random.default_rng(fs)
    for n in LENGTHS:
        msg = rng.integers(0, 256, n, dtype=np.uint8)
        assert R.fec_enc_len(fs, n) == L.fxr_fec_enc_len(fs, n), n
        assert np.array_equal(R.fec_encode(fs, msg), o_encode(L, fs, msg)), n


def test_packet_encoder_matches_oracle(L):
    rng = np.random.default_rng(7)
    for n in list(range(0, 40)) + [221, 222, 223, 297, 298, 299, 446, 447]:
        for check, fec0, fec1 in ((R.CRC_24, R.FEC_V27, R.FEC_NONE), (R.CRC_32, R.FEC_RS, R.FEC_V27P23),
                                  (R.CRC_8, R.FEC_GOLAY, R.FEC_SD39), (R.CRC_16, R.FEC_V27P78, R.FEC_H128),
                                  (R.CRC_CHECKSUM, R.FEC_SD72, R.FEC_H74), (R.CRC_NONE, R.FEC_H84, R.FEC_RS)):
            msg = rng.integers(0, 256, n, dtype=np.uint8)
            el = L.fxr_packet_enc_len(n, check, fec0, fec1)
            assert el == R.packet_dims(n, check, fec0, fec1)[2]
            out = np.zeros(el + 8, np.uint8)
            L.fxr_packet_encode(n, check, fec0, fec1, msg.ctypes.data, out.ctypes.data)
            assert np.array_equal(R.packet_encode(msg, check, fec0, fec1), out[:el]), (n, check, fec0, fec1)


@pytest.mark.parametrize("fs", R.ALL_FEC)
def test_encoders_match_product_generator(fx, oracle, fs):
    """the product's host generator (flexframegen_*) on a clean channel: the oracle receiver's carrier-recovered payload
    symbols, demapped by the reference, are the reference encoder's channel bytes for the payload, bit for bit"""
    from parity_util import oracle_frames
    rng = np.random.default_rng(100 + fs)
    mod = R.QAM16 if fs % 2 else R.PSK8
    for n in (0, 1, 2, 3, 7, 31, 222, 223, 224, 300):
        g = fx.FrameGen(mod, fs, R.FEC_NONE if fs != R.FEC_V27 else R.FEC_H84, R.CRC_24)
        msg = rng.integers(0, 256, n, dtype=np.uint8)
        x = np.concatenate([np.zeros(300, np.complex64), g.frame(msg), np.zeros(600, np.complex64)])
        g.close()
        (f,) = oracle_frames(oracle, x)
        assert f.header_valid and f.payload_valid and f.payload == msg.tobytes()
        k, l0, l1 = R.packet_dims(n, f.check, f.fec0, f.fec1)
        lab, margin = R.demap_hard(f.mod_scheme, f.framesyms)
        assert len(margin) == 0 or margin.min() > 0.1
        assert np.array_equal(R.symbols_to_bytes(f.mod_scheme, lab, l1), R.packet_encode(msg, f.check, f.fec0, f.fec1)), n


# ---------------------------------------------------------------------------------------------------- interleaver, scrambler, CRC
def test_interleaver_and_scrambler_match_oracle(L):
    rng = np.random.default_rng(3)
    for n in list(range(0, 700)) + [1023, 1024, 2056, 4099, 8224, 131078]:
        x = rng.integers(0, 256, n, dtype=np.uint8)
        for decode in (0, 1):
            y = x.copy()
            L.fxr_interleave(y.ctypes.data, n, decode)
            assert np.array_equal(R.interleave(x, bool(decode)), y), (n, decode)
        assert np.array_equal(R.interleave(R.interleave(x), True), x)
        soft = rng.integers(0, 256, 8 * n, dtype=np.uint8)
        assert np.array_equal(R.interleave_soft(R.interleave_soft(soft, n), n, True), soft)
        if n < 300:
            z = x.copy()
            L.fxr_scramble(z.ctypes.data, n)
            assert np.array_equal(R.scramble(x), z)
    # the soft permutation is the hard one, bit for bit
    x = rng.integers(0, 256, 333, dtype=np.uint8)
    assert np.array_equal(np.packbits(R.interleave_soft(np.unpackbits(x), 333)), R.interleave(x))


def test_crc_check_values(L):
    s = np.frombuffer(b"123456789", np.uint8).copy()
    want = {R.CRC_CHECKSUM: 0x23, R.CRC_8: 0x2f, R.CRC_16: 0xb4c8, R.CRC_24: 0x2f27ee, R.CRC_32: 0xcbf43926}
    for check, v in want.items():
        assert R.crc_key(check, s) == v == L.fxr_crc_key(check, s.ctypes.data, 9), check
    rng = np.random.default_rng(4)
    for n in (0, 1, 2, 3, 5, 64, 257):
        m = rng.integers(0, 256, n, dtype=np.uint8)
        for check in want:
            assert R.crc_key(check, m) == L.fxr_crc_key(check, m.ctypes.data, n)


# ---------------------------------------------------------------------------------------------------- modems
class Modem(C.Structure):
    _fields_ = [("ms", C.c_int), ("bps", C.c_uint), ("dpsk_phi", C.c_float)]


@pytest.mark.parametrize("ms", R.PAYLOAD_MODS + (R.QPSK,))
def test_demappers_match_oracle_over_the_plane(L, oracle, ms):
    """hard decisions equal fxr_modem_demod on random points out to 1.5x the outermost point (symbols within the tie margin
    skipped, and for DPSK the next symbol too); soft bytes within 1 of fxr_modem_demod_soft, equal away from rounding ties"""
    L.fxr_modem_init.argtypes = [C.POINTER(Modem), C.c_int]
    L.fxr_modem_demod.restype = C.c_uint
    L.fxr_modem_demod.argtypes = [C.POINTER(Modem), oracle.C32, C.POINTER(oracle.C32), C.POINTER(C.c_float)]
    rng = np.random.default_rng(ms)
    pts, _ = R.constellation(ms)
    rad = 1.5 * np.abs(pts).max()
    N = 6000
    r = (rng.uniform(-rad, rad, N) + 1j * rng.uniform(-rad, rad, N)).astype(np.complex64)
    r[:200] = (pts[rng.integers(0, len(pts), 200)] * rng.uniform(0.0, 1.5, 200)).astype(np.complex64)    # on the rays too
    lab, margin = R.demap_hard(ms, r)
    q = Modem()
    L.fxr_modem_init(C.byref(q), ms)
    got = np.array([L.fxr_modem_demod(C.byref(q), oracle.C32(float(v.real), float(v.imag)), None, None) for v in r])
    ok = margin >= 1e-5
    if ms in R.DPSK:
        ok[1:] &= ok[:-1].copy()
    assert ok.mean() > 0.99
    assert np.array_equal(got[ok], lab[ok]), np.nonzero((got != lab) & ok)[0][:5]
    # soft
    k = R.bps(ms)
    soft = R.demap_soft(ms, r, lab)
    gamma16 = 16.0 * 1.2 * (1 << k)
    exact = np.ones(soft.shape, bool)
    if ms not in R.DPSK:
        d2 = np.abs(r.astype(np.complex128)[:, None] - pts[None, :]) ** 2
        labs = R.constellation(ms)[1]
        for b in range(k):
            one = ((labs >> (k - 1 - b)) & 1).astype(bool)
            v = 127.0 + gamma16 * (d2[:, ~one].min(axis=1) - d2[:, one].min(axis=1))
            exact[:, b] = np.abs(v - np.floor(v) - 0.5) > 0.01
    buf = np.zeros(8, np.uint8)
    for i in np.nonzero(ok)[0]:
        L.fxr_modem_demod_soft(ms, oracle.C32(float(r[i].real), float(r[i].imag)), int(got[i]), buf.ctypes.data)
        d = np.abs(buf[:k].astype(int) - soft[i].astype(int))
        assert d.max() <= 1 and not (d[exact[i]] != 0).any(), (i, r[i], buf[:k], soft[i])


# ---------------------------------------------------------------------------------------------------- block codes
def _packed_stream(fs, words):
    """a coded stream holding the given received words back to back, and its message length"""
    k, w, _ = R.code_table(fs)
    n = len(words) * k // 8
    assert len(words) * k % 8 == 0
    return R.bytes_of(R.bits_of_words(words, w), R.fec_enc_len(fs, n)), n


def test_golay_all_patterns_up_to_weight_3_and_every_weight_4(L):
    rng = np.random.default_rng(24)
    tab = R.code_table(R.FEC_GOLAY)[2]
    pats = [0] + [sum(1 << b for b in c) for w in (1, 2, 3) for c in itertools.combinations(range(24), w)]
    assert len(pats) == 2325
    for _ in range(16):
        d = int(rng.integers(0, 4096))
        words = tab[d] ^ np.array(pats + pats[:1], np.int64)               # (an even count of words: whole bytes)
        enc, n = _packed_stream(R.FEC_GOLAY, words)
        want = R.bytes_of(R.bits_of_words(np.full(len(words), d), 12), n)
        assert np.array_equal(R.fec_decode(R.FEC_GOLAY, enc, n), want)
        assert np.array_equal(o_decode(L, R.FEC_GOLAY, enc, n), want)
    p4 = np.array([sum(1 << b for b in c) for c in itertools.combinations(range(24), 4)], np.int64)
    assert len(p4) == 10626
    words = tab[0x5a3] ^ p4
    enc, n = _packed_stream(R.FEC_GOLAY, words)
    ref = R.fec_decode(R.FEC_GOLAY, enc, n)
    assert np.array_equal(ref, R.bytes_of(R.bits_of_words(words >> 12, 12), n))      # detected, left as received
    assert np.array_equal(o_decode(L, R.FEC_GOLAY, enc, n), ref)


@pytest.mark.parametrize("fs", [R.FEC_H74, R.FEC_H84, R.FEC_H128])
def test_hamming_every_received_word(L, fs):
    k, w, tab = R.code_table(fs)
    words = np.arange(1 << w, dtype=np.int64)
    if fs == R.FEC_H84:
        enc, n = words.astype(np.uint8), len(words) // 2
    else:
        enc, n = _packed_stream(fs, words)
    ref = R.fec_decode(fs, enc, n)
    assert np.array_equal(o_decode(L, fs, enc, n), ref)
    data, dist = R.nearest_codeword(fs, words)
    assert (dist <= 1).all() if fs == R.FEC_H74 else (dist <= 2).all()
    assert np.array_equal(tab[np.arange(1 << k)] ^ 0, tab) and len(set(tab.tolist())) == 1 << k
    # single errors are corrected
    for d in range(0, 1 << k, 7):
        for b in range(w):
            assert R.nearest_codeword(fs, [tab[d] ^ (1 << b)])[0][0] == d


@pytest.mark.parametrize("fs", [R.FEC_SD22, R.FEC_SD39, R.FEC_SD72])
def test_secded_all_single_and_double_errors(L, fs):
    nd = R.SECDED[fs][0]
    rng = np.random.default_rng(fs)
    for n in (nd, 3 * nd) + tuple(range(1, nd)):                      # whole blocks, then a lone partial block of every size
        part = n % nd if n % nd else nd
        msg = rng.integers(0, 256, n, dtype=np.uint8)
        enc = R.fec_encode(fs, msg)
        nbits = 8 * (part + 1)
        off = 8 * (len(enc) - part - 1)                               # the last block's bits
        for w in (1, 2):
            for c in itertools.combinations(range(nbits), w):
                bad = R.bits_of(enc)
                for b in c:
                    bad[off + b] ^= 1
                bad = np.packbits(bad)
                ref = R.fec_decode(fs, bad, n)
                if w == 1:
                    assert np.array_equal(ref, msg), c
                else:
                    assert np.array_equal(ref[n - part:], bad[len(enc) - part:]), c           # detected: data as received
                assert np.array_equal(o_decode(L, fs, bad, n), ref), (n, c)


@pytest.mark.parametrize("n", [1, 2, 31, 222, 223, 224, 300, 446, 447, 1000])
def test_reed_solomon_up_to_24_byte_errors(L, n):
    rng = np.random.default_rng(n)
    nb, dl = R.rs_dims(n)
    msg = rng.integers(0, 256, n, dtype=np.uint8)
    enc = R.fec_encode(R.FEC_RS, msg)
    for e in range(0, 25):
        bad = enc.copy().reshape(nb, dl + 32)
        for b in range(nb):
            pos = rng.choice(dl + 32, min(e, dl + 32), replace=False)
            bad[b, pos] ^= rng.integers(1, 256, len(pos)).astype(np.uint8)
        bad = bad.ravel()
        ref = R.fec_decode(R.FEC_RS, bad, n)
        if e <= 16:
            assert np.array_equal(ref, msg), e
        else:                                           # unchanged, or the codeword within 16 of what was received
            for b in range(nb):
                blk, fixed = R.rs_decode_block(bad[b * (dl + 32):(b + 1) * (dl + 32)])
                assert fixed == -1 or (fixed <= 16 and not R.rs_syndromes(blk[None]).any())
        assert np.array_equal(o_decode(L, R.FEC_RS, bad, n), ref), (n, e)


# ---------------------------------------------------------------------------------------------------- Viterbi
VIT_LENGTHS = list(range(1, 41)) + list(range(47, 301, 23)) + [300]


@pytest.mark.parametrize("fs", R.CONV)
def test_viterbi_hard_and_soft_maximum_likelihood(L, fs):
    """the reference Viterbi equals fxr_fec_decode (hard) and fxr_packet_decode_soft (soft) exactly at 0-15 % channel
    errors, and its output is a maximum-likelihood path: metric(decoded) = the final metric <= metric(true message)"""
    rng = np.random.default_rng(fs)
    bers = (0.0, 0.02, 0.06, 0.15)
    for n in VIT_LENGTHS:
        msgs = rng.integers(0, 256, (len(bers), n), dtype=np.uint8)
        code = np.stack([R.conv_encode_bits(fs, m) for m in msgs])
        nbits = code.shape[1]
        flips = rng.random(code.shape) < np.array(bers)[:, None]
        hard = code ^ flips
        dec, metric = R.viterbi(fs, hard, n, 1)
        el = R.fec_enc_len(fs, n)
        for i in range(len(bers)):
            assert np.array_equal(o_decode(L, fs, R.bytes_of(hard[i], el), n), dec[i]), (n, bers[i])
            assert R.conv_metric(fs, dec[i], hard[i], 1) == metric[i] <= R.conv_metric(fs, msgs[i], hard[i], 1)
        # soft: values biased toward the codeword, some crossing over
        soft = np.clip(np.where(code == 1, 200, 55) + rng.normal(0, 1, code.shape) * np.array([10, 60, 90, 120])[:, None],
                       0, 255).astype(np.int64)
        sdec, smetric = R.viterbi(fs, soft, n, 255)
        for i in range(len(bers)):
            assert R.conv_metric(fs, sdec[i], soft[i], 255) == smetric[i] <= R.conv_metric(fs, msgs[i], soft[i], 255)
            # the oracle's soft decoder, through its packet decoder (no CRC, no outer code: the values go through both
            # interleavers first, the output comes descrambled)
            ch = np.zeros(8 * el, np.uint8)
            ch[:nbits] = soft[i]
            ch = R.interleave_soft(R.interleave_soft(ch, el), el)
            out = np.zeros(n + 8, np.uint8)
            clobbered = ch.copy()
            L.fxr_packet_decode_soft(n, R.CRC_NONE, fs, R.FEC_NONE, clobbered.ctypes.data, out.ctypes.data)
            assert np.array_equal(out[:n], R.scramble(sdec[i])), (n, i)
            assert R.packet_decode_soft(ch, n, R.CRC_NONE, fs, R.FEC_NONE)[0] == R.scramble(sdec[i]).tobytes()
