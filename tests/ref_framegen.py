"""Float64 statement of the frame generator and of the tables every reference takes as data -- test infrastructure.

The transmit side: payload bytes and frame properties -> the samples of one flexframe at
two samples per symbol.  Written from the definitions below, sharing no code with the oracle (oracle/fxref_*.c), the host
generator (fx_codec.hpp, fx_tx.cpp) or the kernels: numpy float64 / complex128 and np.exp throughout -- no float32
arithmetic, no sin/cos table.  The packet codes, the interleaver, the CRCs and the constellations are ref_decode's; the
header's code chain is ref_header_soft.header_encode; the header's byte layout is the inverse of ref_sync.parse_header.

  m-sequence   liquid's msequence(m, g, a): a register v of m bits, started at a.  Each step emits
               b = parity(v AND (g >> 1)) and shifts it in at the bottom: v = ((v << 1) | b) mod 2^m (Fibonacci form; g is
               the generator polynomial with its constant term, which the shift drops).
  preamble     msequence(7, 0x0089, 1) (the reference project's call site, frame_detector_cc_impl.cc:47-51): 64 symbols,
               two sequence bits each, the first the real part, the second the imaginary part, bit 1 -> +sqrt(1/2),
               bit 0 -> -sqrt(1/2).
  pilots       msequence(4, 0x13, 1) (liquid's default polynomial for m = 4, what qpilotgen takes for 15 pilots): 15 words
               of two bits, the first bit the word's MSB.  CONVENTION (liquid's qpilotgen): word s sits at phase
               pi/4 + s pi/2, i.e. 0 -> (+, +), 1 -> (-, +), 2 -> (-, -), 3 -> (+, -), each component +-sqrt(1/2).
  pulse        liquid_firdes_arkaiser(k, m, beta, dt), n = 2 k m + 1 taps:
                   rho = c0 + c1 ln(beta) + c2 ln(beta)^2,  c0 = 0.762886 + 0.067663 ln(m),  c1 = 0.065515,
                   c2 = ln(1 - 0.088 m^-1.6)                                      (the published fit of the r-Kaiser rho)
                   transition width  del = beta rho / k;   cut-off  fc = (1 + beta (1 - rho)) / (2 k)
                   stop band  As = 14.26 del n + 7.95      (Kaiser's length estimate n = (As - 7.95) / (14.26 del), solved)
                   Kaiser beta_w = 0.1102 (As - 8.7) for As > 50,  0.5842 (As - 21)^0.4 + 0.07886 (As - 21) for As > 21
                   t_i = i - (n - 1) / 2 + dt;   h_i = sinc(2 fc t_i) I0(beta_w sqrt(1 - (2 t_i / n)^2)) / I0(beta_w)
                   scaled to sum h^2 = k.
               beta and dt are float32 arguments in liquid's interface: their values are taken exactly as those float32
               values (beta = float32(0.3) = 0.300000011920929, not 0.3; a conversion, no float32 arithmetic).
               TX pulse: k = 2, m = 7 (29 taps).  Receive prototype: k = 64 (32 branches x 2), m = 7 (897 taps), dt = 0.
  equaliser    eqlms_create_lowpass(13, fc = 0.4): h_i = 2 fc sinc(2 fc t_i) w_i, the Kaiser window at As = 40 dB.
  header       20 bytes: 14 user bytes, then protocol (102), payload length high, low, modulation, check << 5 | fec0, fec1
               (compose_header).  CRC-32, SECDED(72,64), Hamming(8,4): 54 bytes = 216 two-bit words, MSB first; word w is the
               QPSK point of ref_decode.constellation(QPSK) (bit 1 of the word: imaginary part negative; bit 0: real part
               negative).  231 header symbols: a pilot at every 16th position (0, 16, ..., 224), the words in between.
  payload      ref_decode.packet_encode -> bits, MSB first, in words of bps bits (the last word padded with zero bits at
               its low end) -> the point whose label is the word.  Differential PSK: the word is gray(d), the phase index
               is the running sum of the d's modulo M from 0 at the payload's first symbol, the point exp(2 pi j index / M).
  frame        symbols x: 64 p/n, 231 header, npay payload, 14 zeros (2 m, the pulse's flush).  Samples
               y[2 n + i] = sum_t h[i + 2 t] x[n - t], i = 0, 1, t = 0..14: the zero-stuffed symbols through the 29 taps,
               cut to 2 nsym samples.  CONVENTION: dt enters t_i with a plus sign, so the pulse's peak sits at
               i = 14 - dt: a positive dt ADVANCES the frame by dt samples (the receiver reports tau ~ -dt).

Negative controls (keyword arguments of frame(); their defaults are the definition): dpsk_restart (the DPSK sum starts again
at that payload symbol), pilot_shift (pilots one position late), dt_sign (-1: dt negated), tap_shift (the taps one sample
late), qam32_split ((2, 3): QAM32 as a 4 x 8 rectangle), lsb_first (payload words filled from their low end).

Tolerance against a float32 generator (the oracle, the host generator, the kernels).  u = 2^-24 = 6e-8.
  Every output component is a chain of at most 15 fused multiply-adds of a float32 tap and a float32 point component:
  15 roundings of the running sum, the tap's rounding (u / 2 relative) and the point's (u: the 1024-entry sin/cos table's
  entry, or a level times a rounded scale constant) -- at most (15 + 2) u relative to sum_t |h[i + 2 t]| |x[n - t]|, and
  |x| is at most CORNER = 1.53 (64-QAM's corner) on either component:
      sample_tol(dt) = (15 + 2) u  max_i sum_t |h[i + 2 t]|  CORNER         with h this module's own taps for that dt.
  dt = 0: the tap sums of the two phases are 1.41 and 1.92 -> 2.97e-6, the largest over the delays tests/framegen_cases.py
  uses; the smallest is 2.63e-6 (dt = +-0.5: 1.70 and 1.70).  A wrong symbol index moves a sample by 0.1 or more, five
  orders above this.
  Table entries against float32 tables: at most 1 float32 ulp of the entry (two correctly written float64 designs may round
  differently); p/n symbols and pilots: exactly the float32 neighbours of +-sqrt(1/2).

Measured: see MEASURED below, kept next to the bound it must stay 4x under.
"""
import math

import numpy as np

import ref_decode as R
import ref_header_soft as RH
import ref_sync as RS

U = 2.0 ** -24
K = 2                                   # samples per symbol
M_SPAN = 7                              # pulse half-length in symbols
BETA = float(np.float32(0.3))           # the excess bandwidth, as the float32 argument liquid's interface takes
NPFB = 32
PN_LEN, HDR_SYM, HDR_MOD, PILOT_SPACING, N_PILOTS = 64, 231, 216, 16, 15
FLUSH = 2 * M_SPAN
PROTOCOL = 102
CORNER = 7.0 * math.sqrt(2.0 / 42.0)
DTS = (0.0, 0.5, -0.5, 1e-3, -0.37, float(np.float32(1.0 / 3.0)))      # the delays of tests/framegen_cases.py

# worst |reference - implementation| over tests/framegen_cases.py's frames, per component: against the oracle (CPU,
# tests/test_ref_framegen.py) and against fx_txenc_kernel / fx_txgen_kernel (MI355X, tests/test_gpu_ref_framegen.py).
# min over DTS of sample_tol(dt) must stay >= 4x both.
MEASURED = dict(oracle=5.7e-7, gpu=5.7e-7)


# ---------------------------------------------------------------------------------------------------- sequences
def msequence(m, g, a, n):
    """The first n output bits of liquid's msequence(m, g, a)."""
    taps, mask, v = g >> 1, (1 << m) - 1, a
    out = np.empty(n, np.int64)
    for i in range(n):
        b = bin(v & taps).count("1") & 1
        v = ((v << 1) | b) & mask
        out[i] = b
    return out


def preamble():
    b = msequence(7, 0x0089, 1, 2 * PN_LEN).astype(np.float64)
    return ((2.0 * b[0::2] - 1.0) + 1j * (2.0 * b[1::2] - 1.0)) * math.sqrt(0.5)


def pilots():
    """CONVENTION (liquid's qpilotgen): the two-bit word s, first bit its MSB, sits at phase pi/4 + s pi/2 --
    0 -> (+, +), 1 -> (-, +), 2 -> (-, -), 3 -> (+, -)."""
    b = msequence(4, 0x13, 1, 2 * N_PILOTS)
    s = 2 * b[0::2] + b[1::2]
    re = np.where((s == 0) | (s == 3), 1.0, -1.0)
    im = np.where(s < 2, 1.0, -1.0)
    return (re + 1j * im) * math.sqrt(0.5)


# ---------------------------------------------------------------------------------------------------- filter designs
def _i0(z):
    """Modified Bessel function of the first kind, order 0, by its series sum_k ((z / 2)^k / k!)^2."""
    z = np.asarray(z, np.float64)
    term, total = np.ones_like(z), np.ones_like(z)
    for k in range(1, 200):
        term = term * (0.5 * z / k) ** 2
        total = total + term
        if np.all(term <= 1e-20 * total):
            break
    return total


def _sinc(x):
    x = np.asarray(x, np.float64)
    safe = np.where(x == 0.0, 1.0, x)
    return np.where(x == 0.0, 1.0, np.sin(np.pi * safe) / (np.pi * safe))


def kaiser_beta(As):
    As = abs(As)
    if As > 50.0:
        return 0.1102 * (As - 8.7)
    if As > 21.0:
        return 0.5842 * (As - 21.0) ** 0.4 + 0.07886 * (As - 21.0)
    return 0.0


def _kaiser_sinc(n, fc, As, dt):
    t = np.arange(n, dtype=np.float64) - 0.5 * (n - 1) + dt
    bw = kaiser_beta(As)
    r = 2.0 * t / n
    return _sinc(2.0 * fc * t) * _i0(bw * np.sqrt(np.maximum(0.0, 1.0 - r * r))) / _i0(bw)


def arkaiser(k, m, beta, dt=0.0):
    """liquid_firdes_arkaiser: 2 k m + 1 float64 taps.  beta and dt are used as given: pass the float32 values' floats."""
    beta, dt = float(beta), float(dt)
    lb = math.log(beta)
    rho = 0.762886 + 0.067663 * math.log(m) + 0.065515 * lb + math.log(1.0 - 0.088 * float(m) ** -1.6) * lb * lb
    assert 0.0 < rho < 1.0
    n = 2 * k * m + 1
    As = 14.26 * (beta * rho / k) * n + 7.95
    fc = 0.5 * (1.0 + beta * (1.0 - rho)) / k
    h = _kaiser_sinc(n, fc, As, dt)
    return h * math.sqrt(k / float(np.sum(h * h)))


def tx_taps(dt=0.0):
    """The 29-tap transmit pulse for a delay given as (or rounded once to) a float32 value."""
    return arkaiser(K, M_SPAN, BETA, float(np.float32(dt)))


def mf_proto():
    return arkaiser(NPFB * K, M_SPAN, BETA, 0.0)


def eq_init():
    fc = 0.4
    return 2.0 * fc * _kaiser_sinc(RS.EQ_TAPS, fc, 40.0, 0.0)


def tables():
    """ref_sync.Tables from the definitions above: no oracle."""
    return RS.Tables(preamble(), pilots(), mf_proto(), eq_init())


def sample_tol(dt=0.0):
    h = np.abs(tx_taps(dt))
    return (15 + 2) * U * max(float(h[0::2].sum()), float(h[1::2].sum())) * CORNER


# ---------------------------------------------------------------------------------------------------- header
def compose_header(user14, payload_len, mod, check, fec0, fec1):
    """The 20 header bytes: the inverse of ref_sync.parse_header."""
    user = np.zeros(14, np.uint8) if user14 is None else np.asarray(user14, np.uint8)
    assert len(user) == 14 and 0 <= payload_len < 65536
    return np.concatenate([user, np.array([PROTOCOL, payload_len >> 8, payload_len & 0xff, mod, ((check & 7) << 5) | (fec0 & 31),
                                           fec1 & 31], np.uint8)])


def _points_of_labels(ms, words, pts_lab=None):
    pts, lab = R.constellation(ms) if pts_lab is None else pts_lab
    by_label = np.empty(len(pts), np.complex128)
    by_label[np.asarray(lab)] = pts
    return by_label[words]


def header_symbols(hdr20, pilot_shift=0):
    enc = RH.header_encode(hdr20)
    data = _points_of_labels(R.QPSK, R.words_of(R.bits_of(enc), 2))
    assert len(data) == HDR_MOD
    i = np.arange(HDR_SYM)
    is_pilot = (i % PILOT_SPACING) == pilot_shift
    out = np.empty(HDR_SYM, np.complex128)
    out[is_pilot] = pilots()[:int(is_pilot.sum())]
    out[~is_pilot] = data[:int((~is_pilot).sum())]
    return out


# ---------------------------------------------------------------------------------------------------- payload
def _qam_rect(mi, mq):
    """(points, labels) of a 2^mi x 2^mq rectangle by ref_decode.constellation's formula (for the qam32_split control)."""
    Li, Lq = 1 << mi, 1 << mq
    ii, iq = np.meshgrid(np.arange(Li), np.arange(Lq), indexing="ij")
    li, lq = 2.0 * ii - (Li - 1), 2.0 * iq - (Lq - 1)
    alpha = 1.0 / math.sqrt(float((li ** 2 + lq ** 2).mean()))
    return (alpha * (li + 1j * lq)).ravel(), ((R.gray(ii) << mq) | R.gray(iq)).ravel()


def payload_words(enc, bps, lsb_first=False):
    bits = R.bits_of(enc)
    nsym = (len(bits) + bps - 1) // bps
    padded = np.zeros(nsym * bps, np.uint8)
    padded[:len(bits)] = bits
    if lsb_first:
        padded = padded.reshape(-1, bps)[:, ::-1].ravel()
    return R.words_of(padded, bps) if nsym else np.zeros(0, np.int64)


def payload_points(payload, mod, check, fec0, fec1, dpsk_restart=None, qam32_split=(3, 2), lsb_first=False):
    enc = R.packet_encode(np.asarray(payload, np.uint8), check, fec0, fec1)
    words = payload_words(enc, R.bps(mod), lsb_first)
    if mod in R.DPSK:
        Mo = 1 << R.bps(mod)
        lab = np.asarray(R.constellation(mod)[1])
        step_of_word = np.empty(Mo, np.int64)
        step_of_word[lab] = np.arange(Mo)                         # word = gray(d)  ->  d
        d = step_of_word[words]
        if dpsk_restart is None:
            index = np.cumsum(d) % Mo
        else:
            index = np.concatenate([np.cumsum(d[:dpsk_restart]), np.cumsum(d[dpsk_restart:])]) % Mo
        return np.exp(2j * np.pi * index / Mo)
    if mod == R.QAM32 and tuple(qam32_split) != (3, 2):
        return _points_of_labels(mod, words, _qam_rect(*qam32_split))
    return _points_of_labels(mod, words)


# ---------------------------------------------------------------------------------------------------- frame
def num_payload_symbols(n, mod, fec0, fec1, check):
    return R.num_symbols(mod, R.packet_dims(n, check, fec0, fec1)[2])


def frame_len(n, mod, fec0, fec1, check):
    return K * (PN_LEN + HDR_SYM + num_payload_symbols(n, mod, fec0, fec1, check) + FLUSH)


def frame_symbols(payload, mod, fec0, fec1, check, header=None, pilot_shift=0, hdr20=None, points=None, **payload_controls):
    """hdr20: all 20 header bytes as given (the six protocol bytes are then NOT derived from the payload's properties: a test
    can state a header no generator would build); the payload symbols are still those of (payload, mod, fec0, fec1, check),
    stated separately, or `points` when given explicitly."""
    payload = np.asarray(payload, np.uint8)
    if hdr20 is None:
        hdr = compose_header(header, len(payload), mod, check, fec0, fec1)
    else:
        assert header is None
        hdr = np.asarray(hdr20, np.uint8)
        assert len(hdr) == RS.HDR_DEC
    pts = payload_points(payload, mod, check, fec0, fec1, **payload_controls) if points is None else np.asarray(points, np.complex128)
    return np.concatenate([preamble(), header_symbols(hdr, pilot_shift), pts, np.zeros(FLUSH, np.complex128)])


def frame(payload, mod, fec0, fec1, check, header=None, dt=0.0, dt_sign=1, tap_shift=0, hdr20=None, **symbol_controls):
    """The frame's samples, complex128.  dt: the delay, rounded once to the float32 the generators take."""
    x = frame_symbols(payload, mod, fec0, fec1, check, header, hdr20=hdr20, **symbol_controls)
    h = tx_taps(dt_sign * float(np.float32(dt)))
    if tap_shift:
        h = np.concatenate([np.zeros(tap_shift), h[:len(h) - tap_shift]])
    up = np.zeros(K * len(x), np.complex128)
    up[::K] = x
    return np.convolve(up, h)[:K * len(x)]


def compare(ref, got):
    """The worst absolute error of a sample's component; inf when the lengths differ."""
    got = np.asarray(got, np.complex128)
    if len(ref) != len(got):
        return float("inf")
    if not len(ref):
        return 0.0
    d = got - ref
    return float(max(np.abs(d.real).max(), np.abs(d.imag).max()))
