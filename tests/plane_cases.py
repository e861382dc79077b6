"""Payload symbols all over the plane: one list of frames whose payload symbols are arbitrary complex points, not coded
packets, so that the receiver's demappers -- the hard decision, the decided point and the per-bit soft values -- are
judged far from the constellation, where noisy traffic never goes.  tests/test_ref_plane.py proves (no GPU) that each frame is
what it says and that the numpy reference and the oracle agree on it; tests/test_gpu_plane.py puts the same streams through the
library, hard, soft, equalised and as a continuing stream.

Every frame states CRC_NONE, FEC_NONE / FEC_NONE (l1 = n: the payload bytes are a bijection of the hard labels, a single
wrong label shows in the payload), dt = 0, and is built by ref_framegen.frame_symbols(points=...): preamble and header are
ordinary.  Each of the 11 payload schemes gets three frames, back to back in one stream (gaps of 300 samples and more):
    plane   about 1535 symbols -- two work items of fx_softdemod_kernel, the second a partial one: 64 settling constellation
            points, 200 points on the rays through constellation points at radius 0 .. 1.5, the rest uniform on the square
            of half-width 1.5 x the outermost point.  For bps 3, 5 and 6 the length n makes 8 n no multiple of bps: the last
            symbol is padded (PLANE_N).
    far     256 symbols (64-QAM: 352, its list does not fit into 256): 64 settling points, then every constellation point
            times 2, 4 and 8 and, for the grid schemes, points one coordinate of which lies 2, 4 and 8 level spacings
            beyond the outermost level, on either side, while the other sweeps the levels; filled up with more scaled
            points.  Points come in conjugate pairs, whose phase errors cancel in the loop.  FAR_FACTORS records the factors
            per scheme: (2, 4, 8) everywhere, none had to be lowered.
    tiny    1 payload byte: 8, 4, 3, 2, 2, 2 symbols for bps 1 .. 6, uniform on the same square.
33 frames, 19 844 payload symbols, 11 streams of 7 569 samples (zeros behind the shorter ones, to one length).

guard_streams() are a separate handful for one property of fx_softdemod_kernel, see there.

The tie rule.  A symbol is a tie when its ref_decode.demap_hard margin (distance to the runner-up point minus distance to
the nearest) is below the scheme's value in test_gpu_ref_decode.TIE / TIE_GRID -- imported, not copied.  For the differential
schemes the symbol after a tie is a tie as well (its label is a difference).  Ties are left out of the label comparison
only: soft values, symbol counts and the decided point's error sum are compared on every symbol (the error sum with the
allowance a tie can make, see test_gpu_plane.py).

Measured (the oracle receiver on the CPU; an MI355X gives the same symbols bit for bit, test_gpu_plane.py asserts it):
    ties per scheme (of all payload symbols): MEASURED_TIES -- none but one of 64-QAM's 1889 symbols (0.05 %; twice an inner
        point lies on a decision boundary), against the cap of 0.5 %
    far factor used: 8 for every scheme -- the oracle keeps every frame and header
    received |r|: 0.0014 .. 12.2 (64-QAM's corner times 8; PSK 8.0)
    worst |evm_sum - float64 sum| / derived bound (test_gpu_plane.evm_bound) on an MI355X: MEASURED_EVM_RATIO, 64-QAM's far frame

Everything here is deterministic (seeded) and computed once per process; the arrays handed out must not be modified."""
import functools

import numpy as np

import ref_decode as R
import ref_framegen as G
from test_gpu_ref_decode import TIE, TIE_GRID

GAPS = (300, 303, 301)
LEAD = 333
TAIL = 700
SETTLE = 64
RAYS = 200
SPREAD = 1.5                                # the plane: half-width of the square and the rays' reach, in outermost points
TIE_CAP = 0.005                             # a condition on the cases: at most this share of a scheme's symbols may be ties
KINDS = ("plane", "far", "tiny")
GRID = (R.ASK4, R.QAM16, R.QAM32, R.QAM64)
PSK = (R.PSK2, R.PSK4, R.PSK8, R.PSK16) + R.DPSK
# payload bytes of the plane frame per bits per symbol: 1536, 1536, 1534, 1536, 1535, 1535 symbols; for bps 3, 5, 6 the last
# symbol carries 1, 2, 4 bits of the packet and 2, 3, 2 pad bits
PLANE_N = {1: 192, 2: 384, 3: 575, 4: 768, 5: 959, 6: 1151}
FAR_FACTORS = {ms: (2, 4, 8) for ms in R.PAYLOAD_MODS}
SEED = {"plane": 100, "far": 300, "tiny": 500}          # default_rng(SEED[kind] + ms)
# ties counted by tests/test_ref_plane.py (printed there), per scheme in the order of R.PAYLOAD_MODS
MEASURED_TIES = {R.PSK2: 0, R.PSK4: 0, R.PSK8: 0, R.PSK16: 0, R.DPSK2: 0, R.DPSK4: 0, R.DPSK8: 0, R.ASK4: 0, R.QAM16: 0, R.QAM32: 0, R.QAM64: 1}
MEASURED_EVM_RATIO = 0.41


def tie_limit(ms):
    return TIE.get(ms, TIE_GRID)


def tie_mask(ms, margin):
    """the tie rule of the module docstring"""
    t = np.asarray(margin) < tie_limit(ms)
    if ms in R.DPSK:
        t[1:] |= t[:-1].copy()
    return t


def axes(ms):
    """grid schemes: (alpha, levels on I, levels on Q); ASK4 has one axis"""
    if ms == R.ASK4:
        return 1.0 / np.sqrt(5.0), 4, 1
    mi, mq = {R.QAM16: (2, 2), R.QAM32: (3, 2), R.QAM64: (3, 3)}[ms]
    Li, Lq = 1 << mi, 1 << mq
    lev = np.add.outer((2.0 * np.arange(Li) - (Li - 1)) ** 2, (2.0 * np.arange(Lq) - (Lq - 1)) ** 2)
    return 1.0 / np.sqrt(lev.mean()), Li, Lq


def level_indices(ms, labels):
    """grid schemes: (level index on I, on Q) of hard labels -- the inverse of label = gray(i_I) << mq | gray(i_Q)"""
    _, Li, Lq = axes(ms)
    mq = Lq.bit_length() - 1
    ungray = np.zeros(max(Li, Lq), np.int64)
    ungray[R.gray(np.arange(max(Li, Lq)))] = np.arange(max(Li, Lq))
    labels = np.asarray(labels, np.int64)
    return ungray[labels >> mq], ungray[labels & (Lq - 1)]


def _square(rng, ms, count):
    rad = SPREAD * np.abs(R.constellation(ms)[0]).max()
    return rng.uniform(-rad, rad, count) + 1j * rng.uniform(-rad, rad, count)


def _conjugate_pairs(pts):
    """the same points, each followed by its conjugate where the list holds it: their phase errors cancel in the loop"""
    pts, out, used = list(pts), [], set()
    for i, p in enumerate(pts):
        if i in used:
            continue
        used.add(i)
        out.append(p)
        j = next((j for j in range(i + 1, len(pts)) if j not in used and abs(pts[j] - np.conj(p)) < 1e-9), None)
        if j is not None:
            used.add(j)
            out.append(pts[j])
    return np.array(out, np.complex128)


def far_points(ms):
    """the listed points of a far frame, without the settling points and the fill"""
    pts = R.constellation(ms)[0]
    out = [f * pts for f in FAR_FACTORS[ms]]
    if ms in GRID:
        al, Li, Lq = axes(ms)
        li, lq = al * (2.0 * np.arange(Li) - (Li - 1)), al * (2.0 * np.arange(Lq) - (Lq - 1))
        if ms == R.ASK4:
            lq = np.array([-0.7, 0.0, 0.7])
        for s in FAR_FACTORS[ms]:
            for side in (1.0, -1.0):
                out.append(side * (li[-1] + 2.0 * al * s) + 1j * lq)
                if ms != R.ASK4:
                    out.append(li + 1j * side * (lq[-1] + 2.0 * al * s))
    return _conjugate_pairs(np.concatenate(out))


def _build(ms):
    k = R.bps(ms)
    pts = R.constellation(ms)[0]
    cs = []

    def add(kind, n, points, **meta):
        points = np.asarray(points, np.complex128)
        assert len(points) == R.num_symbols(ms, n), (kind, ms, len(points), n)
        points.setflags(write=False)
        cs.append(dict(kind=kind, name="%s/%d" % (kind, ms), mod=ms, fec0=R.FEC_NONE, fec1=R.FEC_NONE, check=R.CRC_NONE, n=n, points=points,
                       nsym=len(points), gap=GAPS[len(cs)], padded=(8 * n) % k != 0, **meta))

    rng = np.random.default_rng(SEED["plane"] + ms)
    n = PLANE_N[k]
    nsym = R.num_symbols(ms, n)
    assert 1025 <= nsym <= 2047 and ((8 * n) % k != 0) == (k in (3, 5, 6))
    p = _square(rng, ms, nsym)
    p[:SETTLE] = pts[rng.integers(0, len(pts), SETTLE)]
    p[SETTLE:SETTLE + RAYS] = pts[rng.integers(0, len(pts), RAYS)] * rng.uniform(0.0, SPREAD, RAYS)
    add("plane", n, p)

    rng = np.random.default_rng(SEED["far"] + ms)
    listed = far_points(ms)
    nsym = max(256, 8 * ((SETTLE + len(listed) + 7) // 8))
    fill = nsym - SETTLE - len(listed)
    more = pts[rng.integers(0, len(pts), fill)] * np.array(FAR_FACTORS[ms])[rng.integers(0, 3, fill)]
    p = np.concatenate([pts[rng.integers(0, len(pts), SETTLE)], listed, more])
    assert (nsym * k) % 8 == 0
    add("far", nsym * k // 8, p, listed=len(listed), factors=FAR_FACTORS[ms])

    rng = np.random.default_rng(SEED["tiny"] + ms)
    add("tiny", 1, _square(rng, ms, R.num_symbols(ms, 1)))
    return cs


@functools.lru_cache(None)
def cases():
    """per scheme, in the order of R.PAYLOAD_MODS: its three cases (plane, far, tiny)"""
    return tuple(tuple(_build(ms)) for ms in R.PAYLOAD_MODS)


# ---------------------------------------------------------------------------------------------------- frames and streams
def frame(c, points=None):
    """the case's frame, complex128: the header of (n, mod, check, fec0, fec1), the points as payload symbols, the pulse of
    ref_framegen.frame at dt = 0 (as crafted_cases.frame)"""
    x = G.frame_symbols(np.zeros(c["n"], np.uint8), c["mod"], c["fec0"], c["fec1"], c["check"], points=c["points"] if points is None else points)
    up = np.zeros(G.K * len(x), np.complex128)
    up[::G.K] = x
    return np.convolve(up, G.tx_taps(0.0))[:G.K * len(x)]


def layout(cs):
    """[(offset, case)] back to back with each case's gap (>= 300 samples) behind it, and the total length"""
    out, off = [], LEAD
    for c in cs:
        out.append((off, c))
        off += G.frame_len(c["n"], c["mod"], c["fec0"], c["fec1"], c["check"]) + c["gap"]
    return out, off + TAIL


def _stream(cs, total, points=None):
    x = np.zeros(total, np.complex128)
    for i, (off, c) in enumerate(layout(cs)[0]):
        f = frame(c, None if points is None else points[i])
        x[off:off + len(f)] = f
    x = x.astype(np.complex64)
    x.setflags(write=False)
    return x


@functools.lru_cache(None)
def streams():
    """one complex64 stream per scheme, all of one length (zeros behind the shorter ones): ((samples, cases), ...)"""
    total = max(layout(cs)[1] for cs in cases())
    return tuple((_stream(cs, total), cs) for cs in cases())


# ---------------------------------------------------------------------------------------------------- the guard streams
GUARD_MODS = tuple(ms for ms in R.PAYLOAD_MODS if R.bps(ms) in (3, 5, 6))


@functools.lru_cache(None)
def guard_streams():
    """For `q < nbits` in fx_softdemod_kernel.  A padded last symbol has bits the packet does not hold; the first of them
    would land on the byte behind the frame's soft values.  Per scheme with bps 3, 5, 6: one frame of 1 payload byte, all
    symbols constellation points, in two variants "a" and "b" that differ in the last symbol alone -- chosen so that the soft
    value of that first absent bit is as low as a constellation point makes it in "a" and as high in "b".
    Returns dict(a=streams, b=streams, cases=[case], bit=[index of the first absent bit in the last symbol])."""
    out = dict(a=[], b=[], cases=[], bit=[])
    for ms in GUARD_MODS:
        k = R.bps(ms)
        pts = R.constellation(ms)[0]
        nsym, bit = R.num_symbols(ms, 1), 8 % k
        lead = np.full(nsym - 1, pts[0])
        if ms in R.DPSK:                                    # the label is the step from the symbol before, here phase index 0
            soft = R.demap_soft(ms, pts, R.gray(np.arange(len(pts))))[:, bit].astype(int)
        else:
            soft = R.demap_soft(ms, pts)[:, bit].astype(int)
        c = dict(kind="guard", name="guard/%d" % ms, mod=ms, fec0=R.FEC_NONE, fec1=R.FEC_NONE, check=R.CRC_NONE, n=1, nsym=nsym, gap=GAPS[0],
                 padded=True, points=np.concatenate([lead, pts[[int(soft.argmin())]]]))
        total = layout([c])[1]
        out["a"].append(_stream([c], total))
        out["b"].append(_stream([c], total, [np.concatenate([lead, pts[[int(soft.argmax())]]])]))
        out["cases"].append(c)
        out["bit"].append(bit)
    return out


# ---------------------------------------------------------------------------------------------------- the reference's view of a frame
def payload_label_bits(ms, payload, n):
    """payload bytes of a CRC_NONE, FEC_NONE / FEC_NONE packet back to the bits of the hard labels: (bits (nsym, bps), exists
    (nsym, bps)) -- a padded last symbol's absent bits are marked"""
    k = R.bps(ms)
    pkt = R.interleave(R.interleave(R.scramble(np.frombuffer(payload, np.uint8))))
    nsym = R.num_symbols(ms, n)
    bits = np.zeros(nsym * k, np.uint8)
    bits[:8 * n] = R.bits_of(pkt)
    exists = np.arange(nsym * k) < 8 * n
    return bits.reshape(nsym, k), exists.reshape(nsym, k)


class View:
    """ref_decode's view of one delivered frame, from its carrier-recovered symbols (float32 values taken exactly)"""

    def __init__(self, c, syms):
        ms, n = c["mod"], c["n"]
        self.ms, self.n, self.k = ms, n, R.bps(ms)
        self.syms = np.asarray(syms)
        self.r = self.syms.astype(np.complex128)
        assert len(self.r) == c["nsym"] == R.num_symbols(ms, n)
        self.labels, self.margin = R.demap_hard(ms, self.r)
        self.tie = tie_mask(ms, self.margin)
        self.bits = R.bits_of_words(self.labels, self.k).reshape(-1, self.k)
        pts = R.constellation(ms)[0]
        d = np.abs(self.r[:, None] - pts[None, :])
        self.index = d.argmin(axis=1)                       # the nearest point (differential PSK: the absolute point)
        self.dist = d.min(axis=1)

    def labels_with(self, other_bits):
        """the labels' bits with the other implementation's at tie symbols"""
        b = self.bits.copy()
        b[self.tie] = np.asarray(other_bits)[self.tie]
        return b

    def payload_of(self, bits):
        """ref_decode.packet_decode of label bits"""
        pkt = R.bytes_of(np.asarray(bits, np.uint8).ravel()[:8 * self.n], self.n)
        return R.packet_decode(pkt, self.n, R.CRC_NONE, R.FEC_NONE, R.FEC_NONE)

    def soft(self, label_bits=None):
        """(ref_decode.demap_soft (nsym, bps), whether the float64 value is more than 0.01 from a rounding tie); differential
        PSK: from the given hard labels' bits"""
        if self.ms in R.DPSK:
            lab = self.labels if label_bits is None else R.words_of(np.asarray(label_bits).ravel(), self.k)
            return R.demap_soft(self.ms, self.r, lab), np.ones((len(self.r), self.k), bool)
        pts, labs = R.constellation(self.ms)
        d2 = np.abs(self.r[:, None] - pts[None, :]) ** 2
        exact = np.ones((len(self.r), self.k), bool)
        for b in range(self.k):
            one = ((labs >> (self.k - 1 - b)) & 1).astype(bool)
            v = 127.0 + 16.0 * 1.2 * (1 << self.k) * (d2[:, ~one].min(axis=1) - d2[:, one].min(axis=1))
            exact[:, b] = np.abs(v - np.floor(v) - 0.5) > 0.01
        return R.demap_soft(self.ms, self.r), exact

    def soft_decode(self, soft_bits):
        return R.packet_decode_soft(soft_bits, self.n, R.CRC_NONE, R.FEC_NONE, R.FEC_NONE)
