"""Float64 statement of "aligned frame -> payload symbols" -- test infrastructure.

The middle of the receive chain: NCO mix, polyphase matched filter, the optional
equaliser, the pilot estimates over the header and the decision-directed payload PLL.  Written from the definitions
below, sharing no code with the oracle (oracle/fxref_frame.c) or the kernels (gr-liquiddsp_amd/csrc/fx_kernels.hip):
numpy complex128 and np.exp throughout -- no float32, no sin/cos table, no series, no 32-bit phase, no tree sums.
Conventions come in as *data* (the 64 p/n symbols, the 15 pilots, the 897-tap receive prototype, the 13 equaliser start
taps: `Tables`); constellations and decisions are ref_decode's.  `Tables.from_reference()` (= ref_framegen.tables()) builds
them from their definitions in tests/ref_framegen.py, `Tables.from_oracle()` reads the oracle's; tests/test_ref_framegen.py
pins the two to each other (p/n and pilots exactly, taps within one float32 ulp).

Inputs: the capture x, a frame's `start` (aligned sample 0 is x[start]) and the ALIGN estimates tau, gamma, dphi, phi as
the receiver reported them (float32 values taken exactly; tests/ref_detect.py pins those).

  mix      v[n] = x[start + n] exp(-j (phi + dphi n)),  n = 0, 1, ...                  (v[n] = 0 for n < 0)
  timing   tau > 0 : branch b = floor(32 tau) mod 32,      symbol c is read at sample n(c) = 2 c
           tau <= 0: branch b = floor(32 (1 + tau)) mod 32, symbol c is read at n(0) = 0, n(c) = 2 c - 1 (c >= 1)
           CONVENTION (liquid's mf_counter, kept by oracle and kernels): the filter runs at every sample and a counter,
           started at 0 (tau > 0) or 1 (tau <= 0), releases a symbol when it reaches 1 and then drops by 2.  For
           tau <= 0 that releases samples 0 AND 1, so there the grid is the odd samples, one sample EARLIER than for
           tau > 0, with one extra symbol (c = 0) inside the filter delay: branch 32 (1 + tau) read one sample early is
           the instant tau.  Stated as "tau > 0 first symbol one sample later, tau <= 0 at once" the grids come out one
           sample off this (half a symbol: test_ref_sync's truth test rejects that reading at an EVM of about 0 dB); the
           `late` argument below is that reading, kept as a negative control.
  filter   z[n]  = (0.5 / gamma) sum_{t<28} h[b + 32 t] v[n - t]      y(c) = z[n(c)]   (no equaliser)
  roles    c < 14 filter delay (7 symbols each of the 29-tap TX pulse and of the receive filter); c = 14..77 the p/n
           symbols; c = 78..308 the 231 header symbols; payload from c = 309.  With the equaliser every role is 3 later.
  equal.   window buf_i = z[n - 12 + i], i = 0..12 (buf_12 the newest), at every sample; y(c) = sum_i conj(w_i) buf_i at
           n = n(c); w starts as the 13 real start taps; at each p/n symbol d, after its output y: e = d - y,
           w_i += (mu / ||buf||^2) buf_i conj(e), mu = 0.05, skipped when ||buf||^2 = 0; frozen afterwards.
  pilots   header symbols 0, 16, ..., 224 times the conjugate pilots -> q_p; Q[k] = sum_p q_p exp(-j 2 pi k p / 32);
           k0 = first maximum of |Q|^2; vertex of the parabola through |Q| at k0 - 1, k0, k0 + 1 (indices mod 32);
           dphi = (k0 (- 32 if k0 >= 16) + vertex) 2 pi / 512 rad/symbol; S = sum_p q_p exp(-j dphi 16 p);
           phi = arg S; gain = |S| / 15.
  header   data symbol i (header index, pilots skipped): hdr[i] exp(-j (phi + dphi i)) / gain.  CONVENTION: two bits per
           symbol, MSB first, the imaginary axis first: bit = 1 where im <= 0, then bit = 1 where re <= 0 (a component
           of exactly 0 reads as 1).  54 bytes -> ref_decode.packet_decode(.., 20, CRC_32, SECDED(72,64), Hamming(8,4)).
           A header is valid when its CRC holds, byte 14 is the protocol number 102, and modulation, check and both
           codes are ones the receiver knows.
  PLL      theta_0 = phi + 231 dphi, f_0 = dphi.  Per payload symbol: r = y exp(-j theta); xhat = the nearest
           constellation point (differential PSK: the absolute PSK point, as ref_decode treats DPSK);
           pe = Im(r conj(xhat)); f += alpha pe; theta += f + beta pe; alpha = 1e-4, beta = 1e-2;
           evm_sum += |r - xhat|^2.

Tolerances against a float32 implementation (the oracle, the kernels) on the same capture and the same ALIGN estimates.
eps = 2^-24 = 6e-8.  Symbols are scaled to a unit-energy constellation (corner 1.53 for 64-QAM); noise at 6 dB lifts the
largest |y| seen to about 3.
The sum below is taken at the corner, |r| = 1.53; the paragraph after it treats symbols beyond the corner.
  matched filter: 28 fused multiply-adds per component.  Worst case 28 eps sum|h_t v_t| with sum|h_t| <= 2.2 max|h| and
      0.5 / gamma bringing the result to |y| ~ 1: <= 28 x 6e-8 x 2.2 x 1.5 = 5.5e-6; as a random walk sqrt(28) eps |y| = 5e-7.
  mixer sin/cos: 1024-entry table plus third-order series: truncation d^4/24 = 6e-11 (d <= 2 pi / 1024), rounding of
      the table product 2 eps: 1.5e-7 relative on every v[n], adding incoherently under the filter: < 3e-7 |y|.
  32-bit phase grid: phi is rounded to 2 pi / 2^32 (7e-10 rad) and dphi to half a grid step, 7.3e-10 rad/sample:
      over the 618 samples to the end of the header at most 4.5e-7 rad, which the pilot phi absorbs; over a payload
      of 2100 symbols a ramp of 1.5e-9 rad/symbol, which a second-order loop follows without a standing error; its
      transient is bounded by the ramp over the loop's memory of 1 / beta = 100 symbols: 1.5e-7 rad.
  pilot estimates: q_p carries the errors above (<= 1e-6 relative); the 15-term DFT adds 15 eps.  The vertex is
      -b / 2a with |a| >= 0.1 |Q[k0]| on the 15-of-32 window's main lobe (neighbours <= 0.9 of the peak):
      2e-6 / 0.2 = 1e-5 of a bin = 1.2e-7 rad/symbol; the float32 product (k0 + vertex) x 2 pi / 512 adds an ulp of dphi
      (<= 1.2e-8 at 0.2 rad/symbol): PILOT["dphi"] = 3e-7 rad/symbol.
      phi = arg S turns by 112 x (dphi error) (the pilots' centre is header symbol 112): 1.4e-5, plus the polynomial
      arg() (2e-7) and the sum (1e-6): PILOT["phi"] = 3e-5 rad.  gain = |S| / 15: 1e-6 relative plus second order in the
      dphi error: PILOT["gain_rel"] = 1e-5.
  first payload symbols: theta_0 = phi + 231 dphi is 119 symbols past the pilots' centre: 119 x 1.2e-7 + 1e-6 = 1.5e-5 rad
      worst case, times |r| <= 1.53 at the corner: 2.3e-5.  The loop removes it with its time constant of 100 symbols.
  the loop: the oracle re-reads its phasor from the table every 8th symbol and turns it by a fifth-order series in
      between (7 turns x 2 eps = 8e-7 rad), rounds the step to the 32-bit grid (7e-10 rad per symbol) and keeps f in grid
      units in float32 (an ulp of f at 0.2 rad/symbol: 8 units = 1.2e-8 rad).  None of these accumulate: an error e in
      theta comes back as pe = -|xhat|^2 e (more exactly Im(r conj xhat)) and is pulled in by beta per symbol, so the
      standing error is (per-symbol disturbance) / beta = 100 x (7e-10 + 1.2e-8) = 1.3e-6 rad, plus the 8e-7 of the phasor.
  sum, at the corner of the largest constellation: 5.5e-6 + 3e-7 x 1.53 + (1.5e-5 + 1.3e-6 + 8e-7) x 1.53 = 3.2e-5.
SYM_TOL = 4e-5 absolute for symbols inside the constellation, |r| <= CORNER = 1.53 (the project's contract for payload
symbols, parity_util.TOL_SYM, is 1e-4 on a unit-energy constellation).  That sum is a worst case for a symbol at the corner
only.  Every term of it is a relative error -- a rounding of the filter sum or a turn of the symbol by a phase error -- so
for a noisy symbol beyond the corner (|r| up to about 3 at 6 dB) each term grows with |r|, and the same sum at |r| = 3 is
6.3e-5, above 4e-5.  The bound in force is therefore sym_tol(r) = SYM_TOL max(1, |r| / CORNER), never more than the
contract's 1e-4 (reached at |r| = 3.8): 4e-5 on every symbol inside the constellation, 7.8e-5 at |r| = 3.
EVM_REL: evm_sum = sum |r - xhat|^2 over the compared span; each term moves by 2 |r - xhat| SYM_TOL, so the sum by
      2 tol sum|e_j| <= 2 tol sqrt(n evm_sum) with tol = sym_tol at the largest |r| of the span; the float32 running sum adds
      n eps / 2 relative (sequential, n <= 2100: 6e-5).  Checked in that form (evm_bound), floor 1e-9 absolute for
      noise-free frames whose evm_sum is itself rounding.

Measured (reference against the oracle, tests/test_ref_sync.py's grid and noisy cases; the oracle is the checker's
peer, not the code under test): see MEASURED below, kept next to the bounds it must stay 4x under.
"""
import numpy as np

import ref_decode as R

K = 2
NPFB = 32
MF_TAPS = 28
PN_LEN = 64
HDR_SYM = 231
HDR_MOD = 216
PILOT_SPACING = 16
N_PILOTS = 15
PRE_DELAY = 14                       # symbols of filter delay in front of the first p/n symbol
EQ_TAPS = 13
EQ_DELAY = 3
EQ_MU = 0.05
ALPHA = 1e-4
BETA = 1e-2
PROTOCOL = 102
HDR_DEC, HDR_ENC, HDR_USER = 20, 54, 14

SYM_TOL = 4e-5
CORNER = 7.0 * np.sqrt(2.0 / 42.0)       # the largest |point| of any scheme: 64-QAM's corner, 1.53
SYM_CONTRACT = 1e-4
PILOT = dict(dphi=3e-7, phi=3e-5, gain_rel=1e-5)
# decision margins under which a hard decision may legitimately differ (tests/test_gpu_ref_decode.py's)
TIE_PSK, TIE_GRID = 1e-5, 2e-6
# worst reference-vs-oracle differences over test_ref_sync.py's cases (CPU), and reference-vs-GPU over
# test_gpu_ref_sync.py's traffic (MI355X); the bounds above must stay >= 4x these
MEASURED = dict(oracle=dict(sym=9.7e-7, dphi=3.7e-8, phi=2.1e-6, gain_rel=3.6e-7),
                gpu={False: dict(sym=7.7e-7, dphi=2.1e-8, phi=2.3e-6, gain_rel=2.2e-7),       # equaliser off
                     True: dict(sym=9.0e-7, dphi=2.2e-8, phi=1.6e-6, gain_rel=3.3e-7)})        # equaliser on


class Tables:
    """The conventions, as data: pn (64), pilots (15), proto (897 real taps), eq0 (13 real start taps)."""

    def __init__(self, pn, pilots, proto, eq0):
        self.pn = np.asarray(pn, np.complex128)
        self.pilots = np.asarray(pilots, np.complex128)
        self.proto = np.asarray(proto, np.float64)
        self.eq0 = np.asarray(eq0, np.float64)
        assert len(self.pn) == PN_LEN and len(self.pilots) == N_PILOTS and len(self.proto) == NPFB * MF_TAPS + 1 and len(self.eq0) == EQ_TAPS

    @classmethod
    def from_oracle(cls, oracle):
        return cls(oracle.table("fxr_preamble_pn", PN_LEN), oracle.table("fxr_pilots", N_PILOTS),
                   oracle.table("fxr_mf_proto", NPFB * MF_TAPS + 1, complex_=False), oracle.eq_init_taps())

    @classmethod
    def from_reference(cls):
        """The tables from their definitions (tests/ref_framegen.py), in float64: no oracle."""
        import ref_framegen
        return ref_framegen.tables()


def tie_margin(ms):
    return TIE_PSK if ms in (R.PSK2, R.PSK4, R.PSK8, R.PSK16) + R.DPSK else TIE_GRID


def timing(tau, branch_shift=0, late=0):
    """(branch, mf_counter0, n) with n(c) the sample at which symbol c is read."""
    tau = float(tau)
    if tau > 0.0:
        b, counter0 = int(np.floor(NPFB * tau)) % NPFB, 0
        n = lambda c: 2 * np.asarray(c) + late
    else:
        b, counter0 = int(np.floor(NPFB * (1.0 + tau))) % NPFB, 1
        n = lambda c: np.where(np.asarray(c) == 0, 0, 2 * np.asarray(c) - 1) + late
    return (b + branch_shift) % NPFB, counter0, n


def near_branch_edge(tau, eps=1e-4):
    """32 tau (or 32 (1 + tau)) within eps of an integer: float32 may land on the other side of the floor."""
    t = NPFB * float(tau)
    return abs(t - np.rint(t)) < eps


def matched_filter(x, start, gamma, dphi, phi, branch, nsamp, tb):
    """z[n], n = 0..nsamp-1: the mixed samples through branch `branch`, scaled by 0.5 / gamma."""
    seg = np.asarray(x[start:start + nsamp], np.complex128)
    n = np.arange(len(seg), dtype=np.float64)
    v = seg * np.exp(-1j * (float(phi) + float(dphi) * n))
    h = tb.proto[branch + NPFB * np.arange(MF_TAPS)]
    return (0.5 / float(gamma)) * np.convolve(v, h)[:len(v)]


def pilot_sync(hdr, tb, origin=0):
    """(dphi, phi, gain) from the 231 header symbols.  origin: negative control (the pilots' index origin)."""
    p = np.arange(N_PILOTS)
    q = hdr[(PILOT_SPACING * p + origin) % HDR_SYM] * np.conj(tb.pilots)
    k = np.arange(32)
    Q = (q[None, :] * np.exp(-2j * np.pi * np.outer(k, p) / 32.0)).sum(axis=1)
    m = np.abs(Q)
    k0 = int(np.argmax(m * m))
    ym, y0, yp = m[(k0 - 1) % 32], m[k0], m[(k0 + 1) % 32]
    a, b = 0.5 * (yp + ym) - y0, 0.5 * (yp - ym)
    vertex = 0.0 if a == 0.0 else -b / (2.0 * a)
    dphi = ((k0 - 32 if k0 >= 16 else k0) + vertex) * 2.0 * np.pi / 512.0
    S = np.sum(q * np.exp(-1j * dphi * PILOT_SPACING * p))
    return float(dphi), float(np.angle(S)), float(np.abs(S) / N_PILOTS)


def header_bytes(hdr, dphi, phi, gain):
    """(54 hard bytes, the 216 recovered data symbols)"""
    i = np.arange(HDR_SYM)
    d = (hdr * np.exp(-1j * (phi + dphi * i)) / gain)[i % PILOT_SPACING != 0]
    bits = np.empty(2 * HDR_MOD, np.uint8)
    bits[0::2] = d.imag <= 0.0
    bits[1::2] = d.real <= 0.0
    return np.packbits(bits), d


def parse_header(hb):
    """54 bytes -> (valid, the 20 decoded bytes, dict(payload_len, ms, check, fec0, fec1))"""
    dec, ok = R.packet_decode(hb, HDR_DEC, R.CRC_32, R.FEC_SD72, R.FEC_H84)
    dec = np.frombuffer(dec, np.uint8)
    h = dec[HDR_USER:]
    p = dict(payload_len=(int(h[1]) << 8) | int(h[2]), ms=int(h[3]), check=(int(h[4]) >> 5) & 7, fec0=int(h[4]) & 31, fec1=int(h[5]) & 31)
    ok = bool(ok) and h[0] == PROTOCOL and p["ms"] in R.PAYLOAD_MODS and R.CRC_NONE <= p["check"] <= R.CRC_32 \
        and p["fec0"] in R.ALL_FEC and p["fec1"] in R.ALL_FEC
    return ok, dec, p


def pll(y, ms, theta0, f0, alpha=ALPHA, beta=BETA):
    """The decision-directed loop over the payload's filter outputs y.  Returns (r, per-symbol |r - xhat|^2)."""
    pts = R.constellation(ms)[0]
    r = np.empty(len(y), np.complex128)
    e2 = np.empty(len(y), np.float64)
    theta, f = float(theta0), float(f0)
    for j in range(len(y)):
        rj = y[j] * np.exp(-1j * theta)
        xh = pts[int(np.argmin(np.abs(rj - pts)))]
        pe = (rj * np.conj(xh)).imag
        f += alpha * pe
        theta += f + beta * pe
        r[j] = rj
        e2[j] = abs(rj - xh) ** 2
    return r, e2


def sync(x, start, tau, gamma, dphi, phi, tb, equalizer=False, branch_shift=0, late=0, pilot_origin=0, alpha=ALPHA, beta=BETA,
         theta0_symbols=HDR_SYM, eq_delay=EQ_DELAY):
    """The frame whose aligned sample 0 is x[start].  The keyword arguments after `equalizer` are negative controls (mutations
    of this statement's own parameters); their defaults are the definition.  Returns a dict: pfb_index, mf_counter0, hdr
    (231), pilot_dphi / pilot_phi / pilot_gain, header_bytes (54), header_valid, header (20 decoded bytes), props, and for a
    valid header whose payload lies inside the capture: r (payload symbols), labels, margin, e2 (per symbol), evm_sum.
    `short` is set when the capture ends before the frame does."""
    branch, counter0, n_of = timing(tau, branch_shift, late)
    dly = eq_delay if equalizer else 0
    c_hdr, c_pay = PRE_DELAY + PN_LEN + dly, PRE_DELAY + PN_LEN + HDR_SYM + dly
    avail = len(x) - start
    out = dict(pfb_index=branch, mf_counter0=counter0, short=False, header_valid=False)
    if int(n_of(c_pay - 1)) >= avail:
        out["short"] = True
        return out
    z = matched_filter(x, start, gamma, dphi, phi, branch, avail, tb)
    zp = np.concatenate([np.zeros(EQ_TAPS - 1, np.complex128), z])      # zp[n + 12] = z[n]

    if equalizer:
        w = tb.eq0.astype(np.complex128)
        for c in range(PRE_DELAY + dly, c_hdr):
            n = int(n_of(c))
            buf = zp[n:n + EQ_TAPS]
            y = np.sum(np.conj(w) * buf)
            p2 = float(np.sum(np.abs(buf) ** 2))
            if p2 > 0.0:
                w = w + (EQ_MU / p2) * buf * np.conj(tb.pn[c - PRE_DELAY - dly] - y)
        out["eq_taps"] = w

        def symbols(c):
            n = n_of(c)
            return (zp[n[:, None] + np.arange(EQ_TAPS)[None, :]] * np.conj(w)[None, :]).sum(axis=1)
    else:
        def symbols(c):
            return z[n_of(c)]

    hdr = symbols(np.arange(c_hdr, c_pay))
    pd, pp, pg = pilot_sync(hdr, tb, pilot_origin)
    hb, hdata = header_bytes(hdr, pd, pp, pg)
    ok, dec, props = parse_header(hb)
    out.update(hdr=hdr, pilot_dphi=pd, pilot_phi=pp, pilot_gain=pg, header_bytes=hb, header_data=hdata, header_valid=ok,
               header=dec.tobytes(), props=props)
    if not ok:
        return out
    l1 = R.packet_dims(props["payload_len"], props["check"], props["fec0"], props["fec1"])[2]
    npay = R.num_symbols(props["ms"], l1)
    out["num_symbols"] = npay
    if npay and int(n_of(c_pay + npay - 1)) >= avail:
        out["short"] = True
        return out
    y = symbols(np.arange(c_pay, c_pay + npay)) if npay else np.zeros(0, np.complex128)
    r, e2 = pll(y, props["ms"], pp + theta0_symbols * pd, pd, alpha, beta)
    labels, margin = R.demap_hard(props["ms"], r) if npay else (np.zeros(0, np.int64), np.zeros(0))
    out.update(y=y, r=r, e2=e2, labels=np.asarray(labels), margin=margin, evm_sum=float(e2.sum()))
    return out


def compared_span(ref):
    """Number of leading payload symbols to compare: up to (not including) the first whose decision margin in the
    reference is under the tie margin -- after a flipped decision two loops legitimately part for a few hundred symbols."""
    m = ref["margin"]
    low = np.nonzero(m < tie_margin(ref["props"]["ms"]))[0]
    return int(low[0]) if len(low) else len(m)


def sym_tol(r):
    """The symbol bound in force: SYM_TOL inside the constellation, growing with |r| beyond its corner, capped by the contract."""
    return np.minimum(SYM_CONTRACT, SYM_TOL * np.maximum(1.0, np.abs(r) / CORNER))


def evm_bound(ref, n):
    """Allowed |evm_sum difference| over the first n payload symbols (derivation in the header)."""
    s = float(ref["e2"][:n].sum())
    tol = float(sym_tol(ref["r"][:n]).max()) if n else SYM_TOL
    return 2.0 * tol * np.sqrt(n * s) + n * tol ** 2 + 0.5 * n * 2.0 ** -24 * s + 1e-9


def compare(ref, got_info, got_syms, got_header, full_evm_sum=None, check_branch=True, check_counter=True):
    """The comparison of test_ref_sync 2c / test_gpu_ref_sync: ref = sync(...) of a header-valid frame, got_* the float32
    implementation's view (got_info: pfb_index, mf_counter0, pilot_dphi, pilot_phi, pilot_gain).  check_counter=False is for
    an implementation that does not report mf_counter0 (the library's result record has no such field; there the symbol grid
    is pinned through the symbols themselves, which sit half a symbol off on the other grid).  Hard labels: the
    implementation's symbols demapped by ref_decode.demap_hard must give the reference's labels over the compared span.
    Returns (list of failure strings, dict of worst differences, compared span, tie-shortened?)."""
    bad, n = [], compared_span(ref)
    w = dict(sym=0.0, sym_ratio=0.0, dphi=0.0, phi=0.0, gain_rel=0.0, evm=0.0, evm_bound=0.0)
    if check_branch:
        if ref["pfb_index"] != got_info["pfb_index"]:
            bad.append("pfb_index %d vs %d" % (ref["pfb_index"], got_info["pfb_index"]))
        if check_counter and ref["mf_counter0"] != got_info["mf_counter0"]:
            bad.append("mf_counter0 %d vs %d" % (ref["mf_counter0"], got_info["mf_counter0"]))
    w["dphi"] = abs(ref["pilot_dphi"] - got_info["pilot_dphi"])
    w["phi"] = abs((ref["pilot_phi"] - got_info["pilot_phi"] + np.pi) % (2.0 * np.pi) - np.pi)
    w["gain_rel"] = abs(ref["pilot_gain"] - got_info["pilot_gain"]) / ref["pilot_gain"]
    for k in PILOT:
        if not w[k] <= PILOT[k]:
            bad.append("pilot %s off by %.3g (bound %.3g)" % (k, w[k], PILOT[k]))
    if bytes(got_header) != ref["header"][:len(got_header)]:
        bad.append("header bytes differ")
    if len(got_syms) != len(ref["r"]):
        bad.append("payload symbols: %d vs %d" % (len(got_syms), len(ref["r"])))
        return bad, w, n, n < len(ref["r"])
    if n:
        got = np.asarray(got_syms, np.complex128)
        d, tol = np.abs(got[:n] - ref["r"][:n]), sym_tol(ref["r"][:n])
        j = int(np.argmax(d / tol))
        w["sym"], w["sym_ratio"] = float(d.max()), float(d[j] / tol[j])
        if not w["sym_ratio"] <= 1.0:
            bad.append("payload symbols off by %.3g (bound %.3g) at %d" % (d[j], tol[j], j))
        if not np.array_equal(np.asarray(R.demap_hard(ref["props"]["ms"], got)[0][:n]), ref["labels"][:n]):
            bad.append("hard labels differ")
    if n == len(ref["r"]) and full_evm_sum is not None:
        w["evm"], w["evm_bound"] = abs(full_evm_sum - ref["evm_sum"]), evm_bound(ref, n)
        if not w["evm"] <= w["evm_bound"]:
            bad.append("evm_sum %.6g vs %.6g (bound %.3g)" % (full_evm_sum, ref["evm_sum"], w["evm_bound"]))
    return bad, w, n, n < len(ref["r"])
