"""Float64 statement of one qdetector hop and a truth model of the channel -- test infrastructure.

Written from the definitions, sharing no code with the oracle (oracle/fxref_frame.c) or the kernels
(gr-liquiddsp_amd/csrc/fx_kernels.hip).  The template is rebuilt here from the 64 p/n symbols and the 29-tap
interpolator, both taken as *data*; the correlations are stated as sums and evaluated with numpy FFTs (no butterfly
network, no tables, no float32).

One hop of the detector on a 512-sample window x[0..512):

    R_k[l] = N * sum_{m<156} x[(m + l) mod N] * conj(s[m]) * exp(-j 2 pi k m / N),   k = -24..24, l = 0..511

(N = 512, s = template) -- the unnormalised IFFT of X[i] conj(S[i - k]) the detector computes.  With the window energy
E = sum |x|^2 the detector's normalised peak is

    rxy = max |R| / (N * sqrt(E * 156 / N) * sqrt(Es)),   Es = sum |s|^2,

and the winner is the first maximum of |R|^2 in (bin, lag) order.  On the aligned window (winner at lag 0):

    timing: parabola through sqrt|R_k| at lags -1, 0, +1 -> tau = vertex, gamma = (vertex value)^2 / (N Es)
    CFO:    P[i] = x[i] conj(s[i]) (i < 156, zero-padded to 512), |FFT(P)| peak + parabola -> dphi (rad/sample)
    phase:  phi = arg sum_i P[i] exp(-j dphi i)       (the phase at template sample 0)

The truth model (`expected`, `check_truth`) states what a receiver must report for a frame that went through
    y[n] = g exp(j (theta + w n)) f(n - lead - d) + noise,   sigma_n^2 = 10^(-snr/10) per complex sample,
where f is the dt = 0 frame (unit power per sample) and d a fractional delay; each tolerance carries its derivation.
"""
import numpy as np

N = 512
S_LEN = 156
RANGE = 24
BINS = np.arange(-RANGE, RANGE + 1)
K = 2                       # samples per symbol
TWO_PI = 2.0 * np.pi


def build_template(pn, taps):
    """Interpolate the 64 p/n symbols by K = 2 with the 29-tap pulse, flushed with 2m symbols: 156 samples, complex128.
    y[2n+i] = sum_t h[i+2t] pn[n-t] is the full convolution of the zero-stuffed symbols with h."""
    pn = np.asarray(pn, np.complex128)
    up = np.zeros(K * len(pn), np.complex128)
    up[::K] = pn
    s = np.convolve(up, np.asarray(taps, np.float64))
    assert len(s) == S_LEN
    return s


def xcorr(window, s, bins=BINS):
    """R_k[l] for every bin k and lag l (complex128, shape (len(bins), 512)), by its definition above: the circular
    cross-correlation of x with t_k[m] = s[m] exp(+j 2 pi k m / N), evaluated through numpy's FFT."""
    x = np.asarray(window, np.complex128)
    assert len(x) == N
    m = np.arange(S_LEN)
    t = np.zeros((len(bins), N), np.complex128)
    t[:, :S_LEN] = s[None, :] * np.exp(1j * TWO_PI * np.outer(bins, m) / N)
    return N * np.fft.ifft(np.fft.fft(x)[None, :] * np.conj(np.fft.fft(t, axis=1)), axis=1)


def seek(window, s):
    """One SEEK hop: dict(rxy, bin, lag, r2 (|R|^2, 49 x 512), bin_peaks (max |R|^2 per bin), margin (relative gap
    between the two strongest bins), silent (g0 < 1e-10, the detector's silence cut))."""
    x = np.asarray(window, np.complex128)
    es = float(np.sum(np.abs(s) ** 2))
    g0 = np.sqrt(np.sum(np.abs(x) ** 2) * S_LEN / N)
    r2 = np.abs(xcorr(x, s)) ** 2
    flat = int(np.argmax(r2))               # first maximum in (bin, lag) order
    bi, lag = divmod(flat, N)
    peaks = r2.max(axis=1)
    top = np.sort(peaks)[::-1]
    return dict(rxy=float(np.sqrt(r2.flat[flat]) / (N * g0 * np.sqrt(es))) if g0 > 0 else 0.0, bin=int(BINS[bi]), lag=lag,
                r2=r2, bin_peaks=peaks, margin=float((top[0] - top[1]) / top[0]) if top[0] > 0 else 0.0, silent=bool(g0 < 1e-10))


def walk(x, s, threshold, lead_zeros=256):
    """The detector's hop grid on a stream until its first detection: windows [w, w+512), w = -256, 0, 256, ... (the
    detector starts with 256 zeros of history); a hop detects when rxy > threshold and the lag leaves room for the
    template (lag < N - 156).  Returns (pos, seek dict) or (None, None)."""
    x = np.concatenate([np.zeros(lead_zeros, np.complex128), np.asarray(x, np.complex128)])
    for w in range(0, len(x) - N + 1, N // 2):
        h = seek(x[w:w + N], s)
        if not h["silent"] and h["rxy"] > threshold and h["lag"] < N - S_LEN:
            return w - lead_zeros + h["lag"], h
    return None, None


def _vertex(ym, y0, yp):
    a = 0.5 * (yp + ym) - y0
    b = 0.5 * (yp - ym)
    v = 0.0 if a == 0.0 else -b / (2.0 * a)
    return a, b, v


def align(window, s, k):
    """The ALIGN estimates on the aligned 512-sample window for bin k: dict(tau, gamma, dphi, phi)."""
    x = np.asarray(window, np.complex128)
    es = float(np.sum(np.abs(s) ** 2))
    r = xcorr(x, s, bins=np.array([k]))[0]
    ym, y0, yp = np.sqrt(np.abs(r[[N - 1, 0, 1]]))
    a, b, tau = _vertex(ym, y0, yp)
    if not abs(tau) < 1.0:
        tau = 0.0
    gh = (a * tau + b) * tau + y0
    p = np.zeros(N, np.complex128)
    p[:S_LEN] = x[:S_LEN] * np.conj(s)
    f = np.abs(np.fft.fft(p))
    i0 = int(np.argmax(f))
    _, _, di = _vertex(f[(i0 - 1) % N], f[i0], f[(i0 + 1) % N])
    idx = i0 + di
    dphi = (idx - N if i0 > N // 2 else idx) * TWO_PI / N
    phi = float(np.angle(np.sum(p[:S_LEN] * np.exp(-1j * dphi * np.arange(S_LEN)))))
    return dict(tau=float(tau), gamma=float(gh * gh / (N * es)), dphi=float(dphi), phi=phi)


def wrap(a):
    """Angle difference into [-pi, pi)."""
    return (np.asarray(a, np.float64) + np.pi) % TWO_PI - np.pi


# ---------------------------------------------------------------------------------------------------- parity bounds
# ref_detect (float64) against a float32 implementation on the same window.  The inputs are float32; the float32
# pipeline's relative rounding on |R| after a 512-point FFT pair is ~ 9 stages x 2^-24 ~ 6e-7.
# tau   = -b / 2a with |a| >= 0.1 y0 on this template's peak (sqrt|R| at lag +-1 is <= 0.9 of lag 0): 6e-7 / (2 x 0.1)
#         -> 3e-6; bound 2e-5 absolute.
# gamma = vertex^2 / (N Es): relative 2 x 6e-7 plus tau's effect (second order): bound 2e-5 relative.
# dphi  = (i0 + vertex - 512) x 2 pi / 512 in float32: the index near 512 carries an ulp of 3e-5 bin = 3.7e-7 rad/sample;
#         bound 1e-6 rad/sample.
# phi   = the phase at template sample 0, 77.5 samples from the centre where the sum is anchored: 77.5 x the dphi bound
#         plus 2e-5 for the sum and arg(): bound 1e-4 rad.
# Near a tie of two lags or bins the winner itself can flip on a float32 ulp; those cases are compared for `bin` only
# through TIE_MARGIN (two strongest bins closer than 1e-4 relative in |R|^2: 100x the float32 rounding of |R|^2).
PARITY = dict(tau=2e-5, gamma_rel=2e-5, dphi=1e-6, phi=1e-4)
TIE_MARGIN = 1e-4


def parity_errors(ref, got):
    """Absolute / relative differences of the ALIGN estimates (phase wrapped)."""
    return dict(tau=abs(ref["tau"] - got["tau"]), gamma_rel=abs(ref["gamma"] - got["gamma"]) / max(abs(ref["gamma"]), 1e-300),
                dphi=abs(ref["dphi"] - got["dphi"]), phi=abs(float(wrap(ref["phi"] - got["phi"]))))


def parity_ok(ref, got):
    e = parity_errors(ref, got)
    return all(e[k] <= PARITY[k] for k in PARITY), e


# ---------------------------------------------------------------------------------------------------- truth model
def fractional_delay(x, d):
    """x delayed by d samples (d any real), by a linear phase ramp on its FFT; x must carry enough zeros at both ends."""
    x = np.asarray(x, np.complex128)
    f = np.fft.fftfreq(len(x))
    return np.fft.ifft(np.fft.fft(x) * np.exp(-1j * TWO_PI * f * d))


def channel(frame, lead, d, gain, cfo, phase, snr_db, rng, total):
    """One frame through the channel, float64: g exp(j(theta + w n)) f(n - lead - d) + noise, n = 0..total-1.  The noise is
    scaled with the gain (sigma^2 = g^2 10^(-snr/10) per complex sample), so the SNR does not depend on the amplitude.
    snr_db=None: noise-free.  Returns complex128."""
    y = np.zeros(total, np.complex128)
    y[lead:lead + len(frame)] = frame
    y = fractional_delay(y, d)
    n = np.arange(total, dtype=np.float64)
    y = gain * y * np.exp(1j * (phase + cfo * n))
    if snr_db is not None:
        sig = gain * np.sqrt(0.5 * 10.0 ** (-snr_db / 10.0))
        y = y + sig * (rng.standard_normal(total) + 1j * rng.standard_normal(total))
    return y


# Per-estimate tolerances.  Two channel quantities set them:
#   delta   = w - k 2 pi / N, the residual CFO left by the winning bin k (|delta| <= pi / N inside the sweep);
#   sigma_r = sigma_n / (g sqrt(2 Es)), the relative noise on the correlation peak along the signal (Es = 128, the
#             template energy at unit power per sample).
# Noise terms are Z = 6 standard deviations.
ES = 128.0
Z = 6.0


def residual(cfo):
    """(winning bin, residual CFO) the sweep leaves for a channel CFO: the nearest bin, clamped to the sweep's edge."""
    k = int(np.clip(np.round(cfo * N / TWO_PI), -RANGE, RANGE))
    return k, cfo - k * TWO_PI / N


_TMPL = {}


def _template():
    if "s" not in _TMPL:
        raise RuntimeError("ref_detect.set_template(s) first")
    return _TMPL["s"]


def set_template(s):
    _TMPL.clear()
    _TMPL["s"] = np.asarray(s, np.complex128)


def mismatch_loss(delta):
    """|sum_m |s_m|^2 exp(j delta m)| / Es: what a residual CFO delta takes off the correlation peak, hence off gamma."""
    s = _template()
    e = np.abs(s) ** 2
    return float(np.abs(np.sum(e * np.exp(1j * delta * np.arange(S_LEN)))) / np.sum(e))


def timing_bias(delta=0.0, taus=np.linspace(-0.5, 0.5, 33)):
    """Noise-free vertex error of the timing parabola on the template alone, delayed by tau and turned by a residual CFO
    delta: the deterministic part of the `arrival` bound (max over tau of |tau_hat - tau|)."""
    key = round(float(delta), 6)
    if key in _TMPL:
        return _TMPL[key]
    s = _template()
    worst = 0.0
    for tau in taus:
        w = np.zeros(3 * N, np.complex128)
        w[N:N + S_LEN] = s * np.exp(1j * delta * np.arange(S_LEN))
        w = fractional_delay(w, tau)[N:2 * N]
        worst = max(worst, abs(align(w, s, 0)["tau"] - tau))
    _TMPL[key] = worst
    return worst


def tolerances(snr_db, delta=0.0):
    sr = 0.0 if snr_db is None else np.sqrt(10.0 ** (-snr_db / 10.0) / (2.0 * ES))
    loss = mismatch_loss(delta)
    return dict(
        # start + tau vs lead + d: the parabola through sqrt|R| at lags -1,0,+1 is not the peak's shape and a residual CFO
        # skews the peak: timing_bias(delta), 0.003 at delta = 0, 0.06 at half a bin.  The frame's own symbols next to the
        # preamble correlate with the template too (self-noise; 0.014 seen at delta = 0): + 0.03.  Noise: tau = -b/2a with
        # |a| >= 0.1 y0 and b carrying sqrt(2) x sigma_r / 2 relative -> sigma_tau <= 3.6 sigma_r / loss.
        arrival=timing_bias(delta) + 0.03 + Z * 3.6 * sr / loss,
        # detector dphi vs w: a timing offset tau leaves a phase ramp in P = x conj(s) that the FFT peak reads as
        # -0.0044 tau rad/sample (<= 0.0022 at |tau| <= 0.5) and the parabola on |FFT(P)| (a 3.3-bin wide peak) misreads
        # by <= 5e-4: 3e-3.  Noise: the slope of a 156-sample phase ramp, sigma = sqrt(12) / 156 x sqrt(2) sigma_r.
        dphi=3e-3 + Z * np.sqrt(12.0) / S_LEN * np.sqrt(2.0) * sr / loss,
        # dphi + pilot_dphi/2 vs w: the pilots measure what the detector left, on a grid of 2 pi / 512 rad/symbol read by a
        # parabola (< 5 % of a half step = 1.5e-4 rad/sample), + 1.5e-4 for the pilots' timing offset: 3e-4.  Noise: LS
        # slope of 15 pilot phases 32 samples apart, each of std sigma_n / (g sqrt(2)) after the matched filter:
        # sigma = sigma_n / sqrt(2) / (32 sqrt(280)).
        cfo_fine=3e-4 + Z * (0.0 if snr_db is None else np.sqrt(10.0 ** (-snr_db / 10.0) / 2.0)) / (32.0 * np.sqrt(280.0)),
        # phi + 77.5 dphi vs theta + w (start + 77.5): the phase at the template centre is first-order insensitive to the
        # slope error; what is left (timing offset x the template's mean frequency) is <= 0.011 rad noise-free: 0.015.
        # Noise: arg of the correlation, std sigma_r / loss.
        phase=0.015 + Z * sr / loss,
        # gamma vs g x mismatch_loss(delta): the parabola's vertex value under-reads the peak by <= 0.4 % plus the
        # self-noise of the neighbouring symbols: 1.5 %.  Noise: 2 sigma_r / loss relative (|R| at the vertex, squared
        # root taken twice, plus the vertex shift).
        gain_rel=0.015 + Z * 2.0 * sr / loss,
    )


TEMPLATE_CENTRE = (S_LEN - 1) / 2.0      # 77.5


def check_truth(est, lead, d, gain, cfo, phase, snr_db):
    """est: dict with start, tau, dphi, phi, gamma and optionally cfo_bin, pilot_dphi (rad/symbol), rssi_db, cfo.
    Returns a list of failure strings (empty = consistent with the channel)."""
    k, delta = residual(cfo)
    t = tolerances(snr_db, delta)
    bad = []
    if "cfo_bin" in est:
        # the winning bin is the nearest one, or one of the two when w sits within the noise of a half bin
        half = abs(abs(delta) - np.pi / N) <= Z * np.sqrt(12.0) / S_LEN * np.sqrt(2.0) * (0.0 if snr_db is None else np.sqrt(10.0 ** (-snr_db / 10.0) / (2.0 * ES))) + 1e-9
        ok = est["cfo_bin"] == k or (half and abs(est["cfo_bin"] - cfo * N / TWO_PI) <= 0.5 + 1e-6)
        if not ok:
            bad.append("cfo_bin %d vs %d" % (est["cfo_bin"], k))
    arr = est["start"] + est["tau"]
    if abs(arr - (lead + d)) > t["arrival"]:
        bad.append("arrival %.4f vs %.4f" % (arr, lead + d))
    if abs(est["dphi"] - cfo) > t["dphi"]:
        bad.append("dphi %.5f vs %.5f" % (est["dphi"], cfo))
    if "cfo" in est and abs(est["cfo"] - cfo) > t["dphi"]:
        bad.append("stats cfo %.5f vs %.5f" % (est["cfo"], cfo))
    if est.get("pilot_dphi") is not None and abs(est["dphi"] + est["pilot_dphi"] / K - cfo) > t["cfo_fine"]:
        bad.append("dphi + pilot_dphi/2 = %.6f vs %.6f" % (est["dphi"] + est["pilot_dphi"] / K, cfo))
    cp = est["phi"] + TEMPLATE_CENTRE * est["dphi"]
    want = phase + cfo * (est["start"] + TEMPLATE_CENTRE)
    if abs(float(wrap(cp - want))) > t["phase"]:
        bad.append("centre phase %.4f vs %.4f" % (float(wrap(cp)), float(wrap(want))))
    g_exp = gain * mismatch_loss(delta)
    if abs(est["gamma"] / g_exp - 1.0) > t["gain_rel"]:
        bad.append("gamma %.6g vs %.6g" % (est["gamma"], g_exp))
    if "rssi_db" in est and abs(est["rssi_db"] - 20.0 * np.log10(g_exp)) > -20.0 * np.log10(1.0 - t["gain_rel"]):
        bad.append("rssi %.3f dB vs %.3f dB" % (est["rssi_db"], 20.0 * np.log10(g_exp)))
    return bad


def evm_bounds_db(snr_db, n_syms, delta=0.0):
    """Expected payload EVM (dB) of a PSK frame.  The receiver's matched filter (sum h^2 = 2) scaled by 0.5/gamma passes
    sigma_n^2 x 2 x 0.25 = sigma_n^2 / 2 of noise per symbol: evm_db = -snr + c, c = 10 log10(1/2) = -3.01 dB.  On top sits
    the noise-free floor (ISI of the pulse pair at the timing error left): >= -60 dB, <= -28 dB for |delta| up to a
    quarter bin and <= -20 dB up to a half bin (the timing bias above grows with delta).  The mean over n_syms symbols of
    |e|^2 (chi-square, 2 degrees of freedom) has relative std 1/sqrt(n_syms): Z of those either side."""
    floor_hi = 10.0 ** (-2.8) if abs(delta) <= np.pi / (2 * N) + 1e-12 else 10.0 ** (-2.0)
    if snr_db is None:
        return -60.0, 10.0 * np.log10(floor_hi)
    nv = 10.0 ** (-snr_db / 10.0) / 2.0
    s = Z / np.sqrt(n_syms)
    return 10.0 * np.log10(nv * max(1.0 - s, 0.05)), 10.0 * np.log10((nv + floor_hi) * (1.0 + s))
