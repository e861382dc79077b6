"""The middle of the receive chain -- NCO mix, polyphase matched filter, equaliser, pilot estimates, payload PLL -- against
tests/ref_sync.py, a float64 statement written from the definitions that shares no code with the oracle.  CPU only.
  a. the receive prototype (taken as data) is symmetric, Nyquist with the TX pulse on every branch, and indexed the right way;
  b. truth: on noise-free frames the reference's payload symbols are the transmitted points and its header is the sent one;
  c. the oracle's synchroniser against the reference over delays across the start/tau wrap, all 11 modulations, payload
     symbol counts at the kernels' tile edges, 20 / 10 / 6 dB, equaliser off and on;
  d. negative controls: mutations of the reference's own parameters must fail c."""
import collections

import numpy as np
import pytest

import ref_decode as R
import ref_detect as rd
import ref_sync as rs
from sync_cases import BIN, SHAPES, SMALL_COUNTS, TILE_COUNTS, USER_HEADER, menu_counts, props

TWO_PI = 2.0 * np.pi
LEAD = 700
DS = [-0.75, -0.5, -0.3, 0.0, 0.25, 0.5, 0.77, 1.25]          # test_ref_detect's delays across the start/tau wrap
GAINS = [1e-6, 1.0, 1e8]
CFOS = [5 * BIN, -7.25 * BIN]                                 # a bin centre and a quarter bin


@pytest.fixture(scope="module")
def tb(oracle):
    return rs.Tables.from_oracle(oracle)


@pytest.fixture(scope="module")
def tx_taps(oracle):
    return oracle.table("fxr_tx_taps", 29, complex_=False).astype(np.float64)


# ---------------------------------------------------------------------------------------------------- a. the prototype
def _train(tx_taps, nsym=48, seed=5):
    """a noise-free pulse train: nsym QPSK symbols through the 29-tap interpolator, zeros either side (float64)"""
    rng = np.random.default_rng(seed)
    s = ((2 * rng.integers(0, 2, nsym) - 1) + 1j * (2 * rng.integers(0, 2, nsym) - 1)) / np.sqrt(2.0)
    up = np.zeros(2 * nsym, np.complex128)
    up[::2] = s
    return np.concatenate([np.zeros(64, np.complex128), np.convolve(up, tx_taps), np.zeros(64, np.complex128)])


def _branch(tb, b):
    return tb.proto[b + rs.NPFB * np.arange(rs.MF_TAPS)]


def test_prototype_symmetry_and_nyquist(tb, tx_taps):
    """h[i] = h[896 - i]; the TX pulse delayed by b / 32 samples through branch b, scaled by 0.5 and sampled every 2 samples,
    is 1 at its centre and ISI elsewhere.  Bounds.  The yardstick is measured on other data, the 29 TX taps alone: the ISI of
    the TX pulse with itself (its autocorrelation at the even lags), the design's own residual -- the approximate r-Kaiser
    pulse is only nearly root-Nyquist.  Branch 0 is the same design sampled at the same instants, and branch b with the
    pulse delayed by b / 32 the same pair again, up to the bank's interpolation error, which test_prototype_direction
    measures at 3 % of a branch step: the allowance is 1 dB over the yardstick for every branch.  The yardstick itself is
    pinned to the design's value, -50.8 dB (m = 7, beta = 0.3), within 1 dB either way."""
    assert np.array_equal(tb.proto, tb.proto[::-1])
    ac = 0.5 * np.convolve(tx_taps, tx_taps[::-1])[0::2]             # lags -28, -26, ..., 28: the centre is index 14
    own = np.sqrt(np.sum(ac ** 2) - ac[14] ** 2)
    assert abs(ac[14] - 1.0) < 1e-6 and abs(20 * np.log10(own) + 50.8) <= 1.0, (ac[14], 20 * np.log10(own))
    worst_isi, worst_peak = 0.0, 0.0
    for b in range(32):
        p = np.zeros(256, np.complex128)
        p[100:129] = tx_taps
        g = 0.5 * np.convolve(rd.fractional_delay(p, b / 32.0), _branch(tb, b))
        centre = 100 + 14 + 14          # the TX pulse's centre (14) + branch 0's delay (448 / 32 = 14); branch b reads b / 32 later
        sym = g[centre % 2::2]
        k0 = centre // 2
        isi = np.sqrt(np.sum(np.abs(sym) ** 2) - abs(sym[k0]) ** 2)
        worst_isi, worst_peak = max(worst_isi, isi), max(worst_peak, abs(sym[k0] - 1.0))
        assert abs(g[centre].imag) < 1e-9
    print("\nTX pulse with itself: rms ISI %.4g (%.2f dB); TX pulse x receive branch, all 32 branches: worst rms ISI %.4g (%.2f dB), worst |peak - 1| %.3g"
          % (own, 20 * np.log10(own), worst_isi, 20 * np.log10(worst_isi), worst_peak))
    assert worst_isi <= own * 10.0 ** (1.0 / 20.0) and worst_peak <= 1e-4


def test_prototype_direction(tb, tx_taps):
    """A pulse train delayed by b / 32 samples and filtered by branch b equals the undelayed train through branch 0.
    Bound: one branch step is the unit.  d1 = rms(branch 1 - branch 0) on the undelayed train is what a timing shift of 1/32
    sample does.  A correct bank leaves only the interpolation error of the bank itself (the prototype is a windowed sinc
    sampled 32 times finer than the signal; its spectrum beyond the signal's Nyquist band is the window's stopband), far
    under one step; a bank indexed the wrong way reads branch b where 32 - b belongs: 2 b / 32 samples off, i.e. >= 2 steps
    for every b except 0 and 16.  Bound: d1 / 2 -- a factor 4 under the smallest wrong-way error."""
    x = _train(tx_taps)
    ref = np.convolve(x, _branch(tb, 0))
    d1 = np.sqrt(np.mean(np.abs(np.convolve(x, _branch(tb, 1)) - ref) ** 2))
    worst, wrong_min = 0.0, np.inf
    for b in range(32):
        xd = rd.fractional_delay(x, b / 32.0)
        e = np.sqrt(np.mean(np.abs(np.convolve(xd, _branch(tb, b)) - ref) ** 2))
        worst = max(worst, e)
        assert e <= 0.5 * d1, (b, e, d1)
        if b not in (0, 16):
            ew = np.sqrt(np.mean(np.abs(np.convolve(xd, _branch(tb, (32 - b) % 32)) - (ref if b < 16 else np.concatenate([ref[1:], [0]]))) ** 2))
            wrong_min = min(wrong_min, ew)
    print("\nbranch direction: one step d1 = %.3g rms, worst right-way error %.3g, smallest wrong-way error %.3g" % (d1, worst, wrong_min))
    assert wrong_min >= 1.5 * d1


# ---------------------------------------------------------------------------------------------------- traffic
def test_symbol_count_menu():
    """the counts sync_cases.SHAPES aims at: every count in 0..10 that the menu reaches is a shape, and 1, 9 and 1025 are not
    on the menu (a coded byte is 8 bits: one byte is at least 2 symbols at 6 bits each, and no bps in 1..6 puts a byte
    boundary in (8, 9] or (1024, 1025] symbols)"""
    menu = menu_counts()
    assert {c for c in menu if c <= 10} == SMALL_COUNTS and not ({1, 9, 1025} & menu)
    below = sorted(c for c in menu if c < 1024)[-3:]
    above = sorted(c for c in menu if c > 1024)[:3]
    assert below == [1021, 1022, 1023] and above == [1026, 1027, 1028]
    got = {c for _, c in SHAPES}
    assert SMALL_COUNTS | TILE_COUNTS <= got and {ms for ms, _ in SHAPES} == set(R.PAYLOAD_MODS) and max(got) > 2048


Case = collections.namedtuple("Case", "name ms check payload sent x info oframe eq snr")


def _one(oracle, name, ms, check, payload, d, gain, cfo, phase, snr, seed, eq=False, echo=None):
    fr = oracle.gen_frame(payload, mod=ms, fec0=oracle.FEC_NONE, fec1=oracle.FEC_NONE, check=check, header=np.frombuffer(USER_HEADER, np.uint8)).astype(np.complex128)
    y = rd.channel(fr, LEAD, d, gain, cfo, phase, snr, np.random.default_rng(seed), LEAD + len(fr) + 900)
    if echo is not None:
        y = np.convolve(y, echo)[:len(y)]
    x = y.astype(np.complex64)
    s = oracle.Sync(equalizer=eq)
    got = list(s.execute(x))
    s.close()
    assert len(got) >= 1 and abs(got[0].info["start"] - LEAD - d) < 2, (name, [g.info["start"] for g in got])
    pts, lab = R.constellation(ms)
    enc = R.packet_encode(payload, check, R.FEC_NONE, R.FEC_NONE)
    n = R.num_symbols(ms, len(enc))
    bits = np.zeros(n * R.bps(ms), np.uint8)
    bits[:8 * len(enc)] = R.bits_of(enc)
    labels = R.words_of(bits, R.bps(ms)) if n else np.zeros(0, np.int64)
    if ms in R.DPSK:
        inv = {int(g): i for i, g in enumerate(R.gray(np.arange(len(pts))))}
        idx = np.cumsum([inv[int(v)] for v in labels]) % len(pts) if n else np.zeros(0, np.int64)
        sent = pts[idx]
    else:
        where = {int(v): i for i, v in enumerate(lab)}
        sent = pts[[where[int(v)] for v in labels]] if n else np.zeros(0, np.complex128)
    return Case(name, ms, check, payload.tobytes(), (labels, sent), x, got[0].info, got[0], eq, snr)


@pytest.fixture(scope="module")
def grid(oracle):
    """b's noise-free frames: delays across the wrap x a bin centre / a quarter bin x gains 1e-6 / 1 / 1e8 (PSK4, 252 symbols)"""
    out = []
    pl = np.random.default_rng(1).integers(0, 256, 60, dtype=np.uint8)
    for i, d in enumerate(DS):
        for j, cfo in enumerate(CFOS):
            for k, g in enumerate(GAINS):
                out.append(_one(oracle, "grid d=%g cfo=%.4f g=%g" % (d, cfo, g), R.PSK4, R.CRC_24, pl, d, g, cfo, [3.1, -0.4, 1.3][(i + j + k) % 3], None, 7))
    return out


@pytest.fixture(scope="module")
def shaped(oracle):
    """c's cases: {shape index: [frames at 20, 10, 6 dB (equaliser off) and at 20 dB with the equaliser on]}"""
    out = {}
    for i, (ms, count) in enumerate(SHAPES):
        chk, n = props(ms, count, i)
        pl = np.random.default_rng(100 + i).integers(0, 256, n, dtype=np.uint8)
        frames = []
        for j, (snr, eq) in enumerate([(20.0, False), (10.0, False), (6.0, False), (20.0, True)]):
            d, g = DS[(i + 3 * j) % len(DS)] + 0.013 * j, GAINS[(i + j) % 3]
            frames.append(_one(oracle, "%d syms of mod %d at %g dB%s" % (count, ms, snr, " eq" if eq else ""), ms, chk, pl, d, g,
                               ((i * 7 + j * 3) % 41 - 20 + 0.25 * (i % 4)) * BIN, 0.7 * i - 2.0 * j, snr, 1000 + 10 * i + j, eq=eq))
        out[i] = frames
    return out


_REF = {}


def _ref(c, tb, **mut):
    key = (c.name, tuple(sorted(mut.items())))
    if key not in _REF:
        i = c.info
        _REF[key] = rs.sync(c.x, i["start"], i["tau"], i["gamma"], i["dphi"], i["phi"], tb, equalizer=c.eq, **mut)
    return _REF[key]


def _against_oracle(c, ref):
    """ref_sync.compare against the oracle's frame, plus the hard labels through the payload bytes: with no FEC the
    reference's labels packed and decoded by ref_decode must give the oracle's payload and validity"""
    f, i = c.oframe, c.info
    if not ref["header_valid"] or "r" not in ref:
        bad = ["reference finds no valid header / payload"]
        if "pilot_dphi" in ref:
            d = dict(dphi=abs(ref["pilot_dphi"] - i["pilot_dphi"]), gain_rel=abs(ref["pilot_gain"] - i["pilot_gain"]) / i["pilot_gain"])
            bad += ["pilot %s off by %.3g (bound %.3g)" % (k, v, rs.PILOT[k]) for k, v in d.items() if v > rs.PILOT[k]]
        return bad, dict(sym=np.inf), 0, False
    bad, w, n, cut = rs.compare(ref, i, f.framesyms, f.header, full_evm_sum=i["evm_sum"], check_branch=not rs.near_branch_edge(i["tau"]))
    if not cut and len(ref["r"]) == len(f.framesyms):
        p = ref["props"]
        l1 = R.packet_dims(p["payload_len"], p["check"], p["fec0"], p["fec1"])[2]
        pay, ok = R.packet_decode(R.symbols_to_bytes(p["ms"], ref["labels"], l1), p["payload_len"], p["check"], p["fec0"], p["fec1"])
        if (pay, ok) != (f.payload, f.payload_valid):
            bad.append("hard labels differ (payload bytes / validity)")
    return bad, w, n, cut


# ---------------------------------------------------------------------------------------------------- b. truth
def _evm_db(r, sent):
    return 10.0 * np.log10(np.mean(np.abs(r - sent) ** 2))


def test_truth_noise_free_frames_land_on_the_sent_points(oracle, tb, grid):
    """The reference's payload symbols against the *transmitted* points (payload re-encoded by ref_decode.packet_encode and
    mapped through ref_decode.constellation), header against the sent header.  Allowed error: ref_detect.evm_bounds_db(None)."""
    worst = -np.inf
    for c in grid:
        ref = _ref(c, tb)
        assert ref["header_valid"] and ref["header"][:14] == USER_HEADER, c.name
        assert ref["props"] == dict(payload_len=60, ms=R.PSK4, check=R.CRC_24, fec0=R.FEC_NONE, fec1=R.FEC_NONE)
        assert np.array_equal(ref["labels"], c.sent[0]), c.name
        _, delta = rd.residual([q for q in CFOS if ("cfo=%.4f" % q) in c.name][0])
        lo, hi = rd.evm_bounds_db(None, len(ref["r"]), delta)
        e = _evm_db(ref["r"], c.sent[1])
        worst = max(worst, e)
        assert e <= hi, (c.name, e, hi)
    print("\ntruth: %d noise-free frames, worst EVM against the sent points %.1f dB (floor %.1f dB)" % (len(grid), worst, hi))


def test_truth_rejects_the_other_reading_of_the_symbol_grid(oracle, tb, grid):
    """symbol instants one sample later (ref_sync's header: the other reading of the timing rule) miss the sent points by
    half a symbol: the header fails or the EVM is near 0 dB"""
    for c in grid[::7]:
        ref = _ref(c, tb, late=1)
        assert (not ref["header_valid"]) or _evm_db(ref["r"], c.sent[1]) > -10.0, c.name


def test_truth_with_the_equaliser_on_a_two_ray_channel(oracle, tb):
    """Two rays (the direct one and 0.35 exp(j 1.1) three samples later), noise-free: with the equaliser the symbols land on
    the sent points with a lower EVM than without (by more than 1 dB, test_equalizer_stage_on_a_multipath_channel's mark)."""
    echo = np.zeros(4, np.complex128); echo[0] = 1.0; echo[3] = 0.35 * np.exp(1j * 1.1)
    pl = np.random.default_rng(2).integers(0, 256, 60, dtype=np.uint8)
    for d, cfo in ((0.25, 3 * BIN), (-0.3, -11.25 * BIN)):
        e = {}
        for eq in (False, True):
            c = _one(oracle, "two-ray d=%g eq=%d" % (d, eq), R.PSK4, R.CRC_24, pl, d, 1.0, cfo, 0.5, None, 3, eq=eq, echo=echo)
            ref = _ref(c, tb)
            assert ref["header_valid"] and ref["header"][:14] == USER_HEADER
            assert np.array_equal(ref["labels"], c.sent[0]), c.name
            e[eq] = _evm_db(ref["r"], c.sent[1])
            bad, w, n, cut = _against_oracle(c, ref)
            assert not bad and not cut, (c.name, bad)
        print("\ntwo-ray channel d=%g: EVM %.1f dB without, %.1f dB with the equaliser" % (d, e[False], e[True]))
        assert e[True] < e[False] - 1.0


# ---------------------------------------------------------------------------------------------------- c. oracle vs reference
def test_oracle_against_the_reference(oracle, tb, grid, shaped):
    worst = collections.defaultdict(float)
    cases = [[c] for c in grid] + list(shaped.values())
    frames = cut_frames = edge = invalid = 0
    for group in cases:
        full = 0
        for c in group:
            if not c.oframe.header_valid:
                invalid += 1
                continue
            ref = _ref(c, tb)
            bad, w, n, cut = _against_oracle(c, ref)
            assert not bad, (c.name, bad, c.info)
            frames += 1
            cut_frames += int(cut)
            edge += int(rs.near_branch_edge(c.info["tau"]))
            full += int(not cut)
            assert not (cut and c.snr is None), c.name
            for k, v in w.items():
                worst[k] = max(worst[k], v)
            if w["evm_bound"]:
                worst["evm / bound"] = max(worst["evm / bound"], w["evm"] / w["evm_bound"])
        assert full >= 1, group[0].name
    print("\nreference vs oracle: %d frames (%d with an invalid header skipped), %d cut short by a tie, %d at a branch edge" % (frames, invalid, cut_frames, edge))
    print("worst differences: sym %.3g (bound %.3g), pilot dphi %.3g (%.3g), phi %.3g (%.3g), gain_rel %.3g (%.3g), evm_sum / its bound %.3g, sym / sym_tol(r) %.3g"
          % (worst["sym"], rs.SYM_TOL, worst["dphi"], rs.PILOT["dphi"], worst["phi"], rs.PILOT["phi"], worst["gain_rel"], rs.PILOT["gain_rel"], worst["evm / bound"], worst["sym_ratio"]))
    assert cut_frames < 0.02 * frames and invalid <= 3
    # the bounds in force are the derived ones, and they keep their float32 headroom over what this run saw
    assert rs.SYM_TOL <= 1e-4
    assert 4.0 * worst["sym"] <= rs.SYM_TOL and 4.0 * worst["sym_ratio"] <= 1.0 and all(4.0 * worst[k] <= rs.PILOT[k] for k in rs.PILOT)
    m = rs.MEASURED["oracle"]                       # the recorded figures are this run's, rounded up: they cannot drift
    assert all(0.5 * m[k] <= worst[k] <= m[k] for k in m), ("ref_sync.MEASURED['oracle'] is not this run's", {k: worst[k] for k in m})


# ---------------------------------------------------------------------------------------------------- d. negative controls
CONTROLS = {
    "branch + 1": (dict(branch_shift=1), False),
    "symbol instants one sample late": (dict(late=1), False),
    "pilot index origin off by one": (dict(pilot_origin=1), False),
    "beta = 2e-2": (dict(beta=2e-2), False),
    "alpha and beta swapped": (dict(alpha=rs.BETA, beta=rs.ALPHA), False),
    "theta_0 without 231 dphi": (dict(theta0_symbols=0), False),
    "equaliser delay 2": (dict(eq_delay=2), True),
}


@pytest.mark.parametrize("name", sorted(CONTROLS))
def test_negative_controls_fail_against_the_oracle(oracle, tb, shaped, name):
    """each mutation of the reference's own parameters fails the comparison of c on every frame tried: a 1024-symbol 16-QAM
    frame and a 1022-symbol 8-PSK frame (quarter-bin CFOs: the pilots see a slope), at 20 dB"""
    mut, eq = CONTROLS[name]
    for si in (SHAPES.index((R.QAM16, 1024)), SHAPES.index((R.PSK8, 1022))):
        c = shaped[si][3 if eq else 0]
        good, _, _, _ = _against_oracle(c, _ref(c, tb))
        assert not good
        ref = _ref(c, tb, **mut)
        bad, w, n, cut = _against_oracle(c, ref)
        print("\n%s on %s: %s" % (name, c.name, "; ".join(bad)))
        numeric = [b for b in bad if not b.startswith(("pfb_index", "mf_counter0"))]
        assert numeric, (name, c.name)
