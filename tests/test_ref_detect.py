"""The front end of the receiver (qdetector SEEK / ALIGN and the framesync estimates) against two statements that share
no code with the oracle: tests/ref_detect.py's float64 restatement of one hop, and its truth model of the channel.
CPU only: the oracle's detector and receiver on frames sent through a float64 channel over every CFO bin, half-bin
ties, CFOs outside the sweep, fractional delays across the start/tau wrap, phases across +-pi and gains 1e-6 .. 1e8."""
import numpy as np
import pytest
import ref_detect as rd

TWO_PI = 2.0 * np.pi
BIN = TWO_PI / 512
LEAD = 700


@pytest.fixture(scope="module")
def tmpl(oracle):
    s = rd.build_template(oracle.table("fxr_preamble_pn", 64), oracle.table("fxr_tx_taps", 29, complex_=False))
    rd.set_template(s)
    return s


@pytest.fixture(scope="module")
def frame(oracle):
    pl = np.random.default_rng(1).integers(0, 256, 60, dtype=np.uint8)
    return oracle.gen_frame(pl, mod=2, fec0=oracle.FEC_NONE, fec1=oracle.FEC_NONE, check=oracle.CRC_24).astype(np.complex128), pl.tobytes()


def _grid():
    """(cfo, d, phase, gain, snr) points: every bin centre, half-bin ties, outside the sweep; delays across the wrap."""
    g = []
    ds = [-0.75, -0.5, -0.3, 0.0, 0.25, 0.5, 0.77, 1.25]
    for i, k in enumerate(range(-24, 25)):
        g.append((k * BIN, ds[i % len(ds)], [np.pi - 1e-3, -np.pi, 0.4][i % 3], [1e-6, 1e-3, 1.0, 32767.0, 1e8][i % 5], None))
    for i, k in enumerate([-23.5, -12.5, -0.5, 0.5, 11.5, 23.5]):
        g.append((k * BIN, ds[(i + 3) % len(ds)], 2.0, 1.0, None))
    for i, c in enumerate([0.31, -0.31, 0.35, -0.35]):
        g.append((c, [0.0, 0.5, -0.5, 0.25][i], -2.0, 1.0, None))
    for i, k in enumerate([-24, -17, -6, 6, 17, 24]):
        g.append((k * BIN, ds[(i + 5) % len(ds)], 1.0, [1e-6, 1.0, 1e8][i % 3], 20.0))
    return g


GRID = _grid()


def _run(oracle, frame, cfo, d, phase, gain, snr, seed):
    y = rd.channel(frame, LEAD, d, gain, cfo, phase, snr, np.random.default_rng(seed), LEAD + len(frame) + 1500).astype(np.complex64)
    s = oracle.Sync()
    fr = list(s.execute(y))
    s.close()
    return y, fr


def test_template_rebuilt_from_symbols_and_pulse(oracle, tmpl):
    """The template rebuilt in float64 from the p/n symbols and the 29 taps is the oracle's table to float32 rounding;
    the correlation is its definition (direct sum at a few bins and lags)."""
    st = oracle.table("fxr_template", 156).astype(np.complex128)
    assert np.abs(tmpl - st).max() <= 4 * 2.0 ** -24 * np.abs(st).max()
    rng = np.random.default_rng(3)
    x = rng.standard_normal(512) + 1j * rng.standard_normal(512)
    r = rd.xcorr(x, tmpl)
    m = np.arange(156)
    for k in (-24, -1, 0, 13, 24):
        for lag in (0, 1, 300, 511):
            want = 512 * np.sum(x[(m + lag) % 512] * np.conj(tmpl) * np.exp(-1j * TWO_PI * k * m / 512))
            assert abs(r[k + 24, lag] - want) <= 1e-9 * abs(want) + 1e-9


def test_ref_detect_against_the_oracle_detector(oracle, tmpl, frame):
    """Oracle qdetector (fxr_qdet_*) against the float64 hop: same position and bin (or a float64 tie), estimates within
    the float32 bounds of ref_detect.PARITY, recomputed on the oracle's own aligned window."""
    ties = 0
    worst = dict.fromkeys(rd.PARITY, 0.0)
    for j, (cfo, d, ph, g, snr) in enumerate(GRID):
        y = rd.channel(frame[0], LEAD, d, g, cfo, ph, snr, np.random.default_rng(j), LEAD + len(frame[0]) + 1500).astype(np.complex64)
        det = oracle.Detector(0.5).run(y)
        pos, h = rd.walk(y, tmpl, 0.5)
        assert bool(det) == (pos is not None), (cfo, d, g)
        if not det:                                 # only beyond the sweep, where the loss of a 0.06 rad/sample residual
            assert abs(cfo) > 0.33                  # over the template takes the peak under the threshold
            continue
        o = det[0]
        if abs(cfo) > 24 * BIN + BIN / 2:
            assert o["offset"] == np.sign(cfo) * 24
        if o["offset"] != h["bin"]:
            assert h["margin"] <= rd.TIE_MARGIN and abs(o["offset"] - h["bin"]) == 1, (cfo, o["offset"], h["bin"], h["margin"])
            ties += 1
        assert o["pos"] == pos, (cfo, d, o["pos"], pos)
        assert abs(o["rxy"] - h["rxy"]) <= 2e-5 * h["rxy"]
        a = rd.align(y[pos:pos + 512], tmpl, o["offset"])
        ok, e = rd.parity_ok(a, o)
        assert ok, (cfo, d, g, e)
        worst = {k: max(worst[k], e[k]) for k in worst}
    print("ref_detect vs oracle detector: %d frames, %d half-bin ties, worst %s" % (len(GRID), ties, worst))


def test_oracle_receiver_against_the_channel(oracle, tmpl, frame):
    """oracle.Sync's estimates and framesyncstats against the truth model of the channel that made the frame."""
    for j, (cfo, d, ph, g, snr) in enumerate(GRID):
        y, fr = _run(oracle, frame[0], cfo, d, ph, g, snr, 100 + j)
        if abs(cfo) > 0.33 and not fr:
            continue
        assert len(fr) == 1, (cfo, d, g, len(fr))
        f = fr[0]
        i = f.info
        assert f.payload_valid and f.payload == frame[1], (cfo, d, g)
        est = dict(start=i["start"], tau=i["tau"], dphi=i["dphi"], phi=i["phi"], gamma=i["gamma"], pilot_dphi=i["pilot_dphi"],
                   rssi_db=f.rssi, cfo=f.cfo, cfo_bin=i["offset"])
        bad = rd.check_truth(est, LEAD, d, g, cfo, ph, snr)
        _, delta = rd.residual(cfo)
        if abs(cfo) <= 24 * BIN + BIN / 2:
            lo, hi = rd.evm_bounds_db(snr, len(f.framesyms), delta)
            if not lo <= f.evm <= hi:
                bad.append("evm %.2f dB outside [%.2f, %.2f]" % (f.evm, lo, hi))
        assert not bad, (cfo, d, ph, g, snr, bad)
        # the polyphase branch and mf_counter follow tau's sign (both cases of the ALIGN hand-off)
        assert i["mf_counter0"] == (0 if i["tau"] > 0 else 1)


def test_generator_dt_is_an_advance(oracle, tmpl):
    """fxr_gen_frame(dt) designs the pulse at t = i - (n-1)/2 + dt (liquid's firdes convention): the frame comes out dt
    samples EARLY, so the detector reports tau ~ -dt."""
    pl = np.zeros(8, np.uint8)
    for dt in (-0.4, -0.2, 0.2, 0.4):
        x = np.concatenate([np.zeros(LEAD, np.complex64), oracle.gen_frame(pl, fec0=oracle.FEC_NONE, dt=dt), np.zeros(1500, np.complex64)])
        s = oracle.Sync()
        f = s.execute(x)[0].info
        s.close()
        assert abs(f["start"] + f["tau"] - (LEAD - dt)) <= 0.04, (dt, f["start"], f["tau"])
        assert abs(f["start"] + f["tau"] - (LEAD + dt)) > 0.3


def test_silence_below_the_energy_cut(oracle, tmpl, frame):
    """At gain 1e-12 the window energy is under the detector's g0 < 1e-10 cut: oracle and ref both find nothing."""
    y = rd.channel(frame[0], LEAD, 0.2, 1e-12, 5 * BIN, 0.3, 20.0, np.random.default_rng(9), LEAD + len(frame[0]) + 1500).astype(np.complex64)
    assert oracle.Detector(0.5).run(y) == []
    assert rd.walk(y, tmpl, 0.5) == (None, None)
    _, fr = _run(oracle, frame[0], 5 * BIN, 0.2, 0.3, 1e-12, 20.0, 9)
    assert fr == []


# ---------------------------------------------------------------------------------------------------- negative controls
def _good_estimate(oracle, frame, cfo, d, ph, g):
    _, fr = _run(oracle, frame[0], cfo, d, ph, g, None, 7)
    i = fr[0].info
    return dict(start=i["start"], tau=i["tau"], dphi=i["dphi"], phi=i["phi"], gamma=i["gamma"], pilot_dphi=i["pilot_dphi"],
                rssi_db=fr[0].rssi, cfo=fr[0].cfo, cfo_bin=i["offset"])


WRONG = {
    "tau negated": lambda e: dict(e, tau=-e["tau"]),
    "dphi in rad/symbol": lambda e: dict(e, dphi=2 * e["dphi"], cfo=2 * e["cfo"]),
    "phi at the template centre": lambda e: dict(e, phi=e["phi"] + rd.TEMPLATE_CENTRE * e["dphi"]),
    "start + 1 without tau": lambda e: dict(e, start=e["start"] + 1),
    "start - 1 without tau": lambda e: dict(e, start=e["start"] - 1),
    "cfo_bin + 1": lambda e: dict(e, cfo_bin=e["cfo_bin"] + 1, dphi=e["dphi"] + BIN, cfo=e["cfo"] + BIN),
    "cfo_bin - 1": lambda e: dict(e, cfo_bin=e["cfo_bin"] - 1, dphi=e["dphi"] - BIN, cfo=e["cfo"] - BIN),
    "gamma squared": lambda e: dict(e, gamma=e["gamma"] ** 2, rssi_db=2 * e["rssi_db"]),
}


@pytest.mark.parametrize("snr", [None, 20.0, 8.0])
@pytest.mark.parametrize("name", sorted(WRONG))
def test_truth_checker_rejects_wrong_receivers(oracle, tmpl, frame, name, snr):
    """A receiver that makes any of these mistakes fails the truth bounds at every SNR the GPU tests use (the bounds are
    widest at 8 dB): the channel is a far bin, a fractional delay of 0.3, a phase away from 0 and a gain away from 1."""
    cfo, d, ph, g = 17 * BIN, 0.3, 2.2, 3.0
    good = _good_estimate(oracle, frame, cfo, d, ph, g)
    assert rd.check_truth(good, LEAD, d, g, cfo, ph, snr) == []
    bad = rd.check_truth(WRONG[name](good), LEAD, d, g, cfo, ph, snr)
    assert bad, name


def test_each_truth_tolerance_fails_a_negative_control(oracle, tmpl, frame):
    """Every bound of rd.tolerances is the one that rejects at least one control (at 20 dB)."""
    cfo, d, ph, g = 17 * BIN, 0.3, 2.2, 3.0
    good = _good_estimate(oracle, frame, cfo, d, ph, g)
    hit = set()
    for f in WRONG.values():
        for b in rd.check_truth(f(good), LEAD, d, g, cfo, ph, 20.0):
            hit.add(b.split(" ")[0])
    assert {"arrival", "dphi", "centre", "gamma", "rssi", "stats", "cfo_bin"} <= hit, hit
