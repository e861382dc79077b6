"""The HIP front end over the whole channel range (`-m gpu`): every CFO bin of the detector sweep, half-bin ties, CFOs
outside the sweep, every polyphase branch on both sides of tau = 0, phases across +-pi, gains 1e-6 .. 1e8 at fixed SNR
and 1e-12 (silence), noise-free / 20 dB / 8 dB.  Each frame goes through its own float64 channel (noise scaled with the
gain); frames are laid back to back, one stream per (gain, SNR).  Three checks on every frame: exact oracle parity, the
float64 hop of tests/ref_detect.py on the kernel's own aligned window, and the truth model of the channel.  Coverage
floors keep the traffic honest.  Also: fxtx_apply_channel (the device channel of synth_streams_device) against float64."""
import ctypes as C
from collections import Counter

import numpy as np
import pytest
import ref_detect as rd
from parity_util import oracle_frames, compare_frames

pytestmark = pytest.mark.gpu

TWO_PI = 2.0 * np.pi
BIN = TWO_PI / 512
PRE, GAP = 400, 700                  # zeros before each frame's arrival / after it, inside its channel segment
GAINS = [1e-6, 1e-3, 1.0, 32767.0, 1e8]
SNRS = [None, 20.0, 8.0]


def _cfos(snr):
    """Bin centres -24..24, exact half-bin points, and CFOs outside the sweep (+-0.35 only noise-free, where the peak
    still clears the threshold)."""
    c = [k * BIN for k in range(-24, 25)]
    c += [(k + 0.5) * BIN for k in (-24, -13, -7, -1, 0, 6, 12, 23)]
    c += [0.31, -0.31] + ([0.35, -0.35] if snr is None else [])
    return c


# tau over every branch: d = (j + 0.5) / 32 - 0.5 puts tau ~ -d... in each 1/32 cell of (-0.5, 0.5); plus d = +-0.5 exactly
DELAYS = [(j + 0.5) / 32.0 - 0.5 for j in range(32)] + [0.5, -0.5]
PHASES = [np.pi - 1e-4, -np.pi, np.pi / 2, -3.0, 0.0, 3.1]


@pytest.fixture(scope="module")
def tmpl(oracle):
    s = rd.build_template(oracle.table("fxr_preamble_pn", 64), oracle.table("fxr_tx_taps", 29, complex_=False))
    rd.set_template(s)
    return s


def _stream(fx, gain, snr, seed):
    """One stream: a frame per CFO of the grid, each through its own channel.  Returns (complex64 samples, channel list)."""
    rng = np.random.default_rng(seed)
    g = fx.FrameGen(2, 11, 1, fx.CRC_24)                 # PSK4, r1/2 convolutional, CRC-24
    parts, chans, off = [], [], 0
    for j, cfo in enumerate(_cfos(snr)):
        pl = rng.integers(0, 256, 48, dtype=np.uint8)
        fr = g.frame(pl).astype(np.complex128)
        d = DELAYS[(j + seed) % len(DELAYS)]
        ph = PHASES[(j + seed) % len(PHASES)]
        n = PRE + len(fr) + GAP
        # the segment's own sample 0 is stream sample `off`: phase referred to the stream's sample 0
        y = rd.channel(fr, PRE, d, gain, cfo, ph, snr, rng, n)
        parts.append(y)
        chans.append(dict(lead=off + PRE, d=d, gain=gain, cfo=cfo, phase=ph - cfo * off, payload=pl.tobytes(), snr=snr))
        off += n
    g.close()
    return np.concatenate(parts).astype(np.complex64), chans


@pytest.fixture(scope="module")
def traffic(fx):
    """(streams, channels, (gain, snr) labels): one stream per gain and SNR, plus a silent one at gain 1e-12."""
    xs, chs, lab = [], [], []
    for si, snr in enumerate(SNRS):
        for gi, gain in enumerate(GAINS):
            x, c = _stream(fx, gain, snr, 10 * si + gi)
            xs.append(x); chs.append(c); lab.append((gain, snr))
    x, c = _stream(fx, 1e-12, 20.0, 99)
    xs.append(x); chs.append(c); lab.append((1e-12, 20.0))
    return xs, chs, lab


def _match(chans, start):
    """The channel whose frame a detection at `start` belongs to (None: not a frame of the grid)."""
    for c in chans:
        if abs(start - c["lead"]) <= 2:
            return c
    return None


def _check_frames(fx, frames, x, chans, snr, tmpl, stats, mode_key):
    """ref_detect on the kernel's aligned window + truth on every frame; coverage counters into stats."""
    for f in frames:
        c = _match(chans, f["start"])
        if c is None and mode_key == "det":
            # the detector alone does not skip a frame's body: its data can cross the threshold again (as in the oracle)
            stats["other_det"] = stats.get("other_det", 0) + 1
            continue
        if c is None:
            # the only other detections: inside the segment of a frame at +-0.35, beyond the sweep, whose preamble the
            # detector does not find (its p/n symbols then meet the template at a wrong lag / bin)
            assert any(abs(q["cfo"]) > 0.33 and q["lead"] - PRE <= f["start"] < q["lead"] + 2600 for q in chans), f["start"]
            stats["stray_" + mode_key] = stats.get("stray_" + mode_key, 0) + 1
            continue
        win = x[f["start"]:f["start"] + 512]
        a = rd.align(win, tmpl, f["cfo_bin"])
        ok, e = rd.parity_ok(a, f)
        assert ok, (mode_key, c["cfo"], c["d"], e)
        est = dict(start=f["start"], tau=f["tau"], dphi=f["dphi"], phi=f["phi"], gamma=f["gamma"], cfo_bin=f["cfo_bin"])
        if mode_key == "flex":
            est.update(rssi_db=f["rssi_db"], cfo=f["cfo"])
            if f["header_valid"]:
                est["pilot_dphi"] = f["pilot_dphi"]
        bad = rd.check_truth(est, c["lead"], c["d"], c["gain"], c["cfo"], c["phase"], snr)
        assert not bad, (mode_key, c["cfo"], c["d"], c["gain"], snr, bad)
        stats["bins_" + mode_key][f["cfo_bin"]] += 1
        if "pfb_index" in f and mode_key == "flex":
            stats["pfb"][f["pfb_index"]] += 1
        _, delta = rd.residual(c["cfo"])
        if abs(abs(delta) - BIN / 2) < 1e-9:
            stats["half_bin_" + mode_key] += 1


def _oracle_all(oracle, xs, **kw):
    return [oracle_frames(oracle, x, **kw) for x in xs]


@pytest.fixture(scope="module")
def oracle_rx(oracle, traffic):
    return _oracle_all(oracle, traffic[0])


CONFIGS = [("default", {}, 0), ("skip_seek_0", {}, 0), ("seg4k", {}, 4096), ("seg64k", {}, 65536), ("seg1M", {}, 1 << 20)]


def test_flex_rx_over_the_channel_range(fx, oracle, tmpl, traffic, oracle_rx, monkeypatch):
    """Batched RxContext, default configuration, FXRX_SKIP_SEEK=0 and segment lengths 4 Ki .. 1 Mi samples: exact parity
    with the oracle, the float64 hop on the kernel's windows, the channel's truth; coverage floors."""
    xs, chs, lab = traffic
    stats = dict(bins_flex=Counter(), pfb=Counter(), half_bin_flex=0)
    repairs, vfail = {}, Counter()
    decoded = Counter()
    for name, kw, seg in CONFIGS:
        if name == "skip_seek_0":
            monkeypatch.setenv("FXRX_SKIP_SEEK", "0")
        else:
            monkeypatch.delenv("FXRX_SKIP_SEEK", raising=False)
        ctx = fx.RxContext(len(xs), want_framesyms=True, segment_len=seg, **kw)
        got = ctx.process(xs)
        tm = ctx.timing()
        ctx.close()
        repairs[name] = tm["repairs"]
        for s, x in enumerate(xs):
            mine = [g for g in got if g["stream"] == s]
            compare_frames(oracle_rx[s], mine)
            gain, snr = lab[s]
            if gain < 1e-10:
                assert mine == [], "frames found in silence"
                continue
            if name == "default":
                _check_frames(fx, mine, x, chs[s], snr, tmpl, stats, "flex")
                for f in mine:
                    c = _match(chs[s], f["start"])
                    if c is None:
                        continue
                    if f["payload_valid"] and f["payload"] == c["payload"]:
                        decoded[(gain, snr)] += 1
                    _, delta = rd.residual(c["cfo"])
                    if f["header_valid"] and snr != 8.0 and abs(c["cfo"]) <= 24 * BIN + BIN / 2:
                        lo, hi = rd.evm_bounds_db(snr, f["num_framesyms"], delta)
                        assert lo <= f["evm_db"] <= hi, (gain, snr, c["cfo"], c["d"], f["evm_db"], lo, hi)
        if name == "default":
            vfail["total"] = tm["verify_failures"]
    print("flex_rx bins won:", dict(sorted(stats["bins_flex"].items())))
    print("pfb branches reached:", len(stats["pfb"]), dict(sorted(stats["pfb"].items())))
    print("half-bin frames:", stats["half_bin_flex"], "stray detections beyond the sweep:", stats.get("stray_flex", 0), "repairs per segmentation:", repairs, "verify_failures (default):", vfail["total"])
    print("decoded per (gain, snr):", dict(decoded))
    assert set(stats["bins_flex"]) >= set(range(-24, 25)), sorted(set(range(-24, 25)) - set(stats["bins_flex"]))
    assert set(stats["pfb"]) == set(range(32)), sorted(set(range(32)) - set(stats["pfb"]))
    for gain in GAINS:
        for snr in (None, 20.0):
            assert decoded[(gain, snr)] >= len(_cfos(snr)) - 2, (gain, snr, decoded[(gain, snr)])
    assert max(repairs.values()) > 0, repairs


def test_verify_failures_per_cfo_band(fx, oracle, tmpl, monkeypatch):
    """Report (no assertion beyond parity: the design does not promise it) how often the locked walker's differential
    coarse scan misses a preamble the full detector finds, per CFO band, on half-bin traffic at 8 dB."""
    monkeypatch.delenv("FXRX_SKIP_SEEK", raising=False)
    out = {}
    for band, ks in (("|k|<=5", [-5, -2, 0, 3, 5]), ("6..15", [-15, -9, 6, 11, 15]), ("16..24", [-24, -19, 16, 20, 24])):
        rng = np.random.default_rng(len(band))
        g = fx.FrameGen(2, 11, 1, fx.CRC_24)
        parts = []
        for rep in range(6):
            for k in ks:
                y = rd.channel(g.frame(rng.integers(0, 256, 48, dtype=np.uint8)).astype(np.complex128), PRE, DELAYS[rep * 5 % 34],
                               1.0, (k + 0.5 * np.sign(k or 1)) * BIN, PHASES[rep % 6], 8.0, rng, PRE + 1800 + GAP)
                parts.append(y)
        g.close()
        x = np.concatenate(parts).astype(np.complex64)
        of = oracle_frames(oracle, x)
        ctx = fx.RxContext(1, want_framesyms=True, segment_len=8192)
        compare_frames(of, ctx.process([x]))
        tm = ctx.timing()
        ctx.close()
        out[band] = (tm["verify_hops"], tm["verify_failures"], tm["repairs"], len(of))
    print("verify (hops, failures, repairs, frames) per CFO band at 8 dB, half-bin:", out)


@pytest.mark.parametrize("opt", ["equalizer", "soft_header"])
def test_options_keep_the_front_end(fx, oracle, tmpl, traffic, opt):
    """The equalizer and soft_header options on the noise-free and 20 dB streams: exact parity (the equalizer against the
    oracle's equalizer; soft header decoding against the hard oracle on the streams where that decodes every header)."""
    xs, chs, lab = traffic
    sel = [s for s in range(len(xs)) if lab[s][1] != 8.0 and lab[s][0] > 1e-10]
    ctx = fx.RxContext(len(sel), want_framesyms=True, **{opt: True})
    got = ctx.process([xs[s] for s in sel])
    ctx.close()
    compared = 0
    for i, s in enumerate(sel):
        of = oracle_frames(oracle, xs[s], equalizer=(opt == "equalizer"))
        if opt == "soft_header" and not all(f.header_valid for f in of):
            continue                    # a header the hard decoder rejects may decode softly: then the frame lists differ
        compare_frames(of, [g for g in got if g["stream"] == i])
        compared += 1
    assert compared >= 5, compared


def test_detector_mode_over_the_channel_range(fx, oracle, tmpl, traffic):
    """frame_detector_cc path: positions and bins identical to the oracle's qdetector, estimates within 1e-5, the float64
    hop within ref_detect.PARITY on the kernel's windows, truth within the model's bounds; every bin won."""
    xs, chs, lab = traffic
    stats = dict(bins_det=Counter(), half_bin_det=0)
    ctx = fx.RxContext(len(xs), mode=fx.MODE_DETECTOR, threshold=0.5, segment_len=20000)
    got = ctx.process(xs)
    ctx.close()
    for s, x in enumerate(xs):
        od = oracle.Detector(0.5).run(x)
        mine = [g for g in got if g["stream"] == s]
        assert [d["pos"] for d in od] == [g["start"] for g in mine]
        assert [d["offset"] for d in od] == [g["cfo_bin"] for g in mine]
        for d, g in zip(od, mine):
            for k in ("tau", "gamma", "dphi", "phi", "rxy"):
                assert abs(d[k] - g[k]) <= 1e-5 * max(1.0, abs(d[k]) if k == "gamma" else 1.0), (k, d[k], g[k])
        gain, snr = lab[s]
        if gain < 1e-10:
            assert mine == []
            continue
        _check_frames(fx, mine, x, chs[s], snr, tmpl, stats, "det")
    print("detector bins won:", dict(sorted(stats["bins_det"].items())), "half-bin frames:", stats["half_bin_det"],
          "detections inside frame bodies:", stats.get("other_det", 0))
    assert set(stats["bins_det"]) >= set(range(-24, 25)), sorted(set(range(-24, 25)) - set(stats["bins_det"]))


def _far_bin_stream(fx):
    rng = np.random.default_rng(4242)
    g = fx.FrameGen(2, 11, 1, fx.CRC_24)
    parts, chans, off = [], [], 0
    for k, d, ph, gain in ((-24, 0.3, 2.0, 1.0), (-17.5, -0.4, -3.1, 1e3), (13, 0.5, 0.5, 1e-3), (24, -0.1, np.pi, 1.0), (0.31 / BIN, 0.2, 1.0, 1.0)):
        pl = rng.integers(0, 256, 48, dtype=np.uint8)
        fr = g.frame(pl).astype(np.complex128)
        n = PRE + len(fr) + GAP
        parts.append(rd.channel(fr, PRE, d, gain, k * BIN, ph, 20.0, rng, n))
        chans.append(dict(lead=off + PRE, d=d, gain=gain, cfo=k * BIN, phase=ph - k * BIN * off, payload=pl.tobytes()))
        off += n
    g.close()
    return np.concatenate(parts).astype(np.complex64), chans


def test_dropin_flexframesync_far_bins(fx, oracle, tmpl):
    """flexframesync_execute in 256-sample calls: framesyncstats cfo / rssi / evm equal the oracle's and match the channel."""
    L = fx.lib()
    x, chans = _far_bin_stream(fx)
    of = oracle_frames(oracle, x)
    got = []

    def cb(header, hv, payload, plen, pv, st, ud):
        got.append(dict(hv=hv, pv=pv, payload=C.string_at(payload, plen) if plen else b"", evm=st.evm, rssi=st.rssi, cfo=st.cfo))
        return 0
    cbf = fx._ffi.FRAMESYNC_CALLBACK(cb)
    q = L.flexframesync_create(cbf, None)
    assert q
    L.fxrx_sync_set_block(q, 8192)
    for i in range(0, len(x), 256):
        blk = x[i:i + 256]
        L.flexframesync_execute(q, blk.ctypes.data, len(blk))
    L.fxrx_sync_flush(q)
    while L.fxrx_sync_pending(q):
        L.flexframesync_execute(q, None, 0)
    L.flexframesync_destroy(q)
    assert len(got) == len(of) == len(chans)
    for a, b, c in zip(of, got, chans):
        assert (a.header_valid, a.payload_valid, a.payload) == (b["hv"], b["pv"], b["payload"]) and b["payload"] == c["payload"]
        assert abs(a.evm - b["evm"]) < 1e-3 and abs(a.rssi - b["rssi"]) < 1e-3 and abs(a.cfo - b["cfo"]) < 1e-6
        i = a.info
        est = dict(start=i["start"], tau=i["tau"], dphi=b["cfo"], phi=i["phi"], gamma=10.0 ** (b["rssi"] / 20.0), cfo=b["cfo"],
                   rssi_db=b["rssi"], pilot_dphi=i["pilot_dphi"])
        assert not rd.check_truth(est, c["lead"], c["d"], c["gain"], c["cfo"], c["phase"], 20.0), c


def test_dropin_qdetector_far_bins(fx, oracle, tmpl):
    """qdetector_cccf_execute per sample: every detection at the oracle's position with its estimates; the returned window
    fed to the float64 hop reproduces them."""
    L = fx.lib()
    x, chans = _far_bin_stream(fx)
    x = np.concatenate([x, np.zeros(70_000, np.complex64)])          # flush the block queue (64 Ki samples)
    od = oracle.Detector(0.5).run(x)
    pn = oracle.table("fxr_preamble_pn", 64)
    q = L.qdetector_cccf_create_linear(np.ascontiguousarray(pn).ctypes.data, 64, 7, 2, 7, C.c_float(0.3))
    assert q
    L.qdetector_cccf_set_threshold(q, 0.5)
    got = []
    xs = x.view(np.float32).reshape(-1, 2)
    for i in range(len(x)):
        p = L.qdetector_cccf_execute(q, fx._ffi.FxComplex(float(xs[i, 0]), float(xs[i, 1])))
        if p:
            win = np.frombuffer(C.cast(p, C.POINTER(C.c_float * 1024)).contents, np.complex64).copy()
            got.append(dict(tau=L.qdetector_cccf_get_tau(q), gamma=L.qdetector_cccf_get_gamma(q), dphi=L.qdetector_cccf_get_dphi(q),
                            phi=L.qdetector_cccf_get_phi(q), win=win))
    L.qdetector_cccf_destroy(q)
    assert len(got) == len(od)
    found = 0
    for d, g in zip(od, got):
        for k in ("tau", "gamma", "dphi", "phi"):
            assert abs(d[k] - g[k]) < 1e-5, (k, d[k], g[k])
        assert np.array_equal(g["win"], x[d["pos"]:d["pos"] + 512])
        ok, e = rd.parity_ok(rd.align(g["win"], tmpl, d["offset"]), g)
        assert ok, e
        c = _match(chans, d["pos"])
        if c is None:                   # the detector alone re-detects inside a frame's body, as the oracle does
            continue
        found += 1
        est = dict(start=d["pos"], tau=g["tau"], dphi=g["dphi"], phi=g["phi"], gamma=g["gamma"], cfo_bin=d["offset"])
        assert not rd.check_truth(est, c["lead"], c["d"], c["gain"], c["cfo"], c["phase"], 20.0), c
    assert found == len(chans)


# ---------------------------------------------------------------------------------------------------- device channel
def _units(rad):
    """fxtx_apply_channel's rounding of an angle (passed as float32) to a 32-bit phase: nearbyint(rad 2^32 / 2 pi) mod 2^32."""
    return int(np.rint(float(np.float32(rad)) * (4294967296.0 / 6.283185307179586))) % (1 << 32)


def test_device_channel_rotation_against_float64(fx):
    """sigma = 0: y[n] = g x[n] exp(j theta_n), theta_n = theta_0 + n dl mod 2^32 computed in integers, at CFOs up to +-0.3
    and sample indices up to 2^28.  Bound: the sin/cos table plus correction holds 3e-7; the complex product adds 2 float32
    roundings: 1e-6 |g x|."""
    import torch
    tx = fx.TxContext(0)
    n = (1 << 28) + 1024
    idx = np.unique(np.concatenate([np.arange(0, 4096), np.random.default_rng(1).integers(0, n, 20000), n - 1 - np.arange(2048)]
                                   + [(1 << k) + np.arange(-3, 3) for k in range(12, 28)]))
    ti = torch.from_numpy(idx.astype(np.int64)).cuda()
    worst = 0.0
    for cfo, ph, gain in ((0.3, 3.1, 1.0), (-0.3, -np.pi, 2.5), (-0.0123, 0.7, 1e-3), (0.29452431127404, -2.0, 32767.0)):
        gen = torch.Generator(device="cuda").manual_seed(5)
        x = torch.randn((n,), dtype=torch.complex64, device="cuda", generator=gen)
        xin = x[ti].cpu().numpy().astype(np.complex128)
        torch.cuda.synchronize()                                     # x is written on torch's stream
        tx.channel(x.data_ptr(), 1, n, [(cfo, ph, gain, 0.0, 7)])
        torch.cuda.synchronize()
        y = x[ti].cpu().numpy().astype(np.complex128)
        del x
        th = (_units(ph) + _units(cfo) * (idx.astype(object))) % (1 << 32)
        ang = np.array([int(t) for t in th], np.float64) * (TWO_PI / 4294967296.0)
        want = float(np.float32(gain)) * xin * np.exp(1j * ang)
        err = np.abs(y - want) / np.maximum(np.abs(float(np.float32(gain)) * xin), 1e-30)
        worst = max(worst, float(err.max()))
        assert err.max() <= 1e-6, (cfo, ph, gain, float(err.max()), int(idx[np.argmax(err)]))
    tx.close()
    torch.cuda.empty_cache()
    print("device channel rotation: worst relative error %.3g" % worst)


def test_device_channel_noise_statistics(fx):
    """x = 0: y = sigma w, w white Gaussian from (seed, n).  Mean, variance sigma^2, excess kurtosis 0, and no correlation
    between neighbouring streams, re / im, neighbouring samples, or seeds -- each within 6 standard errors.  Same seed and
    index give the same value (counter-based)."""
    import torch
    tx = fx.TxContext(0)
    ns, n, sigma = 4, 1 << 20, 0.7
    x = torch.zeros((ns, n), dtype=torch.complex64, device="cuda")
    torch.cuda.synchronize()                                         # the zeros are written on torch's stream
    tx.channel(x.data_ptr(), ns, n, [(0.1 * s, 0.3, 1.0, sigma, 1000 + s) for s in range(ns)])
    y = x.cpu().numpy().astype(np.complex128)
    z = torch.zeros((1, n), dtype=torch.complex64, device="cuda")
    torch.cuda.synchronize()
    tx.channel(z.data_ptr(), 1, n, [(0.0, 0.0, 5.0, sigma, 1000)])
    again = z.cpu().numpy()[0]
    tx.close()
    assert np.array_equal(again, x[0].cpu().numpy())                 # a function of (seed, n) alone: CFO / gain do not enter
    m = 2 * ns * n
    r = np.concatenate([y.real.ravel(), y.imag.ravel()])
    se = 6.0
    assert abs(r.mean()) <= se * sigma / np.sqrt(m)
    assert abs(r.var() / sigma ** 2 - 1.0) <= se * np.sqrt(2.0 / m)
    kurt = np.mean((r / r.std()) ** 4) - 3.0
    assert abs(kurt) <= se * np.sqrt(24.0 / m), kurt
    lim = se / np.sqrt(n)

    def corr(a, b):
        a = a - a.mean(); b = b - b.mean()
        return float(np.sum(a * b) / np.sqrt(np.sum(a * a) * np.sum(b * b)))
    for s in range(ns):
        assert abs(corr(y[s].real, y[s].imag)) <= lim
        for lag in (1, 2, 3):
            assert abs(corr(y[s].real[:-lag], y[s].real[lag:])) <= lim
            assert abs(corr(y[s].imag[:-lag], y[s].imag[lag:])) <= lim
            assert abs(corr(y[s].real[:-lag], y[s].imag[lag:])) <= lim
        if s + 1 < ns:
            assert abs(corr(y[s].real, y[s + 1].real)) <= lim and abs(corr(y[s].imag, y[s + 1].imag)) <= lim
    # the pair structure (two samples per counter value): even vs odd samples uncorrelated
    assert abs(corr(y[0].real[0::2], y[0].real[1::2])) <= se / np.sqrt(n / 2)
