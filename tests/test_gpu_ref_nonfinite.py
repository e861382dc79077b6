"""Non-finite and overflowing IQ samples through the library, against tests/ref_stream.py's bad= path and the oracle, on the
streams of tests/nonfinite_cases.py (the contract of DESIGN.md section 4, "Bad samples").  `-m gpu`.  Every test runs its cases
as the streams of one batch.
  - every case at segment_len 0, 4096 and 6000: untouched decisions against the reference under the existing bounds, touched
    ones by its rules, and everything -- touched header bytes, payload bytes and validity included -- equal to the oracle's;
  - isolation: in batches of 1, 3 and 65 streams the results of every other stream are bit-identical whether one stream holds
    its bad samples or zeros in their place;
  - the equaliser cases; the soft options against the reference and, where the oracle has the decoder (soft_decision), the oracle;
    the detector-only mode and qdetector_cccf_execute against the reference and the oracle's detector;
  - recovery: the cut cases as three continuing blocks at depth 3 against the one-shot run (the carry) and the zero-replaced run
    (the last block's frames and counters), and through flexframesync_execute in 256-sample calls with no flush;
  - the upload path: the detector's aligned windows from device-resident and pageable input, bit for bit the input samples;
  - integer IQ: an sc16 scale at which 32767 * scale is +Inf."""
import ctypes as C
import time

import numpy as np
import pytest

import nonfinite_cases as NC
import ref_detect as rd
import ref_stream as S
import ref_sync as rs
from parity_util import TOL_EST, compare_frames, oracle_frames

pytestmark = pytest.mark.gpu

ORACLE_ONLY = (NC.LARGE, NC.SCALE)
PLAIN = [c for c in NC.CASES if not c["eq"]]
EQ = [c for c in NC.CASES if c["eq"]]


@pytest.fixture(scope="module")
def world(oracle):
    """per case: the stream, its zero-replaced twin, the reference's frames (None where the case is oracle <-> kernels only)
    and the oracle's; computed once and left unchanged"""
    w = {}
    for c in NC.CASES:
        x = NC.build(c)
        ref = None
        if c["declared"] not in ORACLE_ONLY:
            ref, unc = S.receive(x, equalizer=c["eq"], bad=S.classify(x))
            assert not unc, (c["name"], unc)
        w[c["name"]] = (x, NC.zeroed(x), ref, oracle_frames(oracle, x, threshold=0.5, equalizer=c["eq"]))
    return w


def _nan_pattern_equal(of, mine):
    """touched symbols: NaN where the oracle's are NaN, nowhere else"""
    for a, b in zip(of, mine):
        if a.header_valid and b["framesyms"] is not None and len(a.framesyms):
            assert np.array_equal(np.isnan(a.framesyms.view(np.float32)), np.isnan(b["framesyms"].view(np.float32))), a.info["start"]


def _check(cases, world, got, worst, counts, eq=False):
    for s, c in enumerate(cases):
        x, x0, ref, of = world[c["name"]]
        mine = [g for g in got if g["stream"] == s]
        if ref is not None:
            bad = S.compare_masked(ref, [S.view_library(g) for g in mine], x0, equalizer=eq, worst=worst, counts=counts)
            assert not bad, (c["name"], bad)
        compare_frames(of, mine)
        _nan_pattern_equal(of, mine)


@pytest.mark.parametrize("seg", [0, 4096, 6000])
def test_every_case_against_reference_and_oracle(fx, world, seg):
    xs = [world[c["name"]][0] for c in PLAIN]
    ctx = fx.RxContext(len(xs), want_framesyms=True, segment_len=seg, threshold=0.5)
    got = ctx.process(xs)
    ctx.close()
    worst, counts = {}, {}
    _check(PLAIN, world, got, worst, counts)
    print("\nsegment_len %d: %d cases, %r; worst vs the reference %s" % (seg, len(xs), counts, {k: "%.3g" % v for k, v in worst.items()}))
    assert all(4.0 * worst[k] <= rd.PARITY[k] for k in rd.PARITY) and 4.0 * worst["rxy_rel"] <= S.RXY_MARGIN
    assert 4.0 * worst["sym"] <= rs.SYM_TOL and 4.0 * worst["sym_ratio"] <= 1.0
    m = S.MEASURED["nonfinite_gpu"]                # the recorded figures are this run's, rounded up: they cannot drift
    assert all(0.5 * m[k] <= worst[k] <= m[k] for k in m), ("ref_stream.MEASURED['nonfinite_gpu'] is not this run's", {k: worst[k] for k in m})


def _bits(frames, skip):
    return [(g["stream"], g["start"], g["cfo_bin"], g["header_valid"], bytes(g["header"]), g["payload_valid"], bytes(g["payload"]),
             np.float32(g["rxy"]).tobytes(), np.float32(g["tau"]).tobytes(), np.float32(g["evm_sum"]).tobytes(),
             g["framesyms"].tobytes() if g["framesyms"] is not None else b"") for g in frames if g["stream"] != skip]


@pytest.mark.parametrize("n,k", [(1, 0), (3, 1), (65, 0), (65, 64)])
def test_isolation(fx, world, n, k):
    """stream k holds its bad samples in one run and zeros in the other; every other stream is the same in both"""
    cases = [PLAIN[(7 * i + 2) % len(PLAIN)] for i in range(n)]
    cases[k] = NC.BY_NAME["nan at payload middle" if n < 65 else "run of 300 nan from payload last"]
    clean = [world[c["name"]][1] for c in cases]
    poisoned = list(clean)
    poisoned[k] = world[cases[k]["name"]][0]
    out = []
    for xs in (poisoned, clean):
        ctx = fx.RxContext(n, want_framesyms=True, segment_len=4096, threshold=0.5)
        out.append(ctx.process(xs))
        ctx.close()
    assert _bits(out[0], k) == _bits(out[1], k)
    assert len(_bits(out[0], -1)) >= 2 * n and (n == 1 or _bits(out[0], k))


def test_equaliser_cases(fx, world):
    """a touched frame's taps are not the next frame's: the frames behind it equal the reference's and the oracle's"""
    xs = [world[c["name"]][0] for c in EQ]
    ctx = fx.RxContext(len(xs), want_framesyms=True, segment_len=4096, threshold=0.5, equalizer=True)
    got = ctx.process(xs)
    ctx.close()
    _check(EQ, world, got, {}, {}, eq=True)


@pytest.mark.parametrize("opt", ["soft_header", "soft_decision", "soft_block_chain"])
def test_soft_options(fx, oracle, world, opt):
    """Integer soft values from NaN symbols.  soft_decision: everything, touched frames' header bytes, payload bytes and validity
    included, equals the oracle's soft receiver (fxr_sync_set_soft).  soft_header and soft_block + soft_chain have no oracle
    decoder: they are held to the reference (ref_stream with ref_header_soft resp. the touched rules), and every frame the reference
    leaves untouched must arrive with its payload."""
    kw = dict(soft_header=dict(soft_header=True), soft_decision=dict(soft_decision=True),
              soft_block_chain=dict(soft_decision=True, soft_block=True, soft_chain=True))[opt]
    cases = [c for c in PLAIN if c["declared"] not in ORACLE_ONLY] if opt != "soft_decision" else PLAIN
    xs = [world[c["name"]][0] for c in cases]
    ctx = fx.RxContext(len(xs), want_framesyms=True, segment_len=4096, threshold=0.5, **kw)
    got = ctx.process(xs)
    ctx.close()
    for s, c in enumerate(cases):
        x, x0, ref, _ = world[c["name"]]
        mine = [g for g in got if g["stream"] == s]
        if opt == "soft_decision":
            of = oracle_frames(oracle, x, threshold=0.5, soft=True)
            compare_frames(of, mine)
            _nan_pattern_equal(of, mine)
        if ref is None:
            continue
        if opt == "soft_header":
            ref, unc = S.receive(x, soft_header=True, bad=S.classify(x))
            assert not unc, (c["name"], unc)
        bad = S.compare_masked(ref, [S.view_library(g) for g in mine], x0)
        if opt != "soft_header":                   # soft payload decoding may rescue or lose a payload the hard decoder does not
            bad = [b for b in bad if "payload bytes / validity" not in b]
        assert not bad, (c["name"], bad)
        byat = {g["start"]: g for g in mine}
        for f in ref:
            if not f.get("touched") and f["header_valid"]:
                assert byat[f["start"]]["payload_valid"] and bytes(byat[f["start"]]["payload"]) == f["payload"], (c["name"], f["start"])


def _same_float(a, b):
    """NaN where the other has NaN, else within parity_util's bound on estimates (oracle <-> kernels)"""
    a, b = np.float32(a), np.float32(b)
    return bool((np.isnan(a) and np.isnan(b)) or abs(a - b) <= TOL_EST)


def test_detector_mode(fx, world, oracle):
    cases = [c for c in PLAIN if c["declared"] not in ORACLE_ONLY]
    xs = [world[c["name"]][0] for c in cases]
    for seg in (0, 4096):
        ctx = fx.RxContext(len(xs), mode=fx.MODE_DETECTOR, threshold=0.5, segment_len=seg)
        got = ctx.process(xs)
        ctx.close()
        for s, (c, x) in enumerate(zip(cases, xs)):
            d, unc = S.detect(x, bad=S.classify(x))
            mine = [dict(g, pos=g["start"]) for g in got if g["stream"] == s]
            assert not unc and [e["pos"] for e in d] == [g["pos"] for g in mine], (c["name"], seg)
            keep = [i for i, e in enumerate(d) if not e.get("touched")]
            bad = S.compare_detections([d[i] for i in keep], [mine[i] for i in keep])
            assert not bad, (c["name"], seg, bad)
            od = oracle.Detector(0.5).run(x)                           # the oracle's detector: every estimate, NaN where it has NaN
            assert [e["pos"] for e in od] == [g["pos"] for g in mine], (c["name"], seg)
            for e, g in zip(od, mine):
                assert e["offset"] == g["cfo_bin"] and all(_same_float(e[k], g[k]) for k in ("tau", "gamma", "dphi", "phi", "rxy")), (c["name"], seg, e, g)
            for e, g in zip(d, mine):
                if e.get("touched"):
                    assert not S.touched_estimates_off(e, g), (c["name"], seg, S.touched_estimates_off(e, g))


def _three_blocks(fx, xs):
    ctx = fx.RxContext(len(xs), want_framesyms=True, segment_len=4096, threshold=0.5)
    ctx.set_depth(3)
    cuts = (0,) + NC.BLOCK_CUTS
    keep = []
    for k in range(3):
        parts = [np.ascontiguousarray(x[cuts[k]:(cuts[k + 1] if k < 2 else len(x))]) for x in xs]
        keep.append(parts)
        ctx.submit_raw([p.ctypes.data for p in parts], [len(p) for p in parts], False)
    blocks, tm = [], []
    for k in range(3):
        blocks.append(ctx.results(ctx.collect_raw()))
        tm.append(ctx.timing())
    ctx.close()
    return blocks, tm


def test_recovery_in_three_continuing_blocks(fx, world):
    """The bad sample sits on a block cut (the last sample of a block or the first of the next) or inside a block.  All three
    blocks together deliver exactly what the one-shot run of the same stream delivers (the carry buffers hold the bad sample as it
    is); and where the bad sample is out of every carry by block 3, the frames that begin there and the block's counters equal
    those of the run whose bad samples were zeros."""
    cases = NC.CUT_CASES
    assert {c["pos"] for c in cases} >= {c - 1 for c in NC.BLOCK_CUTS} | set(NC.BLOCK_CUTS)
    xs = [world[c["name"]][0] for c in cases]
    blocks, _ = _three_blocks(fx, xs)
    ctx = fx.RxContext(len(xs), want_framesyms=True, segment_len=4096, threshold=0.5)
    one_shot = ctx.process(xs)
    ctx.close()
    key = lambda g: (g["stream"], g["start"])
    assert _bits(sorted((g for b in blocks for g in b), key=key), -1) == _bits(sorted(one_shot, key=key), -1)
    early = [c for c in cases if c["pos"] < NC.BLOCK_CUTS[1] - 1024]
    assert len(early) >= 4
    bad_run, tm_bad = _three_blocks(fx, [world[c["name"]][0] for c in early])
    zero_run, tm_zero = _three_blocks(fx, [world[c["name"]][1] for c in early])
    last = lambda bl: [g for b in bl for g in b if g["start"] >= NC.BLOCK_CUTS[1]]
    assert _bits(last(bad_run), -1) == _bits(last(zero_run), -1) and len(last(bad_run)) >= len(early)
    for k in ("vb_clean", "late_decodes", "replays"):
        assert tm_bad[2][k] == tm_zero[2][k], (k, tm_bad[2][k], tm_zero[2][k])


def _dropin(fx, x, n_want):
    """flexframesync_execute in 256-sample calls, streaming delivery, no flush: [(header, hv, pv, payload, symbols)]"""
    L = fx.lib()
    got = []

    def cb(hd, hv, pl, n, pv, st, ud):
        syms = C.string_at(st.framesyms, 8 * st.num_framesyms) if st.num_framesyms else b""
        got.append((C.string_at(hd, 20), int(hv), int(pv), C.string_at(pl, n) if (pl and n) else b"", syms))
        return 0
    cbf = fx._ffi.FRAMESYNC_CALLBACK(cb)
    q = L.flexframesync_create(cbf, None)
    assert q
    L.fxrx_sync_set_streaming(q, 8192)
    for i in range(0, len(x), 256):
        L.flexframesync_execute(q, x[i:i + 256].ctypes.data, 256)
    zeros, extra, t0 = np.zeros(256, np.complex64), 0, time.monotonic()
    while len(got) < n_want and extra < 4_000_000 and time.monotonic() - t0 < 10.0:      # (a guard against hanging, not a latency claim)
        L.flexframesync_execute(q, zeros.ctypes.data, 256)
        extra += 256
    err = L.fxrx_sync_errors(q)
    L.flexframesync_destroy(q)
    assert err == 0
    return got


def test_recovery_through_the_drop_in(fx, world):
    """the block API itself: every call returns, the frames are the oracle's (touched ones included), and the frames behind the
    bad sample's frame are those of the zero-replaced stream, symbols included"""
    for c in NC.CUT_CASES[:4] + [NC.BY_NAME["nan at aligned only"], NC.BY_NAME["-3e38 at payload middle"]]:
        x, x0, ref, of = world[c["name"]]
        assert len(x) % 256 == 0
        got, clean = _dropin(fx, x, len(of)), _dropin(fx, x0, len(of))
        want = [(f.header20, f.header_valid, f.payload_valid if f.header_valid else 0, f.payload if f.header_valid else b"") for f in of]
        assert [g[:4] for g in got] == want, (c["name"], [g[1:3] for g in got], [w[1:3] for w in want])
        assert len(clean) == len(got) and got[-1] == clean[-1] and not ref[-1].get("touched"), c["name"]


def _windows(fx, xs, device):
    import torch
    ctx = fx.RxContext(len(xs), mode=fx.MODE_DETECTOR, threshold=0.5, want_framesyms=True, segment_len=4096)
    got = ctx.process([torch.from_numpy(x).cuda() for x in xs] if device else xs)
    ctx.close()
    return got


@pytest.mark.parametrize("device", [False, True])
def test_upload_passes_every_bit_through(fx, world, device):
    """detector mode with want_framesyms hands out the aligned windows: each must be the input samples bit for bit -- NaN payload
    and sign bits, Inf, 3e38 and the subnormal-energy streams included -- from pageable and from device-resident input"""
    xs = [world[c["name"]][0].copy() for c in NC.CASES]
    for k, x in enumerate(xs):                                              # NaNs with payload bits and a sign, not the default quiet NaN alone
        v = x.view(np.uint32)
        v[np.isnan(x.view(np.float32))] = (0x7FC12345, 0xFFA54321, 0x7F800001)[k % 3]
    got = _windows(fx, xs, device)
    seen_bad = 0
    for s, x in enumerate(xs):
        mine = [g for g in got if g["stream"] == s]
        assert mine or NC.CASES[s]["declared"] == NC.SCALE, NC.CASES[s]["name"]
        for g in mine:
            w = np.zeros(512, np.complex64)
            lo = max(g["start"], 0)
            w[lo - g["start"]:] = x[lo:g["start"] + 512]
            assert np.array_equal(g["framesyms"].view(np.uint32), w.view(np.uint32)), (NC.CASES[s]["name"], g["start"])
            seen_bad += int(not np.isfinite(w.view(np.float32)).all())
    assert seen_bad >= 5                                                    # windows that hold the bad sample itself were compared


def test_qdetector_per_sample(fx, oracle, world):
    """qdetector_cccf_execute, one sample per call: the windows it hands out are the input bit for bit at the oracle's positions,
    the estimates the oracle's (NaN where it has NaN)"""
    L = fx.lib()
    pn = S.conventions()[0].pn.astype(np.complex64)
    for name in ("nan at aligned only", "run of 2 +inf at window first", "nan re at payload first", "-3e38 at payload middle", "run of 300 2e19 before preamble"):
        x = world[name][0]
        od = oracle.Detector(0.5).run(x)
        q = L.qdetector_cccf_create_linear(pn.ctypes.data, 64, 7, 2, 7, C.c_float(0.3))
        assert q
        L.qdetector_cccf_set_threshold(q, 0.5)
        got = []

        def take(p):
            win = np.frombuffer(C.cast(p, C.POINTER(C.c_float * 1024)).contents, np.complex64).copy()
            got.append(dict(tau=L.qdetector_cccf_get_tau(q), gamma=L.qdetector_cccf_get_gamma(q), dphi=L.qdetector_cccf_get_dphi(q),
                            phi=L.qdetector_cccf_get_phi(q), win=win))
        v = x.view(np.float32).reshape(-1, 2)
        for i in range(len(x)):
            p = L.qdetector_cccf_execute(q, fx._ffi.FxComplex(float(v[i, 0]), float(v[i, 1])))
            if p:
                take(p)
        L.fxrx_qdet_flush(q)
        while L.fxrx_qdet_pending(q):
            p = L.qdetector_cccf_execute(q, fx._ffi.FxComplex(0.0, 0.0))
            if p:
                take(p)
        assert L.fxrx_qdet_errors(q) == 0
        L.qdetector_cccf_destroy(q)
        assert len(got) == len(od), (name, len(got), [d["pos"] for d in od])
        for d, g in zip(od, got):
            w = np.zeros(512, np.complex64)
            lo = max(d["pos"], 0)
            w[lo - d["pos"]:] = x[lo:d["pos"] + 512]
            assert np.array_equal(np.isnan(g["win"].view(np.float32)), np.isnan(w.view(np.float32))), (name, d["pos"])
            ok = ~np.isnan(w.view(np.float32))
            assert np.array_equal(g["win"].view(np.uint32)[ok], w.view(np.uint32)[ok]), (name, d["pos"])
            assert all(_same_float(d[k], g[k]) for k in ("tau", "gamma", "dphi", "phi")), (name, d, g)


def test_sc16_scale_that_overflows(fx):
    """fxrx_set_iq_scale admits any finite positive scale, so 32767 * scale may be +Inf: the conversion then yields Inf (and
    values whose squares overflow), the call returns, and the results are those of the float array the conversion produces"""
    L = fx.lib()
    x = NC.clean("base")[0]
    q = np.clip(np.rint(x.view(np.float32).reshape(-1, 2) * 4096.0), -32767, 32767).astype(np.int16)
    q[5000] = (32767, -32767)
    scale = float(np.float32(2.0) ** 114)
    ctx = fx.RxContext(1, want_framesyms=True, segment_len=4096, threshold=0.5)
    ref_ctx = fx.RxContext(1, want_framesyms=True, segment_len=4096, threshold=0.5)
    assert L.fxrx_set_iq_scale(ctx.h, fx._ffi.IQ_SC16, C.c_float(float("inf"))) == -1      # a non-finite scale itself is rejected
    ctx.set_iq_scale(fx._ffi.IQ_SC16, scale)
    xf = fx.iq_convert(q, scale=scale)
    assert np.isposinf(xf[5000].real) and np.isneginf(xf[5000].imag) and np.isfinite(xf[:5000].view(np.float32)).all()
    got, ref = ctx.process([np.ascontiguousarray(q)]), ref_ctx.process([xf])
    assert _bits(got, -1) == _bits(ref, -1)
    ctx.set_iq_scale(fx._ffi.IQ_SC16, 1.0 / 4096.0)                                        # and back: the same context decodes the stream
    ctx.reset()
    q[5000] = 0
    assert sum(g["payload_valid"] for g in ctx.process([np.ascontiguousarray(q)])) == 3
    ctx.close(); ref_ctx.close()
