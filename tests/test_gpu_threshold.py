"""The detection threshold (fxrx_config.threshold, fxrx_sync_set_threshold, qdetector_cccf_set_threshold) at every value of
threshold_cases.T on the captures of tests/threshold_cases.py, whose claims tests/test_ref_threshold.py holds on the CPU.  `-m gpu`.

Three kernels compare against the threshold: the walker's sweep, the seek verification of skipped hops and the pre-lock scan.  At
0.2 the detector fires on noise in most hops -- false detections, rejected headers, speculative segments that disagree with the
stream, fired skipped hops, repair rounds --, at 0.9 frames that a segment speculated on vanish.  Every run is compared with the
oracle at the same threshold through parity_util.compare_frames (all 20 header bytes, rejected headers included; nothing is left
out) and with tests/ref_stream.py under that module's bounds; runs of the library against each other are compared bit for bit.
The contract for values that are no threshold (include/fxrx.h, fxrx_config.threshold) is pinned at the end."""
import ctypes as C
import math
import struct

import numpy as np
import pytest

import ref_detect as rd
import ref_stream as S
import ref_sync as rs
import threshold_cases as TC
from parity_util import compare_frames, oracle_frames
from test_gpu_cuts import differences, feed

pytestmark = pytest.mark.gpu

SEGS = (0, 4096, 6000)
_XS, _REF, _SYNC = {}, {}, {}


def capture(c):
    if c["name"] not in _XS:
        _XS[c["name"]] = TC.build(c)
    return _XS[c["name"]]


def refs(oracle, c, t, **opt):
    """(reference frames, oracle frames or None) of a capture at t, once; without options also (reference detections, oracle's)"""
    k = (c["name"], t, tuple(sorted(opt)))
    if k not in _REF:
        x = capture(c)
        fr, unc = S.receive(x, t, **opt)
        if math.isinf(t):                       # (ref_stream's relative margin around an infinite threshold holds every hop: Inf <= Inf)
            unc = []
        assert not unc, (c["name"], t, opt, unc)
        of = None if opt.get("soft_header") else oracle_frames(oracle, x, threshold=t, equalizer=bool(opt.get("equalizer")))
        det = od = None
        if not opt:
            det, unc = S.detect(x, t)
            assert not unc or math.isinf(t), (c["name"], t, unc)
            d = oracle.Detector(t)
            od = d.run(x)
            d.close()
        _REF[k] = (fr, of, det, od)
    return _REF[k]


def dkey(g):
    return (g["start"], g["cfo_bin"], struct.pack("<5f", g["rxy"], g["tau"], g["gamma"], g["dphi"], g["phi"]), None if g["framesyms"] is None else g["framesyms"].tobytes())


def window(x, p):
    """the 512 aligned samples of a detection at p: (0, 0) below the stream's first sample"""
    out = np.zeros(rd.N, np.complex64)
    lo = max(p, 0)
    out[lo - p:] = x[lo:p + rd.N]
    return out


def per_stream(got, n):
    return [[g for g in got if g["stream"] == s] for s in range(n)]


def run(fx, t, mode=None, **cfg):
    xs = [capture(c) for c in TC.CAPTURES]
    ctx = fx.RxContext(len(xs), mode=fx.MODE_FLEX_RX if mode is None else mode, want_framesyms=True, threshold=t, **cfg)
    got = ctx.process(xs)
    tm, pre = ctx.timing(), ctx.prescan_stats()
    ctx.close()
    return per_stream(got, len(xs)), tm, pre


def against_references(oracle, c, t, mine, worst, **opt):
    x = capture(c)
    fr, of, _, _ = refs(oracle, c, t, **opt)
    if of is not None:
        compare_frames(of, mine)
    bad = S.compare(fr, [S.view_library(g) for g in mine], x, equalizer=bool(opt.get("equalizer")), worst=worst, cache=_SYNC)
    assert not bad, (c["name"], t, opt, bad[:4])


def bounds_hold(worst):
    assert all(4.0 * worst.get(k, 0.0) <= rd.PARITY[k] for k in rd.PARITY) and 4.0 * worst.get("rxy_rel", 0.0) <= S.RXY_MARGIN, worst
    assert 4.0 * worst.get("sym", 0.0) <= rs.SYM_TOL and 4.0 * worst.get("sym_ratio", 0.0) <= 1.0, worst


# ---------------------------------------------------------------------------------------------------- both modes, every segment length
@pytest.mark.parametrize("t", TC.T)
def test_flex_rx_against_oracle_and_reference(fx, oracle, t):
    worst, n = {}, 0
    for seg in SEGS:
        got, tm, _ = run(fx, t, segment_len=seg)
        for c, mine in zip(TC.CAPTURES, got):
            against_references(oracle, c, t, mine, worst)
            n += len(mine)
        print("\nthreshold %.2f, segment_len %d: %d frames, repairs %d, verify_failures %d" % (t, seg, sum(len(g) for g in got), tm["repairs"], tm["verify_failures"]))
    assert n > 0
    bounds_hold(worst)


@pytest.mark.parametrize("t", TC.T)
def test_detector_against_oracle_and_reference(fx, oracle, t):
    worst = {}
    for seg in SEGS:
        got, _, _ = run(fx, t, mode=fx.MODE_DETECTOR, segment_len=seg)
        for c, mine in zip(TC.CAPTURES, got):
            x = capture(c)
            _, _, det, od = refs(oracle, c, t)
            assert [q["pos"] for q in od] == [g["start"] for g in mine], (c["name"], t, seg)
            for q, g in zip(od, mine):
                assert rd.parity_ok(q, g)[0], (c["name"], t, seg, q["pos"])
                assert np.array_equal(g["framesyms"], window(x, g["start"])), (c["name"], t, seg, g["start"])
            bad = S.compare_detections(det, [dict(g, pos=g["start"]) for g in mine], worst)
            assert not bad, (c["name"], t, seg, bad[:4])
    bounds_hold(worst)


@pytest.mark.parametrize("t", TC.T)
def test_options(fx, oracle, t):
    """the ladder with the equaliser, the dense capture with the soft header decoder"""
    worst = {}
    for c in TC.CAPTURES:
        opt = TC.RUNS.get(c["name"])
        if not opt:
            continue
        ctx = fx.RxContext(1, want_framesyms=True, threshold=t, segment_len=4096, **opt)
        mine = ctx.process([capture(c)])
        ctx.close()
        against_references(oracle, c, t, mine, worst, **opt)
    bounds_hold(worst)


# ---------------------------------------------------------------------------------------------------- continuing blocks
@pytest.mark.parametrize("t", TC.T)
def test_five_unequal_blocks(fx, t):
    """the one-pass run (held to oracle and reference above) is the standard: every field identical, both modes, depth 1 and 3"""
    xs = [capture(c) for c in TC.CAPTURES]
    cuts = [TC.five_blocks(len(x)) for x in xs]
    for mode in (fx.MODE_FLEX_RX, fx.MODE_DETECTOR):
        one, _, _ = run(fx, t, mode=mode, segment_len=4096)
        for depth in (1, 3):
            ctx = fx.RxContext(len(xs), mode=mode, want_framesyms=True, threshold=t, segment_len=4096)
            got, tm = feed(ctx, xs, cuts, depth)
            ctx.close()
            for c, a, b in zip(TC.CAPTURES, one, got):
                if mode == fx.MODE_FLEX_RX:
                    assert not differences(a, b), (c["name"], t, depth, differences(a, b)[:3])
                else:
                    assert [dkey(g) for g in a] == [dkey(g) for g in b], (c["name"], t, depth)


# ---------------------------------------------------------------------------------------------------- the kernels that hold the threshold
@pytest.mark.parametrize("t", TC.T)
def test_path_variants(fx, monkeypatch, t):
    """FXRX_PRESCAN=1 against =0 and FXRX_SKIP_SEEK=0 against =1: every field identical.  At 0.2 the counters must show that the
    repair rounds, the seek verification and the pre-lock scan's table were in the run."""
    def with_env(**env):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        return run(fx, t, segment_len=4096)
    plain, tm, pre0 = with_env(FXRX_PRESCAN="0", FXRX_SKIP_SEEK="1")
    scanned, tm_p, pre = with_env(FXRX_PRESCAN="1", FXRX_SKIP_SEEK="1")
    exact, tm_e, _ = with_env(FXRX_PRESCAN="0", FXRX_SKIP_SEEK="0")
    for c, a, b, d in zip(TC.CAPTURES, plain, scanned, exact):
        assert not differences(a, b), ("FXRX_PRESCAN", c["name"], t, differences(a, b)[:3])
        assert not differences(a, d), ("FXRX_SKIP_SEEK", c["name"], t, differences(a, d)[:3])
    print("\nthreshold %.2f: repairs %d, verify %d hops / %d failures, prescan %r; FXRX_SKIP_SEEK=0: verify hops %d" %
          (t, tm["repairs"], tm["verify_hops"], tm["verify_failures"], pre, tm_e["verify_hops"]))
    assert pre0 == (0, 0, 0) and tm_e["verify_hops"] == 0 and tm_e["verify_failures"] == 0
    assert pre[0] > 0, "path not exercised: no segment was pre-scanned"
    if t == 0.2:
        assert tm["repairs"] > 0, "path not exercised: no repair round"
        assert tm["verify_failures"] > 0, "path not exercised: no skipped hop fired in the seek verification"
        assert pre[1] > 0, "path not exercised: no segment took a candidate from the scan's table"


# ---------------------------------------------------------------------------------------------------- the drop-in setters
def _batched(fx, x, t, mode):
    ctx = fx.RxContext(1, mode=mode, want_framesyms=True, threshold=t)
    got = ctx.process([x])
    ctx.close()
    return got


@pytest.mark.parametrize("t", [0.2, 0.7])
def test_drop_in_setters(fx, t):
    """fxrx_sync_set_threshold then 256-sample flexframesync_execute calls and a flush: the batched context's frames at t;
    qdetector_cccf_set_threshold then one call per sample: the batched detector's detections, estimates and windows at t.  A NaN
    handed to either setter afterwards changes nothing: same value, same context, no error counted."""
    L = fx.lib()
    x = capture(TC.SMALLEST)
    x = np.ascontiguousarray(x[:len(x) // 256 * 256])
    want = _batched(fx, x, t, fx.MODE_FLEX_RX)
    other = _batched(fx, x, 0.5, fx.MODE_FLEX_RX)
    assert [g["start"] for g in want] != [g["start"] for g in other], "0.5 decides the same: the setter would not be missed"
    got = []
    cbf = fx._ffi.FRAMESYNC_CALLBACK(lambda hd, hv, pl, n, pv, st, ud: got.append(
        (C.string_at(hd, 20), int(hv), int(pv), C.string_at(pl, n) if (pl and n) else b"", st.num_framesyms)) or 0)
    q = L.flexframesync_create(cbf, None)
    assert q
    try:
        L.fxrx_sync_set_threshold(q, t)
        ctx = L.fxrx_sync_context(q)
        L.fxrx_sync_set_threshold(q, float("nan"))
        assert L.fxrx_sync_context(q) == ctx and L.fxrx_sync_errors(q) == 0
        for i in range(0, len(x), 256):
            L.flexframesync_execute(q, x[i:i + 256].ctypes.data, 256)
        L.fxrx_sync_flush(q)
        while L.fxrx_sync_pending(q):
            L.flexframesync_execute(q, None, 0)
        assert L.fxrx_sync_errors(q) == 0
    finally:
        L.flexframesync_destroy(q)
    assert len(got) == len(want), (t, len(got), len(want))
    for g, w in zip(got, want):
        assert g[:2] == (w["header"], w["header_valid"]), (t, w["start"])
        if w["header_valid"]:
            assert g[2:] == (w["payload_valid"], w["payload"], w["num_framesyms"]), (t, w["start"])

    want = _batched(fx, x, t, fx.MODE_DETECTOR)
    other = _batched(fx, x, 0.45, fx.MODE_DETECTOR)
    assert [g["start"] for g in want] != [g["start"] for g in other]
    pn = S.conventions()[0].pn.astype(np.complex64)
    q = L.qdetector_cccf_create_linear(pn.ctypes.data, 64, 7, 2, 7, C.c_float(0.3))
    assert q
    got = []

    def take(p):
        win = np.frombuffer(C.cast(p, C.POINTER(C.c_float * 1024)).contents, np.complex64).copy()
        got.append((struct.pack("<4f", L.qdetector_cccf_get_tau(q), L.qdetector_cccf_get_gamma(q), L.qdetector_cccf_get_dphi(q), L.qdetector_cccf_get_phi(q)), win.tobytes()))
    try:
        L.qdetector_cccf_set_threshold(q, t)
        ctx = L.fxrx_qdet_context(q)
        L.qdetector_cccf_set_threshold(q, float("nan"))
        assert L.fxrx_qdet_context(q) == ctx and L.fxrx_qdet_errors(q) == 0
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
    finally:
        L.qdetector_cccf_destroy(q)
    assert len(got) == len(want), (t, len(got), len(want))
    for g, w in zip(got, want):
        assert g == (struct.pack("<4f", w["tau"], w["gamma"], w["dphi"], w["phi"]), w["framesyms"].tobytes()), (t, w["start"])


# ---------------------------------------------------------------------------------------------------- values that are no threshold
def test_nan_is_refused(fx):
    for mode in (fx.MODE_FLEX_RX, fx.MODE_DETECTOR):
        with pytest.raises(fx.rx.RxError, match="FXRX_ERR_ARG"):
            fx.RxContext(1, mode=mode, threshold=float("nan"))


@pytest.mark.parametrize("t", [0.0, -1.0, -math.inf])
def test_zero_and_below_select_the_default(fx, oracle, t):
    for mode, default in ((fx.MODE_FLEX_RX, 0.5), (fx.MODE_DETECTOR, 0.45)):
        got, _, _ = run(fx, t, mode=mode)
        for c, mine in zip(TC.CAPTURES, got):
            fr, of, det, od = refs(oracle, c, default)
            if mode == fx.MODE_FLEX_RX:
                compare_frames(of, mine)
            else:
                assert [q["pos"] for q in od] == [g["start"] for g in mine] and all(rd.parity_ok(q, g)[0] for q, g in zip(od, mine)), (c["name"], t)


@pytest.mark.parametrize("t", [1.5, 2.0, math.inf])
def test_unreachable_thresholds_find_nothing(fx, oracle, t):
    """2 and +Inf are above sqrt(512 / 156) = 1.81, the largest rxy there is (a preamble alone in a silent window): no results, no
    error, in one pass and block by block, and the next context at 0.5 finds what it always finds.  1.5 is not above every rxy: a
    frame far stronger than what its window holds beside it reaches it -- the ladder's last frame, 29 dB over the noise, and two
    frames of the dense capture behind a gap.  Reference and oracle say so; the library is held to them there as everywhere."""
    xs = [capture(c) for c in TC.CAPTURES]
    want = [refs(oracle, c, t) for c in TC.CAPTURES]
    if t == 1.5:
        assert 0 < sum(len(w[1]) for w in want) <= 4 and 0 < sum(len(w[3]) for w in want) <= 4
    else:
        assert all(w[0] == [] and w[1] == [] and w[2] == [] and w[3] == [] for w in want)
    for mode in (fx.MODE_FLEX_RX, fx.MODE_DETECTOR):
        got, tm, _ = run(fx, t, mode=mode, segment_len=4096)
        assert tm["hops"] > 0
        ctx = fx.RxContext(len(xs), mode=mode, want_framesyms=True, threshold=t)
        cut, _ = feed(ctx, xs, [TC.five_blocks(len(x)) for x in xs], 3)
        ctx.close()
        for w, a, b in zip(want, got, cut):
            if mode == fx.MODE_FLEX_RX:
                compare_frames(w[1], a)
                assert not differences(a, b)
            else:
                assert [q["pos"] for q in w[3]] == [g["start"] for g in a] == [g["start"] for g in b]
            assert t == 1.5 or (a == [] and b == [])
    got, _, _ = run(fx, 0.5)
    for c, mine in zip(TC.CAPTURES, got):
        compare_frames(refs(oracle, c, 0.5)[1], mine)
