"""The library's sequencing -- segment walkers, stitch, repair rounds, hand-offs, cross-block state, header rejection, the
detector-only mode -- against tests/ref_stream.py, a float64 stream receiver that shares no code with the kernels or the oracle,
on the streams of tests/stream_cases.py.  `-m gpu`.

Every case goes through RxContext.process at segment_len 0, 4096, 6000 and 8192 (all cases as the streams of one call) and is
compared with the reference by tests/test_ref_stream.py's rules and with the oracle through parity_util.compare_frames (all 20
header bytes, rejected headers included).  The rejected-header and hidden-frame streams also run with the soft header, with the
equaliser, cut into three continuing blocks at depth 3 and through the drop-in flexframesync_execute in 256-sample calls; the
capture-end cases one-shot and as two continuing blocks; the detector cases in MODE_DETECTOR and through qdetector_cccf_execute."""
import ctypes as C

import numpy as np
import pytest

import ref_detect as rd
import ref_stream as S
import ref_sync as rs
import stream_cases as SC
from parity_util import compare_frames, oracle_frames
from stream_cases import check_roles

pytestmark = pytest.mark.gpu

SEGS = (0, 4096, 6000, 8192)
OPTION_CASES = SC.REJECTED + [SC.HIDDEN]


def _capture(c):
    x = SC.build(c)
    return x[:c["cut"]] if "cut" in c else x


@pytest.fixture(scope="module")
def world():
    """per case: the capture and the reference's frames, computed once and left unchanged"""
    w = {}
    for c in SC.CASES:
        x = _capture(c)
        fr, unc = S.receive(x, c["threshold"])
        assert not unc, (c["name"], unc)
        w[c["name"]] = (x, fr)
    return w


_SYNC = {}              # ref_sync.sync from the library's estimates, shared by every run that reports the same frame


def _against_reference(c, x, ref, got, eq=False, worst=None):
    """eq: the roles of tests/stream_cases.py are stated for the receiver without the equaliser (a preamble cut by the detector's
    restart trains the equaliser on 27 zeros, and that frame's header then fails in reference, oracle and library alike): with it
    only the rejected headers are held against their roles"""
    bad = S.compare(ref, [S.view_library(g) for g in got], x, equalizer=eq, worst=worst, cache=_SYNC)
    assert not bad, (c["name"], bad)
    if eq:
        c = dict(c, frames=[f for f in c["frames"] if f["role"] == "rejected"])
    elif c in SC.REJECTED:          # exactly one header_valid == 0 frame, at the placed start
        assert [g["start"] for g in got if not g["header_valid"]] == [f["at"] for f in c["frames"] if f["role"] == "rejected"], c["name"]
    assert not check_roles(c, got, len(x)), (c["name"], check_roles(c, got, len(x)))


def _walked_frames(fx, ctx):
    """frames the walk jobs of the last block found, speculative ones included (fxrx_debug_walk_jobs: 6 words per job)"""
    out = (C.c_uint32 * (6 * 4096))()
    n = fx.lib().fxrx_debug_walk_jobs(ctx.h, out, 4096)
    assert n >= 0
    return sum(out[6 * i + 5] for i in range(n)), n


@pytest.mark.parametrize("seg", SEGS)
def test_every_case_against_reference_and_oracle(fx, oracle, world, seg):
    xs = [world[c["name"]][0] for c in SC.CASES]
    ctx = fx.RxContext(len(xs), want_framesyms=True, segment_len=seg, threshold=0.5)
    got = ctx.process(xs)
    ctx.close()
    worst, frames = {}, 0
    for s, c in enumerate(SC.CASES):
        x, ref = world[c["name"]]
        mine = [g for g in got if g["stream"] == s]
        _against_reference(c, x, ref, mine, worst=worst)
        compare_frames(oracle_frames(oracle, x, threshold=c["threshold"]), mine)
        frames += len(mine)
    print("\nsegment_len %d: %d cases, %d frames; worst vs the reference %s" % (seg, len(xs), frames, {k: "%.3g" % v for k, v in worst.items()}))
    assert all(4.0 * worst[k] <= rd.PARITY[k] for k in rd.PARITY) and 4.0 * worst["rxy_rel"] <= S.RXY_MARGIN
    assert 4.0 * worst["sym"] <= rs.SYM_TOL and 4.0 * worst["sym_ratio"] <= 1.0
    m = S.MEASURED["gpu"]                          # the recorded figures are this run's, rounded up: they cannot drift
    assert all(0.5 * m[k] <= worst[k] <= m[k] for k in m), ("ref_stream.MEASURED['gpu'] is not this run's", {k: worst[k] for k in m})


@pytest.mark.parametrize("seg", [4096, 6000])
def test_hidden_frames_take_the_speculative_path(fx, world, seg):
    """at segments of 4096 and 6000 samples a walker starts inside the outer payload in front of a hidden preamble and finds it: the stitch has to discard
    its frames, or a repair round walks the stretch again -- the counters must show one of the two"""
    x, ref = world[SC.HIDDEN["name"]]
    ctx = fx.RxContext(1, want_framesyms=True, segment_len=seg, threshold=0.5)
    got = ctx.process([x])
    tm = ctx.timing()
    walked, jobs = _walked_frames(fx, ctx)
    ctx.close()
    _against_reference(SC.HIDDEN, x, ref, got)
    print("\nsegment_len %d: %d walk jobs found %d frames, %d delivered, %d repairs" % (seg, jobs, walked, len(got), tm["repairs"]))
    assert jobs > 1 and (walked > len(got) or tm["repairs"] > 0)


@pytest.mark.parametrize("opt", ["soft_header", "equalizer"])
def test_rejected_and_hidden_streams_with_options(fx, oracle, opt):
    eq = opt == "equalizer"
    xs = [SC.build(c) for c in OPTION_CASES]
    ctx = fx.RxContext(len(xs), want_framesyms=True, segment_len=4096, threshold=0.5, **{opt: True})
    got = ctx.process(xs)
    ctx.close()
    for s, (c, x) in enumerate(zip(OPTION_CASES, xs)):
        ref, unc = S.receive(x, c["threshold"], equalizer=eq, soft_header=not eq)
        assert not unc, (c["name"], unc)
        mine = [g for g in got if g["stream"] == s]
        _against_reference(c, x, ref, mine, eq=eq)
        if eq:
            compare_frames(oracle_frames(oracle, x, threshold=c["threshold"], equalizer=True), mine)


def test_rejected_and_hidden_streams_in_three_continuing_blocks(fx, world):
    """depth 3; one cut inside the rejected header's claimed payload resp. inside the first hidden frame, the next 900 samples on"""
    xs = [world[c["name"]][0] for c in OPTION_CASES]
    cuts = []
    for c, x in zip(OPTION_CASES, xs):
        a = (SC.HIDDEN["frames"][1]["at"] + 300) if c is SC.HIDDEN else c["frames"][0]["at"] + SC.HDR_SPAN + 100
        cuts.append([0, a, a + 900, len(x)])
        assert a + 900 < len(x)
    ctx = fx.RxContext(len(xs), want_framesyms=True, segment_len=4096, threshold=0.5)
    ctx.set_depth(3)
    keep = []
    for k in range(3):
        parts = [np.ascontiguousarray(x[b[k]:b[k + 1]]) for x, b in zip(xs, cuts)]
        keep.append(parts)
        ctx.submit_raw([p.ctypes.data for p in parts], [len(p) for p in parts], False)
    got = []
    for k in range(3):
        got += ctx.results(ctx.collect_raw())
    ctx.close()
    for s, c in enumerate(OPTION_CASES):
        x, ref = world[c["name"]]
        _against_reference(c, x, ref, sorted((g for g in got if g["stream"] == s), key=lambda g: g["start"]))


def test_rejected_and_hidden_streams_through_the_drop_in(fx, world):
    """flexframesync_execute in 256-sample calls, one handle, reset between the streams: the callback's 20 header bytes, the
    validities and the payload are the reference's, frame by frame"""
    L = fx.lib()
    got = []
    cbf = fx._ffi.FRAMESYNC_CALLBACK(lambda hd, hv, pl, n, pv, st, ud: got.append(
        (C.string_at(hd, 20), int(hv), int(pv), C.string_at(pl, n) if (pl and n) else b"")) or 0)
    q = L.flexframesync_create(cbf, None)
    assert q
    try:
        for c in OPTION_CASES:
            x, ref = world[c["name"]]
            xx = np.ascontiguousarray(x[:len(x) // 256 * 256])
            assert all(f["last"] < len(xx) for f in ref) and len(x) - len(xx) < 256 < c["total"] - max(f["at"] + SC.length(f) for f in c["frames"])
            del got[:]
            L.flexframesync_reset(q)
            for i in range(0, len(xx), 256):
                L.flexframesync_execute(q, xx[i:i + 256].ctypes.data, 256)
            L.fxrx_sync_flush(q)
            while L.fxrx_sync_pending(q):
                L.flexframesync_execute(q, None, 0)
            assert L.fxrx_sync_errors(q) == 0
            want = [(f["header"], int(f["header_valid"]), f.get("payload_valid", 0), f.get("payload", b"")) for f in ref]
            assert len(got) == len(want), (c["name"], len(got), len(want))
            for k, (g, w, f) in enumerate(zip(got, want, ref)):
                assert g[:2] == w[:2], (c["name"], k)
                if f["header_valid"] and f["full"]:
                    assert g[2:] == w[2:], (c["name"], k)
    finally:
        L.flexframesync_destroy(q)


def test_capture_ends(fx, world):
    """one-shot the frame the capture cuts is not delivered; fed the rest as the next block of the same stream it is"""
    for c in SC.CAPTURE_ENDS:
        x, ref = world[c["name"]]
        whole = SC.build(c)
        ref_whole, unc = S.receive(whole, c["threshold"])
        assert not unc and len(ref_whole) == 1 and len(ref) == (1 if c["cut"] > ref_whole[0]["last"] else 0), c["name"]
        for seg in (0, 4096):
            ctx = fx.RxContext(1, want_framesyms=True, segment_len=seg, threshold=0.5)
            first = ctx.process([x])
            _against_reference(c, x, ref, first)
            rest = np.ascontiguousarray(whole[c["cut"]:])
            both = first + ctx.process([rest])
            ctx.close()
            _against_reference(dict(c, frames=[dict(c["frames"][0], role="good")]), whole, ref_whole, both)


@pytest.mark.parametrize("thr", [0.45, 0.5])
def test_detector_mode(fx, thr):
    cases = [c for c, t in SC.DETECTOR_CASES if t == thr]
    xs = [SC.build(c) for c in cases]
    refs = []
    for c, x in zip(cases, xs):
        d, unc = S.detect(x, thr)
        assert not unc, (c["name"], unc)
        refs.append(d)
    for seg in SEGS:
        ctx = fx.RxContext(len(xs), mode=fx.MODE_DETECTOR, threshold=thr, segment_len=seg)
        got = ctx.process(xs)
        ctx.close()
        for s, (c, ref) in enumerate(zip(cases, refs)):
            mine = [dict(g, pos=g["start"]) for g in got if g["stream"] == s]
            bad = S.compare_detections(ref, mine)
            assert not bad, (c["name"], thr, seg, bad)
    # the per-sample entry: positions through the windows it hands out
    L = fx.lib()
    tb, _ = S.conventions()
    pn = tb.pn.astype(np.complex64)
    for c, x, ref in zip(cases, xs, refs):
        q = L.qdetector_cccf_create_linear(pn.ctypes.data, 64, 7, 2, 7, C.c_float(0.3))
        assert q
        L.qdetector_cccf_set_threshold(q, thr)
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
        assert len(got) == len(ref), (c["name"], thr, len(got), [d["pos"] for d in ref])
        for d, g in zip(ref, got):
            assert np.array_equal(g["win"], x[d["pos"]:d["pos"] + 512]), (c["name"], d["pos"])
            ok, e = rd.parity_ok(d, g)
            assert ok, (c["name"], d["pos"], e)
