"""The captures of tests/threshold_cases.py are what they claim, on the float64 reference (tests/ref_stream.py) and the oracle
alone, at every threshold of T.  CPU only.
  a. reference and oracle agree on every capture at every threshold, in both modes and with each capture's option, under the rules
     of tests/test_ref_stream.py; at most 2 % of a capture's decisions are uncertain in the reference (ref_stream's margins);
  b. the ladder has frames clearly over and clearly under every threshold;
  c. coverage floors: what the low and the high thresholds do to the frames that 0.5 decodes."""
import numpy as np
import pytest

import ref_detect as rd
import ref_stream as S
import ref_sync as rs
import threshold_cases as TC

UNCERTAIN_CAP = 0.02
_W = {}


def world(name, t):
    """(capture, reference frames, their uncertain events, hop trace, reference detections, their uncertain events), once"""
    if (name, t) not in _W:
        c = next(c for c in TC.CAPTURES if c["name"] == name)
        if name not in _W:
            _W[name] = TC.build(c)
        x, trace = _W[name], []
        fr, unc = S.receive(x, t, trace=trace)
        det, dunc = S.detect(x, t)
        _W[(name, t)] = (x, fr, unc, trace, det, dunc)
    return _W[(name, t)]


def decisions(frames):
    """what a threshold decides, as a comparable list"""
    return [(f["start"], bool(f["header_valid"]), f.get("payload_valid", 0)) for f in frames]


def found(case_frame, frames):
    """the placed frame is delivered at its own start with a valid header and a valid payload"""
    return any(g["start"] == case_frame["at"] and g["header_valid"] and g.get("payload_valid") for g in frames)


# ---------------------------------------------------------------------------------------------------- a. reference vs oracle
@pytest.mark.parametrize("t", TC.T)
def test_oracle_against_the_reference(oracle, t):
    worst, n_dec = {}, 0
    for c in TC.CAPTURES:
        x, fr, unc, trace, det, dunc = world(c["name"], t)
        assert len(x) <= TC.MAX_SAMPLES
        # the cap on what a comparison may leave out; with these seeds nothing is (a decision inside a margin would show here)
        assert len(unc) <= UNCERTAIN_CAP * len(fr) and len(dunc) <= UNCERTAIN_CAP * len(det), (c["name"], t, unc, dunc)
        assert not unc and not dunc, (c["name"], t, unc, dunc)
        s = oracle.Sync(threshold=t)
        of = [S.view_oracle(f) for f in s.execute(x)]
        s.close()
        bad = S.compare(fr, of, x, worst=worst)
        assert not bad, (c["name"], t, bad)
        d = oracle.Detector(t)
        od = d.run(x)
        d.close()
        bad = S.compare_detections(det, od, worst)
        assert not bad, (c["name"], t, bad)
        n_dec += len(fr) + len(det)
        opt = TC.RUNS.get(c["name"])
        if opt:
            fro, unco = S.receive(x, t, **opt)
            assert len(unco) <= UNCERTAIN_CAP * len(fro) and not unco, (c["name"], t, opt, unco)
            if opt.get("equalizer"):                     # (the oracle has no soft header decoder: that run is held on the GPU)
                s = oracle.Sync(threshold=t, equalizer=True)
                of = [S.view_oracle(f) for f in s.execute(x)]
                s.close()
                bad = S.compare(fro, of, x, equalizer=True, worst=worst)
                assert not bad, (c["name"], t, opt, bad)
    print("\nthreshold %.2f: %d decisions; worst %s" % (t, n_dec, {k: "%.3g" % v for k, v in worst.items()}))
    assert all(4.0 * worst[k] <= rd.PARITY[k] for k in rd.PARITY) and 4.0 * worst["rxy_rel"] <= S.RXY_MARGIN
    assert 4.0 * worst.get("sym", 0.0) <= rs.SYM_TOL and 4.0 * worst.get("sym_ratio", 0.0) <= 1.0


# ---------------------------------------------------------------------------------------------------- b. the ladder
CLEAR = 0.02            # "clearly" over or under a threshold: 200 x ref_stream.RXY_MARGIN, and narrow enough for a frame between 0.45 and 0.5


def own_rxy(x, f):
    """a placed frame's own rxy: ref_detect.seek on the window that holds its preamble at lag 100, read at that lag (+-1 for the
    frame's dt) instead of at the window's peak -- under 0.25 the peak of such a window is the noise's"""
    h = rd.seek(x[f["at"] - 100:f["at"] - 100 + rd.N].astype(np.complex128), S.conventions()[1])
    return float(h["rxy"] * np.sqrt(h["r2"][:, 99:102].max() / h["r2"].max()))


def test_ladder_has_frames_over_and_under_every_threshold():
    x = TC.build(TC.LADDER)
    r = np.array([own_rxy(x, f) for f in TC.LADDER["frames"]])
    print("\nrxy of the ladder's frames:", np.round(r, 3))
    assert np.all(np.abs(r - np.array(TC.LADDER_RXY)) < 0.01), r
    for t in TC.T:
        assert np.sum(r > (1.0 + CLEAR) * t) >= 1 and np.sum(r < (1.0 - CLEAR) * t) >= 1, (t, r)
        assert not np.any((r >= (1.0 - CLEAR) * t) & (r <= (1.0 + CLEAR) * t)), (t, r)
    for a, b in zip(TC.T[:-1], TC.T[1:]):               # a frame between any two neighbours
        assert np.any((r > a) & (r < b)), (a, b, r)
    for t in TC.T:                                      # and the reference finds the frames over the threshold at their starts
        starts = {g["start"] for g in world(TC.LADDER["name"], t)[1]}
        for f, v in zip(TC.LADDER["frames"], r):
            if t >= 0.45:                               # (under 0.45 a false detection may take the frame's span first)
                assert (f["at"] in starts) == (v > t), (t, f["at"], v)


# ---------------------------------------------------------------------------------------------------- c. coverage floors
def test_low_threshold_floors():
    """at 0.2: false detections with rejected headers; one of them inside the span a frame decoded at 0.5 would own; a frame
    decoded at 0.5 thereby not delivered from its own start"""
    false_det = inside = lost = 0
    for c in TC.CAPTURES:
        lo, mid = world(c["name"], 0.2)[1], world(c["name"], 0.5)[1]
        placed = [f for f in c["frames"] if found(f, mid)]
        false = [g for g in lo if not g["header_valid"] and not any(abs(g["start"] - f["at"]) <= 2 for f in c["frames"])]
        false_det += len(false)
        inside += sum(1 for g in false if any(f["at"] - TC.SC.HDR_SPAN < g["start"] < f["at"] + TC.span(f) for f in placed))
        lost += sum(1 for f in placed if not found(f, lo))
        assert len(lo) >= 0.5 * len(false), c["name"]
    print("\nat 0.2: %d false detections with rejected headers, %d of them over the span of a frame decoded at 0.5, %d such frames not delivered" % (false_det, inside, lost))
    assert false_det >= 20 and inside >= 1 and lost >= 1
    # the dense capture is where a false detection in a gap hides the next preamble
    lo, mid = world(TC.DENSE["name"], 0.2)[1], world(TC.DENSE["name"], 0.5)[1]
    assert sum(1 for f in TC.DENSE["frames"] if found(f, mid) and not found(f, lo)) >= 1


def test_high_threshold_floor():
    """at 0.9 at least one frame decoded at 0.5 is absent"""
    gone = 0
    for c in TC.CAPTURES:
        hi, mid = world(c["name"], 0.9)[1], world(c["name"], 0.5)[1]
        gone += sum(1 for f in c["frames"] if found(f, mid) and not any(abs(g["start"] - f["at"]) <= 2 for g in hi))
    assert gone >= 1


def test_every_threshold_changes_the_decisions():
    """relative to its neighbour in T, on the captures together, in the frame mode and in the detector mode; on the ladder alone too"""
    for a, b in zip(TC.T[:-1], TC.T[1:]):
        fa = [decisions(world(c["name"], a)[1]) for c in TC.CAPTURES]
        fb = [decisions(world(c["name"], b)[1]) for c in TC.CAPTURES]
        da = [[d["pos"] for d in world(c["name"], a)[4]] for c in TC.CAPTURES]
        db = [[d["pos"] for d in world(c["name"], b)[4]] for c in TC.CAPTURES]
        assert fa != fb and da != db, (a, b)
        assert decisions(world(TC.LADDER["name"], a)[1]) != decisions(world(TC.LADDER["name"], b)[1]), (a, b)
