"""The receiver's sequencing -- hop grid, detection rule, resume points, detector history, header rejection, the detector-only
mode -- against tests/ref_stream.py, a float64 stream receiver composed of the other references.  CPU only.
  a. the case list holds what it promises, and no case is uncertain in the reference;
  b. the oracle's synchroniser and detector against the reference on every case;
  c. truth: every frame a case places is found, rejected or absent as the case declares;
  d. negative controls: mutations of the reference's own rules must fail b on a named case."""
import numpy as np
import pytest

import ref_decode as R
import ref_detect as rd
import ref_stream as S
import ref_sync as rs
import stream_cases as SC
from stream_cases import check_roles

BY_NAME = {c["name"]: c for c in SC.CASES + [SC.OVERLAP]}


def _capture(c):
    x = SC.build(c)
    return x[:c["cut"]] if "cut" in c else x


_W = {}


def _world(oracle, name):
    """(capture, reference frames, uncertain events, hop trace, oracle frames as ref_stream dicts), once per case"""
    if name not in _W:
        c = BY_NAME[name]
        x, trace = _capture(c), []
        frames, unc = S.receive(x, c["threshold"], trace=trace)
        s = oracle.Sync(threshold=c["threshold"])
        of = [S.view_oracle(f) for f in s.execute(x)]
        s.close()
        _W[name] = (x, frames, unc, trace, of)
    return _W[name]


# ---------------------------------------------------------------------------------------------------- a. the case list
def test_case_list_holds_what_it_promises(oracle):
    names = [c["name"] for c in SC.CASES]
    for d in SC.DS:
        for what in ("valid frame", "rejected header"):
            c = BY_NAME["resume after a %s, d=%d" % (what, d)]
            _, fr, _, _, _ = _world(oracle, c["name"])
            assert len(fr) == 2 and fr[1]["start"] - (fr[0]["last"] + 1) == d == c["gap"], c["name"]      # the gap is the one the name states
            assert bool(fr[0]["header_valid"]) == (what == "valid frame")
    assert SC.DS == (0, 1, 50, 99, 100, 101, 255, 256, 257)
    assert {"good frame %d samples into a rejected header" % o for o in (400, 590)} <= set(names)
    want = {("protocol", 101), ("protocol", 103), ("mod", 0), ("mod", 5), ("mod", 255), ("check", 0), ("check", 7), ("fec0", 0), ("fec0", 2),
            ("fec0", 31), ("fec1", 2)}
    assert {c["field"] for c in SC.CASES if "field" in c} == want
    for c in SC.CASES:
        if "field" in c:                                    # the good frame starts inside the span 2000 bytes would have claimed
            bad, good = c["frames"]
            h = SC.hdr20(bad)
            assert (int(h[15]) << 8 | int(h[16])) == 2000 and bad["at"] + SC.HDR_SPAN < good["at"] < bad["at"] + SC.HDR_SPAN + 2 * 8 * 2000
    assert {"control: protocol 102, modulation %d" % ms for ms in R.PAYLOAD_MODS} | {"control: check 1", "zero payload symbols"} <= set(names)
    o, h1, h2, _ = SC.HIDDEN["frames"]
    assert (o["mod"], o["fec0"], o["n"]) == (R.PSK2, R.FEC_V27, 100) and h1["amp"] == 2.0 and h1["at"] == o["at"] + SC.HDR_SPAN + 1200
    assert h1["at"] + SC.length(h1) < o["at"] + SC.span(o) < h2["at"] + SC.length(h2)
    assert len(SC.CAPTURE_ENDS) == 4 and {(c["name"], t) for c, t in SC.DETECTOR_CASES} >= {(c["name"], t) for c in (SC.DENSE, SC.HIDDEN) for t in (0.45, 0.5)}
    for c in SC.CASES + [SC.OVERLAP]:
        assert c["total"] <= 40_000 and all(f["n"] <= 100 for f in c["frames"]) and c["snr_db"] >= 12.0, c["name"]


def test_no_case_is_uncertain(oracle):
    """every decision of the reference is clear of its margins on every case, in both modes and with the options the GPU test uses"""
    for c in SC.CASES:
        assert not _world(oracle, c["name"])[2], (c["name"], _world(oracle, c["name"])[2])
    for c in SC.REJECTED + [SC.HIDDEN]:
        for kw in (dict(soft_header=True), dict(equalizer=True)):
            assert not S.receive(_capture(c), c["threshold"], **kw)[1], (c["name"], kw)
    for c, thr in SC.DETECTOR_CASES:
        assert not S.detect(SC.build(c), thr)[1], (c["name"], thr)


def test_amplitude_steps_stay_clear_of_the_threshold(oracle):
    """no hop of that stream has rxy within 5 % of the threshold; weak preambles sit under it and over it"""
    _, fr, _, trace, _ = _world(oracle, SC.STEPS["name"])
    thr = SC.STEPS["threshold"]
    r = np.array([t["rxy"] for t in trace])
    assert not np.any((r > 0.95 * thr) & (r < 1.05 * thr)), r[(r > 0.95 * thr) & (r < 1.05 * thr)]
    assert np.any((r > 0.8 * thr) & (r <= 0.95 * thr)) and np.any((r >= 1.05 * thr) & (r < 1.25 * thr))
    print("\nrxy of the hops over 0.8 of the threshold:", np.round(r[r > 0.8 * thr], 3))


# ---------------------------------------------------------------------------------------------------- b. oracle vs reference
def test_oracle_against_the_reference(oracle):
    worst, frames, rejected = {}, 0, 0
    for c in SC.CASES:
        x, fr, unc, _, of = _world(oracle, c["name"])
        bad = S.compare(fr, of, x, worst=worst)
        assert not bad, (c["name"], bad)
        frames += len(fr)
        rejected += sum(1 for f in fr if not f["header_valid"])
    for c, thr in SC.DETECTOR_CASES:
        x = SC.build(c)
        bad = S.compare_detections(S.detect(x, thr)[0], oracle.Detector(thr).run(x), worst)
        assert not bad, (c["name"], thr, bad)
    print("\nreference vs oracle: %d cases, %d frames (%d rejected); worst %s" % (len(SC.CASES), frames, rejected, {k: "%.3g" % v for k, v in worst.items()}))
    assert all(4.0 * worst[k] <= rd.PARITY[k] for k in rd.PARITY) and 4.0 * worst["rxy_rel"] <= S.RXY_MARGIN
    assert 4.0 * worst["sym"] <= rs.SYM_TOL and 4.0 * worst["sym_ratio"] <= 1.0
    m = S.MEASURED["oracle"]                       # the recorded figures are this run's, rounded up: they cannot drift
    assert all(0.5 * m[k] <= worst[k] <= m[k] for k in m), ("ref_stream.MEASURED['oracle'] is not this run's", {k: worst[k] for k in m})


# ---------------------------------------------------------------------------------------------------- c. truth
def test_reference_against_truth(oracle):
    for c in SC.CASES:
        x, fr, _, _, _ = _world(oracle, c["name"])
        bad = check_roles(c, fr, len(x))
        assert not bad, (c["name"], bad)
        if c in SC.REJECTED:                        # exactly one rejected frame, at the placed start
            assert [f["start"] for f in fr if not f["header_valid"]] == [g["at"] for g in c["frames"] if g["role"] == "rejected"], c["name"]
    for c in SC.CAPTURE_ENDS:                       # the whole capture (what two continuing blocks see) holds the frame
        whole = S.receive(SC.build(c), c["threshold"])[0]
        assert not check_roles(dict(c, frames=[dict(c["frames"][0], role="good")]), whole, c["total"]), c["name"]
    for c, thr in SC.DETECTOR_CASES:                # the detector-only mode reports every preamble, the hidden ones included
        pos = [d["pos"] for d in S.detect(SC.build(c), thr)[0]]
        assert all(f["at"] in pos for f in c["frames"]), (c["name"], thr, pos)


# ---------------------------------------------------------------------------------------------------- d. negative controls
CONTROLS = {
    "resume one sample early": (dict(resume_shift=-1), ["resume after a valid frame, d=99", "good frame 590 samples into a rejected header"]),
    "resume one sample late": (dict(resume_shift=1), ["resume after a valid frame, d=0", "resume after a rejected header, d=100"]),
    "history kept across the reset": (dict(keep_history=True), ["good frame 590 samples into a rejected header", "resume after a valid frame, d=0"]),
    "no room rule": (dict(room=False), ["a weak preamble without room in front of a strong one", "resume after a valid frame, d=100"]),
    "a rejected header consumes nothing": (dict(reject_consumes=False), ["good frame 400 samples into a rejected header", "resume after a rejected header, d=0"]),
    "the protocol byte is ignored": (dict(check_protocol=False), ["rejected header: protocol 101", "rejected header: protocol 103"]),
}


@pytest.mark.parametrize("name", sorted(CONTROLS))
def test_negative_controls_fail_against_the_oracle(oracle, name):
    mut, cases = CONTROLS[name]
    for cn in cases:
        x, fr, _, _, of = _world(oracle, cn)
        assert not S.compare(fr, of, x), cn
        bad = S.compare(S.receive(x, BY_NAME[cn]["threshold"], **mut)[0], of, x)
        print("\n%s on '%s': %s" % (name, cn, "; ".join(bad)[:300]))
        assert bad, (name, cn)


def test_negative_control_detector_without_overlap(oracle):
    c = SC.OVERLAP
    x = SC.build(c)
    for thr in (0.45, 0.5):
        od = oracle.Detector(thr).run(x)
        assert not S.compare_detections(S.detect(x, thr)[0], od)
        bad = S.compare_detections(S.detect(x, thr, overlap=False)[0], od)
        print("\nno overlap on '%s' at %.2f: %s" % (c["name"], thr, "; ".join(bad)))
        assert bad
