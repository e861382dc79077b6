"""Non-finite and overflowing IQ samples through the receiver: the contract of DESIGN.md section 4 ("Bad samples"), on the CPU.
tests/ref_stream.py's bad= path states, by index arithmetic alone, which decisions read a bad sample (`touched`); everything else
must equal the float64 reference as on clean input.
  a. the case list holds what it promises; the committed fixture is the one nonfinite_cases.py writes;
  b. the oracle against the reference on every case: untouched decisions under the existing bounds, touched ones by the rules;
  c. truth and the cap: every untouched frame is found where it was placed, at most one of a stream's three frames is touched
     (declared cases aside), and the share of fully compared frames is asserted;
  d. negative controls: mutations of the touched rules must fail b on a named case;
  e. the oracle over every case under ASan + UBSan + float-cast-overflow (tests/cpp/oracle_nonfinite.c, a stand-alone program)."""
import glob
import os
import subprocess

import numpy as np
import pytest

import nonfinite_cases as NC
import ref_detect as rd
import ref_stream as S
import ref_sync as rs
from stream_cases import check_roles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_ONLY = (NC.LARGE, NC.SCALE)          # declared: compared oracle <-> kernels only
REF_CASES = [c for c in NC.CASES if c["declared"] not in ORACLE_ONLY]
_W = {}


def world(oracle, name):
    """(stream, zeroed stream, reference frames, uncertain events, oracle frames), once per case"""
    if name not in _W:
        c = NC.BY_NAME[name]
        x = NC.build(c)
        fr, unc = S.receive(x, equalizer=c["eq"], bad=S.classify(x))
        q = oracle.Sync(threshold=0.5, equalizer=c["eq"])
        of = [S.view_oracle(f) for f in q.execute(x)]
        q.close()
        _W[name] = (x, NC.zeroed(x), fr, unc, of)
    return _W[name]


# ---------------------------------------------------------------------------------------------------- a. the case list
def test_case_list_holds_what_it_promises():
    assert 35 <= len(NC.CASES) <= 50 and all(8192 <= NC.LAYOUTS[c["layout"]]["total"] <= 12288 for c in NC.CASES)
    assert [v[0] for v in NC.VALUES] == ["nan re", "nan im", "nan", "+inf", "-inf", "+3e38", "-3e38", "2e19", "4e17", "-0.0"]
    for vn, v, wh in NC.VALUES:                # every value is used, as stated
        hit = [c for c in NC.CASES if c["name"].startswith(vn + " at ")]
        assert hit and all(c["which"] == wh and (c["value"] == v or v != v) and str(c["value"]) == str(float(v)) for c in hit), vn
    assert {c["run"] for c in NC.CASES} >= {1, 2, 300}
    x, fr = NC.clean("base")
    P = NC._positions("base")
    b = fr[1]
    w = b["start"] - b["lag"]
    assert all(abs(P["silence"] - a) >= 1024 for f in fr for a in (f["start"], f["last"]))
    assert P["before preamble"] == b["start"] - 1 and (P["window first"], P["window last"]) == (w, w + 511)
    assert w + 512 <= P["aligned only"] < b["start"] + 512 and 512 < P["header pilot"] - b["start"] < 640
    assert P["after frame"] == b["last"] + 1 and P["capture last"] == len(x) - 1
    for cut in NC.SEG_CUTS:                     # the cut lies inside a frame's payload
        assert any(f["start"] + 618 < cut - 1 and cut < f["last"] - 28 for f in NC.clean("cut%d" % cut)[1]), cut
    assert set(NC.BLOCK_CUTS) <= set(NC.SEG_CUTS)
    S_cls = S.classify(np.array([np.nan, 1j * np.inf, 2e19, -3e38, 4e17, 1.8e19, 1e15, -0.0], np.complex64))
    assert list(S_cls) == [S.BAD, S.BAD, S.BAD, S.BAD, S.LARGE, S.LARGE, 0, 0]
    with np.errstate(over="ignore"):
        assert np.float32(S.SQRT_FLT_MAX) ** 2 == np.inf and np.nextafter(np.float32(S.SQRT_FLT_MAX), np.float32(0)) ** 2 < np.inf
    with open(NC.GOLDEN, "rb") as f:
        assert f.read() == NC.fixture_bytes(), "tests/golden/nonfinite_cases.bin is stale: python tests/nonfinite_cases.py"
    assert os.path.getsize(NC.GOLDEN) < 1 << 20


def test_no_case_is_uncertain_but_the_declared_ones(oracle):
    for c in REF_CASES:
        assert not world(oracle, c["name"])[3], (c["name"], world(oracle, c["name"])[3])
    for c in NC.CASES:
        if c["declared"] == NC.LARGE:          # the reference says so itself
            x = NC.build(c)
            assert any(u[0] == "large" for u in S.receive(x, bad=S.classify(x))[1]), c["name"]


# ---------------------------------------------------------------------------------------------------- b. oracle vs reference
def test_oracle_against_the_reference(oracle):
    worst, counts = {}, {}
    for c in REF_CASES:
        x, x0, fr, _, of = world(oracle, c["name"])
        bad = S.compare_masked(fr, of, x0, equalizer=c["eq"], worst=worst, counts=counts)
        assert not bad, (c["name"], bad)
        d, unc = S.detect(x, bad=S.classify(x))                                # the detector-only mode
        od = oracle.Detector(0.5).run(x)
        assert not unc and [e["pos"] for e in d] == [e["pos"] for e in od], (c["name"], [e["pos"] for e in d], [e["pos"] for e in od])
        bad = S.compare_detections([e for e in d if not e.get("touched")], [g for e, g in zip(d, od) if not e.get("touched")], worst)
        assert not bad, (c["name"], bad)
        for e, g in zip(d, od):
            if e.get("touched"):
                assert not S.touched_estimates_off(e, g), (c["name"], e["pos"], S.touched_estimates_off(e, g))
    for c in NC.CASES:                                                         # the declared ones: the call returns
        if c["declared"] in ORACLE_ONLY:
            q = oracle.Sync(threshold=0.5)
            q.execute(NC.build(c))
            q.close()
    share = counts["compared"] / float(counts["compared"] + counts["touched"])
    print("\nreference vs oracle: %d cases, %r, share %.4f; worst %s" % (len(REF_CASES), counts, share, {k: "%.3g" % v for k, v in worst.items()}))
    assert all(4.0 * worst[k] <= rd.PARITY[k] for k in rd.PARITY) and 4.0 * worst["rxy_rel"] <= S.RXY_MARGIN
    assert 4.0 * worst["sym"] <= rs.SYM_TOL and 4.0 * worst["sym_ratio"] <= 1.0
    m = S.MEASURED["nonfinite_oracle"]             # the recorded figures are this run's, rounded up: they cannot drift
    assert all(0.5 * m[k] <= worst[k] <= m[k] for k in m), ("ref_stream.MEASURED['nonfinite_oracle'] is not this run's", {k: worst[k] for k in m})


# ---------------------------------------------------------------------------------------------------- c. truth and the cap
def test_reference_against_truth_and_the_cap(oracle):
    """every untouched frame is found at its place with its payload; a stream loses at most one of its three frames to the bad
    samples unless it is declared; two of three frames per stream stay compared, so the share is at least 2/3 by construction"""
    compared = total = 0
    for c in REF_CASES:
        x, _, fr, _, _ = world(oracle, c["name"])
        lay = NC.LAYOUTS[c["layout"]]
        clean = [f for f in fr if not f.get("touched")]
        found = [f for f in lay["frames"] if any(g["start"] == f["at"] for g in clean)]
        case = dict(name=c["name"], frames=found, snr_db=NC.SNR_DB)
        assert not check_roles(case, clean, len(x)), (c["name"], check_roles(case, clean, len(x)))
        assert len(found) >= (2 if c["declared"] is None else 1), (c["name"], [f["start"] for f in fr])
        if c["value"] == 0.0 or "silence" in c["name"] or "after frame" in c["name"] or "capture last" in c["name"]:
            assert len(found) == 3 and len(fr) == 3, c["name"]                 # the controls: nothing is touched
        compared += len(found)
        total += 3
    share = compared / float(total)
    print("\nshare of placed frames found untouched: %d / %d = %.4f" % (compared, total, share))
    assert share >= 2.0 / 3.0 and abs(share - S.MEASURED["nonfinite_share"]) < 5e-4, share


# ---------------------------------------------------------------------------------------------------- d. negative controls
CONTROLS = {
    "mask ignored (bad samples treated as zeros)": (dict(bad=None), "nan at window last"),
    "a touched window may detect": (dict(touched_detects=True), "nan at before preamble"),
    "a touched header is accepted": (dict(touched_header_ok=True), "nan at header pilot"),
    "resume right behind the bad sample of a touched payload": (dict(touched_payload_resume=True), "nan at payload first"),
    "history kept across the fresh detector": (dict(keep_history=True), "nan at payload last"),
}


@pytest.mark.parametrize("name", sorted(CONTROLS))
def test_negative_controls_fail_against_the_oracle(oracle, name):
    mut, cn = CONTROLS[name]
    x, x0, fr, _, of = world(oracle, cn)
    assert not S.compare_masked(fr, of, x0), cn
    kw = dict(bad=S.classify(x))
    kw.update(mut)
    bad = S.compare_masked(S.receive(x if kw["bad"] is not None else x0, **kw)[0], of, x0)
    print("\n%s on '%s': %s" % (name, cn, "; ".join(bad)[:300]))
    assert bad, (name, cn)


# ---------------------------------------------------------------------------------------------------- e. the sanitizer driver
def test_oracle_on_every_case_under_sanitizers(tmp_path):
    exe = str(tmp_path / "oracle_nonfinite")
    src = sorted(glob.glob(os.path.join(ROOT, "oracle", "fxref_*.c")))
    san = ["-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"]
    subprocess.check_call(["gcc", "-O1", "-std=gnu11", "-mfma", "-mavx2", "-ffp-contract=off", "-fno-fast-math", "-Wall"] + san +
                          ["-o", exe, os.path.join(ROOT, "tests", "cpp", "oracle_nonfinite.c")] + src + ["-lm"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, NC.GOLDEN], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "%d cases done" % len(NC.CASES) in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
