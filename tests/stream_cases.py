"""The streams of tests/test_ref_stream.py and tests/test_gpu_ref_stream.py, as data.

A case is a dict: name, seed, snr_db (noise over the whole capture, relative to a frame of amplitude 1), total (samples), frames,
threshold, and for the capture-end cases `cut` (the one-shot capture is the first `cut` samples; the whole is what two
continuing blocks see).  A frame is a dict: at (sample of frame sample 0), dt, amp, n / pseed (payload bytes and their seed),
mod, fec0, fec1, check, hdr (overrides of the six protocol fields, or None), role:
    good      found at `at` with a valid header and its payload
    rejected  found at `at` with header_valid == 0
    broken    found at `at`; its payload may fail its check
    detected  found at `at`; nothing is asked of its header or payload (a weak frame above the threshold)
    absent    nothing is reported at `at` (hidden inside what another frame consumes, or below the threshold)
    cut       the capture ends inside it: not delivered one-shot
Every frame is a ref_framegen frame: nothing here comes from a product generator.  dt is -0.25 or +0.25, so that tau is near
+0.25 (symbols on the even samples) or -0.25 (odd samples) and far from a branch edge; `span` below is ref_sync's n(c) for
either.  build(case) returns the complex64 capture."""
import numpy as np

import ref_decode as R
import ref_framegen as rf

PROTOCOL = 102
HDR_SPAN = 2 * (14 + 64 + 231)             # sample after header symbol 230 on the even grid: at + 617 is the next one


def F(at, n=24, mod=R.PSK4, fec0=R.FEC_NONE, fec1=R.FEC_NONE, check=R.CRC_24, dt=-0.25, amp=1.0, pseed=1, hdr=None, role="good"):
    return dict(at=int(at), n=n, mod=mod, fec0=fec0, fec1=fec1, check=check, dt=dt, amp=amp, pseed=pseed, hdr=hdr, role=role)


def npay(f):
    return rf.num_payload_symbols(f["n"], f["mod"], f["fec0"], f["fec1"], f["check"])


def span(f, valid=True):
    """samples the receiver consumes from `at` on: the next sample is at + span"""
    return HDR_SPAN - 1 + (2 * npay(f) if valid else 0) - (1 if f["dt"] > 0 else 0)


def length(f):
    return 2 * (64 + 231 + npay(f) + 14)


def hdr20(f):
    h = dict(protocol=PROTOCOL, payload_len=f["n"], mod=f["mod"], check=f["check"], fec0=f["fec0"], fec1=f["fec1"])
    h.update(f["hdr"] or {})
    user = (np.arange(14) * 17 + f["pseed"]) % 256
    return np.array(list(user) + [h["protocol"], h["payload_len"] >> 8, h["payload_len"] & 255, h["mod"], ((h["check"] & 7) << 5) | (h["fec0"] & 31),
                                  h["fec1"] & 31], np.uint8)


def payload(f):
    return np.random.default_rng(9000 + f["pseed"]).integers(0, 256, f["n"], dtype=np.uint8)


def samples(f):
    return f["amp"] * rf.frame(payload(f), f["mod"], f["fec0"], f["fec1"], f["check"], dt=f["dt"], hdr20=hdr20(f))


def build(case):
    rng = np.random.default_rng(case["seed"])
    n = case["total"]
    sig = np.sqrt(0.5 * 10.0 ** (-case["snr_db"] / 10.0))
    x = sig * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    for f in case["frames"]:
        s = samples(f)
        assert f["at"] >= 0 and f["at"] + len(s) <= n, (case["name"], f["at"], len(s), n)
        x[f["at"]:f["at"] + len(s)] += s
    return x.astype(np.complex64)


def check_roles(case, frames, x_len):
    """the frames a case placed against what a receiver reports (dicts with start, tau, header_valid, header, payload,
    payload_valid): list of failure strings"""
    import ref_detect as rd
    import ref_stream as S
    rd.set_template(S.conventions()[1])
    bad = []
    for f in case["frames"]:
        hit = [g for g in frames if abs(g["start"] - f["at"]) <= 2]
        role = f["role"]
        if role in ("absent", "cut"):
            if hit:
                bad.append("%s frame at %d is reported" % (role, f["at"]))
            continue
        if len(hit) != 1 or hit[0]["start"] != f["at"]:
            bad.append("%s frame at %d: reported starts %r" % (role, f["at"], [g["start"] for g in hit]))
            continue
        g = hit[0]
        if role == "detected":
            continue
        # check_truth's start rule: start + tau against the arrival time.  The frame is advanced by dt (ref_framegen's convention)
        tol = rd.tolerances(case["snr_db"] + 20.0 * np.log10(f["amp"]))["arrival"]
        if abs(g["start"] + g["tau"] - (f["at"] - f["dt"])) > tol:
            bad.append("%s frame at %d: arrival %.4f vs %.4f (tolerance %.3f)" % (role, f["at"], g["start"] + g["tau"], f["at"] - f["dt"], tol))
        if bytes(g["header"]) != hdr20(f).tobytes():
            bad.append("%s frame at %d: header bytes" % (role, f["at"]))
        if role == "rejected":
            if g["header_valid"]:
                bad.append("rejected frame at %d has a valid header" % f["at"])
        elif not g["header_valid"]:
            bad.append("%s frame at %d: header not valid" % (role, f["at"]))
        elif role == "good" and not (g["payload_valid"] and bytes(g["payload"]) == payload(f).tobytes()):
            bad.append("good frame at %d: payload" % f["at"])
    return bad


def _case(name, frames, seed, snr_db=15.0, threshold=0.5, tail=700, **kw):
    total = max(f["at"] + length(f) for f in frames) + tail
    assert total <= 40_000 and all(f["n"] <= 100 for f in frames) and snr_db >= 12.0
    return dict(name=name, frames=frames, seed=seed, snr_db=snr_db, threshold=threshold, total=total, **kw)


DS = (0, 1, 50, 99, 100, 101, 255, 256, 257)
LEAD = 300
CASES = []

# ---- resume after a valid frame: the next frame d samples after the last consumed one.  The fresh detector's first window is
# half zeros, so the preamble sits at lag 256 + d there: d < 100 detects in it, d >= 100 only in the next window (lag d).
for i, d in enumerate(DS):
    a = F(LEAD, n=40, fec0=R.FEC_V27, dt=-0.25 if i % 2 == 0 else 0.25, pseed=10 + i)
    b = F(LEAD + span(a) + d, n=30, mod=R.QAM16, dt=0.25 if i % 3 == 0 else -0.25, pseed=30 + i)
    CASES.append(_case("resume after a valid frame, d=%d" % d, [a, b], 100 + i, gap=d))

# ---- resume after a rejected header (protocol 101, CRC-valid): d from the end of the header
BAD = dict(payload_len=2000, mod=R.PSK4, check=R.CRC_24, fec0=R.FEC_V27, fec1=R.FEC_NONE)
for i, d in enumerate(DS):
    a = F(LEAD, n=0, check=R.CRC_NONE, dt=-0.25 if i % 2 else 0.25, pseed=50 + i, hdr=dict(BAD, protocol=101), role="rejected")
    b = F(LEAD + span(a, False) + d, n=30, mod=R.PSK8, pseed=70 + i)
    CASES.append(_case("resume after a rejected header, d=%d" % d, [a, b], 200 + i, gap=d))
# a good frame that starts inside the rejected header's own span: at 400 its preamble is consumed with the header (absent); at
# 590 its preamble straddles the restart, and the fresh detector finds it with its start in front of its own first sample
for i, (off, role) in enumerate(((400, "absent"), (590, "good"))):
    a = F(LEAD, n=0, check=R.CRC_NONE, pseed=90 + i, hdr=dict(BAD, protocol=101), role="rejected")
    b = F(LEAD + off, n=30, mod=R.PSK8, amp=0.4 if off == 400 else 1.0, pseed=(95, 93)[i], role=role)
    c = F(LEAD + off + length(b) + 200, n=16, pseed=94 + i)
    CASES.append(_case("good frame %d samples into a rejected header" % off, [a, b, c], 220 + i, snr_db=20.0))

# ---- CRC-valid headers that must be rejected for a field, each followed by a good frame inside the span its payload length
# (2000 bytes) would have claimed; and the controls, which must be accepted
REJECTED_FIELDS = [("protocol", 101), ("protocol", 103), ("mod", 0), ("mod", 5), ("mod", 255), ("check", 0), ("check", 7),
                   ("fec0", 0), ("fec0", 2), ("fec0", 31), ("fec1", 2)]
for i, (field, v) in enumerate(REJECTED_FIELDS):
    a = F(LEAD, n=0, check=R.CRC_NONE, dt=-0.25 if i % 2 == 0 else 0.25, pseed=110 + i, hdr=dict(BAD, **{field: v}), role="rejected")
    b = F(LEAD + span(a, False) + 300 + 37 * i, n=20 + i, fec0=R.FEC_V27, pseed=130 + i)
    CASES.append(_case("rejected header: %s %d" % (field, v), [a, b], 300 + i, field=(field, v)))
for i, ms in enumerate(R.PAYLOAD_MODS):
    a = F(LEAD, n=18 + i, mod=ms, dt=-0.25 if i % 2 == 0 else 0.25, pseed=150 + i, hdr=dict(protocol=PROTOCOL))
    b = F(LEAD + span(a) + 120 + 11 * i, n=12, pseed=170 + i)
    CASES.append(_case("control: protocol 102, modulation %d" % ms, [a, b], 340 + i, snr_db=24.0 if R.bps(ms) >= 4 else 15.0))
a = F(LEAD, n=25, check=R.CRC_NONE, pseed=190, hdr=dict(check=R.CRC_NONE))
CASES.append(_case("control: check 1", [a, F(LEAD + span(a) + 130, n=12, pseed=191)], 360))

# ---- zero payload symbols: delivered at header symbol 230, the next frame right behind
a = F(LEAD, n=0, check=R.CRC_NONE, pseed=200)
assert npay(a) == 0
CASES.append(_case("zero payload symbols", [a, F(LEAD + span(a) + 50, n=12, pseed=201), ], 400))

# ---- a preamble hidden in a payload: the outer frame PSK2, V27, 100 bytes; inside its payload a frame at twice the amplitude
# (from 1200 samples into the payload, ending before it) and one that ends after it; then traffic goes on
OUT = LEAD + 2300                           # so that segments of 4096 and of 6000 samples start inside the outer payload, in front of a hidden preamble
outer = F(OUT, n=100, mod=R.PSK2, fec0=R.FEC_V27, pseed=210, role="broken")
h1 = F(OUT + HDR_SPAN + 1200, n=20, amp=2.0, pseed=211, role="absent")
h2 = F(OUT + span(outer) - 500, n=20, pseed=212, role="absent")
after = F(OUT + span(outer) + length(h2) - 500 + 400, n=24, mod=R.PSK8, pseed=213)
assert h1["at"] + length(h1) < OUT + span(outer) < h2["at"] + length(h2) and h2["at"] + 156 < OUT + span(outer)
assert OUT + HDR_SPAN < 4096 < h1["at"] < 6000 < h2["at"]
HIDDEN = _case("preambles hidden in a payload", [outer, h1, h2, after], 500, snr_db=20.0, tail=4300)    # two segments of 6000 samples
CASES.append(HIDDEN)

# ---- amplitude steps around the threshold: at 12 dB of noise under a unit frame, frames at amplitudes whose rxy the reference
# puts at least 5 % under or over the threshold (tests/test_ref_stream.py asserts the band is empty)
AMPS = ((0.10, "absent"), (1.0, "good"), (0.125, "absent"), (0.5, "detected"), (0.12, "absent"), (0.35, "detected"), (0.17, "detected"), (2.0, "good"))
fr, at = [], LEAD
for i, (amp, role) in enumerate(AMPS):
    f = F(at, n=16, amp=amp, dt=-0.25 if i % 2 else 0.25, pseed=230 + i, role=role)
    fr.append(f)
    at += length(f) + 600 + 53 * i
STEPS = _case("amplitude steps around the threshold", fr, 600, snr_db=12.0)
CASES.append(STEPS)

# ---- the room rule: a weak preamble at lag 400 of its window (its template cut off by the window's end) right in front of a strong
# one.  The hop that holds it whole holds the strong one's first samples too, at a lag without room, and those win: the weak
# frame is never detected.  Without the rule it would be, one hop earlier.
weak = F(512 + 400, n=16, amp=0.5, pseed=240, role="absent")
strong = F(weak["at"] + 300, n=16, amp=2.0, pseed=241)
ROOM = _case("a weak preamble without room in front of a strong one", [weak, strong], 650, snr_db=20.0)
CASES.append(ROOM)

# ---- the capture ends inside the preamble window, inside the header, one sample short of the payload's end, and exactly at it
a = F(LEAD, n=40, fec0=R.FEC_V27, pseed=250, role="cut")
CAPTURE_ENDS = []
for i, (what, cut) in enumerate((("inside the preamble window", LEAD + 400), ("inside the header", LEAD + 560),
                                 ("one sample short of the payload's end", LEAD + span(a) - 1), ("exactly at the payload's end", LEAD + span(a)))):
    c = _case("capture ends " + what, [dict(a, role="good" if cut == LEAD + span(a) else "cut")], 700, cut=cut)
    CAPTURE_ENDS.append(c)
    CASES.append(c)

# ---- detector-only mode: dense tiny frames and the hidden-frame stream, at 0.45 and 0.5
fr, at = [], 200
for i in range(14):
    f = F(at, n=i % 5, mod=R.QAM64, dt=-0.25 if i % 2 else 0.25, pseed=270 + i)
    fr.append(f)
    at += length(f) + (0, 3, 17, 40, 1, 150, 260)[i % 7]
DENSE = _case("dense tiny frames", fr, 800, snr_db=25.0)
CASES.append(DENSE)
# a second preamble 400 samples after a detection: only the window that overlaps the aligned one by its second half holds it whole
OVERLAP = _case("a preamble 400 samples behind another", [F(LEAD, n=8, pseed=290, role="detected"), F(LEAD + 400, n=8, amp=2.0, pseed=291, role="detected"),
                                                          F(LEAD + 1500, n=8, pseed=292, role="detected")], 810, snr_db=20.0)
DETECTOR_CASES = [(c, thr) for c in (DENSE, HIDDEN, OVERLAP) for thr in (0.45, 0.5)]

REJECTED = [c for c in CASES if any(f["role"] == "rejected" for f in c["frames"])]
assert len({c["name"] for c in CASES}) == len(CASES)
