"""The captures and block-cut layouts of tests/test_ref_cuts.py and tests/test_gpu_cuts.py, as data.

A continuing stream reaches the library in blocks (fxrx_submit / fxrx_collect); DESIGN.md sections 2.1-2.2 promise the frames of
a single pass for any cut.  What bridges a cut is the state ring (35 entries per stream), three rotating carry buffers per
stream (block b reads carry[b % 3] and writes carry[(b + 1) % 3]) and two-piece addressing (samples below index 0 of a block
come from the carried tail).  The layouts below put a cut at every place where one of those has to hand something over, named
by the geometry tests/ref_stream.py and tests/ref_sync.py state -- their constants, not copies of them:

  a                 the aligned start of a frame (stream_cases: a frame placed at `at` is found at start == at)
  N, HOP, S_LEN     the detector's 512-sample window, its 256-sample hop, the 156-sample template (the room rule)
  n(c)              ref_sync.timing: the sample at which symbol c is read; its matched-filter span is the MF_TAPS = 28 samples
                    that end there (40 with the equaliser: EQ_TAPS - 1 more)
  c = 77 / 78       the last p/n symbol / the first header symbol; c = 308 header symbol 230; payload symbol j is c = 309 + j
  last, resume      the last sample a frame consumes (stream_cases.span) and the first sample of the fresh detector behind it

A cut at p means: one block ends with sample p - 1, the next one starts with sample p.  A layout is a list of cuts, in order; a
repeated cut is a block of zero samples.  Every capture is built the way tests/stream_cases.py builds its own (ref_framegen
frames, seeded noise), and one capture is shared by all its layouts so that the float64 reference runs once per capture.
"""
import numpy as np

import ref_decode as R
import ref_detect as rd
import ref_sync as rs
import stream_cases as SC
from stream_cases import F, length, npay, span

N, HOP, S_LEN = rd.N, rd.N // 2, rd.S_LEN
REACH = rs.MF_TAPS - 1                           # samples in front of a symbol's own that its filter reads
REACH_EQ = REACH + rs.EQ_TAPS - 1
C_LAST_PN = rs.PRE_DELAY + rs.PN_LEN - 1
C_HDR = rs.PRE_DELAY + rs.PN_LEN
C_PAY = C_HDR + rs.HDR_SYM
LEAD = 700                                       # a - N >= 0 with room for a block in front of it
BAD = SC.BAD


def n_of(f, c, eq=False):
    """the sample (relative to the capture) at which symbol c of frame f is read"""
    return f["at"] + int(rs.timing(-f["dt"])[2](c + (rs.EQ_DELAY if eq else 0)))


def sym_span(f, c, eq=False):
    hi = n_of(f, c, eq)
    return hi - (REACH_EQ if eq else REACH), hi


def last_sample(f, valid=True):
    return f["at"] + span(f, valid) - 1


def _capture(name, frames, seed, snr_db, tail=900):
    total = max(f["at"] + length(f) for f in frames) + tail
    assert total <= 40_000
    return dict(name=name, frames=frames, seed=seed, snr_db=snr_db, threshold=0.5, total=total)


# ---- QPSK, r1/2, 300 bytes: more than 1024 payload symbols (a second fx_paymf4_kernel item); two frames with no sample between
# them and a third 257 samples behind
q0 = F(LEAD, n=300, fec0=R.FEC_V27, pseed=301)
q1 = F(q0["at"] + length(q0), n=300, fec0=R.FEC_V27, dt=0.25, pseed=302)
q2 = F(q1["at"] + length(q1) + HOP + 1, n=300, fec0=R.FEC_V27, pseed=303)
assert npay(q0) > 1026
QPSK = _capture("QPSK r1/2 300 B: zero gap, then 257 samples", [q0, q1, q2], 2100, 15.0)

# ---- QAM16, punctured fec0, Golay fec1, 200 bytes at 17 dB: channel errors in every frame, so no frame is `clean` and the trellis
# kernels stay in the chain
m0 = F(LEAD, n=200, mod=R.QAM16, fec0=R.FEC_V27P34, fec1=R.FEC_GOLAY, pseed=311)
m1 = F(m0["at"] + length(m0) + 90, n=200, mod=R.QAM16, fec0=R.FEC_V27P34, fec1=R.FEC_GOLAY, dt=0.25, pseed=312)
QAM = _capture("QAM16 V27P34 + Golay 200 B", [m0, m1], 2200, 17.0)

# ---- DPSK4: the differential decoder's running sum crosses the cut
d0 = F(LEAD, n=150, mod=R.DPSK4, fec0=R.FEC_V27, pseed=321)
d1 = F(d0["at"] + length(d0) + 40, n=150, mod=R.DPSK4, fec0=R.FEC_V27, dt=0.25, pseed=322)
DPSK = _capture("DPSK4 r1/2 150 B", [d0, d1], 2300, 15.0)

# ---- a CRC-valid header that is rejected (protocol 101) claiming 2000 bytes, and a good frame 60 samples behind its header
r0 = F(LEAD, n=0, check=R.CRC_NONE, pseed=331, hdr=dict(BAD, protocol=101), role="rejected")
r1 = F(r0["at"] + span(r0, False) + 60, n=120, mod=R.PSK8, fec0=R.FEC_V27, pseed=332)
REJ = _capture("rejected header, good frame 60 samples behind", [r0, r1], 2400, 15.0)

CAPTURES = [QPSK, QAM, DPSK, REJ]


def build(cap):
    return SC.build(cap)


def cut_points(f, eq=False):
    """name -> cut position for one frame: every place of the module docstring that the frame has"""
    a, P = f["at"], {}
    for d in (-N, -HOP - 1, -HOP, -HOP + 1, -1, 0, 1, S_LEN - 1, S_LEN, S_LEN + 1, HOP - 1, HOP, N - 1, N):
        P["a%+d" % d] = a + d
    valid = f["role"] != "rejected"
    spans = [("last p/n symbol", C_LAST_PN), ("first header symbol", C_HDR)]
    if valid and npay(f):
        spans.append(("first payload symbol", C_PAY))
    for what, c in spans:
        lo, hi = sym_span(f, c, eq)
        P.update({what + ": first sample of its span": lo, what + ": middle of its span": (lo + hi) // 2, what + ": its own sample": hi})
    h230 = n_of(f, C_PAY - 1, eq)
    P.update({"header symbol 230 -1": h230 - 1, "header symbol 230": h230, "header symbol 230 +1": h230 + 1})
    if valid and npay(f):
        js = [7, 8, 9, 1023, 1024, 1025] + list(range(npay(f) - 4, npay(f)))
        for j in js:
            if 0 <= j < npay(f):
                P["payload symbol %d" % j] = n_of(f, C_PAY + j, eq)
    last = last_sample(f, valid)
    P.update({"last sample -1": last - 1, "last sample": last, "resume": last + 1, "resume +1": last + 2})
    return P


def layouts(cap):
    """[(name, [cuts])] for a capture: one cut at every cut_points position of its first frame, a few around the starts of the
    others, and the layouts with several cuts"""
    fr = cap["frames"]
    f0 = fr[0]
    out = [("frame 0: " + k, [p]) for k, p in cut_points(f0).items()]
    for i, f in enumerate(fr[1:], 1):
        P = cut_points(f)
        out += [("frame %d: %s" % (i, k), [P[k]]) for k in ("a%+d" % d for d in (-HOP, -1, 0, S_LEN, N))]
        if f["at"] == fr[i - 1]["at"] + length(fr[i - 1]):
            out.append(("between the zero-gap frames %d and %d" % (i - 1, i), [f["at"]]))
    big = max(fr, key=length)
    a, L = big["at"], length(big)
    out.append(("two cuts inside one frame", [a + L // 4, a + L // 2]))
    out.append(("three cuts inside one frame", [a + L // 5, a + 2 * L // 5, a + 3 * L // 5]))       # the same tail through all three carry buffers
    out.append(("a block of 1 sample inside a frame", [a + 900, a + 901]))
    out.append(("a block of 255 samples inside a frame", [a + 900, a + 900 + HOP - 1]))
    out.append(("a block of 1 and a block of 255 samples inside a frame", [a + L // 3, a + L // 3 + 1, a + L // 3 + HOP]))
    # the stream gets nothing in the second block while every other layout's stream does, with a tail to carry on (cut inside a
    # payload, and inside a header): carry[1] -> carry[2] with nothing new behind it
    out.append(("zero-length block with a payload tail", [a + L // 2, a + L // 2]))
    out.append(("zero-length block with a header tail", [a + 400, a + 400, a + 400]))
    out.append(("zero-length first block", [0]))
    for name, cuts in out:
        assert all(0 <= p <= cap["total"] for p in cuts) and cuts == sorted(cuts), (cap["name"], name, cuts)
    assert len({n for n, _ in out}) == len(out)
    return out


ZERO_BLOCK = "zero-length block with a payload tail"
THREE_CUTS = "three cuts inside one frame"
MID_PAYLOAD = "frame 0: payload symbol 8"


def pieces(total, cuts, n_blocks=None):
    """block lengths of a layout, padded with empty blocks to n_blocks"""
    e = [0] + list(cuts) + [total]
    out = [b - a for a, b in zip(e[:-1], e[1:])]
    return out + [0] * ((n_blocks or len(out)) - len(out))


def many_blocks(total, n=72):
    """n blocks of unequal small sizes (weights 1..11 by a quadratic residue pattern): the state ring wraps twice -- it has
    kStateRing = kMaxDepth + 3 = 35 entries per stream (fx_host.cpp; tests/test_gpu_controls.py reads both there), block b uses
    entry b % 35, so blocks 35 and 70 start a new round -- and every b % 3 meets a frame boundary"""
    w = np.array([1 + (k * k * 37) % 11 for k in range(n)], np.float64)
    cuts = [int(v) for v in np.floor(np.cumsum(w)[:-1] / w.sum() * total)]
    assert len(set(cuts)) == n - 1 and len(set(np.diff([0] + cuts + [total]))) > 5
    return cuts


# ---- reduced layout lists for the options of tests/test_gpu_cuts.py
def equalizer_layouts(cap):
    """cuts inside the 40-sample span of the first header and payload symbols and inside a training (p/n) symbol's span"""
    f0 = cap["frames"][0]
    out = []
    for what, c in (("p/n symbol 0", rs.PRE_DELAY), ("p/n symbol 32", rs.PRE_DELAY + 32), ("first header symbol", C_HDR), ("first payload symbol", C_PAY)):
        lo, hi = sym_span(f0, c, eq=True)
        out += [("eq %s: first sample of its span" % what, [lo]), ("eq %s: sample %d of its span" % (what, rs.MF_TAPS), [lo + rs.MF_TAPS]), ("eq %s: its own sample" % what, [hi])]
    return out + [(n, c) for n, c in layouts(cap) if n in (ZERO_BLOCK, THREE_CUTS)]


def reduced_layouts(cap):
    keep = ("frame 0: a-256", "frame 0: a+0", "frame 0: a+156", "frame 0: first header symbol: middle of its span", "frame 0: header symbol 230",
            "frame 0: first payload symbol: middle of its span", MID_PAYLOAD, "frame 0: last sample", "frame 0: resume", ZERO_BLOCK, THREE_CUTS)
    out = [(n, c) for n, c in layouts(cap) if n in keep]                 # (a rejected first frame has no payload positions)
    assert len(out) == len(keep) - (0 if cap["frames"][0]["role"] != "rejected" else 2)
    return out


def detector_layouts(cap):
    a = cap["frames"][0]["at"]
    return [("detector a%+d" % d, [a + d]) for d in (-HOP, -HOP + 1, -1, 0, 1, S_LEN - 1, S_LEN, S_LEN + 1, HOP - 1, HOP, HOP + 1, N - 1, N)]


# ---- the recorded pair (DESIGN.md section 6, round-5 log): two continuing streams in one context, blocks of 100 000 samples
PAIR = dict(ids=(1540, 1541), snr_db=(14.0, 4.0), payload_len=(500, 800), block=100_000, straddler=98_318, next_start=107_256,
            frame_len=(8682, 13482), neighbour_straddler=96_166, oracle_first_200k=((22, 22), (14, 9)))


def pair_streams(fx, n_samples):
    return [fx.synth_stream(n_samples, stream_id=i, snr_db=s, payload_len=p, return_payloads=False) for i, s, p in zip(PAIR["ids"], PAIR["snr_db"], PAIR["payload_len"])]
