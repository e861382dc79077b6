"""Float64 statement of the receiver's sequencing: capture -> list of frames -- test infrastructure.

What the other references leave open: which windows the detector looks at, when a hop counts, where the synchroniser
resumes after a frame or after a header that fails, what history the detector restarts with, and what the detector-only
mode does after a detection.  Composed of ref_detect (one hop, ALIGN), ref_sync (aligned frame -> symbols), ref_decode and
ref_header_soft only; the tables are ref_framegen.tables() and the template ref_detect.build_template of them.  It shares no
code with the oracle (oracle/fxref_frame.c) or the kernels: numpy float64 / complex128 throughout.

Margins (a decision inside one of them is `uncertain`: a float32 implementation may decide otherwise, and from the first such
event on this statement's output is not compared; tests/stream_cases.py holds only cases without one):
  RXY_MARGIN     relative, on rxy against the threshold.  rxy = |R| / (N g0 sqrt(Es)): |R| carries ref_detect's 6e-7 (TIE_MARGIN
                 is 100x that on |R|^2, i.e. 5e-5 on |R|), g0 is the root of a float32 sum of 512 squares (at most 512 x 2^-24 / 2
                 = 1.5e-5 relative, sequentially): 5e-5 + 1.5e-5 < 1e-4 = ref_detect.TIE_MARGIN, taken as the margin.
  TIE_MARGIN     ref_detect's, on the two strongest (bin, lag) cells of a hop that may detect.
  BRANCH_MARGIN  on 32 tau against an integer (ref_sync.near_branch_edge's eps).  There tau is the implementation's own float32
                 value; here it is this statement's, which a float32 detector may miss by ref_detect.PARITY["tau"]:
                 32 x 2e-5 = 6.4e-4.  An integer of 32 tau at 0 is also the sign of tau, i.e. the symbol grid.
  HEADER_MARGIN  on the real and imaginary part of a header data symbol against 0.  The symbols are normalised by the pilot
                 gain to unit modulus; ref_sync.SYM_TOL (4e-5) is its derived bound for a float32 symbol on a unit-energy
                 constellation, and it covers ref_sync.tie_margin of every scheme (1e-5 at most).
"""
import numpy as np

import ref_decode as R
import ref_detect as rd
import ref_header_soft as RH
import ref_sync as rs

N, HOP, S_LEN = rd.N, rd.N // 2, rd.S_LEN
RXY_MARGIN = rd.TIE_MARGIN
BRANCH_MARGIN = rs.NPFB * rd.PARITY["tau"]
HEADER_MARGIN = max(rs.SYM_TOL, rs.TIE_PSK, rs.TIE_GRID)

# worst reference-vs-implementation differences over tests/stream_cases.py: against the oracle (CPU, tests/test_ref_stream.py)
# and against the library (MI355X, tests/test_gpu_ref_stream.py, every segment size).  The estimates' bounds are
# ref_detect.PARITY, rxy's is RXY_MARGIN, the symbols' ref_sync.SYM_TOL; each must stay >= 4x these.
MEASURED = dict(oracle=dict(tau=1.8e-7, gamma_rel=4.2e-7, dphi=1.3e-7, phi=9.1e-6, rxy_rel=2.7e-7, sym=8.9e-7),        # both modes
                gpu=dict(tau=1.8e-7, gamma_rel=4.2e-7, dphi=4.7e-9, phi=4.0e-7, rxy_rel=2.7e-7, sym=8.9e-7),           # the frame mode
                # tests/nonfinite_cases.py, untouched decisions only (tests/test_ref_nonfinite.py, tests/test_gpu_ref_nonfinite.py);
                # the share is that of the placed frames the reference finds untouched
                nonfinite_oracle=dict(tau=1.8e-7, gamma_rel=2.9e-7, dphi=6.5e-8, phi=5.4e-6, rxy_rel=3.1e-7, sym=6.8e-7),
                nonfinite_gpu=dict(tau=1.8e-7, gamma_rel=2.9e-7, dphi=2.6e-9, phi=1.9e-7, rxy_rel=3.1e-7, sym=4.7e-7),
                nonfinite_share=0.7259)

# bad samples (classify): BAD = non-finite, or a component whose square overflows binary32 (|c| >= 2^64, 1.85e19): whatever
# reads one computes NaN, Inf or Inf - Inf under IEEE rules.  LARGE = finite, a component in [1e16, 1.85e19): its own square is finite
# but |R|^2 of a correlation over it ((156 |c|)^2 from 1.2e17 on) is not -- binary32 then sees an infinite peak over a finite energy
# and detects where this float64 statement does not.  A decision that reads a LARGE sample is `uncertain`.
BAD, LARGE = 1, 2
SQRT_FLT_MAX = 2.0 ** 64                     # the smallest binary32 value whose square is not finite

_CONV = {}


def classify(x):
    """int8 per sample: 0, BAD or LARGE"""
    v = np.asarray(x).astype(np.complex128)
    a = np.maximum(np.abs(v.real), np.abs(v.imag))                  # NaN propagates through maximum
    out = np.zeros(len(v), np.int8)
    out[(a >= 1e16) & (a < SQRT_FLT_MAX)] = LARGE
    out[~(a < SQRT_FLT_MAX)] = BAD                                   # NaN, Inf, and what squares to Inf
    return out


class _Mask:
    """the bad-sample classes as the detector sees them (256 zeros in front, nothing in front of `floor`), by prefix sums"""

    def __init__(self, cls, floor):
        m = np.concatenate([np.zeros(HOP, np.int8), cls])
        m[:HOP + floor] = 0
        self.c = [np.concatenate([[0], np.cumsum(m == k)]) for k in (BAD, LARGE)]
        self.m = m

    def any(self, lo, hi, k=BAD):
        """a sample of class k in capture samples [lo, hi]"""
        lo, hi = max(int(lo) + HOP, 0), min(int(hi) + HOP, len(self.m) - 1)
        return hi >= lo and self.c[k - 1][hi + 1] - self.c[k - 1][lo] > 0

    def first(self, lo, hi):
        lo, hi = max(int(lo) + HOP, 0), min(int(hi) + HOP, len(self.m) - 1)
        return int(np.nonzero(self.m[lo:hi + 1] == BAD)[0][0]) + lo - HOP


def conventions():
    """(ref_sync.Tables, the 156-sample template), from the definitions in tests/ref_framegen.py"""
    if not _CONV:
        import ref_framegen as rf
        tb = rf.tables()
        _CONV["tb"], _CONV["s"] = tb, rd.build_template(tb.pn, rf.tx_taps(0.0))
    return _CONV["tb"], _CONV["s"]


def _hop(xp, w, s, threshold, room, unc, trace):
    """One SEEK hop on xp[w + 256 : w + 768) (xp = 256 zeros + the capture as this detector sees it).  Returns the seek dict
    when the hop detects, else None."""
    h = rd.seek(xp[w + HOP:w + HOP + N], s)
    fits = h["lag"] < N - S_LEN or not room
    if trace is not None:
        trace.append(dict(w=w, rxy=h["rxy"], lag=h["lag"], bin=h["bin"], silent=h["silent"]))
    if h["silent"]:
        return None
    if fits and abs(h["rxy"] - threshold) <= RXY_MARGIN * threshold:
        unc.append(("threshold", w, h["rxy"]))
    if h["rxy"] > threshold * (1.0 - RXY_MARGIN):
        top = np.partition(h["r2"].ravel(), -2)[-2:]
        if top[1] > 0.0 and (top[1] - top[0]) / top[1] < rd.TIE_MARGIN:
            unc.append(("tie", w, float((top[1] - top[0]) / top[1])))
    return h if (h["rxy"] > threshold and fits) else None


def _padded(x, floor):
    """256 zeros + the capture, with everything in front of capture sample `floor` read as zero"""
    xp = np.concatenate([np.zeros(HOP, np.complex128), np.asarray(x, np.complex128)])
    xp[:HOP + floor] = 0.0
    return xp


def _touched_align(xp, mk, start, s, cfo_bin):
    """ALIGN on a window that holds a BAD sample: the correlation over all 512 samples is NaN, so tau reads 0 and gamma is NaN;
    the carrier estimates come from the window's first 156 samples times the template alone, and are NaN only when the bad sample
    is among those -- else they are what ALIGN gives (the samples behind do not enter them)."""
    est = dict(tau=0.0, gamma=np.nan, dphi=np.nan, phi=np.nan)
    if not mk.any(start, start + S_LEN - 1):
        full = rd.align(xp[start + HOP:start + HOP + N], s, cfo_bin)
        est.update(dphi=full["dphi"], phi=full["phi"])
    return est


def receive(x, threshold=0.5, equalizer=False, soft_header=False, trace=None,
            resume_shift=0, keep_history=False, room=True, reject_consumes=True, check_protocol=True,
            bad=None, touched_detects=False, touched_header_ok=False, touched_payload_resume=False):
    """The frames of capture x and the uncertain events: (list of frame dicts, list of (kind, position, value)).

    Rules:
      - The detector starts with 256 zeros of history.  Its windows are [w, w + 512), w = -256, 0, 256, ...: they advance by 256.
      - A hop detects when its window is not silent, rxy > threshold and lag < 512 - 156 (room for the template).
      - The aligned window starts at start = w + lag and must lie inside the capture (the detector waits for its last sample).
      - ALIGN is ref_detect.align on that window for the winning bin; it is not thresholded again.
      - The frame is ref_sync.sync(x, start, tau, gamma, dphi, phi) on the samples as the detector saw them.
      - The last sample the frame consumes is that of header symbol 230, or that of the last payload symbol when the header is
        valid (ref_sync's n(c): start + 616 resp. start + 2 (308 + npay) for tau > 0, one sample less for tau <= 0, the
        equaliser's 3 symbols on top).  A valid header with zero payload symbols delivers at once, at header symbol 230.
      - The sample after it is the first one of a fresh detector, again with 256 zeros of history: whatever lies in front of
        it reads as zero, in the hops and in a frame whose aligned window reaches back there.
      - A frame whose last sample lies beyond the capture is `short` and is not delivered; nothing follows it.

    The keyword arguments after `trace` are negative controls (mutations of these rules; their defaults are the definition):
    resume_shift (the fresh detector starts that many samples late), keep_history (the samples in front of it are kept, not
    zeroed), room=False (any lag detects), reject_consumes=False (a rejected header consumes nothing: seeking goes on along the
    old hop grid with the old history), check_protocol=False (the protocol byte is not looked at).
    trace: a list that receives one dict per hop (w, rxy, lag, bin, silent).

    bad: classify(x), or None.  The arithmetic then runs on x with every classified sample replaced by zero, and a decision is
    *touched* when an operation it depends on reads a BAD sample (see above), found by the same index arithmetic:
      - a hop whose 512-sample window holds one detects nothing (its energy or its peak is NaN: rxy > threshold is false);
      - an aligned window that holds one yields NaN timing and gain estimates (the carrier estimates too when it is among the
        window's first 156 samples: _touched_align): tau reads 0 (|tau| < 1 is false), so the frame is on the odd sample
        grid with branch 0, every symbol is NaN, the header is rejected and consumes what a rejected header at tau = 0 does;
        the frame dict carries touched = "align" (start, cfo_bin and rxy are the untouched hop's);
      - a header symbol whose filter span (28 samples; with the equaliser 40, and every training symbol's too) holds one: with a
        pilot among them the pilot sums are NaN, so every data symbol is NaN and the header is rejected (touched = "header");
        with data symbols only the header decoder may still correct them: `uncertain`;
      - a payload symbol whose span holds one: the loop is a recurrence, so every symbol from the first such one on is
        unspecified; the frame is consumed to the length its header names (touched = "payload", touched_from = that symbol).
        A NaN symbol still yields a hard decision (every comparison is false), so the frame's code may correct the touched
        symbols and the check may pass: payload_valid is not forced to 0.  What holds is that a payload delivered as valid
        under a check other than "none" carries the bytes of the zero-replaced run (`payload` here) when that run's check passed.
    A LARGE sample in any of these spans makes the decision `uncertain` instead.  Samples in front of a fresh detector's first
    one read as zero, whatever they hold.  The three keyword arguments after `bad` are negative controls: a touched window may
    detect, a touched header is taken as decoded, the detector resumes right behind the first bad sample of a touched payload.

    A frame dict holds ref_sync.sync's fields and start, cfo_bin, rxy, lag, tau, gamma, dphi, phi, floor (the first sample
    its detector saw), last (the last sample consumed), and for a valid header payload, payload_valid and full (ref_sync.compared_span covers the whole payload)."""
    tb, s = conventions()
    cls = None if bad is None else np.asarray(bad, np.int8)
    x = np.asarray(x, np.complex128) if cls is None else np.where(cls != 0, 0.0, np.asarray(x).astype(np.complex128))
    frames, unc = [], []
    floor, w = 0, -HOP
    xp = _padded(x, 0)
    mk = None if cls is None else _Mask(cls, 0)
    dly = rs.EQ_DELAY if equalizer else 0
    c_hdr, c_pay = rs.PRE_DELAY + rs.PN_LEN + dly, rs.PRE_DELAY + rs.PN_LEN + rs.HDR_SYM + dly
    reach = rs.MF_TAPS - 1 + (rs.EQ_TAPS - 1 if equalizer else 0)      # samples in front of a symbol's own that it reads
    while w + N <= len(x):
        if mk is not None and mk.any(w, w + N - 1, LARGE) and not mk.any(w, w + N - 1):
            unc.append(("large", w, 0.0))
        if mk is not None and mk.any(w, w + N - 1) and not touched_detects:
            if trace is not None:
                trace.append(dict(w=w, touched=True))
            w += HOP
            continue
        h = _hop(xp, w, s, threshold, room, unc, trace)
        if h is None:
            w += HOP
            continue
        start = w + h["lag"]
        if start + N > len(x):
            break
        if mk is not None and mk.any(start, start + N - 1) and not touched_detects:
            n_of = rs.timing(0.0)[2]
            if int(n_of(c_pay - 1)) >= len(x) - start:
                break
            fr = dict(start=start, cfo_bin=h["bin"], rxy=h["rxy"], lag=h["lag"], floor=floor, **_touched_align(xp, mk, start, s, h["bin"]))
            fr.update(pfb_index=0, mf_counter0=1, short=False, header_valid=False, touched="align", last=start + int(n_of(c_pay - 1)))
            frames.append(fr)
            floor = fr["last"] + 1
            xp, mk, w = _padded(x, floor), _Mask(cls, floor), floor - HOP
            continue
        est = rd.align(xp[start + HOP:start + HOP + N], s, h["bin"])
        if rs.near_branch_edge(est["tau"], BRANCH_MARGIN):
            unc.append(("branch", start, est["tau"]))
        args = (xp, start + HOP, est["tau"], est["gamma"], est["dphi"], est["phi"], tb)
        fr = rs.sync(*args, equalizer=equalizer)
        if mk is not None and "hdr" in fr:
            n_of = rs.timing(est["tau"])[2]
            first = c_hdr if not equalizer else rs.PRE_DELAY + dly
            lo, hi = start + int(n_of(first)) - reach, start + int(n_of(c_pay - 1))
            if mk.any(start, hi, LARGE):
                unc.append(("large", start, 1.0))
            if mk.any(lo, hi) and not touched_header_ok:
                pil = [c_hdr + rs.PILOT_SPACING * p for p in range(rs.N_PILOTS)]
                if not (equalizer and mk.any(lo, start + int(n_of(c_hdr - 1)))) and not any(mk.any(start + int(n_of(c)) - reach, start + int(n_of(c))) for c in pil):
                    unc.append(("touched header data", start, 0.0))
                fr = dict(pfb_index=fr["pfb_index"], mf_counter0=fr["mf_counter0"], short=False, header_valid=False, touched="header")
        if not check_protocol and not fr["header_valid"] and "header" in fr:
            keep, rs.PROTOCOL = rs.PROTOCOL, fr["header"][rs.HDR_USER]
            try:
                fr = rs.sync(*args, equalizer=equalizer)
            finally:
                rs.PROTOCOL = keep
        if "header_data" in fr and "touched" not in fr:
            d = fr["header_data"]
            m = float(min(np.abs(d.real).min(), np.abs(d.imag).min()))
            if m <= HEADER_MARGIN:
                unc.append(("header", start, m))
            if soft_header:                                       # the header bytes are ref_header_soft's; this statement goes on where
                dec, ok = RH.decode_soft(R.demap_soft(R.QPSK, d).ravel())      # both decoders agree on the CRC, else it does not apply
                if bool(ok[0]) != bool(R.packet_decode(fr["header_bytes"], rs.HDR_DEC, R.CRC_32, R.FEC_SD72, R.FEC_H84)[1]):
                    unc.append(("soft header", start, 0.0))
                elif not ok[0]:
                    fr["header"] = dec[0].tobytes()
                elif dec[0].tobytes() != fr["header"]:
                    unc.append(("soft header", start, 1.0))
        if fr["short"]:
            break
        fr.update(start=start, cfo_bin=h["bin"], rxy=h["rxy"], lag=h["lag"], floor=floor if not keep_history else 0, **est)
        n_of = rs.timing(est["tau"])[2]
        last_c = rs.PRE_DELAY + rs.PN_LEN + rs.HDR_SYM + (rs.EQ_DELAY if equalizer else 0) - 1
        if fr["header_valid"]:
            last_c += fr["num_symbols"]
            p = fr["props"]
            l1 = R.packet_dims(p["payload_len"], p["check"], p["fec0"], p["fec1"])[2]
            pay, ok = R.packet_decode(R.symbols_to_bytes(p["ms"], fr["labels"], l1), p["payload_len"], p["check"], p["fec0"], p["fec1"])
            fr.update(payload=bytes(pay), payload_valid=int(bool(ok)), full=rs.compared_span(fr) == len(fr["r"]))
            lo, hi = start + int(n_of(c_pay)) - reach, start + int(n_of(last_c))
            if mk is not None and fr["num_symbols"] and mk.any(lo, hi, LARGE):
                unc.append(("large", start, 2.0))
            if mk is not None and fr["num_symbols"] and mk.any(lo, hi):
                p0 = mk.first(lo, hi)
                j0 = min(j for j in range(fr["num_symbols"]) if start + int(n_of(c_pay + j)) >= p0)
                fr.update(touched="payload", touched_from=j0, touched_at=p0, full=False)
        fr["last"] = start + int(n_of(last_c))
        frames.append(fr)
        if not fr["header_valid"] and not reject_consumes:
            w += HOP
            continue
        floor = fr["last"] + 1 + resume_shift
        if touched_payload_resume and fr.get("touched") == "payload":
            floor = fr["touched_at"] + 1
        if not keep_history:
            xp = _padded(x, floor)
            mk = None if cls is None else _Mask(cls, floor)
        w = floor - HOP
    return frames, unc


def detect(x, threshold=0.5, trace=None, overlap=True, bad=None):
    """The detector-only mode: (list of detections dict(pos, cfo_bin, rxy, tau, gamma, dphi, phi), uncertain events).

    Rules: the hops are receive()'s.  After a detection at p (the aligned window [p, p + 512)) the next window is
    [p + 256, p + 768): the second half of the aligned window is the overlap, and the hops continue from there by 256; nothing
    is zeroed.  A detection is reported only when its aligned window lies inside the capture: p + 512 <= len(x).
    overlap=False is a negative control: the next window is [p + 512, p + 1024).
    bad: as in receive().  A touched window detects nothing; a detection whose aligned window is touched is reported at its
    position with touched = True and NaN estimates."""
    _, s = conventions()
    cls = None if bad is None else np.asarray(bad, np.int8)
    x = np.asarray(x, np.complex128) if cls is None else np.where(cls != 0, 0.0, np.asarray(x).astype(np.complex128))
    xp = _padded(x, 0)
    mk = None if cls is None else _Mask(cls, 0)
    out, unc, w = [], [], -HOP
    while w + N <= len(x):
        if mk is not None and mk.any(w, w + N - 1, LARGE) and not mk.any(w, w + N - 1):
            unc.append(("large", w, 0.0))
        if mk is not None and mk.any(w, w + N - 1):
            w += HOP
            continue
        h = _hop(xp, w, s, threshold, True, unc, trace)
        if h is None:
            w += HOP
            continue
        p = w + h["lag"]
        if p + N > len(x):
            break
        if mk is not None and mk.any(p, p + N - 1):
            out.append(dict(pos=p, cfo_bin=h["bin"], rxy=h["rxy"], touched=True, **_touched_align(xp, mk, p, s, h["bin"])))
            w = p + HOP
            continue
        est = rd.align(xp[p + HOP:p + HOP + N], s, h["bin"])
        out.append(dict(pos=p, cfo_bin=h["bin"], rxy=h["rxy"], **est))
        w = p + (HOP if overlap else N)
    return out, unc


# ---------------------------------------------------------------------------------------------------- comparison
def view_oracle(f):
    """an oracle_ffi.Frame as the dict compare() takes"""
    i = f.info
    return dict(start=i["start"], cfo_bin=i["offset"], rxy=i["rxy"], tau=i["tau"], gamma=i["gamma"], dphi=i["dphi"], phi=i["phi"],
                pfb_index=i["pfb_index"], mf_counter0=i["mf_counter0"], pilot_dphi=i["pilot_dphi"], pilot_phi=i["pilot_phi"],
                pilot_gain=i["pilot_gain"], header_valid=f.header_valid, header=f.header20, payload=f.payload, payload_valid=f.payload_valid,
                framesyms=f.framesyms, num_framesyms=len(f.framesyms), evm_sum=i["evm_sum"],
                props=(f.mod_scheme, f.check, f.fec0, f.fec1))


def view_library(g):
    """a result dict of the library (RxContext.results) as the dict compare() takes; it carries no mf_counter0"""
    d = {k: g[k] for k in ("start", "cfo_bin", "rxy", "tau", "gamma", "dphi", "phi", "pfb_index", "pilot_dphi", "pilot_phi", "pilot_gain",
                           "header_valid", "header", "payload", "payload_valid", "num_framesyms", "evm_sum")}
    d["framesyms"] = g["framesyms"] if g["framesyms"] is not None else np.zeros(0, np.complex64)
    d["props"] = (g["mod_scheme"], g["check"], g["fec0"], g["fec1"])
    return d


def compare(ref_frames, got, x, equalizer=False, worst=None, cache=None):
    """The reference's frames (receive(x)[0]) against an implementation's (view_oracle / view_library dicts).  Exactly: frame
    count, start, CFO bin, pfb_index, header_valid, all 20 decoded header bytes, the properties, num_framesyms, and payload bytes
    and validity where ref_sync.compared_span covers the whole payload.  rxy within RXY_MARGIN, the ALIGN estimates within
    ref_detect.PARITY.  Symbols through ref_sync.compare, on ref_sync.sync run from the implementation's own float32 estimates
    (ref_sync's stated input).  Returns a list of failure strings; worst: dict updated with the largest differences seen."""
    tb, _ = conventions()
    bad = []
    worst = {} if worst is None else worst
    if len(ref_frames) != len(got):
        return ["frame count %d vs %d: starts %r vs %r" % (len(ref_frames), len(got), [f["start"] for f in ref_frames], [g["start"] for g in got])]
    for k, (f, g) in enumerate(zip(ref_frames, got)):
        tag = "frame %d at %d: " % (k, f["start"])
        for key in ("start", "cfo_bin", "pfb_index"):
            if f[key] != g[key]:
                bad.append(tag + "%s %d vs %d" % (key, f[key], g[key]))
        if bool(f["header_valid"]) != bool(g["header_valid"]):
            bad.append(tag + "header_valid %d vs %d" % (f["header_valid"], g["header_valid"]))
        if bytes(g["header"]) != f["header"]:
            bad.append(tag + "the 20 header bytes differ: %s vs %s" % (f["header"].hex(), bytes(g["header"]).hex()))
        ok, e = rd.parity_ok(f, g)
        e["rxy_rel"] = abs(f["rxy"] - g["rxy"]) / f["rxy"]
        for key, v in e.items():
            worst[key] = max(worst.get(key, 0.0), v)
        if not ok or e["rxy_rel"] > RXY_MARGIN:
            bad.append(tag + "estimates off: %r" % (e,))
        if bad or not f["header_valid"]:
            continue
        p = f["props"]
        if (p["ms"], p["check"], p["fec0"], p["fec1"]) != tuple(g["props"]) or f["num_symbols"] != g["num_framesyms"] or p["payload_len"] != len(g["payload"]):
            bad.append(tag + "properties %r, %d symbols vs %r, %d symbols, %d bytes" % (p, f["num_symbols"], g["props"], g["num_framesyms"], len(g["payload"])))
            continue
        key = (id(x), f["start"], g["tau"], g["gamma"], g["dphi"], g["phi"], equalizer)
        if cache is None or key not in cache:
            f2 = rs.sync(_padded(x, f["floor"]), f["start"] + HOP, g["tau"], g["gamma"], g["dphi"], g["phi"], tb, equalizer=equalizer)
            if cache is not None:
                cache[key] = f2
        else:
            f2 = cache[key]
        if not f2["header_valid"] or "r" not in f2:
            bad.append(tag + "no valid header from the implementation's estimates")
            continue
        b2, w2, n, cut = rs.compare(f2, g, g["framesyms"], g["header"], full_evm_sum=g["evm_sum"], check_counter="mf_counter0" in g)
        bad += [tag + b for b in b2]
        worst["sym"] = max(worst.get("sym", 0.0), w2["sym"])
        worst["sym_ratio"] = max(worst.get("sym_ratio", 0.0), w2["sym_ratio"])
        if f["full"] and not cut and (f["payload"], f["payload_valid"]) != (bytes(g["payload"]), int(g["payload_valid"])):
            bad.append(tag + "payload bytes / validity differ")
    return bad


def compare_detections(ref, got, worst=None):
    """detect(x)[0] against an implementation's detections (dicts with pos, tau, gamma, dphi, phi and, where it reports them,
    cfo_bin and rxy): positions exactly, estimates within ref_detect.PARITY."""
    worst = {} if worst is None else worst
    if [d["pos"] for d in ref] != [g["pos"] for g in got]:
        return ["detections at %r vs %r" % ([d["pos"] for d in ref], [g["pos"] for g in got])]
    bad = []
    for d, g in zip(ref, got):
        ok, e = rd.parity_ok(d, g)
        if "rxy" in g:
            e["rxy_rel"] = abs(d["rxy"] - g["rxy"]) / d["rxy"]
        for key, v in e.items():
            worst[key] = max(worst.get(key, 0.0), v)
        if not ok or e.get("rxy_rel", 0.0) > RXY_MARGIN or ("cfo_bin" in g and g["cfo_bin"] != d["cfo_bin"]):
            bad.append("detection at %d: %r" % (d["pos"], e))
    return bad


def touched_estimates_off(f, g):
    """the estimates of a touched ALIGN (_touched_align) against an implementation's: list of failure strings"""
    bad = []
    if not (g["tau"] == 0.0 and np.isnan(g["gamma"])):
        bad.append("tau %r, gamma %r of a touched aligned window" % (g["tau"], g["gamma"]))
    for k in ("dphi", "phi"):
        if np.isnan(f[k]) != np.isnan(g[k]) or (not np.isnan(f[k]) and abs(f[k] - g[k]) > rd.PARITY[k]):
            bad.append("%s %r vs %r" % (k, f[k], g[k]))
    return bad


def compare_masked(ref_frames, got, x0, equalizer=False, worst=None, cache=None, counts=None):
    """receive(x, bad=classify(x))[0] against an implementation's frames; x0 is x with its bad samples zeroed.  An untouched frame
    goes through compare() unchanged.  A touched one is held to what the contract leaves specified: start, CFO bin and rxy always;
    branch 0 and a rejected header for touched = "align"; the estimates, the branch and a rejected header for "header"; all of
    the header, the properties, the symbol count, the pilot estimates and the symbols in front of the first touched one (through
    ref_sync.compare, as for an untouched frame), and the zero-replaced run's bytes where the payload is delivered as valid, for "payload".
    counts: dict updated with compared / touched frame counts."""
    worst = {} if worst is None else worst
    counts = {} if counts is None else counts
    if len(ref_frames) != len(got):
        return ["frame count %d vs %d: starts %r vs %r" % (len(ref_frames), len(got), [f["start"] for f in ref_frames], [g["start"] for g in got])]
    bad = []
    for k, (f, g) in enumerate(zip(ref_frames, got)):
        t = f.get("touched")
        counts["touched" if t else "compared"] = counts.get("touched" if t else "compared", 0) + 1
        if not t:
            bad += compare([f], [g], x0, equalizer=equalizer, worst=worst, cache=cache)
            continue
        tag = "frame %d at %d (touched %s): " % (k, f["start"], t)
        for key in ("start", "cfo_bin", "pfb_index"):
            if f[key] != g[key]:
                bad.append(tag + "%s %d vs %d" % (key, f[key], g[key]))
        if abs(f["rxy"] - g["rxy"]) > RXY_MARGIN * f["rxy"]:
            bad.append(tag + "rxy %r vs %r" % (f["rxy"], g["rxy"]))
        if t != "align" and not rd.parity_ok(f, g)[0]:
            bad.append(tag + "estimates off: %r" % (rd.parity_ok(f, g)[1],))
        if t == "align":
            bad += [tag + b for b in touched_estimates_off(f, g)]
        if bool(f["header_valid"]) != bool(g["header_valid"]):
            bad.append(tag + "header_valid %d vs %d" % (f["header_valid"], g["header_valid"]))
        if t != "payload" or bad:
            continue
        p = f["props"]
        if bytes(g["header"]) != f["header"] or (p["ms"], p["check"], p["fec0"], p["fec1"]) != tuple(g["props"]) \
                or f["num_symbols"] != g["num_framesyms"] or p["payload_len"] != len(g["payload"]):
            bad.append(tag + "header bytes / properties / lengths differ")
        # the symbols in front of the first touched one, the pilots and the header bytes are untouched: ref_sync.compare on them
        f2 = rs.sync(_padded(x0, f["floor"]), f["start"] + HOP, g["tau"], g["gamma"], g["dphi"], g["phi"], conventions()[0], equalizer=equalizer)
        if not f2["header_valid"] or "r" not in f2:
            bad.append(tag + "no valid header from the implementation's estimates")
            continue
        m = np.array(f2["margin"], np.float64)
        m[f["touched_from"]:] = 0.0
        syms = np.array(g["framesyms"], np.complex128)
        syms[f["touched_from"]:] = 0.0
        b2, w2, n, _ = rs.compare(dict(f2, margin=m), g, syms, g["header"], check_counter="mf_counter0" in g)
        bad += [tag + b for b in b2]
        if n < min(f["touched_from"], rs.compared_span(f2)):
            bad.append(tag + "only %d of %d untouched symbols compared" % (n, f["touched_from"]))
        worst["sym"] = max(worst.get("sym", 0.0), w2["sym"])
        worst["sym_ratio"] = max(worst.get("sym_ratio", 0.0), w2["sym_ratio"])
        if p["check"] != R.CRC_NONE and g["payload_valid"] and f["payload_valid"] and bytes(g["payload"]) != f["payload"]:
            bad.append(tag + "delivered as valid with other bytes than the zero-replaced run's")
    return bad
