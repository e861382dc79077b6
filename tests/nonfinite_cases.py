"""Streams with non-finite and overflowing IQ samples, as data: tests/test_ref_nonfinite.py, tests/test_gpu_ref_nonfinite.py and
the sanitizer driver tests/cpp/oracle_nonfinite.c (through tests/golden/nonfinite_cases.bin, which write_fixture() writes).

A case is a dict: name, layout (key of LAYOUTS: a clean stream of three ref_framegen frames in seeded noise at 20 dB), pos / run
(the bad samples are [pos, pos + run)), value / which (the bad value; which: 1 = the real part only, 2 = the imaginary part only,
3 = both), scale (the whole stream is multiplied by it first; 1.0 but for the two scale cases), eq (run with the equaliser) and
declared (None, or why the case may touch more than one frame / is compared oracle <-> kernels only).

Positions are stated relative to the middle frame B as the clean reference run finds it (start, lag): see _positions()."""
import os
import struct

import numpy as np

import ref_decode as R
import ref_stream as S
import stream_cases as SC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nonfinite_cases.bin")
SNR_DB = 20.0
SEG_CUTS = (4096, 6000, 8192)              # segment cuts of segment_len 4096 and 6000 inside these streams
BLOCK_CUTS = (4096, 8192)                  # the three continuing blocks of the recovery tests

NAN, INF = float("nan"), float("inf")
VALUES = [("nan re", NAN, 1), ("nan im", NAN, 2), ("nan", NAN, 3), ("+inf", INF, 3), ("-inf", -INF, 3), ("+3e38", 3.0e38, 3), ("-3e38", -3.0e38, 3),
          ("2e19", 2e19, 3), ("4e17", 4e17, 3), ("-0.0", -0.0, 3)]


def _frames(ats, mod=R.PSK4, fec0=R.FEC_V27, fec1=R.FEC_NONE, check=R.CRC_24):
    a, b, c = ats
    return [SC.F(a, n=32, fec0=R.FEC_V27, pseed=401), SC.F(b, n=32, mod=mod, fec0=fec0, fec1=fec1, check=check, pseed=402),
            SC.F(c, n=32, fec0=R.FEC_V27, dt=0.25, pseed=403)]


# a frame's payload straddles sample 4096 / 6000 / 8192 in the cut layouts; in "base" every frame has >= 2048 samples of
# silence on either side (a sample in the middle of a gap is >= 1024 from any frame)
LAYOUTS = {
    "base": dict(frames=_frames((1300, 4700, 8100)), total=10496, seed=4100),
    "cut4096": dict(frames=_frames((1100, 3400, 8500)), total=10752, seed=4101),
    "cut6000": dict(frames=_frames((1300, 5300, 8500)), total=10752, seed=4102),
    "cut8192": dict(frames=_frames((1300, 4300, 7500)), total=10496, seed=4103),
    "qam16": dict(frames=_frames((1300, 4700, 8100), mod=R.QAM16, fec0=R.FEC_H128, check=R.CRC_32), total=10496, seed=4104),
    "dpsk4": dict(frames=_frames((1300, 4700, 8100), mod=R.DPSK4), total=10496, seed=4105),
    "ask4": dict(frames=_frames((1300, 4700, 8100), mod=R.ASK4), total=10496, seed=4106),
}
for _l in LAYOUTS.values():
    assert 8192 <= _l["total"] <= 12288 and _l["total"] % 256 == 0

_CLEAN = {}


def clean(layout):
    """(the clean complex64 stream, the reference's frames on it), once per layout"""
    if layout not in _CLEAN:
        l = LAYOUTS[layout]
        x = SC.build(dict(name=layout, frames=l["frames"], seed=l["seed"], snr_db=SNR_DB, total=l["total"]))
        fr, unc = S.receive(x)
        assert not unc and [f["start"] for f in fr] == [f["at"] for f in l["frames"]] and all(f["header_valid"] and f["payload_valid"] for f in fr), layout
        _CLEAN[layout] = (x, fr)
    return _CLEAN[layout]


def _positions(layout):
    """named positions around the middle frame B (tau > 0: header symbol i is read at start + 2 (78 + i), payload symbol j at
    start + 2 (309 + j); a symbol's filter span is the 28 samples that end there)"""
    x, fr = clean(layout)
    b = fr[1]
    st, w = b["start"], b["start"] - b["lag"]
    assert b["tau"] > 0 and 0 < b["lag"] < 356 and b["last"] == st + 2 * (309 + b["num_symbols"] - 1)
    gap = (fr[0]["last"] + 1 + st) // 2
    return {
        "silence": gap,                               # >= 1024 samples from any frame (asserted in the test)
        "before preamble": st - 1,                    # the last sample in front of the preamble
        "window first": w, "window last": w + 511,    # the detecting window's ends
        "aligned only": st + 511,                     # inside the aligned window, outside the detecting one (lag > 0)
        "header pilot": st + 2 * (78 + 208) - 10,     # > 512: in the span of pilot 13 (header symbol 208)
        "payload first": st + 618, "payload middle": st + 618 + 2 * (b["num_symbols"] // 2), "payload last": b["last"],
        "after frame": b["last"] + 1,                 # the fresh detector's first sample
        "capture last": len(x) - 1,
    }


def _case(name, layout, pos, value, which=3, run=1, scale=1.0, eq=False, declared=None):
    return dict(name=name, layout=layout, pos=int(pos), run=run, value=float(value), which=which, scale=scale, eq=eq, declared=declared)


LARGE = "a finite sample under 1.8e19: binary32 overflows in |R|^2 where float64 does not -- oracle <-> kernels only"
CASES = []
_P = _positions("base")
for _k, _p in enumerate(_P):                                                    # every position with a NaN in both parts
    CASES.append(_case("nan at %s" % _p, "base", _P[_p], NAN))
_names = list(_P)
for _i, (_vn, _v, _wh) in enumerate(VALUES):                                    # every value at two positions
    if _vn == "nan":
        continue
    for _p in (_names[(2 * _i + 1) % len(_names)], _names[(2 * _i + 6) % len(_names)]):
        CASES.append(_case("%s at %s" % (_vn, _p), "base", _P[_p], _v, _wh, declared=LARGE if _vn == "4e17" else None))
CASES.append(_case("run of 2 nan at payload middle", "base", _P["payload middle"], NAN, run=2))
CASES.append(_case("run of 2 +inf at window first", "base", _P["window first"], INF, run=2))
CASES.append(_case("run of 300 nan from payload last", "base", _P["payload last"] - 100, NAN, run=300, declared="a 300-sample run"))
CASES.append(_case("run of 300 2e19 before preamble", "base", _P["before preamble"] - 299, 2e19, run=300, declared="a 300-sample run"))
for _l in ("qam16", "dpsk4", "ask4"):                                           # the level / sector conversions on a NaN symbol
    _q = _positions(_l)
    CASES.append(_case("nan at payload middle, %s" % _l, _l, _q["payload middle"], NAN))
    CASES.append(_case("-inf at payload first, %s" % _l, _l, _q["payload first"], -INF))
for _cut in SEG_CUTS:                                                           # on a segment / block cut: its last and its first sample
    CASES.append(_case("nan at %d" % (_cut - 1), "cut%d" % _cut, _cut - 1, NAN))
    CASES.append(_case("+inf at %d" % _cut, "cut%d" % _cut, _cut, INF))
CASES.append(_case("equaliser: nan at aligned only", "base", _P["aligned only"], NAN, eq=True, declared="equaliser"))
CASES.append(_case("equaliser: nan at payload middle", "base", _P["payload middle"], NAN, eq=True, declared="equaliser"))
SCALE = "whole-stream scale: the silence rule is not decided in float64 -- oracle <-> kernels only"
CASES.append(_case("scale 1e-20", "base", 0, 0.0, run=0, scale=1e-20, declared=SCALE))
CASES.append(_case("scale 1e-23", "base", 0, 0.0, run=0, scale=1e-23, declared=SCALE))
assert len({c["name"] for c in CASES}) == len(CASES)
BY_NAME = {c["name"]: c for c in CASES}
CUT_CASES = [c for c in CASES if c["layout"].startswith("cut")]


def build(case):
    """the complex64 stream of a case"""
    x = (clean(case["layout"])[0] * np.float32(case["scale"])).astype(np.complex64)
    v = x.view(np.float32).reshape(-1, 2)
    sl = slice(case["pos"], case["pos"] + case["run"])
    if case["which"] & 1:
        v[sl, 0] = np.float32(case["value"])
    if case["which"] & 2:
        v[sl, 1] = np.float32(case["value"])
    return x


def zeroed(x):
    """x with every bad sample (ref_stream.classify != 0) replaced by zero"""
    y = x.copy()
    y[S.classify(x) != 0] = 0
    return y


def fixture_bytes():
    """the layouts' clean streams and the cases' patches: what tests/cpp/oracle_nonfinite.c reads (little endian: 'FXNF',
    number of layouts, per layout n and n complex64; number of cases, per case layout, pos, run, which, eq, value, scale)"""
    keys = list(LAYOUTS)
    out = [b"FXNF", struct.pack("<I", len(keys))]
    for k in keys:
        x = clean(k)[0]
        out += [struct.pack("<I", len(x)), x.tobytes()]
    out.append(struct.pack("<I", len(CASES)))
    for c in CASES:
        out.append(struct.pack("<IIIIIff", keys.index(c["layout"]), c["pos"], c["run"], c["which"], int(c["eq"]), c["value"], c["scale"]))
    return b"".join(out)


def write_fixture():
    with open(GOLDEN, "wb") as f:
        f.write(fixture_bytes())


if __name__ == "__main__":
    write_fixture()
    print("%d cases, %d bytes" % (len(CASES), os.path.getsize(GOLDEN)))
