"""The captures of tests/test_ref_threshold.py and tests/test_gpu_threshold.py, as data: three streams on which the detection
threshold decides what is found, run at every threshold of T.

Built the way tests/stream_cases.py builds its own (ref_framegen frames, seeded float64 noise; a case is that module's dict), so
nothing here comes from a product generator.  With the noise at `snr_db` under a frame of amplitude 1, a preamble of amplitude a
alone in its window has rxy near sqrt(s / (1 + s)), s = a^2 10^(snr_db / 10) -- the share of the window's energy that correlates
with the template --, and a window of noise alone peaks between 0.15 and 0.3 over its 24 bins and 512 lags: 0.2 fires on noise
in most hops, 0.3 in a few, 0.45 and above never.

  LADDER   ten short PSK2 r1/2 frames at amplitudes from 0.02 to 2.8 under 12 dB noise: every threshold of T has frames at least
           2 % over it and frames at least 2 % under it, and none nearer (tests/test_ref_threshold.py asserts that on each frame's
           own rxy); 2 % because 0.45 and 0.5 are to decide differently on a frame between them.
  FIELD    three PSK2 r1/2 100-byte frames at 8, 10 and 12 dB with noise-only gaps of some 6000 samples: the low thresholds fire
           all over the gaps, and a walker that starts inside one of the 3300-sample payloads fires there too.
  DENSE    short frames back to back, every third gap 300 to 450 samples of noise: a false detection in such a gap consumes a
           header span (617 samples) that holds the next frame's preamble, and that frame is lost or found displaced.

RUNS names, per capture, the receiver options it also runs with."""
import numpy as np

import ref_decode as R
import stream_cases as SC
from stream_cases import F, length, span

T = (0.2, 0.3, 0.45, 0.5, 0.7, 0.9)
LEAD = 300
MAX_SAMPLES = 60_000


def _case(name, frames, seed, snr_db, tail=700):
    total = max(f["at"] + length(f) for f in frames) + tail
    assert total <= MAX_SAMPLES and all(f["n"] <= 100 for f in frames), (name, total)
    return dict(name=name, frames=frames, seed=seed, snr_db=snr_db, total=total)


def expected_rxy(case, f):
    """the model of the module docstring, for choosing amplitudes; the tests measure"""
    s = f["amp"] ** 2 * 10.0 ** (case["snr_db"] / 10.0)
    return float(np.sqrt(s / (1.0 + s)))


# ---- ladder: amplitudes found by bisection on each frame's own rxy under this capture's noise (ref_detect.seek on the window that
# holds its preamble, the cell of its own lag) for the values LADDER_RXY; tests/test_ref_threshold.py measures them again
LADDER_RXY = (0.18, 0.25, 0.37, 0.475, 0.57, 0.62, 0.78, 0.85, 0.95, 0.99)      # (the first: noise alone, whatever a weak frame adds)
AMPS = (0.02, 0.0962, 0.127, 0.1392, 0.189, 0.2288, 0.2568, 0.4412, 0.953, 2.8316)
fr, at = [], LEAD + 400
for i, a in enumerate(AMPS):
    f = F(at, n=16, mod=R.PSK2, fec0=R.FEC_V27, amp=a, dt=-0.25 if i % 2 else 0.25, pseed=400 + i)
    fr.append(f)
    at += length(f) + 700 + 41 * i
LADDER = _case("ladder of amplitudes", fr, 3101, 12.0)

# ---- noise field
fr, at = [], LEAD + 5000
for i, db in enumerate((8.0, 10.0, 12.0)):
    f = F(at, n=100, mod=R.PSK2, fec0=R.FEC_V27, amp=10.0 ** ((db - 10.0) / 20.0), dt=-0.25 if i % 2 else 0.25, pseed=420 + i)
    fr.append(f)
    at += length(f) + 6000 + 777 * i
FIELD = _case("frames in a field of noise", fr, 3200, 10.0, tail=3000)

# ---- dense
GAPS = (0, 3, 300, 17, 1, 420, 40, 0, 350, 5, 150, 450)
fr, at = [], LEAD
for i in range(30):
    f = F(at, n=4 + i % 5, mod=(R.PSK4, R.PSK8, R.PSK2)[i % 3], dt=-0.25 if i % 2 else 0.25, pseed=440 + i)
    fr.append(f)
    at += length(f) + GAPS[i % len(GAPS)]
DENSE = _case("dense short frames", fr, 3301, 15.0)

CAPTURES = [LADDER, FIELD, DENSE]
SMALLEST = min(CAPTURES, key=lambda c: c["total"])
# the options a capture also runs with (keyword arguments of ref_stream.receive and of RxContext alike)
RUNS = {LADDER["name"]: dict(equalizer=True), DENSE["name"]: dict(soft_header=True)}
assert len(CAPTURES) <= 6 and len({c["name"] for c in CAPTURES}) == len(CAPTURES)


def build(case):
    return SC.build(case)


def five_blocks(total):
    """cuts of a capture into 5 unequal blocks (shares 3 : 1 : 4 : 1 : 5, the odd sample left where it falls)"""
    w = np.cumsum([3, 1, 4, 1, 5])
    return [int(total * v // w[-1]) + k for k, v in enumerate(w[:-1])]
