"""The GPU payload demappers over the whole plane, against the float64 statement of tests/ref_decode.py -- not only against
the oracle, which shares their construction.  modem_demod (fx_device.h, called from fx_paypll_kernel: the hard decision, the
decided point xhat, the phase error) and fx_softdemod_kernel (soft_byte, soft_axis) are driven through the real receive path
by the frames of tests/plane_cases.py, whose payload symbols lie anywhere on the plane, out to 8 times the constellation.
tests/test_ref_plane.py has proved, without a GPU, that the frames are what they say and that reference and oracle agree.

The reference is applied to the device's own carrier-recovered symbols (framesyms): how the loop answers such symbols does not
enter.  All 11 streams go through one context per configuration: hard; soft_decision; both with the equaliser; hard as a
continuing stream in blocks of 4096 samples, three in flight.  Per configuration:
  frames   every crafted frame, header valid and the case's, num_framesyms the case's count
  labels   (hard configurations) the payload bytes, unpacked back to label bits, are ref_decode.demap_hard's at every non-tie
           symbol, symbol by symbol; ties (plane_cases' rule) stay under 0.5 % per scheme.  The soft configurations see the same
           symbols bit for bit (asserted), and their payload is a function of the soft bytes, checked there
  soft     soft_bits within 1 of ref_decode.demap_soft everywhere and equal where the float64 value is more than 0.01 from a
           rounding tie; differential PSK exactly 0 / 255 of the device's own hard label; num_soft_bits = 8 l1, a padded last
           symbol's bits that exist compared like all others; the reference's soft chain on these bytes gives the payload
  evm_sum  the float64 sum of |r - nearest point|^2 over the frame's payload symbols (ref_sync.py: the loop adds one term per
           payload symbol, nothing else), within evm_bound() below
  oracle   framesyms, payload, soft_bits, evm_sum and the estimates are the oracle receiver's, bit for bit

evm_bound, derived.  u = 2^-24.  The kernel computes, per symbol, dr = r.re - xh.re, di = r.im - xh.im and the term
fmaf(dr, dr, di * di), and adds the terms one after the other in float32.
  xhat     a grid point's component is a level (an exact small integer) times a float32 constant: two roundings, 2 u relative;
           a PSK point is exact up to 4-PSK and a sin/cos table entry beyond, each component within u of the true one: in
           both cases |xh - p| <= 2 u |p|.  The term |r - p|^2 = t moves by at most 2 sqrt(t) x 2 u |p|.
  term     dr and di carry u relative each (2 u on their squares), di * di one more rounding, the fused add one more:
           4 u t to first order; 5 u t taken, which covers the second order.
  sum      n terms of one sign added in sequence: each of the n - 1 additions rounds a partial sum <= S: (n - 1) u S.
  ties     where the margin is below the tie margin m the kernel may decide the runner-up, d + m' away (m' < m) instead of d:
           the term moves by m' (2 d + m') <= 2 m d + m^2 -- twice the tie margin times the distance to the point.
evm_bound = sum_j (4 u |p_j| sqrt(t_j) + 5 u t_j) + (n - 1) u S (1 + 5 u) + sum_ties (2 m d_j + m^2).  Not tuned: a frame that
misses it is a finding about xhat.  The worst ratio measured is printed (and recorded in plane_cases.MEASURED_EVM_RATIO).

The guard `q < nbits` of fx_softdemod_kernel keeps a padded last symbol's absent bits from being written behind the frame's soft
values.  The byte behind them lies in the slack every frame has in the byte arenas (fx_common.h: stride >= l1 + 8) and is
nobody's: it holds what was there before.  test_nothing_is_written_behind_the_soft_values runs plane_cases.guard_streams
"a a b b a a" through one context: a kernel that writes the first absent bit there leaves its soft value in every run; a kernel
that does not leaves a byte that cannot follow the variants, whichever buffer a run gets."""
import ctypes as C
import struct

import numpy as np
import pytest

import plane_cases as PC
import ref_decode as R
from parity_util import oracle_frames

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
BLOCK = 4096
CONFIGS = {"hard": {}, "soft": dict(soft_decision=True), "hard_eq": dict(equalizer=True), "soft_eq": dict(soft_decision=True, equalizer=True)}
FLOATS = ("rxy", "tau", "gamma", "dphi", "phi", "pilot_dphi", "pilot_phi", "pilot_gain", "evm_sum")
EXACT = ("stream", "start", "cfo_bin", "pfb_index", "header_valid", "header", "payload_valid", "payload", "mod_scheme", "check", "fec0", "fec1", "num_framesyms")


def evm_bound(v):
    """the allowed |evm_sum - float64 sum| of one frame (derivation in the module docstring); v: plane_cases.View"""
    pts = R.constellation(v.ms)[0]
    t, p, n = v.dist ** 2, np.abs(pts[v.index]), len(v.dist)
    m = PC.tie_limit(v.ms)
    ties = v.margin < m
    S = float(t.sum())
    return float((4.0 * U * p * v.dist + 5.0 * U * t).sum()) + max(n - 1, 0) * U * S * (1.0 + 5.0 * U) + float((2.0 * m * v.dist[ties] + m * m).sum()), S


def _by_stream(got):
    return [[g for g in got if g["stream"] == s] for s in range(len(R.PAYLOAD_MODS))]


@pytest.fixture(scope="module")
def traffic():
    st = PC.streams()
    return [np.asarray(x) for x, _ in st], [cs for _, cs in st]


@pytest.fixture(scope="module")
def runs(fx, traffic):
    """configuration -> the frames of one process() call on all 11 streams, computed once"""
    done = {}

    def run(name):
        if name not in done:
            ctx = fx.RxContext(len(traffic[0]), want_framesyms=True, segment_len=BLOCK, **CONFIGS[name])
            done[name] = ctx.process(traffic[0])
            ctx.close()
        return done[name]
    return run


@pytest.fixture(scope="module")
def oracle_runs(oracle, traffic):
    done = {}

    def run(name):
        kw = CONFIGS[name]
        if name not in done:
            done[name] = [oracle_frames(oracle, x, soft=bool(kw.get("soft_decision")), equalizer=bool(kw.get("equalizer"))) for x in traffic[0]]
        return done[name]
    return run


def _frames(got, cs_all):
    """per stream the frames, one per case in order, header valid and the case's; with the reference's view of each"""
    out = []
    for s, (mine, cs) in enumerate(zip(_by_stream(got), cs_all)):
        assert len(mine) == len(cs), "scheme %d: %d frames for %d cases" % (cs[0]["mod"], len(mine), len(cs))
        for g, (off, c) in zip(mine, PC.layout(cs)[0]):
            assert g["header_valid"], c["name"]
            assert (g["mod_scheme"], g["check"], g["fec0"], g["fec1"], len(g["payload"]), g["num_framesyms"]) == (c["mod"], c["check"], c["fec0"], c["fec1"], c["n"], c["nsym"]), c["name"]
            assert abs(g["start"] - off) <= 64, (c["name"], g["start"], off)
            assert g["framesyms"] is not None and len(g["framesyms"]) == c["nsym"] and np.isfinite(g["framesyms"]).all(), c["name"]
        out.append([(g, c, PC.View(c, g["framesyms"])) for g, c in zip(mine, cs)])
    return out


def _check_labels(frames, report):
    for per in frames:
        ms = per[0][1]["mod"]
        ties = total = 0
        for g, c, v in per:
            gb, ex = PC.payload_label_bits(ms, g["payload"], c["n"])
            bad = np.nonzero(((gb != v.bits) & ex & ~v.tie[:, None]).any(axis=1))[0]
            assert not len(bad), "%s: %d labels differ from the reference, first at symbol %d, r = %s: device bits %s, reference %s (bits that exist: %s)" % (
                c["name"], len(bad), bad[0], v.syms[bad[0]], gb[bad[0]], v.bits[bad[0]], ex[bad[0]])
            assert g["payload_valid"] == 1 and (g["payload"], 1) == v.payload_of(np.where(ex, v.labels_with(gb), 0)), c["name"]
            ties, total = ties + int(v.tie.sum()), total + len(v.r)
        assert ties <= PC.TIE_CAP * total, (ms, ties, total)
        report[ms].update(symbols=total, ties=ties, rmin=min(float(np.abs(v.r).min()) for _, _, v in per), rmax=max(float(np.abs(v.r).max()) for _, _, v in per))


def _check_evm(frames, report):
    worst = 0.0
    for per in frames:
        ms = per[0][1]["mod"]
        ratio = 0.0
        for g, c, v in per:
            bound, S = evm_bound(v)
            err = abs(float(g["evm_sum"]) - S)
            assert err <= bound, "%s: evm_sum %.9g, float64 sum of |r - nearest point|^2 %.9g: off by %.3g, bound %.3g" % (c["name"], g["evm_sum"], S, err, bound)
            ratio = max(ratio, err / bound)
        report[ms]["evm_ratio"] = ratio
        worst = max(worst, ratio)
    return worst


def _check_soft(frames, hard_frames, report):
    for per, per_hard in zip(frames, hard_frames):
        ms, k = per[0][1]["mod"], R.bps(per[0][1]["mod"])
        off = 0
        for (g, c, v), (gh, _, _) in zip(per, per_hard):
            n = c["n"]
            assert np.array_equal(g["framesyms"].view(np.uint32), gh["framesyms"].view(np.uint32)), "%s: the soft run's symbols are not the hard run's" % c["name"]
            sb = g["soft_bits"]
            assert sb is not None and len(sb) == 8 * n, (c["name"], None if sb is None else len(sb))
            hb, ex = PC.payload_label_bits(ms, gh["payload"], n)               # the device's own hard label bits
            want, exact = v.soft(np.where(ex, hb, v.bits))
            want, exact = want.ravel()[:8 * n].astype(int), exact.ravel()[:8 * n]
            d = np.abs(sb.astype(int) - want)
            i = int(d.argmax())
            msg = "%s: soft value %d (symbol %d, bit %d, r = %s): device %d, reference %d" % (c["name"], i, i // k, i % k, v.syms[i // k], sb[i], want[i])
            if ms in R.DPSK:
                assert not d.any(), msg
            else:
                assert d.max() <= 1, msg
                j = np.nonzero((d != 0) & exact)[0]
                assert not len(j), "%s: soft value %d (symbol %d, r = %s) is off by one away from a rounding tie: device %d, reference %d" % (
                    c["name"], j[0], j[0] // k, v.syms[j[0] // k], sb[j[0]], want[j[0]])
            if c["padded"]:                                                     # the last symbol's bits that exist, named on their own
                first = k * (c["nsym"] - 1)
                assert 0 < 8 * n - first < k and d[first:].max() <= (0 if ms in R.DPSK else 1), (c["name"], sb[first:], want[first:])
            off += int((d == 1).sum())
            assert (g["payload"], g["payload_valid"]) == v.soft_decode(sb), "%s: the reference's soft chain on the device's soft bytes gives another payload" % c["name"]
        report[ms]["soft_off_by_one"] = off


def _check_oracle(frames, of_all, soft):
    for per, of in zip(frames, of_all):
        assert len(of) == len(per)
        for (g, c, v), f in zip(per, of):
            i = f.info
            assert (f.header_valid, i["start"], i["offset"], i["pfb_index"], f.header20) == (g["header_valid"], g["start"], g["cfo_bin"], g["pfb_index"], g["header"]), c["name"]
            assert np.array_equal(f.framesyms.view(np.uint32), g["framesyms"].view(np.uint32)), "%s: framesyms are not the oracle's" % c["name"]
            assert (f.payload, f.payload_valid) == (g["payload"], g["payload_valid"]), c["name"]
            assert struct.pack("<f", i["evm_sum"]) == struct.pack("<f", g["evm_sum"]), (c["name"], i["evm_sum"], g["evm_sum"])
            for key in ("rxy", "tau", "gamma", "dphi", "phi", "pilot_dphi", "pilot_phi", "pilot_gain"):
                assert struct.pack("<f", i[key]) == struct.pack("<f", g[key]), (c["name"], key, i[key], g[key])
            if soft:
                assert np.array_equal(f.soft, g["soft_bits"]), "%s: soft_bits are not the oracle's" % c["name"]


def _print(name, report, worst):
    print("\n%s: worst |evm_sum - float64 sum| / bound %.3f" % (name, worst))
    for ms in R.PAYLOAD_MODS:
        r = report[ms]
        print("  scheme %2d: %s" % (ms, ", ".join("%s %s" % (k, ("%.4g" % x) if isinstance(x, float) else x) for k, x in r.items())))


@pytest.mark.parametrize("name", list(CONFIGS))
def test_demappers_over_the_plane(runs, oracle_runs, traffic, name):
    soft = "soft_decision" in CONFIGS[name]
    frames = _frames(runs(name), traffic[1])
    report = {ms: {} for ms in R.PAYLOAD_MODS}
    if soft:
        _check_labels(_frames(runs(name.replace("soft", "hard")), traffic[1]), report)       # (the same symbols: _check_soft asserts it)
        _check_soft(frames, _frames(runs(name.replace("soft", "hard")), traffic[1]), report)
    else:
        _check_labels(frames, report)
    worst = _check_evm(frames, report)
    _print(name, report, worst)
    _check_oracle(frames, oracle_runs(name), soft)


def _key(g):
    return tuple(g[k] for k in EXACT) + (struct.pack("<%df" % len(FLOATS), *[g[k] for k in FLOATS]), g["framesyms"].tobytes())


def test_continuing_stream_three_blocks_in_flight(fx, runs, traffic):
    """the same streams in blocks of 4096 samples, three in flight: the demapper across block cuts and through the loop's fetch of
    raw symbols ahead.  Every field of every frame is the one-pass run's, bit for bit, and judged against the reference again."""
    xs, cs_all = traffic
    ctx = fx.RxContext(len(xs), want_framesyms=True, segment_len=BLOCK)
    ctx.set_depth(3)
    got, keep, inflight = [], [], 0
    for i in range(0, len(xs[0]), BLOCK):
        if inflight == 3:
            got += ctx.results(ctx.collect_raw()); inflight -= 1
        bs = [np.ascontiguousarray(x[i:i + BLOCK]) for x in xs]
        keep.append(bs)
        ctx.submit_raw([b.ctypes.data for b in bs], [len(b) for b in bs], False); inflight += 1
    while inflight:
        got += ctx.results(ctx.collect_raw()); inflight -= 1
    ctx.close()
    order = lambda fr: sorted(fr, key=lambda g: (g["stream"], g["start"]))
    got, one = order(got), order(runs("hard"))
    assert len(got) == len(one) == 33
    diff = [(a["stream"], a["start"]) for a, b in zip(one, got) if _key(a) != _key(b)]
    assert not diff, diff[:8]
    frames = _frames(got, cs_all)
    report = {ms: {} for ms in R.PAYLOAD_MODS}
    _check_labels(frames, report)
    _print("continuing", report, _check_evm(frames, report))


def test_nothing_is_written_behind_the_soft_values(fx):
    """see the module docstring.  Per run and frame: the byte behind the soft values, read through the result's own pointer, and
    what the first absent bit's soft value would be (the reference's, from the device's symbols)."""
    g = PC.guard_streams()
    ctx = fx.RxContext(len(g["cases"]), want_framesyms=True, soft_decision=True)
    behind, absent = [], []
    for variant in "aabbaa":
        xs = [np.asarray(x) for x in g[variant]]
        keep, ptrs, counts, on_device, fmt = fx.marshal_streams(xs)
        n = ctx.process_raw(ptrs, counts, on_device, fmt)
        assert n == len(xs)
        f = fx._ffi.Frame()
        row_b, row_a = [], []
        for i, (c, bit) in enumerate(zip(g["cases"], g["bit"])):
            ctx.L.fxrx_result(ctx.h, i, C.byref(f))
            assert f.header_valid and f.stream == i and f.num_framesyms == c["nsym"] and f.num_soft_bits == 8
            syms = np.frombuffer(C.string_at(C.cast(f.framesyms, C.c_void_p), 8 * f.num_framesyms), np.complex64)
            v = PC.View(c, syms)
            row_a.append(int(v.soft()[0][-1, bit]))
            row_b.append(int(f.soft_bits[8]))
            want = v.soft()[0].ravel()[:8].astype(int)
            assert np.abs(np.frombuffer(C.string_at(f.soft_bits, 8), np.uint8).astype(int) - want).max() <= 1, (c["name"], variant)
        behind.append(row_b)
        absent.append(row_a)
        ctx.reset()
    ctx.close()
    behind, absent = np.array(behind), np.array(absent)
    print("\nbyte behind the soft values, per run (rows) and scheme:\n%s\nsoft value of the first absent bit:\n%s" % (behind, absent))
    assert (np.abs(absent[0] - absent[2]) > 100).all(), "the variants do not differ in the absent bit"
    follows = (np.abs(behind - absent) <= 1).all(axis=0)
    assert not follows.any(), "the byte behind the soft values follows the last symbol's absent bit for schemes %s" % [c["mod"] for c, w in zip(g["cases"], follows) if w]
