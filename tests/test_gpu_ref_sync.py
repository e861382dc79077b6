"""The HIP matched filter, pilot sync, equaliser and payload PLL against tests/ref_sync.py -- a float64 statement that shares
no code with the kernels or the oracle (a mistake common to those two passes every parity test).  `-m gpu`.

Traffic (module scope, built once): frames through the float64 channel of ref_detect, rounded to float32.
  shapes    every modulation; every payload symbol count in 0..10 that the (modulation, length) menu reaches (0 2 3 4 5 6 7 8 10: 1 and 9 are not on it), the
            reachable counts around the 1024-symbol tile of fx_paymf_kernel / fx_paymf4_kernel with count mod 4 = 0..3
            (1021 1022 1023 1024 1026 1027 1028) and three frames above 2048; at 20 dB and at 10 dB
  branches  32 short frames at delays (b + 1/2) / 32 - 1/2: all 32 branches, both signs of tau; gains 1e-6 and 1e8
  coded     a synth_stream of rate-1/2 frames at 20 dB: the clean-frame short cut (FXRX_VB_CLEAN default / 0)
Option sets: equaliser off and on (both instances of the walker and of the payload filter); blocks in flight (a ganged
run, confirmed by fxrx_debug_gang_stats, and two blocks of one continuing stream with a frame across the cut).
Every header-valid frame is compared as in tests/test_ref_sync.py: branch, pilot estimates, header, framesyms and evm_sum
within ref_sync's derived bounds, hard labels (framesyms demapped by ref_decode against the reference's, and the
reference's labels decoded against the payload bytes), up to the first symbol within the tie margin.  mf_counter0 is not
compared: the library's result record does not carry it.  Both symbol grids are covered through the sign of tau (asserted),
and a frame read on the wrong grid is half a symbol off, which the symbol bound cannot miss."""
import collections

import numpy as np
import pytest

import ref_decode as R
import ref_detect as rd
import ref_sync as rs
from parity_util import oracle_frames
from sync_cases import BIN, SHAPES, SMALL_COUNTS, TILE_COUNTS, USER_HEADER, props

pytestmark = pytest.mark.gpu

PRE, GAP = 400, 700


def _lay(fx, frames, snr, seed):
    """frames: (ms, check, payload, d, gain, cfo, phase); each through its own channel segment, laid back to back"""
    rng = np.random.default_rng(seed)
    parts = []
    for ms, chk, pl, d, gain, cfo, ph in frames:
        g = fx.FrameGen(ms, 1, 1, chk)
        fr = g.frame(pl, header=np.frombuffer(USER_HEADER, np.uint8)).astype(np.complex128)
        g.close()
        parts.append(rd.channel(fr, PRE, d, gain, cfo, ph, snr, rng, PRE + len(fr) + GAP))
    return np.concatenate(parts).astype(np.complex64)


def _shape_stream(fx, snr, seed):
    frames = []
    for i, (ms, count) in enumerate(SHAPES):
        chk, n = props(ms, count, i)
        pl = np.random.default_rng(300 + i).integers(0, 256, n, dtype=np.uint8)
        frames.append((ms, chk, pl, (i * 0.137) % 1.0 - 0.5, [1.0, 3.0, 0.02][i % 3], ((i * 5) % 31 - 15 + 0.25 * (i % 4)) * BIN, 0.9 * i))
    return _lay(fx, frames, snr, seed)


def _branch_stream(fx, gain, seed):
    pl = np.random.default_rng(seed).integers(0, 256, 48, dtype=np.uint8)
    return _lay(fx, [(R.PSK4, R.CRC_24, pl, (j + 0.5) / 32.0 - 0.5, gain, ((j * 3) % 17 - 8.25) * BIN, 0.4 * j) for j in range(32)], 20.0, seed)


@pytest.fixture(scope="module")
def tb(oracle):
    return rs.Tables.from_oracle(oracle)


@pytest.fixture(scope="module")
def traffic(fx):
    xs = dict(shapes20=_shape_stream(fx, 20.0, 1), shapes10=_shape_stream(fx, 10.0, 2), gain_lo=_branch_stream(fx, 1e-6, 3),
              gain_hi=_branch_stream(fx, 1e8, 4), coded=fx.synth_stream(100_000, stream_id=4400, snr_db=20.0)[0])
    assert all(len(x) <= 200_000 for x in xs.values()), {k: len(x) for k, x in xs.items()}
    return xs


class Checker:
    """ref_sync on every header-valid frame; references cached per (stream, start, estimates, equaliser)"""

    def __init__(self, tb):
        self.tb, self.cache = tb, {}
        self.worst = collections.defaultdict(float)
        self.frames = collections.Counter()
        self.cut = collections.Counter()
        self.full = collections.Counter()
        self.edge = 0
        self.pfb = collections.Counter()

    def frame(self, name, x, g, eq):
        key = (name, g["start"], g["tau"], g["gamma"], g["dphi"], g["phi"], eq)
        if key not in self.cache:
            self.cache[key] = rs.sync(x, g["start"], g["tau"], g["gamma"], g["dphi"], g["phi"], self.tb, equalizer=eq)
        ref = self.cache[key]
        assert ref["header_valid"] and "r" in ref, (name, g["start"], "the reference finds no valid header where the GPU does")
        near = rs.near_branch_edge(g["tau"])
        bad, w, n, cut = rs.compare(ref, g, g["framesyms"] if g["framesyms"] is not None else np.zeros(0, np.complex64),
                                    g["header"][:14], full_evm_sum=g["evm_sum"], check_branch=not near,
                                    check_counter=False)        # the result record carries pfb_index but no mf_counter0
        p = ref["props"]
        assert (p["ms"], p["check"], p["fec0"], p["fec1"], p["payload_len"]) == (g["mod_scheme"], g["check"], g["fec0"], g["fec1"], len(g["payload"]))
        if not cut and not bad:
            l1 = R.packet_dims(p["payload_len"], p["check"], p["fec0"], p["fec1"])[2]
            if "decoded" not in ref:
                ref["decoded"] = R.packet_decode(R.symbols_to_bytes(p["ms"], ref["labels"], l1), p["payload_len"], p["check"], p["fec0"], p["fec1"])
            if ref["decoded"] != (g["payload"], g["payload_valid"]):
                bad.append("hard labels differ (payload bytes / validity)")
        assert not bad, (name, g["start"], eq, bad)
        self.frames[name] += 1
        self.cut[name] += int(cut)
        self.full[name] += int(not cut)
        self.edge += int(near)
        self.pfb[(g["pfb_index"], g["tau"] > 0)] += 1
        for k, v in w.items():
            self.worst[k] = max(self.worst[k], v)
        return ref

    def stream(self, name, x, got, eq):
        n = 0
        for g in got:
            if g["header_valid"]:
                self.frame(name, x, g, eq)
                n += 1
        return n

    def caps(self):
        total, cut = sum(self.frames.values()), sum(self.cut.values())
        assert cut < 0.02 * total, (cut, total)
        assert all(self.full[k] >= 1 for k in self.frames), dict(self.full)

    def report(self, what):
        w = self.worst
        print("\n%s: %d frames, %d cut short by a tie, %d at a branch edge; worst sym %.3g (bound %.3g), pilot dphi %.3g (%.3g), phi %.3g (%.3g), "
              "gain_rel %.3g (%.3g), evm_sum %.3g (its bound %.3g)" % (what, sum(self.frames.values()), sum(self.cut.values()), self.edge, w["sym"], rs.SYM_TOL,
                                                                       w["dphi"], rs.PILOT["dphi"], w["phi"], rs.PILOT["phi"], w["gain_rel"], rs.PILOT["gain_rel"], w["evm"], w["evm_bound"]))


def _process(fx, xs, **kw):
    ctx = fx.RxContext(len(xs), want_framesyms=True, **kw)
    got = ctx.process(xs)
    tm = ctx.timing()
    ctx.close()
    return got, tm


def _bit_equal(oracle, x, mine, eq):
    of = [f for f in oracle_frames(oracle, x, equalizer=eq) if f.header_valid]
    gv = [g for g in mine if g["header_valid"]]
    return len(of) == len(gv) and all(np.array_equal(a.framesyms.view(np.uint32), b["framesyms"].view(np.uint32)) if len(a.framesyms) else b["num_framesyms"] == 0
                                      for a, b in zip(of, gv))


@pytest.mark.parametrize("eq", [False, True], ids=["plain", "equalizer"])
def test_symbols_against_the_reference(fx, oracle, tb, traffic, eq):
    """tile edges and tails, all branches with both symbol grids, the gain range -- with and without the equaliser"""
    names = ["shapes20", "shapes10", "gain_lo", "gain_hi"]
    got, _ = _process(fx, [traffic[k] for k in names], equalizer=eq)
    ck = Checker(tb)
    counts = collections.Counter()
    for s, name in enumerate(names):
        mine = [g for g in got if g["stream"] == s]
        n = ck.stream(name, traffic[name], mine, eq)
        assert n >= (len(SHAPES) - 3 if name.startswith("shapes") else 30), (name, n)
        for g in mine:
            if g["header_valid"] and name.startswith("shapes"):
                counts[g["num_framesyms"]] += 1
        print("%s: GPU framesyms bit-equal to the oracle's: %s" % (name, _bit_equal(oracle, traffic[name], mine, eq)))
    ck.report("reference vs GPU, equaliser %s" % ("on" if eq else "off"))
    ck.caps()
    assert SMALL_COUNTS | TILE_COUNTS | {2050, 2056} <= set(counts), sorted(counts)
    assert {b for b, _ in ck.pfb} == set(range(32)) and {pos for _, pos in ck.pfb} == {True, False}
    assert 4.0 * ck.worst["sym"] <= rs.SYM_TOL and 4.0 * ck.worst["sym_ratio"] <= 1.0 and all(4.0 * ck.worst[k] <= rs.PILOT[k] for k in rs.PILOT), dict(ck.worst)
    m = rs.MEASURED["gpu"][eq]                      # the recorded figures are this run's, rounded up: they cannot drift
    assert all(0.5 * m[k] <= ck.worst[k] <= m[k] for k in m), ("ref_sync.MEASURED['gpu'] is not this run's", {k: ck.worst[k] for k in m})


def test_clean_frame_short_cut(fx, oracle, tb, traffic, monkeypatch):
    """rate-1/2 frames at 20 dB finish in fx_vbpre_kernel by default and go through the trellis with FXRX_VB_CLEAN=0: the
    same framesyms either way, and the reference's"""
    x = traffic["coded"]
    monkeypatch.delenv("FXRX_VB_CLEAN", raising=False)
    a, tma = _process(fx, [x])
    monkeypatch.setenv("FXRX_VB_CLEAN", "0")
    b, tmb = _process(fx, [x])
    assert tma["vb_clean"] > 0 and tmb["vb_clean"] == 0
    assert len(a) == len(b) >= 4
    ck = Checker(tb)
    for ga, gb in zip(a, b):
        assert ga["start"] == gb["start"] and ga["payload"] == gb["payload"] and ga["evm_sum"] == gb["evm_sum"]
        assert np.array_equal(ga["framesyms"].view(np.uint32), gb["framesyms"].view(np.uint32))
    assert ck.stream("coded", x, a, False) >= 4 and ck.stream("coded", x, b, False) >= 4
    ck.report("clean-frame short cut on / off")
    ck.caps()
    print("GPU framesyms bit-equal to the oracle's: %s" % _bit_equal(oracle, x, a, False))


def test_blocks_in_flight(fx, tb, traffic, monkeypatch):
    """The symbols do not depend on which launch carried them.  Tails of several blocks in one launch: a tail is deferred
    only with at least G blocks in flight ahead of it (tests/test_gpu_tail_gang.py), so FXRX_TAIL_GANG=4 gangs from depth 8 on
    and forms nothing at depth 4, where the setting 2 gives pairs: depth 8 with 4 and depth 4 with 2 are run, and the counter
    must show a launch of 4 resp. 2 members.  Then two
    blocks of one continuing stream with the 2056-symbol frame across the cut: the reference sees only the whole capture."""
    names = ["shapes20", "gain_lo", "coded", "shapes10", "gain_hi"]
    ck = Checker(tb)
    for depth, want in ((8, 4), (4, 2)):
        monkeypatch.setenv("FXRX_TAIL_GANG", str(want))
        order = [names[i % len(names)] for i in range(13)]
        ctx = fx.RxContext(1, want_framesyms=True)
        ctx.set_depth(depth)
        res, inflight, sizes, last = [], 0, [], (0, 0)

        def seen():
            nonlocal last
            st = ctx.gang_stats()
            if st[0] != last[0]:
                sizes.append(st[1] - last[1])
            last = st
        for k in order:                                 # the bench's pattern: reset in front of every submit
            if inflight == depth:
                res.append(ctx.results(ctx.collect_raw())); inflight -= 1; seen()
            ctx.reset()
            ctx.submit_raw([traffic[k].ctypes.data], [len(traffic[k])], False); inflight += 1; seen()
        while inflight:
            res.append(ctx.results(ctx.collect_raw())); inflight -= 1; seen()
        ctx.close()
        print("depth %d, FXRX_TAIL_GANG=%d: ganged launches of %r blocks" % (depth, want, sizes))
        assert want in sizes and max(sizes) <= want, (depth, sizes)
        assert len(res) == len(order)
        for k, got in zip(order, res):
            assert ck.stream(k, traffic[k], got, False) >= 4, k
    monkeypatch.delenv("FXRX_TAIL_GANG", raising=False)
    # a continuing stream cut inside its longest frame
    x = traffic["shapes20"]
    whole, _ = _process(fx, [x])
    long_ = max((g for g in whole if g["header_valid"]), key=lambda g: g["num_framesyms"])
    assert long_["num_framesyms"] > 2048
    cut = long_["start"] + 2 * (309 + 1024) + 7
    parts = [np.ascontiguousarray(x[:cut]), np.ascontiguousarray(x[cut:])]
    ctx = fx.RxContext(1, want_framesyms=True)
    ctx.set_depth(2)
    for p in parts:
        ctx.submit_raw([p.ctypes.data], [len(p)], False)
    got = ctx.results(ctx.collect_raw()) + ctx.results(ctx.collect_raw())
    ctx.close()
    assert [g["start"] for g in got] == [g["start"] for g in whole]
    for a, b in zip(got, whole):
        if a["header_valid"]:
            assert np.array_equal(a["framesyms"].view(np.uint32), b["framesyms"].view(np.uint32)) if a["num_framesyms"] else True
    assert ck.stream("shapes20", x, got, False) >= len(SHAPES) - 3
    ck.report("blocks in flight")
    ck.caps()
