"""Every Viterbi and Reed-Solomon implementation of the library on the crafted received words of tests/crafted_cases.py:
noise-free frames whose payload symbols carry coded packets corrupted on purpose (single errors and bursts at both ends,
in the flush steps and the pad bits; exact ties on the trellis block edges; non-zero tails; words far from every codeword for
thousands of steps; Reed-Solomon blocks at 16 and 17 errors), through the real path -- walker, plan, matched filter, PLL,
decode.  tests/test_ref_crafted.py has proved, without a GPU, that each case is what its name says, that the numpy
reference and the oracle agree on every packet, and that the oracle receiver delivers every crafted word.

In every configuration (default, wave-per-frame decoder only, clean-frame short cut off, trellis blocks of 128 / 192 / 4096
steps, forced re-traces and fallbacks; each with the one-block-per-lane and with the packed forward pass): every crafted
frame is delivered with a valid header that states the case's properties, its symbols demap to exactly the crafted word -- no
frame is excluded --, and (payload, payload_valid) is ref_decode.packet_decode's of the crafted bytes.  The timing counters
show that the intended path ran.

What a broken kernel looks like here: with the tie rule of vb2_butterfly flipped (equal goes to the predecessor with MSB 1)
every packed variant and the three-blocks-in-flight test fail on about 400 frames -- bursts and ties first --, while
test_gpu_ref_decode.py, whose noise rarely produces an exact tie, still passes."""
import struct

import numpy as np
import pytest

import crafted_cases as CC
import ref_decode as R

pytestmark = pytest.mark.gpu

ENV_KEYS = ("FXRX_BATCH_VITERBI", "FXRX_VB_CLEAN", "FXRX_VB_BLK", "FXRX_VB_DEBUG")
COUNTERS = ("vb_clean", "vb_blocks", "vb_repairs", "vb_fallbacks")
CONFIGS = {"default": {}, "batch0": dict(FXRX_BATCH_VITERBI=0), "clean0": dict(FXRX_VB_CLEAN=0), "blk128": dict(FXRX_VB_BLK=128),
           "blk192": dict(FXRX_VB_BLK=192), "blk4096": dict(FXRX_VB_BLK=4096), "debug1": dict(FXRX_VB_DEBUG=1), "debug2": dict(FXRX_VB_DEBUG=2)}
FLOATS = ("rxy", "tau", "gamma", "dphi", "phi", "pilot_dphi", "pilot_phi", "pilot_gain", "evm_sum")
EXACT = ("start", "cfo_bin", "pfb_index", "header_valid", "header", "payload_valid", "payload", "mod_scheme", "check", "fec0", "fec1", "num_framesyms")


@pytest.fixture(scope="module")
def traffic():
    """(streams' samples, their cases, the reference's (payload, valid) per case, the rate-1/2 words that are clean codewords)"""
    st, ref = CC.streams(), CC.reference()
    xs, cs = [np.asarray(x) for x, _ in st], [c for _, c in st]
    clean = sum(CC.clean_count(c, met) for c, (_, met) in zip(cs, ref))
    return xs, cs, [out for out, _ in ref], clean


def _run(fx, monkeypatch, xs, env, soft=False, depth=1):
    """one block of the streams xs.  depth > 1: through submit / collect with that many blocks allowed in flight -- the host
    then plans the packed forward pass (fx_vbfwd_kernel, two trellis blocks per lane) where a lone small block gets
    fx_vbfwd1_kernel (fx_traffic.h: plan_tail)."""
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    ctx = fx.RxContext(len(xs), want_framesyms=True, soft_decision=soft)
    if depth > 1:
        ctx.set_depth(depth)
        ctx.submit_raw([x.ctypes.data for x in xs], [len(x) for x in xs], False)
        got = ctx.results(ctx.collect_raw())
    else:
        got = ctx.process(xs)
    tm = ctx.timing()
    ctx.close()
    return got, tm


def _delivered(got, s, cs):
    """stream s's frames, one per crafted case, in order: header valid and the case's, symbols demapping to the crafted word"""
    mine = [g for g in got if g["stream"] == s]
    assert len(mine) == len(cs), ("stream %d (%s): %d frames for %d cases" % (s, cs[0]["family"], len(mine), len(cs)))
    lay, _ = CC.layout(cs)
    for g, (off, c) in zip(mine, lay):
        assert g["header_valid"], c["name"]
        assert (g["mod_scheme"], g["check"], g["fec0"], g["fec1"], len(g["payload"])) == (c["mod"], c["check"], c["fec0"], c["fec1"], c["n"]), c["name"]
        assert abs(g["start"] - off) <= 64, (c["name"], g["start"], off)
        lab, _ = R.demap_hard(c["mod"], g["framesyms"])
        assert np.array_equal(lab, CC.crafted_labels(c)), "symbols do not demap to the crafted word: %s" % c["name"]
    return mine


def _check_hard(got, cs_all, ref_all):
    bad = []
    for s, (cs, ref) in enumerate(zip(cs_all, ref_all)):
        for g, c, want in zip(_delivered(got, s, cs), cs, ref):
            if (g["payload"], g["payload_valid"]) != want:
                bad.append((c["name"], g["payload_valid"], want[1]))
    assert not bad, "%d payloads differ from the reference (case, gpu valid, reference valid): %s" % (len(bad), bad[:12])


@pytest.fixture(scope="module")
def default_run(fx, traffic):
    mp = pytest.MonkeyPatch()
    got, tm = _run(fx, mp, traffic[0], {})
    mp.undo()
    return got, tm


@pytest.mark.parametrize("cfg,fwd", [(c, "lane") for c in CONFIGS] + [(c, "packed") for c in CONFIGS if c != "batch0"])
def test_crafted_words_every_decode_path(fx, monkeypatch, traffic, default_run, cfg, fwd):
    """fwd: the forward pass with one trellis block per lane (a lone block) or two, packed in 16-bit halves (depth 2)"""
    xs, cs, ref, n_clean = traffic
    got, tm = default_run if (cfg, fwd) == ("default", "lane") else _run(fx, monkeypatch, xs, CONFIGS[cfg], depth=2 if fwd == "packed" else 1)
    print("\n%s, %s: %d frames, %s" % (cfg, fwd, len(got), {k: tm[k] for k in COUNTERS}))
    _check_hard(got, cs, ref)
    if cfg == "batch0":
        assert tm["vb_blocks"] == 0 and tm["vb_clean"] == 0 and tm["vb_repairs"] + tm["vb_fallbacks"] == 0
        return
    assert tm["vb_blocks"] > 0
    assert tm["vb_clean"] == (0 if cfg == "clean0" else n_clean), (tm["vb_clean"], n_clean)
    assert tm["vb_repairs"] + tm["vb_fallbacks"] > 0, "no hand-over check failed on the tie and garbage words"
    if cfg == "debug2":
        assert tm["vb_fallbacks"] > 0


def test_tie_and_garbage_words_fail_hand_overs(fx, monkeypatch, traffic):
    """the tie and the garbage streams alone, default configuration: blocks are run again or frames handed back (words far from
    every codeword do not let a warm-up arrive at the true metric differences), and the results are still the reference's"""
    xs, cs, ref, _ = traffic
    pick = [CC.stream_of("tie"), CC.stream_of("garbage")]
    got, tm = _run(fx, monkeypatch, [xs[i] for i in pick], {})
    print("\ntie + garbage:", {k: tm[k] for k in COUNTERS})
    _check_hard(got, [cs[i] for i in pick], [ref[i] for i in pick])
    assert tm["vb_blocks"] > 0 and tm["vb_repairs"] + tm["vb_fallbacks"] > 0


def test_crafted_words_soft_decisions(fx, monkeypatch, traffic):
    """soft_decision=True on the same traffic: payload and validity are ref_decode.packet_decode_soft's on the frame's own
    soft_bits (the soft instance runs the wave-per-frame decoder)"""
    xs, cs_all, _, _ = traffic
    got, tm = _run(fx, monkeypatch, xs, {}, soft=True)
    bad = []
    for s, cs in enumerate(cs_all):
        mine = _delivered(got, s, cs)
        for g, c in zip(mine, cs):
            assert g["soft_bits"] is not None and len(g["soft_bits"]) == 8 * len(c["pkt"]), c["name"]
        want, _ = CC.decode_batch(cs, [g["soft_bits"] for g in mine], soft=True)
        bad += [(c["name"], g["payload_valid"], w[1]) for g, c, w in zip(mine, cs, want) if (g["payload"], g["payload_valid"]) != w]
    assert not bad, "%d payloads differ from the soft reference: %s" % (len(bad), bad[:12])
    assert tm["vb_blocks"] == 0


def _key(g):
    return tuple(g[k] for k in EXACT) + (struct.pack("<%df" % len(FLOATS), *[g[k] for k in FLOATS]), b"" if g["framesyms"] is None else g["framesyms"].tobytes())


def test_tie_stream_in_segments_three_blocks_in_flight(fx, monkeypatch, traffic, default_run):
    """the tie stream as a continuing stream: segment_len 4096, blocks of 50 000 samples, three in flight -- every field of every
    frame is the one-pass run's, bit for bit, and the payloads are the reference's"""
    xs, cs, ref, _ = traffic
    s = CC.stream_of("tie")
    x = xs[s]
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    ctx = fx.RxContext(1, want_framesyms=True, segment_len=4096)
    ctx.set_depth(3)
    got, keep, inflight = [], [], 0
    for i in range(0, len(x), 50_000):
        if inflight == 3:
            got += ctx.results(ctx.collect_raw()); inflight -= 1
        b = np.ascontiguousarray(x[i:i + 50_000])
        keep.append(b)
        ctx.submit_raw([b.ctypes.data], [len(b)], False); inflight += 1
    while inflight:
        got += ctx.results(ctx.collect_raw()); inflight -= 1
    ctx.close()
    one = [g for g in default_run[0] if g["stream"] == s]
    assert len(got) == len(one) == len(cs[s])
    diff = [c["name"] for a, b, c in zip(one, got, cs[s]) if _key(a) != _key(b)]
    assert not diff, diff[:8]
    _check_hard(got, [cs[s]], [ref[s]])
