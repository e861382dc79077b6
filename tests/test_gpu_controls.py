"""The controls of a receive context that move no sample themselves (include/fxrx.h): fxrx_set_depth and the "pipeline full"
refusal, fxrx_ready and fxrx_inflight, fxrx_reset with blocks in flight, the timing levels, fxrx_device_framesyms.

One capture throughout: two streams of 40 000 samples, PSK4 r1/2, 100-byte payloads at 15 dB.  Its frames are the oracle's
(parity_util.compare_frames), computed once; runs of the library against each other are compared field for field and bit for
bit (test_gpu_cuts.differences).  The GPU tests are marked one by one: the first test reads the sources only."""
import ctypes as C
import os
import re
import time

import numpy as np
import pytest

import cut_cases as CC
from parity_util import compare_frames, oracle_frames
from test_gpu_cuts import differences

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_DEPTH, STATE_RING = 32, 35          # kMaxDepth and kStateRing = kMaxDepth + 3 of fx_host.cpp: the first test reads them there
ERR_ARG, ERR_STATE = -1, -4
N, N_BLOCKS = 40_000, 80
STAGES = ("walk_ms", "seekverify_ms", "chain_ms", "paymf_ms", "paypll_ms", "paydec_ms")
FEC_NONE = 1


def test_depth_range_in_the_header_is_the_source_s():
    src = open(os.path.join(ROOT, "gr-liquiddsp_amd", "csrc", "fx_host.cpp")).read()
    hdr = open(os.path.join(ROOT, "include", "fxrx.h")).read()
    assert int(re.search(r"constexpr unsigned kMaxDepth = (\d+);", src).group(1)) == MAX_DEPTH
    assert re.search(r"constexpr unsigned kStateRing = kMaxDepth \+ (\d+);", src).group(1) == str(STATE_RING - MAX_DEPTH)
    assert "depth == 0 || depth > kMaxDepth" in src
    assert "fxrx_set_depth, 1..%d," % MAX_DEPTH in hdr and "1..16" not in hdr
    assert N_BLOCKS > 2 * STATE_RING and len(CC.many_blocks(40_000)) + 1 > 2 * STATE_RING


# ---------------------------------------------------------------------------------------------------- the capture
@pytest.fixture(scope="module")
def cap(fx, oracle):
    """(streams, oracle frames per stream, the library's one-pass frames per stream -- held to the oracle here, once)"""
    xs = [fx.synth_stream(N, stream_id=1700 + s, payload_len=100, snr_db=15.0, return_payloads=False) for s in range(2)]
    of = [oracle_frames(oracle, x) for x in xs]
    assert all(len(f) >= 10 and all(g.header_valid and g.payload_valid for g in f) for f in of)
    ctx = fx.RxContext(2, want_framesyms=True)
    got = ctx.process(xs)
    ctx.close()
    one = [[g for g in got if g["stream"] == s] for s in range(2)]
    for s in range(2):
        compare_frames(of[s], one[s])
    return xs, of, one


def cuts_for(s, n=N, blocks=N_BLOCKS):
    c = CC.many_blocks(n, blocks)
    return c if s == 0 else [n - p for p in reversed(c)]         # the second stream's blocks in the reverse order of sizes


def submit(ctx, parts):
    ctx.submit_raw([p.ctypes.data for p in parts], [len(p) for p in parts], False)


def try_submit(fx, ctx, parts):
    """fxrx_submit's own return value (RxContext.submit_raw raises on a negative one)"""
    n = ctx.n_streams
    return fx.lib().fxrx_submit(ctx.h, (C.c_void_p * n)(*[p.ctypes.data for p in parts]), (C.c_uint64 * n)(*[len(p) for p in parts]), 0)


def poll_ready(L, ctx, budget=10.0):
    """fxrx_ready until it says 1: a sleep of 1 ms between calls, a failure after `budget` seconds"""
    end = time.monotonic() + budget
    while True:
        r = L.fxrx_ready(ctx.h)
        if r == 1:
            return
        assert r == 0, "fxrx_ready returned %d: %s" % (r, L.fxrx_last_error().decode())
        assert time.monotonic() < end, "fxrx_ready did not become 1 within %g s" % budget
        time.sleep(0.001)


def by_stream(got, n=2):
    return [[g for g in got if g["stream"] == s] for s in range(n)]


# ---------------------------------------------------------------------------------------------------- depth
@gpu
def test_depth_outside_its_range(fx, cap):
    xs, of, one = cap
    L = fx.lib()
    ctx = fx.RxContext(2, want_framesyms=True)
    assert L.fxrx_set_depth(ctx.h, 0) == ERR_ARG and L.fxrx_set_depth(ctx.h, MAX_DEPTH + 1) == ERR_ARG and L.fxrx_set_depth(None, 1) == ERR_ARG
    submit(ctx, xs)                                              # the depth is still 1
    assert try_submit(fx, ctx, xs) == ERR_STATE and b"pipeline full" in L.fxrx_last_error()
    ctx.collect_raw()
    assert L.fxrx_set_depth(ctx.h, 3) == 0
    assert L.fxrx_set_depth(ctx.h, 0) == ERR_ARG and L.fxrx_set_depth(ctx.h, MAX_DEPTH + 1) == ERR_ARG and L.fxrx_set_depth(ctx.h, 0xFFFFFFFF) == ERR_ARG
    for k in range(3):                                           # the depth is still 3
        ctx.reset()
        submit(ctx, xs)
    assert try_submit(fx, ctx, xs) == ERR_STATE and L.fxrx_inflight(ctx.h) == 3
    for k in range(3):
        got = by_stream(ctx.results(ctx.collect_raw()))
        assert not differences(one[0], got[0]) and not differences(one[1], got[1]), k
    assert L.fxrx_set_depth(ctx.h, MAX_DEPTH) == 0 and L.fxrx_set_depth(ctx.h, 1) == 0
    ctx.close()


@gpu
def test_depth_change_with_a_block_in_flight(fx, cap):
    xs, of, one = cap
    L = fx.lib()
    ctx = fx.RxContext(2, want_framesyms=True)
    ctx.set_depth(2)
    submit(ctx, xs)
    assert L.fxrx_set_depth(ctx.h, 4) == ERR_STATE and L.fxrx_inflight(ctx.h) == 1
    got = by_stream(ctx.results(ctx.collect_raw()))
    for s in range(2):
        compare_frames(of[s], got[s])
        assert not differences(one[s], got[s])
    submit(ctx, xs)                                              # still 2: the third submit is the one refused
    submit(ctx, xs)
    assert try_submit(fx, ctx, xs) == ERR_STATE
    ctx.collect_raw(), ctx.collect_raw()
    ctx.close()


@gpu
@pytest.mark.parametrize("seg", [0, 4096])
def test_80_blocks_at_the_maximum_depth(fx, cap, seg):
    """the capture as one continuing stream pair in 80 unequal blocks, 32 in flight whenever there are 32 left to submit: the
    state ring of 35 entries wraps twice.  Every field equals the one-pass run.  Whenever exactly 32 are in flight one more
    fxrx_submit is tried: FXRX_ERR_STATE, and nothing changes -- the very block is submitted again after the next collect."""
    xs, of, one = cap
    L = fx.lib()
    sizes = [CC.pieces(N, cuts_for(s)) for s in range(2)]
    assert all(len(z) == N_BLOCKS and sum(z) == N for z in sizes) and sizes[0] != sizes[1]
    ctx = fx.RxContext(2, want_framesyms=True, segment_len=seg)
    ctx.set_depth(MAX_DEPTH)
    got, keep, inflight, at, refused, most = [[], []], [], 0, [0, 0], 0, 0
    for k in range(N_BLOCKS):
        parts = [np.ascontiguousarray(x[at[s]:at[s] + sizes[s][k]]) for s, x in enumerate(xs)]
        at = [a + sizes[s][k] for s, a in enumerate(at)]
        keep.append(parts)
        if inflight == MAX_DEPTH:
            assert try_submit(fx, ctx, parts) == ERR_STATE and b"pipeline full" in L.fxrx_last_error()
            assert L.fxrx_inflight(ctx.h) == MAX_DEPTH
            refused += 1
            for g in ctx.results(ctx.collect_raw()):
                got[g["stream"]].append(g)
            inflight -= 1
            assert L.fxrx_inflight(ctx.h) == inflight
        submit(ctx, parts)
        inflight += 1
        most = max(most, inflight)
        assert L.fxrx_inflight(ctx.h) == inflight
    while inflight:
        for g in ctx.results(ctx.collect_raw()):
            got[g["stream"]].append(g)
        inflight -= 1
        assert L.fxrx_inflight(ctx.h) == inflight
    ctx.close()
    assert most == MAX_DEPTH and refused == N_BLOCKS - MAX_DEPTH
    for s in range(2):
        bad = differences(one[s], got[s])
        assert not bad, (s, bad[:4])


# ---------------------------------------------------------------------------------------------------- readiness
@gpu
def test_ready_follows_a_block(fx, cap):
    xs, of, one = cap
    L = fx.lib()
    assert L.fxrx_ready(None) == ERR_ARG and L.fxrx_inflight(None) == 0
    ctx = fx.RxContext(2, want_framesyms=True)
    ctx.set_timing(2)
    for k in range(2):
        assert L.fxrx_ready(ctx.h) == 0 and L.fxrx_inflight(ctx.h) == 0          # nothing in flight
        ctx.reset()
        submit(ctx, xs)
        assert L.fxrx_inflight(ctx.h) == 1
        poll_ready(L, ctx)
        assert L.fxrx_ready(ctx.h) == 1 and L.fxrx_inflight(ctx.h) == 1          # it stays 1 until the block is collected
        got = by_stream(ctx.results(ctx.collect_raw()))
        tm = ctx.timing()
        print("\nafter fxrx_ready == 1: host_collectwait_ms %.4f, total_ms %.4f" % (tm["host_collectwait_ms"], tm["total_ms"]))
        assert tm["total_ms"] > 0.0 and tm["host_collectwait_ms"] < tm["total_ms"]   # the collect did not wait for the block
        for s in range(2):
            assert not differences(one[s], got[s])
    assert L.fxrx_ready(ctx.h) == 0
    ctx.close()


@gpu
def test_ready_launches_an_open_gang(fx, cap, monkeypatch):
    """depth 4, FXRX_TAIL_GANG=2: four blocks, one collected, a fifth whose tail is deferred; the three in front of it are
    collected, so that the oldest block in flight is the one without a tail.  One fxrx_ready call sends it out."""
    xs, of, one = cap
    L = fx.lib()
    monkeypatch.setenv("FXRX_TAIL_GANG", "2")
    ctx = fx.RxContext(2, want_framesyms=True)
    ctx.set_depth(4)
    res = []
    for k in range(4):
        ctx.reset()
        submit(ctx, xs)
    res.append(ctx.results(ctx.collect_raw()))
    ctx.reset()
    submit(ctx, xs)
    assert L.fxrx_inflight(ctx.h) == 4
    for k in range(3):
        res.append(ctx.results(ctx.collect_raw()))
    assert L.fxrx_inflight(ctx.h) == 1
    assert ctx.gang_open() > 0, "path not exercised: no block in flight has its tail deferred"
    r = L.fxrx_ready(ctx.h)
    assert r in (0, 1) and ctx.gang_open() == 0                   # the call launched the tail
    poll_ready(L, ctx)
    res.append(ctx.results(ctx.collect_raw()))
    assert L.fxrx_inflight(ctx.h) == 0 and L.fxrx_ready(ctx.h) == 0
    ctx.close()
    assert len(res) == 5
    for got in res:
        got = by_stream(got)
        for s in range(2):
            compare_frames(of[s], got[s])
            assert not differences(one[s], got[s])


# ---------------------------------------------------------------------------------------------------- reset
def reset_blocks(xs, of):
    """four blocks in front of the reset and one behind it; the last cut lies 1000 samples into a frame of stream 0"""
    c3 = of[0][len(of[0]) * 3 // 4].info["start"] + 1000
    assert c3 < of[0][len(of[0]) * 3 // 4 + 1].info["start"] - 600 and c3 < N - 8000
    cuts = [c3 // 4 + 3, c3 // 2 + 1, c3 * 3 // 4 + 2, c3]
    e = [0] + cuts + [N]
    return [[np.ascontiguousarray(x[a:b]) for x in xs] for a, b in zip(e[:-1], e[1:])], c3


def run_reset(fx, blocks, left, reset=True, gang_open=None, mode=0):
    """B0 collected at once; B1..B3 submitted, collected until `left` stay in flight; fxrx_reset; B4; collect the rest.
    Returns the results per block."""
    ctx = fx.RxContext(2, mode=mode, want_framesyms=True)
    ctx.set_depth(4)
    res = []
    submit(ctx, blocks[0])
    res.append(ctx.results(ctx.collect_raw()))
    for b in blocks[1:4]:
        submit(ctx, b)
    for k in range(3 - left):
        res.append(ctx.results(ctx.collect_raw()))
    assert fx.lib().fxrx_inflight(ctx.h) == left
    if gang_open is not None:
        assert (ctx.gang_open() > 0) == gang_open, "path not exercised: gang open %d" % ctx.gang_open()
    if reset:
        ctx.reset()
    submit(ctx, blocks[4])
    while fx.lib().fxrx_inflight(ctx.h):
        res.append(ctx.results(ctx.collect_raw()))
    ctx.close()
    assert len(res) == 5
    return [by_stream(r) for r in res]


@gpu
@pytest.mark.parametrize("left,gang", [(0, 1), (1, 1), (3, 1), (3, 2)])
def test_reset_with_blocks_in_flight(fx, cap, monkeypatch, left, gang):
    xs, of, one = cap
    blocks, c3 = reset_blocks(xs, of)
    monkeypatch.setenv("FXRX_TAIL_GANG", str(gang))
    plain = run_reset(fx, blocks, 0, reset=False)                            # the same blocks without the reset
    for s in range(2):
        assert not differences(one[s], [g for blk in plain for g in blk[s]]), s
    assert any(g["start"] < c3 for g in plain[4][0]), "no frame of stream 0 straddles the last cut: the case is not what it was built to be"
    ctx = fx.RxContext(2, want_framesyms=True)
    fresh = by_stream(ctx.process(blocks[4]))
    ctx.close()
    got = run_reset(fx, blocks, left, gang_open=(gang > 1) if left == 3 else None)
    for k in range(4):                                                       # absolute starts counted from the old origin
        for s in range(2):
            assert not differences(plain[k][s], got[k][s]), (k, s, differences(plain[k][s], got[k][s])[:3])
    for s in range(2):
        assert fresh[s] and all(g["start"] >= 0 for g in fresh[s][1:]) and fresh[s][0]["start"] >= -256
        assert not differences(fresh[s], got[4][s]), (s, differences(fresh[s], got[4][s])[:3])
    straddler = [g["start"] for g in plain[4][0] if g["start"] < c3][0]
    assert all(g["start"] + c3 != straddler for g in got[4][0])              # not completed behind the reset


@gpu
def test_reset_in_detector_mode_zeroes_the_windows_below_the_floor(fx, cap):
    """the block behind the reset starts 40 samples into a preamble of stream 0: the detection's window starts below the new
    floor, and those samples read (0, 0) -- not the samples of the block in front of the reset, which the device still holds"""
    xs, of, one = cap
    a = of[0][len(of[0]) // 2].info["start"]
    e = [0, a // 3, a * 2 // 3 + 1, a - 700, a + 40, N]
    blocks = [[np.ascontiguousarray(x[p:q]) for x in xs] for p, q in zip(e[:-1], e[1:])]
    ctx = fx.RxContext(2, mode=fx.MODE_DETECTOR, want_framesyms=True)
    fresh = by_stream(ctx.process(blocks[4]))
    ctx.close()
    key = lambda g: (g["start"], g["tau"], g["gamma"], g["dphi"], g["phi"], g["framesyms"].tobytes())
    assert fresh[0] and fresh[0][0]["start"] < 0, "path not exercised: no detection starts below the floor (%r)" % [g["start"] for g in fresh[0][:2]]
    for left in (0, 3):
        got = run_reset(fx, blocks, left, mode=fx.MODE_DETECTOR)
        for s in range(2):
            assert [key(g) for g in got[4][s]] == [key(g) for g in fresh[s]], (left, s)
        g = got[4][0][0]
        p = g["start"]
        assert not np.any(g["framesyms"][:-p]) and np.array_equal(g["framesyms"][-p:], blocks[4][0][:512 + p]), (left, p)


# ---------------------------------------------------------------------------------------------------- timing levels
@gpu
@pytest.mark.parametrize("depth", [1, 3])
def test_timing_levels(fx, cap, depth):
    xs, of, one = cap
    L = fx.lib()
    e = [0, 9_001, 17_000, 29_500, N]
    blocks = [[np.ascontiguousarray(x[a:b]) for x in xs] for a, b in zip(e[:-1], e[1:])]
    ctx = fx.RxContext(2, want_framesyms=True)
    assert L.fxrx_set_timing(ctx.h, 3) == ERR_ARG and L.fxrx_set_timing(ctx.h, -2) == ERR_ARG and L.fxrx_set_timing(None, 0) == ERR_ARG
    ctx.close()
    for level in (-1, 0, 1, 2):
        ctx = fx.RxContext(2, want_framesyms=True)
        ctx.set_depth(depth)
        ctx.set_timing(level)
        got, tms, inflight = [], [], 0
        for b in blocks:
            if inflight == depth:
                got += ctx.results(ctx.collect_raw()); tms.append(ctx.timing()); inflight -= 1
            submit(ctx, b); inflight += 1
        while inflight:
            got += ctx.results(ctx.collect_raw()); tms.append(ctx.timing()); inflight -= 1
        ctx.close()
        got = by_stream(got)
        for s in range(2):
            assert not differences(one[s], got[s]), (level, depth, s)
        acts_as = level if level >= 0 else (2 if depth == 1 else 0)
        assert sum(tm["frames"] for tm in tms) == len(one[0]) + len(one[1])
        for tm in tms:
            assert tm["hops"] > 0 and tm["samples"] > 0 and tm["walk_jobs"] > 0 and tm["payload_symbols"] > 0, (level, depth, tm)     # the counters are always there
            if acts_as == 0:
                assert all(tm[k] == 0.0 for k in STAGES) and tm["total_ms"] == 0.0, (level, depth, tm)
            elif acts_as == 1:
                assert tm["paypll_ms"] > 0.0 and all(tm[k] == 0.0 for k in STAGES if k != "paypll_ms") and tm["total_ms"] == tm["paypll_ms"], (level, depth, tm)
            else:
                assert all(tm[k] > 0.0 for k in STAGES if k != "seekverify_ms") and tm["seekverify_ms"] >= 0.0 and tm["total_ms"] > tm["paypll_ms"], (level, depth, tm)


# ---------------------------------------------------------------------------------------------------- device-resident symbols
def device_symbols(fx, ctx):
    """(pointer or None, count, the count's complex64 values copied back with the HIP runtime the library itself is linked to)"""
    L = fx.lib()
    n = C.c_uint64(0xDEAD)
    p = L.fxrx_device_framesyms(ctx.h, C.byref(n))
    if not p:
        return None, n.value, None
    out = np.empty(n.value, np.complex64)
    L.hipMemcpy.restype = C.c_int
    L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert L.hipMemcpy(out.ctypes.data, p, out.nbytes, 2) == 0             # hipMemcpyDeviceToHost
    return p, n.value, out


@gpu
@pytest.mark.parametrize("want", [True, False])
@pytest.mark.parametrize("fec0", [None, FEC_NONE])
def test_device_framesyms(fx, cap, want, fec0):
    """After a collect with frames: a pointer and a count; frame i's symbols stand at the sum of the counts of the results in front
    of it, each rounded up to the arena's granule of 8 symbols, bit for bit the host copies.  The capture's own frames have 832
    symbols each -- a multiple of 8 --: there the count is the sum of num_framesyms and the device holds the host symbols
    concatenated.  The uncoded variant (412 symbols a frame) is the one that shows the granules."""
    xs, of, one = cap
    if fec0 is not None:
        xs = [fx.synth_stream(N // 2, stream_id=1710 + s, payload_len=100, fec0=fec0, snr_db=15.0, return_payloads=False) for s in range(2)]
    ref_ctx = fx.RxContext(2, want_framesyms=True)
    ref = ref_ctx.process(xs)
    ref_ctx.close()
    assert len(ref) >= 8 and all(g["header_valid"] and g["num_framesyms"] == (832 if fec0 is None else 412) for g in ref)
    ctx = fx.RxContext(2, want_framesyms=want)
    assert device_symbols(fx, ctx)[0] is None                                  # before any collect
    got = ctx.process(xs)
    p, n, dev = device_symbols(fx, ctx)
    assert p is not None
    assert [g["num_framesyms"] for g in got] == [g["num_framesyms"] for g in ref]
    if not want:
        f = fx._ffi.Frame()
        for i in range(len(got)):
            fx.lib().fxrx_result(ctx.h, i, C.byref(f))
            assert not f.framesyms and f.num_framesyms == ref[i]["num_framesyms"]     # the symbols stay on the device
    off = np.cumsum([0] + [(g["num_framesyms"] + 7) // 8 * 8 for g in got])
    assert n == off[-1]
    for i, g in enumerate(ref):
        assert np.array_equal(dev[off[i]:off[i] + g["num_framesyms"]].view(np.uint32), g["framesyms"].view(np.uint32)), i
    if fec0 is None:
        assert n == sum(g["num_framesyms"] for g in got)
        assert dev.tobytes() == b"".join(g["framesyms"].tobytes() for g in ref)
    rng = np.random.default_rng(1720)
    noise = [(0.05 * (rng.standard_normal(3000) + 1j * rng.standard_normal(3000))).astype(np.complex64) for _ in xs]
    ctx.reset()
    assert ctx.process(noise) == []
    assert device_symbols(fx, ctx)[:2] == (None, 0)                            # a block with no frames
    ctx.close()
