"""Blocks whose traffic the block before did not announce (tests/shift_cases.py; tests/test_ref_shift.py proves on the CPU that every case
is what its name says).  `-m gpu`.

A block's grids -- and whether some of its kernels are launched at all -- follow what the last collected block held; what they do not
cover is completed at fxrx_collect (finish_decode, six reasons) or, for the trellis arena, taken off the batch path by the plan kernel.
Per case, with continuing streams (`cont`) and with a reset before every block (`reset`), at depth 1 and with four blocks in flight:
  * every block's frames are the CPU oracle's, field for field (parity_util.compare_frames, the symbols included);
  * in the blocks that make the shift, every header-valid frame's payload and validity are those of the numpy reference
    (tests/ref_decode.py) decoded from the GPU's own symbols, ties excluded as in tests/test_gpu_ref_decode.py, at most 1 % of them;
  * depth 1: RxContext.late_stats() shows the named reason acting exactly once at the shifted block and nothing acting at the others,
    late_decodes counts the blocks on which any reason acted, the same block a second time (`reset`: the hints are now right) gives
    identical frames with no reason acting, and neither does one when every block runs alone on a fresh context (the control)."""
import numpy as np
import pytest

import ref_detect as rd
import shift_cases as SC
from parity_util import compare_frames
from test_gpu_ref_decode import Ref

pytestmark = pytest.mark.gpu

REASONS = ("more_plain", "more_rs", "more_batch_frames", "more_batch_items", "more_fb", "late_trellis")


def _ctx(fx, monkeypatch, name):
    c = SC.case(name)
    for k in ("FXRX_VB_BLK", "FXRX_VB_DEBUG", "FXRX_TAIL_GANG", "FXRX_DEBUG_CUS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in c.get("env", {}).items():
        monkeypatch.setenv(k, str(v))
    ns = len(c["blocks"][0])
    if c.get("detector"):
        return fx.RxContext(ns, mode=fx.MODE_DETECTOR, threshold=0.45)
    return fx.RxContext(ns, want_framesyms=True)


def feed(ctx, blocks, depth, reset, on_device=False):
    """-> per block: (frames per stream, late_stats() after its collect, timing() after its collect)"""
    import torch
    ctx.set_depth(depth)
    out, keep, inflight = [], [], 0
    ns = len(blocks[0])

    def collect():
        got = ctx.results(ctx.collect_raw())
        out.append(([[g for g in got if g["stream"] == s] for s in range(ns)], ctx.late_stats(), ctx.timing()))
    for b in blocks:
        if inflight == depth:
            collect(); inflight -= 1
        if reset:
            ctx.reset()
        if on_device:
            parts = [torch.from_numpy(np.array(x)).cuda() for x in b]
            torch.cuda.synchronize()
            ptrs = [p.data_ptr() for p in parts]
        else:
            parts = [np.ascontiguousarray(x) for x in b]
            ptrs = [p.ctypes.data for p in parts]
        keep.append(parts)
        ctx.submit_raw(ptrs, [len(x) for x in b], on_device); inflight += 1
    while inflight:
        collect(); inflight -= 1
    return out


def compare_block(name, want, got, k):
    """one block's frames per stream against the oracle's"""
    for s, g in enumerate(got):
        if SC.case(name).get("detector"):
            assert [q["pos"] for q in want[s]] == [f["start"] for f in g], (name, k, s)
            for q, f in zip(want[s], g):
                assert rd.parity_ok(q, f)[0], (name, k, q["pos"])
        else:
            compare_frames(want[s], g)


def check_oracle(name, form, res, repeat=1, every=1):
    """block k of `res` (the case's sequence, every block `every` times in a row, the whole `repeat` times over) against the oracle"""
    want = SC.oracle(name, form, repeat if form == "cont" else 1)
    for k, (got, _, _) in enumerate(res):
        compare_block(name, want[(k // every) % len(want)], got, k)


def same(a, b):
    """two frame lists identical in every field (floats and symbols by their bits)"""
    assert len(a) == len(b), (len(a), len(b))
    for fa, fb in zip(a, b):
        for key in fa:
            va, vb = fa[key], fb[key]
            if isinstance(va, np.ndarray) or isinstance(vb, np.ndarray):
                assert va is not None and vb is not None and np.array_equal(va.view(np.uint8), vb.view(np.uint8)), key
            else:
                assert va == vb or (va != va and vb != vb), (key, va, vb)


_REF = {}


def ref_of(g):
    """the numpy reference's view of a frame, computed once per distinct frame (the runs of a case deliver the same symbols)"""
    key = (g["mod_scheme"], g["check"], g["fec0"], g["fec1"], len(g["payload"]), hash(g["framesyms"].tobytes()))
    if key not in _REF:
        _REF[key] = Ref(g)
    return _REF[key]


def check_reference(name, res, blocks, only=None):
    """only: a predicate on (index within the stream, frame) that picks the frames to decode (default: every header-valid frame)"""
    n = excluded = 0
    bad = []
    for k in blocks:
        for s, got in enumerate(res[k][0]):
            for i, g in enumerate(got):
                if not g["header_valid"] or (only and not only(i, g)):
                    continue
                r = ref_of(g)
                n += 1
                if r.tie:
                    excluded += 1
                elif (g["payload"], g["payload_valid"]) != (r.payload, r.valid):
                    bad.append((k, s, g["start"], g["payload_valid"], r.valid))
    assert not bad, (name, bad[:8])
    assert n > 0 and excluded <= 0.01 * n, (name, excluded, n)


def rises(res):
    """per block: the reasons whose counter rose at its collect (by how much), and the rise of late_decodes"""
    out, prev, prev_ld = [], (0,) * 6, 0
    for _, ls, tm in res:
        out.append(({REASONS[i]: ls[i] - prev[i] for i in range(6) if ls[i] != prev[i]}, tm["late_decodes"] - prev_ld))
        prev, prev_ld = ls[:6], tm["late_decodes"]
    return out


@pytest.mark.parametrize("form", ["cont", "reset"])
@pytest.mark.parametrize("name", list(SC.CASES))
def test_shift_one_block_at_a_time(fx, oracle, monkeypatch, name, form):
    c = SC.case(name)
    blocks = SC.build(name)
    every = 2 if form == "reset" else 1                           # independent captures: every block twice in a row
    seq = [b for b in blocks for _ in range(every)]
    ctx = _ctx(fx, monkeypatch, name)
    assert tuple(ctx.LATE_REASONS) == REASONS
    res = feed(ctx, seq, 1, form == "reset")
    ctx.close()
    up = rises(res)
    print("\n%s (%s): rises per block %s; last-block counts %s" % (name, form, up, [r[1][6:] for r in res]))
    check_oracle(name, form, res, every=every)
    for k, (why, ld) in enumerate(up):
        b, again = k // every, k % every
        named = [] if again else c["expect"].get(b, [])
        for r in named:
            assert why.get(r) == 1, (name, form, "block %d: %s did not act exactly once" % (b, r), why)
        if not named:
            assert not why, (name, form, "block %d%s: nothing should have been left to fxrx_collect" % (b, " again" if again else ""), why)
        assert ld == (1 if why else 0), (name, form, k, why, ld)
        if again:
            for s in range(len(res[k][0])):
                same(res[k - 1][0][s], res[k][0][s])
        if "more_fb" in named:
            assert res[k][2]["vb_fallbacks"] > 32, res[k][2]["vb_fallbacks"]       # ... and it is handed-back frames that outgrew the launch, not leftovers of another reason
    if not c.get("detector"):
        check_reference(name, res, [b * every for b in c["expect"]])


@pytest.mark.parametrize("form", ["cont", "reset"])
@pytest.mark.parametrize("name", list(SC.CASES))
def test_shift_four_blocks_in_flight(fx, oracle, monkeypatch, name, form):
    """The sequence twice over at depth 4 with the tails ganged (the default): the hints a block is sized from are those of a block
    three or four behind it.  Device input for two of the cases."""
    c = SC.case(name)
    blocks = SC.build(name)
    ctx = _ctx(fx, monkeypatch, name)
    res = feed(ctx, blocks * 2, 4, form == "reset", on_device=bool(c.get("device")))
    ctx.close()
    up = rises(res)
    print("\n%s (%s), depth 4: rises per block %s" % (name, form, up))
    check_oracle(name, form, res, repeat=2)
    assert all(ld == (1 if why else 0) for why, ld in up), up
    if not c.get("detector"):
        check_reference(name, res, [len(blocks) + b for b in c["expect"]])


@pytest.mark.parametrize("name", list(SC.CASES))
def test_control_every_block_on_a_fresh_context(fx, oracle, monkeypatch, name):
    """nothing collected yet: everything is launched at capacity, and no reason acts"""
    blocks = SC.build(name)
    want = SC.oracle(name, "reset")
    for b, blk in enumerate(blocks):
        ctx = _ctx(fx, monkeypatch, name)
        res = feed(ctx, [blk], 1, True)
        ctx.close()
        compare_block(name, want[b], res[0][0], b)
        assert rises(res)[0] == ({}, 0), (name, b, rises(res))


def test_arena_overflow_demotes_frames(fx, oracle, monkeypatch):
    """One block of dense QAM64 rate-7/8 traffic whose trellis work items do not fit the arena (1.5 steps per sample): the plan kernel
    takes the frames that do not fit, and every frame behind them, off the batch path; the wave-per-frame decoder has them."""
    name = SC.ARENA
    blocks = SC.build(name)
    ctx = _ctx(fx, monkeypatch, name)
    res = feed(ctx, blocks, 1, True)
    ctx.close()
    ls = res[0][1]
    expected = SC.block_counts(name, "reset")[0]
    print("\narena: %d samples, oracle counts %s, late_stats %s" % (len(blocks[0][0]), expected, ls))
    check_oracle(name, "reset", res)
    demoted = expected["batch"] - ls[7]
    assert demoted > 0 and ls[6] == expected["plain"] + demoted and ls[8] == 0, (expected, ls)
    assert rises(res)[0] == ({}, 0)
    # (the numpy Viterbi decoder takes most of a second per frame of this size: the demoted frames and the last two that kept their place)
    check_reference(name, res, [0], only=lambda i, g: i >= ls[7] - 2)
