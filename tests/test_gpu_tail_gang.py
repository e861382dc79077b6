"""The tails of several blocks in flight -- payload PLL, fx_vbpre_kernel -- in one launch each (FXRX_TAIL_GANG).
Every case runs the same block sequence with the gang off (FXRX_TAIL_GANG=1) and on; the frames must be identical field for
field (evm_sum bit for bit, carrier-recovered symbols and payloads included), they are those of the CPU oracle, and
fxrx_debug_gang_stats, read after every submit and collect, gives the size of every gang that went out: none when off, and
when on the sizes the case is built to produce -- a launch with four members wherever G = 4.

A tail is deferred only with at least G blocks in flight ahead of it whose tails are out, and a gang of G needs G - 1 more
deferred behind those: 2 G - 1 blocks in flight when the submit arrives that fills it.  So gangs of 2 fill from depth 4 on,
gangs of 4 from depth 8 on (at depth 6 the setting 4 gives pairs, at depth 4 nothing): the cases run G = 2 at depth 4 and
G = 4 at depth 8."""
import threading

import numpy as np
import pytest

from parity_util import oracle_frames, compare_frames

CONV_V27P23, HAMMING74, QAM16 = 15, 4, 27
DEPTH_GANG = [(4, 2), (8, 4)]


def _same(a, b):
    assert len(a) == len(b), (len(a), len(b))
    for fa, fb in zip(a, b):
        assert fa.keys() == fb.keys()
        for k in fa:
            va, vb = fa[k], fb[k]
            if isinstance(va, np.ndarray) or isinstance(vb, np.ndarray):
                assert va is not None and vb is not None and np.array_equal(va, vb), k
            else:
                assert va == vb or (va != va and vb != vb), (k, va, vb)



def _within(seconds, fn):
    """The test's own timeout: fn runs on a thread of its own (a call into the library holds no interpreter lock), and a
    wait inside it that never ends fails the test here instead of hanging the suite."""
    box = {}
    def work():
        try:
            box["value"] = fn()
        except BaseException as e:                      # handed to the test's thread
            box["error"] = e
    t = threading.Thread(target=work, daemon=True)
    t.start(); t.join(seconds)
    assert not t.is_alive(), "no result within %d s" % seconds
    if "error" in box:
        raise box["error"]
    return box["value"]


class _Sizes:
    """Sizes of the gangs that went out, from fxrx_debug_gang_stats after every call (one call launches one gang at the most)."""
    def __init__(self, ctx):
        self.ctx, self.last, self.sizes = ctx, ctx.gang_stats(), []

    def step(self):
        st = self.ctx.gang_stats()
        dl, dm = st[0] - self.last[0], st[1] - self.last[1]
        assert dl in (0, 1) and (dm >= 2 if dl else dm == 0), (self.last, st)
        if dl:
            self.sizes.append(dm)
        self.last = st


def _run(fx, monkeypatch, gang, blocks, depth, reset=True, early=0, hook=None):
    """blocks: a list of blocks, each a list with one array per stream.  early: blocks collected straight after their submit, in
    front of the pipelined part (the library defers nothing before its first collect).  hook(ctx, i, drain), if given, is called
    in front of the submit of block i; drain() collects everything in flight.
    Returns (frames per block, sizes of the gangs that went out, in order)."""
    monkeypatch.setenv("FXRX_TAIL_GANG", str(gang))
    ctx = fx.RxContext(len(blocks[0]), want_framesyms=True)
    ctx.set_depth(depth)
    seen = _Sizes(ctx)
    res, inflight = [], 0

    def collect():
        nonlocal inflight
        res.append(ctx.results(ctx.collect_raw())); inflight -= 1
        seen.step()
    def drain():
        while inflight:
            collect()
    for i, b in enumerate(blocks):
        if hook is not None:
            hook(ctx, i, drain); seen.step()
        if inflight == depth:
            collect()
        if reset:
            ctx.reset()
        ctx.submit_raw([a.ctypes.data for a in b], [len(a) for a in b], False); inflight += 1
        seen.step()
        if i < early:
            collect()
    drain()
    assert ctx.gang_open() == 0
    stats = ctx.gang_stats()
    ctx.close()
    assert stats == (len(seen.sizes), sum(seen.sizes)), (stats, seen.sizes)
    return res, seen.sizes


def _off(fx, monkeypatch, blocks, depth, **kw):
    off, sizes = _run(fx, monkeypatch, 1, blocks, depth, **kw)
    assert sizes == [], sizes
    assert len(off) == len(blocks)
    return off


def _on(fx, monkeypatch, off, gang, blocks, depth, want, **kw):
    """want: gang sizes that must have gone out (no gang formed: a failure, not a pass); none may be larger than the setting."""
    on, sizes = _run(fx, monkeypatch, gang, blocks, depth, **kw)
    print("gang %d depth %d %r: gangs of %r" % (gang, depth, kw, sizes))
    assert sizes and max(sizes) <= gang and all(w in sizes for w in want), (gang, depth, sizes, want)
    assert len(on) == len(off)
    for a, b in zip(on, off):
        _same(a, b)


def _off_and_on(fx, monkeypatch, blocks, depth, gang, **kw):
    """Off, then on; with the setting G at least one launch must have carried G members."""
    off = _off(fx, monkeypatch, blocks, depth, **kw)
    _on(fx, monkeypatch, off, gang, blocks, depth, (gang,), **kw)
    return off


@pytest.fixture(scope="module")
def captures(fx, oracle):
    """Nine single-stream captures that differ from each other, with their oracle frames (computed once, never changed)."""
    specs = [
        dict(n=150_000, stream_id=1531, snr_db=5.0),                                  # frames that need the trellis kernels
        dict(n=150_000, stream_id=1500),                                              # clean 1024-byte PSK4
        dict(n=150_000, stream_id=1530),
        dict(n=120_000, stream_id=1510, fec0=CONV_V27P23, payload_len=600),           # punctured: no codeword check
        dict(n=150_000, stream_id=1520, fec1=HAMMING74, payload_len=500),             # outer Hamming(7,4)
        dict(n=150_000, stream_id=1540, mod=QAM16, payload_len=700, snr_db=25.0),     # a second modulation class
        None,                                                                         # noise only
        dict(n=150_000, stream_id=1401, payload_len=800, snr_db=4.0),                 # trellis again, inside a gang
        dict(n=120_000, stream_id=1511, payload_len=3000),                            # beyond the front part's LDS buffer
    ]
    xs, refs = [], []
    for sp in specs:
        if sp is None:
            rng = np.random.RandomState(1541)
            x = (0.05 * (rng.standard_normal(130_000) + 1j * rng.standard_normal(130_000))).astype(np.complex64)
        else:
            sp = dict(sp)
            x = fx.synth_stream(sp.pop("n"), **sp)[0]
        xs.append(x); refs.append(oracle_frames(oracle, x))
    assert all(f.payload_valid for i in (1, 2, 3, 4, 5, 8) for f in refs[i]) and all(len(refs[i]) >= 2 for i in (1, 2, 3, 4, 5, 8))
    assert refs[5][0].mod_scheme == QAM16 and len(refs[6]) == 0
    assert all(sum(1 for f in refs[i] if f.header_valid) >= 4 for i in (0, 7))
    return xs, refs


@pytest.mark.gpu
def test_different_blocks_in_one_gang(fx, captures, monkeypatch):
    """The first blocks are collected at once (the 5 dB one among them: the trellis kernels are in the chain of all that follow).
    Depth 6, two collected at once: with G = 2 the pairs are blocks (4, 5) -- two modulation classes -- and (6, 7) -- noise only
    beside a block whose frames need the trellis -- and the ninth block's gang closes short at collect; with G = 4 blocks 2 to 5
    go alone, 6 and 7 are deferred, and the ninth, with three ahead, sends them out as a pair.
    Depth 8, G = 4, one collected at once: blocks 1 to 4 go alone and 5 to 8 -- 16-QAM, noise only (a member without waves), 4 dB
    (its own trellis launches between and behind the ganged ones), 3000-byte frames -- are one launch of four.  Two collected at
    once: blocks 6, 7, 8 are deferred and go out three strong when collect reaches block 6."""
    xs, refs = captures
    blocks = [[x] for x in xs]
    off = _off(fx, monkeypatch, blocks, 6, early=2)
    for ref, got in zip(refs, off):
        compare_frames(ref, got)
    _on(fx, monkeypatch, off, 2, blocks, 6, (2,), early=2)
    _on(fx, monkeypatch, off, 4, blocks, 6, (2,), early=2)
    _on(fx, monkeypatch, off, 4, blocks, 8, (4,), early=1)
    _on(fx, monkeypatch, off, 4, blocks, 8, (3,), early=2)


@pytest.mark.gpu
@pytest.mark.parametrize("depth,gang", DEPTH_GANG)
def test_collect_straight_after_the_submit_that_opened_a_gang(fx, captures, monkeypatch, depth, gang):
    """Fill the pipeline, collect one block, submit one more -- its tail is deferred, the gang has one member --, then collect
    everything: all blocks arrive (a wait on the deferred block's ev[8] as its earlier use left it would hand out stale results)."""
    xs, refs = captures
    order = [1, 2, 4, 1, 2, 4, 1, 2, 4][:depth + 1]
    blocks = [[xs[i]] for i in order]
    monkeypatch.setenv("FXRX_TAIL_GANG", str(gang))
    ctx = fx.RxContext(1, want_framesyms=True)
    ctx.set_depth(depth)
    res = []
    for b in blocks[:depth]:
        ctx.reset(); ctx.submit_raw([b[0].ctypes.data], [len(b[0])], False)
    res.append(ctx.results(ctx.collect_raw()))
    assert ctx.gang_open() == 0
    ctx.reset(); ctx.submit_raw([blocks[depth][0].ctypes.data], [len(blocks[depth][0])], False)
    assert ctx.gang_open() == 1 and ctx.gang_stats() == (0, 0)      # deferred, and nothing has carried two blocks
    for _ in range(depth):
        res.append(_within(60, lambda: ctx.results(ctx.collect_raw())))
    assert ctx.gang_open() == 0 and ctx.gang_stats() == (0, 0)      # (a gang of one is a block's own tail: not counted)
    ctx.close()
    assert len(res) == depth + 1
    for i, got in zip(order, res):
        compare_frames(refs[i], got)


@pytest.mark.gpu
@pytest.mark.parametrize("depth,gang", DEPTH_GANG)
def test_reset_before_every_submit(fx, captures, monkeypatch, depth, gang):
    """The bench's pattern.  Depth 8, G = 4: the first collect comes in front of block 8; blocks 8 to 11 are deferred one by one,
    each with at least four ahead, and go out four strong with block 11."""
    xs, refs = captures
    order = [1, 2, 4, 5, 1, 3, 2, 4, 5, 1, 2, 3, 4]
    off = _off_and_on(fx, monkeypatch, [[xs[i]] for i in order], depth, gang)
    for i, got in zip(order, off):
        compare_frames(refs[i], got)


@pytest.fixture(scope="module")
def continuing(fx, oracle):
    xa = fx.synth_stream(900_000, stream_id=1400, payload_len=500, snr_db=14.0)[0]
    xb = fx.synth_stream(900_000, stream_id=1401, payload_len=800, snr_db=4.0)[0]
    return xa, xb, oracle_frames(oracle, xa), oracle_frames(oracle, xb)


@pytest.mark.gpu
@pytest.mark.parametrize("depth,gang", DEPTH_GANG)
def test_continuing_streams(fx, continuing, monkeypatch, depth, gang):
    """Nine blocks, the first collected at once; at depth 8 blocks 1 to 4 go alone and 5 to 8 are one launch of four."""
    xa, xb, ra, rb = continuing
    blocks = [[xa[i:i + 100_000], xb[i:i + 100_000]] for i in range(0, len(xa), 100_000)]
    off = _off_and_on(fx, monkeypatch, blocks, depth, gang, reset=False, early=1)
    got = [g for blk in off for g in blk]
    compare_frames(ra, [g for g in got if g["stream"] == 0])
    compare_frames(rb, [g for g in got if g["stream"] == 1])


@pytest.mark.gpu
@pytest.mark.parametrize("depth,gang", DEPTH_GANG)
def test_gang_closing_calls(fx, captures, monkeypatch, depth, gang):
    """set_timing(2) with a gang open (the deferred tail goes out, later blocks record all stage events and go alone); set_depth
    with blocks in flight and a gang open (one member at depth 4, three at depth 8) -- refused as ever, the gang goes out --, and
    again after a drain; then close() with a gang open and nothing of it collected."""
    xs, refs = captures
    order = [1, 2, 4] * 7
    n = len(order)
    at_timing, at_depth = depth + 1, depth + 6
    open_at_depth = {4: 1, 8: 3}[depth]

    def hooks(on):
        def hook(ctx, i, drain):
            if i == at_timing:
                assert ctx.gang_open() == (1 if on else 0)
                ctx.set_timing(2)
                assert ctx.gang_open() == 0
            if i == at_timing + 2:
                ctx.set_timing(0)
            if i == at_depth:
                assert ctx.gang_open() == (open_at_depth if on else 0)
                with pytest.raises(fx.rx.RxError):
                    ctx.set_depth(depth)
                assert ctx.gang_open() == 0
                drain()
                ctx.set_depth(depth)
        return hook
    off, _ = _run(fx, monkeypatch, 1, [[xs[i]] for i in order], depth, hook=hooks(False))
    on, sizes = _run(fx, monkeypatch, gang, [[xs[i]] for i in order], depth, hook=hooks(True))
    assert sizes and (depth != 8 or 3 in sizes), sizes
    assert len(on) == len(off) == n
    for i, a, b in zip(order, on, off):
        _same(a, b)
        compare_frames(refs[i], a)
    # close() with an open gang, nothing of it collected; the next context is none the worse
    monkeypatch.setenv("FXRX_TAIL_GANG", str(gang))
    ctx = fx.RxContext(1, want_framesyms=True)
    ctx.set_depth(depth)
    for k in range(depth):
        ctx.reset(); ctx.submit_raw([xs[1].ctypes.data], [len(xs[1])], False)
    compare_frames(refs[1], ctx.results(ctx.collect_raw()))
    ctx.reset(); ctx.submit_raw([xs[2].ctypes.data], [len(xs[2])], False)
    assert ctx.gang_open() == 1
    ctx.close()
    again, _ = _run(fx, monkeypatch, gang, [[xs[2]]] * 2, depth)
    for got in again:
        compare_frames(refs[2], got)


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [1, 3])
@pytest.mark.parametrize("gang", [2, 4])
def test_shallow_pipelines_never_gang(fx, captures, monkeypatch, depth, gang):
    xs, refs = captures
    order = [1, 2, 4, 1, 2, 4, 1, 2]
    seen_open = []
    res, sizes = _run(fx, monkeypatch, gang, [[xs[i]] for i in order], depth, hook=lambda ctx, i, drain: seen_open.append(ctx.gang_open()))
    assert sizes == [] and not any(seen_open), (sizes, seen_open)
    for i, got in zip(order, res):
        compare_frames(refs[i], got)


@pytest.mark.gpu
@pytest.mark.parametrize("depth,gang", DEPTH_GANG)
def test_unrepaired_handovers_in_a_ganged_run(fx, continuing, monkeypatch, depth, gang):
    """FXRX_VB_DEBUG=2: hand-overs are left unrepaired, the trellis kernels and the fallback decoder run per member between and
    behind the ganged launches (at depth 8: of one launch of four, blocks 5 to 8)."""
    xa, xb, ra, rb = continuing
    monkeypatch.setenv("FXRX_VB_DEBUG", "2")
    blocks = [[xa[i:i + 100_000], xb[i:i + 100_000]] for i in range(0, len(xa), 100_000)]
    off = _off_and_on(fx, monkeypatch, blocks, depth, gang, reset=False, early=1)
    got = [g for blk in off for g in blk]
    compare_frames(ra, [g for g in got if g["stream"] == 0])
    compare_frames(rb, [g for g in got if g["stream"] == 1])
