"""Integer IQ (sc16 / sc8) through the batched receive API on the GPU.

The reference in every case is the float path of the same library on what fxrx_iq_convert_host makes of the same integers
(tests/test_gpu_parity.py and friends pin that path to the oracle); the comparison is exact on every field of every result --
float estimates as bit patterns, payload bytes, payload symbols and soft bits.  One case is compared with the oracle directly.
Signal level of the quantised captures: RMS at 1/4 of full scale (tests/test_ingest.py checks on the CPU that the oracle decodes
every frame at that level in both formats)."""
import ctypes as C
import os
import struct
import numpy as np
import pytest

import failing_submit_cases as fsc
import ref_ingest as ri
from test_ingest import capture, quantised, RMS_OF_FULL_SCALE
from parity_util import oracle_frames, compare_frames

pytestmark = pytest.mark.gpu

FMTS = [ri.IQ_SC16, ri.IQ_SC8]
# sources of a block.  Page-locked host memory has two routes -- the conversion kernel reads it over the bus, or the copy engines
# move the raw bytes and the kernel converts on the device --, chosen by size against FXRX_INGEST_KERNEL_MAX when the context is
# created: "pinned_kernel" / "pinned_copy" force one each, "pinned" is the library's default
WHERE = ["pinned_kernel", "pinned_copy", "pinned", "pageable", "device"]
ROUTE = {"pinned_kernel": str(1 << 40), "pinned_copy": "0"}


def make_ctx(fx, where, *args, **kw):
    """RxContext with the route for page-locked integer IQ that `where` names"""
    before = os.environ.get("FXRX_INGEST_KERNEL_MAX")
    if where in ROUTE:
        os.environ["FXRX_INGEST_KERNEL_MAX"] = ROUTE[where]
    try:
        return fx.RxContext(*args, **kw)
    finally:
        if where in ROUTE:
            if before is None:
                del os.environ["FXRX_INGEST_KERNEL_MAX"]
            else:
                os.environ["FXRX_INGEST_KERNEL_MAX"] = before


def _bits(v):
    return struct.pack("<f", v) if isinstance(v, float) else v


def same(got, ref, what=""):
    """exact equality of two result lists, floats by bit pattern"""
    assert len(got) == len(ref), "%s: %d results, reference %d" % (what, len(got), len(ref))
    for k, (a, b) in enumerate(zip(got, ref)):
        assert a.keys() == b.keys()
        for key in a:
            va, vb = a[key], b[key]
            if isinstance(va, np.ndarray) or isinstance(vb, np.ndarray):
                assert va is not None and vb is not None and va.dtype == vb.dtype and np.array_equal(va.view(np.uint8), vb.view(np.uint8)), (what, k, key)
            else:
                assert _bits(va) == _bits(vb), (what, k, key, va, vb)


class Pinned:
    """page-locked host bytes (fxrx_pinned_alloc) as a numpy uint8 array"""

    def __init__(self, fx, nbytes):
        self.L = fx.lib()
        self.p = self.L.fxrx_pinned_alloc(max(nbytes, 1))
        assert self.p, self.L.fxrx_last_error()
        self.a = np.frombuffer((C.c_ubyte * max(nbytes, 1)).from_address(self.p), np.uint8)

    def free(self):
        self.a = None
        self.L.fxrx_pinned_free(self.p)


def run_int(fx, ctx, qs, fmt, where, raw=False):
    """one block of integer streams qs ((n, 2) arrays) from page-locked / pageable host memory or device memory"""
    if where == "pageable":
        return ctx.process([np.ascontiguousarray(q) for q in qs])                    # (through the dtype dispatch of rx.py)
    if where == "device":
        import torch
        return ctx.process([torch.from_numpy(np.ascontiguousarray(q)).cuda() for q in qs])
    pins = []
    for q in qs:
        p = Pinned(fx, q.nbytes); p.a[:q.nbytes] = np.ascontiguousarray(q).view(np.uint8).reshape(-1); pins.append(p)
    try:
        return ctx.results(ctx.process_raw([p.p for p in pins], [len(q) for q in qs], False, fmt))
    finally:
        for p in pins:
            p.free()


def run_float(fx, ctx, qs, scale=None):
    return ctx.process([fx.iq_convert(q, scale=scale) for q in qs])


def streams_of(fx, fmt, lengths, seed=40):
    """streams of the given lengths cut from quantised captures (different captures, so that streams differ)"""
    out = []
    for k, n in enumerate(lengths):
        x, _ = capture(fx, n_frames=3, payload_len=100 + 60 * k, stream_id=seed + k)
        q, _ = quantised(x, fmt)
        reps = -(-n // len(q)) if n else 1
        out.append(np.ascontiguousarray(np.tile(q, (reps, 1))[:n]))
    return out


@pytest.mark.parametrize("mode", ["flex_rx", "detector"])
@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("fmt", FMTS)
def test_sources_and_modes(fx, fmt, where, mode):
    """several streams of different lengths (0, 1, odd, long) in one block, every source, both modes"""
    m = fx.MODE_DETECTOR if mode == "detector" else fx.MODE_FLEX_RX
    lengths = [9001, 0, 1, 12345, 7, 30011]
    qs = streams_of(fx, fmt, lengths)
    ref_ctx = fx.RxContext(len(qs), mode=m, want_framesyms=(mode == "flex_rx"))
    ctx = make_ctx(fx, where, len(qs), mode=m, want_framesyms=(mode == "flex_rx"))
    ref = run_float(fx, ref_ctx, qs)
    assert len(ref) >= 6, "test input produced only %d results" % len(ref)
    if mode == "flex_rx":
        assert sum(r["payload_valid"] for r in ref) >= 5
    same(run_int(fx, ctx, qs, fmt, where), ref, "%s %s" % (where, mode))
    # a second block continues every stream (carried tails are float already)
    qs2 = [q[::-1].copy() if len(q) < 10 else q for q in qs]
    same(run_int(fx, ctx, qs2, fmt, where), run_float(fx, ref_ctx, qs2), "second block")
    ctx.close(); ref_ctx.close()


@pytest.mark.parametrize("where", ["pinned_kernel", "pinned_copy", "pinned", "pageable"])
def test_large_block(fx, where):
    """more than 64 MiB of raw bytes in one stream (beyond what the float upload kernel fetches from page-locked memory), by every route"""
    x, _ = capture(fx, n_frames=4, payload_len=700, stream_id=3)
    q, _ = quantised(x, ri.IQ_SC16)
    n = (64 << 20) // 4 + 4099
    big = np.ascontiguousarray(np.tile(q, (-(-n // len(q)), 1))[:n])
    assert big.nbytes > 64 << 20
    qs = [big, q[:5001]]
    ref_ctx = fx.RxContext(2); ctx = make_ctx(fx, where, 2)
    ref = run_float(fx, ref_ctx, qs)
    assert sum(r["payload_valid"] for r in ref) >= 4 * (n // len(q)) - 4
    same(run_int(fx, ctx, qs, ri.IQ_SC16, where), ref, "large block")
    ctx.close(); ref_ctx.close()


def test_against_the_oracle_directly(fx, oracle):
    x, injected = capture(fx, n_frames=3, payload_len=1024, stream_id=11)
    for fmt in FMTS:
        q, _ = quantised(x, fmt)
        ctx = make_ctx(fx, "pinned_kernel", 1, want_framesyms=True)
        got = run_int(fx, ctx, [q], fmt, "pinned_kernel")
        compare_frames(oracle_frames(oracle, ri.to_float(q)), got)
        assert [g["payload"] for g in got if g["payload_valid"]] == [pl for _, pl in injected]
        ctx.close()


@pytest.mark.parametrize("where", ["pinned_kernel", "pinned_copy", "device"])
@pytest.mark.parametrize("fmt", FMTS)
def test_every_alignment_inside_a_canary_buffer(fx, fmt, where):
    """The same capture from every sample offset the pointer rules allow (sc8: 0..7 -> 2-byte steps, sc16: 0..3 -> 4-byte steps
    within a 16-byte line), inside a larger buffer whose other bytes hold a pattern that would decode differently if read;
    a second stream follows in the same block and must be exact as well."""
    x, _ = capture(fx, n_frames=2, payload_len=300, stream_id=21)
    q, _ = quantised(x, fmt)
    q = q[:len(q) - 3]                                           # odd tail
    other = streams_of(fx, fmt, [8191], seed=60)[0]
    ref_ctx = fx.RxContext(2, want_framesyms=True)
    lengths = (len(q), len(q) - 1, 5, 1)
    refs = {}
    for n in lengths:
        refs[n] = run_float(fx, ref_ctx, [q[:n], other]); ref_ctx.reset()
    ref_ctx.close()
    assert sum(r["payload_valid"] for r in refs[len(q)]) >= 3
    bps = q.itemsize * 2
    pad = 256
    canary = np.tile(np.array([0x5A, 0x7F, 0xA5, 0x80, 0x33, 0xC3, 0x7E, 0x81], np.uint8), (2 * pad + q.nbytes + 64) // 8 + 1)
    raw = np.ascontiguousarray(q).view(np.uint8).reshape(-1)
    ctx = make_ctx(fx, where, 2, want_framesyms=True)
    pin = Pinned(fx, len(canary)); pin2 = Pinned(fx, other.nbytes)
    pin2.a[:other.nbytes] = other.view(np.uint8).reshape(-1)
    assert pin.p % 16 == 0
    dev = None
    if where == "device":
        import torch
        dev = torch.empty(len(canary), dtype=torch.uint8, device="cuda")
        dev_other = torch.from_numpy(other).cuda()
        assert dev.data_ptr() % 16 == 0
    for off in range(16 // bps):
        for n in lengths:
            buf = canary.copy()
            o = pad + off * bps
            buf[o:o + n * bps] = raw[:n * bps]
            if where == "device":
                dev.copy_(torch.from_numpy(buf)); torch.cuda.synchronize()
                got = ctx.results(ctx.process_raw([dev.data_ptr() + o, dev_other.data_ptr()], [n, len(other)], True, fmt))
            else:
                pin.a[:len(buf)] = buf
                got = ctx.results(ctx.process_raw([pin.p + o, pin2.p], [n, len(other)], False, fmt))
            ctx.reset()
            same(got, refs[n], "offset %d, %d samples" % (off, n))
    pin.free(); pin2.free(); ctx.close()


@pytest.mark.parametrize("depth", [1, 4, 12])
def test_continuing_stream_with_the_format_changing_block_by_block(fx, depth):
    """One capture, quantised once (to sc8 values; as sc16 the same values times 256, so that every format describes the same
    floats at the default scales), cut into blocks at frame-straddling positions and submitted as float, sc16, sc8 in turn:
    equal to one float run over the whole capture, frame positions continuous."""
    x, injected = capture(fx, n_frames=14, payload_len=260, stream_id=5)
    q8, sat = quantised(x, ri.IQ_SC8)
    assert sat == 0
    q16 = q8.astype(np.int16) * np.int16(256)
    xf = fx.iq_convert(q8)
    assert np.array_equal(xf.view(np.uint32), fx.iq_convert(q16).view(np.uint32))
    ref_ctx = fx.RxContext(1, want_framesyms=True)
    ref = ref_ctx.process([xf]); ref_ctx.close()
    assert [r["payload"] for r in ref if r["payload_valid"]] == [pl for _, pl in injected]
    starts = [p for p, _ in injected]
    cuts = [0] + [starts[k] + d for k, d in zip(range(1, 14), [1, 63, 64, 65, 127, 700, 1500, 2001, 2500, 333, 18, 4000, 2])] + [len(x)]
    assert cuts == sorted(cuts)
    ctx = fx.RxContext(1, want_framesyms=True)
    ctx.set_depth(depth)
    pieces = []
    for k, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        pieces.append([np.ascontiguousarray(xf[a:b]), np.ascontiguousarray(q16[a:b]), np.ascontiguousarray(q8[a:b])][k % 3])
    got, inflight = [], 0
    for pc in pieces:
        if inflight == depth:
            got += ctx.collect(); inflight -= 1
        ctx.submit([pc]); inflight += 1
    while inflight:
        got += ctx.collect(); inflight -= 1
    same(got, ref, "depth %d" % depth)
    ctx.close()


@pytest.mark.parametrize("opts,fmt,where", [(dict(soft_decision=True, soft_header=True, soft_block=True), ri.IQ_SC16, "device"),
                                            (dict(equalizer=True), ri.IQ_SC8, "pinned_kernel")])
def test_options(fx, opts, fmt, where):
    g = fx.FrameGen(mod=27, fec0=11, fec1=7)                     # QAM16, r1/2 convolutional + Golay: a block code behind soft values
    rng = np.random.default_rng(8)
    parts = [np.zeros(200, np.complex64)]
    for _ in range(4):
        parts += [g.frame(rng.integers(0, 256, 333, dtype=np.uint8)), np.zeros(300, np.complex64)]
    g.close()
    x = np.concatenate(parts)
    x = (x * np.exp(1j * (0.01 * np.arange(len(x)) + 0.3)) + 0.03 * (rng.standard_normal(len(x)) + 1j * rng.standard_normal(len(x)))).astype(np.complex64)
    q, _ = quantised(x, fmt)
    ref_ctx = fx.RxContext(1, want_framesyms=True, **opts); ctx = make_ctx(fx, where, 1, want_framesyms=True, **opts)
    ref = run_float(fx, ref_ctx, [q])
    assert sum(r["payload_valid"] for r in ref) == 4
    if opts.get("soft_decision"):
        assert all(r["soft_bits"] is not None for r in ref)
    same(run_int(fx, ctx, [q], fmt, where), ref, str(opts))
    ctx.close(); ref_ctx.close()


@pytest.mark.parametrize("fmt", FMTS)
def test_scale_setter(fx, fmt):
    x, _ = capture(fx, n_frames=2, payload_len=400, stream_id=31)
    q, _ = quantised(x, fmt)
    ctx = make_ctx(fx, "pinned_kernel", 1, want_framesyms=True); ref_ctx = fx.RxContext(1, want_framesyms=True)
    L = fx.lib()
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert L.fxrx_set_iq_scale(ctx.h, fmt, C.c_float(bad)) == -1
    assert L.fxrx_set_iq_scale(ctx.h, 0, C.c_float(1.0)) == -1 and L.fxrx_set_iq_scale(ctx.h, 3, C.c_float(1.0)) == -1
    for scale in (None, 1.0 / 2048.0, 0.000123456, 3.7):
        if scale is not None:
            ctx.set_iq_scale(fmt, scale)
        ref = run_float(fx, ref_ctx, [q], scale)
        assert sum(r["payload_valid"] for r in ref) == 2
        same(run_int(fx, ctx, [q], fmt, "pinned_kernel"), ref, "scale %r" % scale)
        ctx.reset(); ref_ctx.reset()
    ctx.close(); ref_ctx.close()


def test_a_failing_submit_leaves_the_context_as_it_was(fx):
    fmt = ri.IQ_SC16
    x, _ = capture(fx, n_frames=6, payload_len=300, stream_id=41)
    q, _ = quantised(x, fmt)
    cut = len(q) // 2 + 77
    ref_ctx = fx.RxContext(1, want_framesyms=True)
    ref1 = run_float(fx, ref_ctx, [q[:cut]]); ref2 = run_float(fx, ref_ctx, [q[cut:]])
    ref_ctx.close()
    assert len(ref1) + len(ref2) == 6
    L = fx.lib()
    ctx = fx.RxContext(1, want_framesyms=True)
    a = Pinned(fx, q.nbytes + 16); a.a[:q.nbytes] = q.view(np.uint8).reshape(-1)
    same(ctx.results(ctx.process_raw([a.p], [cut], False, fmt)), ref1, "first block")
    p2 = a.p + 4 * cut
    ptr = (C.c_void_p * 1)(p2); cnt = (C.c_uint64 * 1)(len(q) - cut)
    assert L.fxrx_submit_fmt(ctx.h, ptr, cnt, 0, 7) == -1                              # unknown format
    assert L.fxrx_submit_fmt(ctx.h, ptr, cnt, 0, -1) == -1
    for mis in (1, 2, 3):
        bad = (C.c_void_p * 1)(p2 + mis)
        assert L.fxrx_submit_fmt(ctx.h, bad, cnt, 0, fmt) == -1, mis                   # sc16 samples are 4-byte aligned
    assert L.fxrx_submit_fmt(ctx.h, (C.c_void_p * 1)(p2 + 1), cnt, 0, ri.IQ_SC8) == -1   # sc8: 2-byte aligned
    assert L.fxrx_debug_fail(ctx.h, 1, 0) == 0
    assert L.fxrx_submit_fmt(ctx.h, ptr, cnt, 0, fmt) == -4                            # FXRX_ERR_STATE, after the bookkeeping
    assert L.fxrx_inflight(ctx.h) == 0
    same(ctx.results(ctx.process_raw([p2], [len(q) - cut], False, fmt)), ref2, "the same block again")
    a.free(); ctx.close()


def route_ctx(fx, route):
    """RxContext for tests/failing_submit_cases.py: FXRX_INGEST_KERNEL_MAX = route while the context is created (None: the default)"""
    where = {None: "pinned", ROUTE["pinned_kernel"]: "pinned_kernel", ROUTE["pinned_copy"]: "pinned_copy"}[route]
    return make_ctx(fx, where, 1, want_framesyms=True)


@pytest.mark.parametrize("source", fsc.SOURCES)
def test_a_failing_submit_reads_nothing_of_the_callers_buffer(fx, source):
    """tests/failing_submit_cases.py: an injected failure behind the last reservation, nothing in flight; the submitted buffer is
    overwritten at once and the block submitted again from another one -- every host-visible source of a block"""
    fsc.run(fx, lambda route: route_ctx(fx, route), same, source)


@pytest.mark.parametrize("fmt", FMTS)
def test_quantize_against_numpy(fx, fmt):
    import torch
    tx = fx.TxContext()
    xd, _ = fx.synth_streams_device(1, 200_001 + 1, first_stream_id=9, tx=tx)
    xd = xd.reshape(-1)[:200_001]
    xh = xd.cpu().numpy()
    full = ri.FULL_SCALE[fmt]
    clipped = False
    for inv in (0.25 * full, 0.1 * full, 0.3333 * full, 1.9 * full):
        want, wsat = ri.quantize(xh, fmt, inv)
        got, gsat = tx.quantize(xd, fmt, inv)
        assert got.shape == (len(xh), 2) and np.array_equal(got.cpu().numpy(), want) and gsat == wsat, inv
        clipped |= wsat > 0
    assert clipped, "no gain clipped"
    hi = float(np.iinfo(ri.DTYPE[fmt]).max); lo = float(np.iinfo(ri.DTYPE[fmt]).min)
    vals = [0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 0.0, -0.0, np.nan, np.inf, -np.inf, hi, hi + 0.5, hi + 1, lo, lo - 0.5, lo - 1, 1e30, -1e30, 0.49999997, 3.5]
    sp = np.array([complex(a, b) for a, b in zip(vals, vals[::-1])] + [complex(np.nan, 1.0)], np.complex64)
    want, wsat = ri.quantize(sp, fmt, 1.0)
    got, gsat = tx.quantize(torch.from_numpy(sp).cuda(), fmt, 1.0)
    assert np.array_equal(got.cpu().numpy(), want) and gsat == wsat and wsat > 0
    got, gsat = tx.quantize(torch.zeros(0, dtype=torch.complex64, device="cuda"), fmt, 1.0)
    assert got.shape == (0, 2) and gsat == 0
    tx.close()


@pytest.mark.parametrize("fmt", FMTS)
def test_whole_loop_on_the_device(fx, fmt):
    """generate -> channel -> quantise -> fxrx_process_fmt with device pointers: every injected payload recovered"""
    tx = fx.TxContext()
    ns, n = 3, 120_000
    xd, injected = fx.synth_streams_device(ns, n, first_stream_id=70, tx=tx)
    ctx = fx.RxContext(ns)
    qd = []
    for s in range(ns):
        q, sat = tx.quantize(xd[s], fmt, RMS_OF_FULL_SCALE * ri.FULL_SCALE[fmt])
        assert sat == 0
        qd.append(q)
    got = ctx.process(qd)
    for s in range(ns):
        assert len(injected[s]) >= 6
        assert [g["payload"] for g in got if g["stream"] == s and g["payload_valid"]] == [pl for _, pl in injected[s]]
    ctx.close(); tx.close()
