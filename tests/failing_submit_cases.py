"""What a failing fxrx_submit may still read of the caller's buffers: nothing (include/fxrx.h, "Failure semantics").  Shared by
tests/test_gpu_boundary.py and tests/test_gpu_ingest.py.

One capture of six frames (payloads of 300 bytes), cut in two blocks of a continuing stream, from each host-visible source of
a block: float IQ in pageable and in page-locked memory, sc16 in page-locked memory through the conversion kernel and through the
copy engines, sc16 in pageable memory.  The first half is processed (or left in flight); a submit of the second half fails -- an
injected failure behind the last reservation, or a batch too large for the arenas --; the submitted buffer is overwritten AT ONCE
with another capture's samples; the true second half follows from a fresh buffer.  Every result must equal, field for field and
float for float by bit pattern, what a context that never failed gives for the same samples resident on the device as float.
(An upload enqueued by the failing call would still be reading the buffer while it is overwritten; whether it would lose that
race is a matter of timing, so this pins the contract and does not prove a race.)"""
import ctypes as C
import numpy as np

import ref_ingest as ri
from test_ingest import capture, quantised

SOURCES = ["fc32_pageable", "fc32_pinned", "sc16_pinned_kernel", "sc16_pinned_copy", "sc16_pageable"]
ROUTE = {"sc16_pinned_kernel": str(1 << 40), "sc16_pinned_copy": "0"}        # FXRX_INGEST_KERNEL_MAX when the context is created


class HostBuf:
    """bytes in page-locked (fxrx_pinned_alloc) or pageable host memory, 16-byte aligned"""

    def __init__(self, fx, data, pinned):
        raw = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        self.L, self.pinned = fx.lib(), pinned
        if pinned:
            self.ptr = self.L.fxrx_pinned_alloc(len(raw))
            assert self.ptr, self.L.fxrx_last_error()
            self.a = np.frombuffer((C.c_ubyte * len(raw)).from_address(self.ptr), np.uint8)
        else:
            self.keep = np.empty(len(raw) + 16, np.uint8)
            off = -self.keep.ctypes.data % 16
            self.a = self.keep[off:off + len(raw)]
            self.ptr = self.a.ctypes.data
        self.write(raw)

    def write(self, data):
        raw = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        self.a[:len(raw)] = raw

    def free(self):
        self.a = None
        if self.pinned:
            self.L.fxrx_pinned_free(self.ptr)


_inputs = {}


def inputs(fx):
    """(integer capture, another one of the same length, the cut, the never-failed results of both blocks): made once"""
    if not _inputs:
        import torch
        q = quantised(capture(fx, n_frames=6, payload_len=300, stream_id=41)[0], ri.IQ_SC16)[0]
        other = quantised(capture(fx, n_frames=6, payload_len=300, stream_id=43)[0], ri.IQ_SC16)[0]
        assert q.shape == other.shape and not np.array_equal(q, other)
        cut = len(q) // 2 + 77
        ref_ctx = fx.RxContext(1, want_framesyms=True)
        ref = [ref_ctx.process([torch.from_numpy(fx.iq_convert(part)).cuda()]) for part in (q[:cut], q[cut:])]
        ref_ctx.close()
        assert len(ref[0]) + len(ref[1]) == 6 and all(r["payload_valid"] for r in ref[0] + ref[1])
        _inputs.update(q=q, other=other, cut=cut, ref=ref)
    return _inputs["q"], _inputs["other"], _inputs["cut"], _inputs["ref"]


def run(fx, make_ctx, same, source, how="injected", in_flight=False):
    """make_ctx(route or None) -> RxContext(1, want_framesyms=True); same: exact comparison of two result lists"""
    L = fx.lib()
    q, other, cut, ref = inputs(fx)
    flt, pinned = source.startswith("fc32"), "pinned" in source
    fmt = ri.IQ_FC32 if flt else ri.IQ_SC16
    as_source = (lambda part: fx.iq_convert(part)) if flt else (lambda part: part)
    ctx = make_ctx(ROUTE.get(source))
    if in_flight:
        ctx.set_depth(2)
    first, failed, again = (HostBuf(fx, as_source(part), pinned) for part in (q[:cut], q[cut:], q[cut:]))
    n2 = len(q) - cut
    if in_flight:
        ctx.submit_raw([first.ptr], [cut], False, fmt)
    else:
        same(ctx.results(ctx.process_raw([first.ptr], [cut], False, fmt)), ref[0], "first block, " + source)
    ptr = (C.c_void_p * 1)(failed.ptr)
    if how == "injected":
        assert L.fxrx_debug_fail(ctx.h, 1, 0) == 0
        assert L.fxrx_submit_fmt(ctx.h, ptr, (C.c_uint64 * 1)(n2), 0, fmt) == -4       # FXRX_ERR_STATE
        assert b"injected" in L.fxrx_last_error()
    else:
        assert L.fxrx_submit_fmt(ctx.h, ptr, (C.c_uint64 * 1)(1 << 34), 0, fmt) == -1  # FXRX_ERR_ARG (never read: far more than the buffer holds)
        assert b"too large" in L.fxrx_last_error()
    failed.write(as_source(other[cut:]))                                               # at once: nothing may be reading it
    assert L.fxrx_inflight(ctx.h) == (1 if in_flight else 0)
    if in_flight:
        ctx.submit_raw([again.ptr], [n2], False, fmt)
        same(ctx.results(ctx.collect_raw()), ref[0], "first block, " + source)
        same(ctx.results(ctx.collect_raw()), ref[1], "second block after a failed submit, " + source)
    else:
        same(ctx.results(ctx.process_raw([again.ptr], [n2], False, fmt)), ref[1], "second block after a failed submit, " + source)
    ctx.close()
    for b in (first, failed, again):
        b.free()
