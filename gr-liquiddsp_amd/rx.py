"""Batched receive context: many independent IQ streams per call (BASELINE configs 2-5).

The reference has one flexframesync handle per flex_rx block (lib/flex_rx_impl.cc:49) fed 256 samples
at a time (:212-215); here one context owns the carried state of every stream and each process() call
runs whole blocks of all streams through the HIP kernels.
"""
import ctypes as C
import numpy as np
from . import _ffi

MODE_FLEX_RX, MODE_DETECTOR = 0, 1
IQ_FC32, IQ_SC16, IQ_SC8 = _ffi.IQ_FC32, _ffi.IQ_SC16, _ffi.IQ_SC8


class RxError(RuntimeError):
    pass


def _frame_to_dict(f, copy_syms):
    d = dict(stream=f.stream, start=f.start, cfo_bin=f.cfo_bin, rxy=f.rxy, tau=f.tau, gamma=f.gamma, dphi=f.dphi,
             phi=f.phi, pfb_index=f.pfb_index, pilot_dphi=f.pilot_dphi, pilot_phi=f.pilot_phi,
             pilot_gain=f.pilot_gain, header_valid=f.header_valid, payload_valid=f.payload_valid,
             header=bytes(f.header), evm_db=f.evm_db, rssi_db=f.rssi_db, cfo=f.cfo, evm_sum=f.evm_sum,
             mod_scheme=f.mod_scheme, mod_bps=f.mod_bps, check=f.check, fec0=f.fec0, fec1=f.fec1,
             num_framesyms=f.num_framesyms)
    d["payload"] = C.string_at(f.payload, f.payload_len) if (f.payload and f.payload_len) else b""
    if copy_syms and f.framesyms and f.num_framesyms:
        buf = C.cast(f.framesyms, C.POINTER(C.c_float * (2 * f.num_framesyms))).contents
        d["framesyms"] = np.frombuffer(buf, dtype=np.complex64).copy()
    else:
        d["framesyms"] = None
    d["soft_bits"] = np.frombuffer(C.string_at(f.soft_bits, f.num_soft_bits), np.uint8) if (copy_syms and f.soft_bits and f.num_soft_bits) else None
    return d


def _int_iq_format(s):
    """FXRX_IQ_SC16 / FXRX_IQ_SC8 for an (n, 2) array or tensor of dtype int16 / int8 (SDR-native IQ), else None."""
    if len(getattr(s, "shape", ())) != 2 or s.shape[1] != 2:
        return None
    name = str(s.dtype).replace("torch.", "")
    return {"int16": IQ_SC16, "int8": IQ_SC8}.get(name)


def iq_convert(q, fmt=None, scale=None):
    """Integer IQ of shape (n, 2) -> complex64 on the host by the library's definition (fxrx_iq_convert_host):
    re = float(i_re) * scale, im = float(i_im) * scale; scale defaults to 1/32768 (int16) / 1/128 (int8)."""
    q = np.ascontiguousarray(q)
    fmt = _int_iq_format(q) if fmt is None else fmt
    if fmt not in (IQ_SC16, IQ_SC8):
        raise ValueError("iq_convert: expected an (n, 2) int16 or int8 array")
    scale = (1.0 / 32768.0 if fmt == IQ_SC16 else 1.0 / 128.0) if scale is None else scale
    out = np.empty(len(q), np.complex64)
    if _ffi.lib().fxrx_iq_convert_host(fmt, C.c_float(scale), q.ctypes.data, len(q), out.ctypes.data) != 0:
        raise RxError("fxrx_iq_convert_host failed: %s" % _ffi.lib().fxrx_last_error().decode())
    return out


def marshal_streams(streams):
    """What process() / submit() hand to the C ABI for a list of streams: (keep-alive objects, addresses, sample counts,
    on_device, FXRX_IQ_* format).  (n, 2) int16 / int8 arrays (host) or tensors (device) select sc16 / sc8 -- all streams of a
    block share the format --; everything else goes the float way: complex64 arrays or tensors."""
    on_device = hasattr(streams[0], "data_ptr")
    fmt = _int_iq_format(streams[0])
    if fmt is not None:
        if any(_int_iq_format(s) != fmt or hasattr(s, "data_ptr") != on_device for s in streams):
            raise ValueError("all streams of a block must share one IQ format")
        if on_device:
            keep = [s.contiguous() for s in streams]
            return keep, [s.data_ptr() for s in keep], [s.shape[0] for s in keep], True, fmt
        keep = [np.ascontiguousarray(s) for s in streams]
        return keep, [s.ctypes.data for s in keep], [len(s) for s in keep], False, fmt
    if on_device:
        keep = [s.contiguous() for s in streams]
        return keep, [s.data_ptr() for s in keep], [s.numel() for s in keep], True, IQ_FC32
    keep = [np.ascontiguousarray(s, dtype=np.complex64) for s in streams]
    return keep, [s.ctypes.data for s in keep], [len(s) for s in keep], False, IQ_FC32


class RxContext:
    """fxrx_ctx wrapper.  Raises RxError when the library or a HIP device is missing (no fallback)."""

    def __init__(self, n_streams=1, mode=MODE_FLEX_RX, device=0, threshold=0.0, segment_len=0, want_framesyms=False, equalizer=False, soft_decision=False,
                 soft_header=False, soft_block=False, soft_chain=False, soft_rs=False, soft_rs_fmax=None, soft_rs_chain=False):
        """soft_rs_fmax: None for no bound, else the even bound 0 .. 32 itself (fxrx_config.soft_rs_fmax holds it plus one)"""
        self.L = _ffi.lib()
        cfg = _ffi.ConfigRsChain(device, mode, n_streams, threshold, segment_len, 1 if want_framesyms else 0, 1 if equalizer else 0, 1 if soft_decision else 0,
                                 1 if soft_header else 0, 1 if soft_block else 0, 1 if soft_chain else 0, 1 if soft_rs else 0,
                                 0 if soft_rs_fmax is None else int(soft_rs_fmax) + 1, 1 if soft_rs_chain else 0)
        self.h = self.L.fxrx_create(C.byref(cfg))
        if not self.h:
            raise RxError("fxrx_create failed: %s" % self.L.fxrx_last_error().decode())
        self.n_streams, self.mode, self.want_framesyms = n_streams, mode, want_framesyms
        self._keep = None
        self._inflight_keep = []

    def close(self):
        if getattr(self, "h", None):
            self.L.fxrx_destroy(self.h)
            self.h = None

    __del__ = close

    def reset(self):
        self.L.fxrx_reset(self.h)

    def process_raw(self, ptrs, counts, on_device, fmt=0):
        """ptrs/counts: one address and sample count per stream; fmt: FXRX_IQ_* of the samples.  Returns number of results."""
        n = self.n_streams
        a = (C.c_void_p * n)(*ptrs)
        c = (C.c_uint64 * n)(*counts)
        if fmt == IQ_FC32:
            r = self.L.fxrx_process(self.h, a, c, 1 if on_device else 0)
        else:
            r = self.L.fxrx_process_fmt(self.h, a, c, 1 if on_device else 0, int(fmt))
        if r < 0:
            raise RxError("fxrx_process failed (%d): %s" % (r, self.L.fxrx_last_error().decode()))
        return r

    def set_iq_scale(self, fmt, scale):
        """Scale of an integer IQ format (default 1/32768 for sc16, 1/128 for sc8), from the next submit on."""
        if self.L.fxrx_set_iq_scale(self.h, int(fmt), C.c_float(scale)) != 0:
            raise RxError("fxrx_set_iq_scale: %s" % self.L.fxrx_last_error().decode())

    def set_depth(self, depth):
        """Allow up to `depth` blocks in flight (submit/collect pipelining over three HIP streams)."""
        if self.L.fxrx_set_depth(self.h, depth) != 0:
            raise RxError("fxrx_set_depth failed: %s" % self.L.fxrx_last_error().decode())

    def set_timing(self, level):
        """Stage events per block: 2 all stages, 1 the PLL only, 0 none, -1 automatic (see include/fxrx.h: fxrx_set_timing)."""
        if self.L.fxrx_set_timing(self.h, int(level)) != 0:
            raise RxError("fxrx_set_timing: bad level")

    def prescan_stats(self):
        """Of the last collected block: (speculative segments pre-scanned, those that took a candidate from the table, those that
        fell back to their own scan): see fxrx_debug_prescan_stats."""
        out = (C.c_uint64 * 3)()
        if self.L.fxrx_debug_prescan_stats(self.h, C.byref(out)) != 0:
            raise RxError("fxrx_debug_prescan_stats failed")
        return int(out[0]), int(out[1]), int(out[2])

    def gang_stats(self):
        """(tail launches so far that served more than one block in flight, blocks they carried): see fxrx_debug_gang_stats."""
        out = (C.c_uint64 * 2)()
        if self.L.fxrx_debug_gang_stats(self.h, C.byref(out)) != 0:
            raise RxError("fxrx_debug_gang_stats failed")
        return int(out[0]), int(out[1])

    LATE_REASONS = ("more_plain", "more_rs", "more_batch_frames", "more_batch_items", "more_fb", "late_trellis")

    def late_stats(self):
        """Ten counts: blocks so far whose decoding fxrx_collect had to complete, per reason (LATE_REASONS), then n_dec_plain, n_dec_batch,
        n_dec_rs and n_vb_items of the last collected block: see fxrx_debug_late_stats."""
        out = (C.c_uint64 * 10)()
        if self.L.fxrx_debug_late_stats(self.h, C.byref(out)) != 0:
            raise RxError("fxrx_debug_late_stats failed")
        return tuple(int(v) for v in out)

    def gang_open(self):
        """Blocks in flight whose tails are deferred at this moment: see fxrx_debug_gang_open."""
        n = self.L.fxrx_debug_gang_open(self.h)
        if n < 0:
            raise RxError("fxrx_debug_gang_open failed")
        return int(n)

    def submit_raw(self, ptrs, counts, on_device, fmt=0):
        n = self.n_streams
        a = (C.c_void_p * n)(*ptrs)
        c = (C.c_uint64 * n)(*counts)
        if fmt == IQ_FC32:
            r = self.L.fxrx_submit(self.h, a, c, 1 if on_device else 0)
        else:
            r = self.L.fxrx_submit_fmt(self.h, a, c, 1 if on_device else 0, int(fmt))
        if r < 0:
            raise RxError("fxrx_submit failed (%d): %s" % (r, self.L.fxrx_last_error().decode()))

    def collect_raw(self):
        r = self.L.fxrx_collect(self.h)
        if r < 0:
            raise RxError("fxrx_collect failed (%d): %s" % (r, self.L.fxrx_last_error().decode()))
        return r

    def process(self, streams):
        """streams: list (len n_streams) of numpy complex64 arrays (host) or torch complex64 CUDA tensors -- or, for SDR-native
        integer IQ, of (n, 2) int16 / int8 numpy arrays (host) or torch tensors (device): sc16 / sc8, converted on the device."""
        if len(streams) != self.n_streams:
            raise ValueError("expected %d streams" % self.n_streams)
        keep, ptrs, counts, on_device, fmt = marshal_streams(streams)
        if on_device:
            import torch
            torch.cuda.synchronize()        # inputs produced on torch's stream must be complete
        self._keep = keep
        return self.results(self.process_raw(ptrs, counts, on_device, fmt))

    def submit(self, streams):
        """Pipelined form of process(): enqueue one block (same inputs as process()); collect() returns the oldest block's
        results.  The inputs of up to `depth` blocks in flight are kept alive here."""
        if len(streams) != self.n_streams:
            raise ValueError("expected %d streams" % self.n_streams)
        keep, ptrs, counts, on_device, fmt = marshal_streams(streams)
        if on_device:
            import torch
            torch.cuda.synchronize()
        self.submit_raw(ptrs, counts, on_device, fmt)
        self._inflight_keep.append(keep)

    def collect(self):
        n = self.collect_raw()
        if self._inflight_keep:
            self._keep = self._inflight_keep.pop(0)
        return self.results(n)

    def results(self, n):
        out = []
        f = _ffi.Frame()
        for i in range(n):
            self.L.fxrx_result(self.h, i, C.byref(f))
            out.append(_frame_to_dict(f, self.want_framesyms))
        return out

    def timing(self):
        t = _ffi.Timing()
        self.L.fxrx_last_timing(self.h, C.byref(t))
        return {k: getattr(t, k) for k, _ in _ffi.Timing._fields_}

    def stream_handle(self):
        return self.L.fxrx_stream(self.h)
