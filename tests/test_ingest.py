"""Integer IQ (sc16 / sc8) in the batched receive API: what needs no GPU.

The conversion's definition on the host (fxrx_iq_convert_host) against the numpy statement in tests/ref_ingest.py, the sample
sizes, the Python dispatch, and a channel-quality check with the CPU oracle, so that the inputs tests/test_gpu_ingest.py
uses are known to be decodable at the chosen signal level."""
import ctypes as C
import numpy as np
import pytest

import ref_ingest as ri

# Signal level of the quantised test captures, here and in tests/test_gpu_ingest.py: RMS of a complex sample at 1/4 of full
# scale.  sc8 then has about 38 dB of signal to quantisation noise (18 dB below the 20 dB channel noise) and clips beyond
# 4 sigma per component.
RMS_OF_FULL_SCALE = 0.25


def capture(fx, n_frames=3, payload_len=1024, stream_id=11, cfo=0.02):
    """config-2-style stream: PSK4 r1/2, CRC-24, 20 dB, a few frames (unit sample power)."""
    flen = fx.lib().fxrx_gen_frame_len(2, 5, 11, 1, payload_len)
    return fx.synth_stream(300 + n_frames * (flen + 256), stream_id=stream_id, payload_len=payload_len, cfo=cfo, lead=300)


def quantised(x, fmt, level=RMS_OF_FULL_SCALE):
    """x (unit power) at an RMS of `level` of full scale, quantised by the numpy reference."""
    return ri.quantize(x, fmt, level * ri.FULL_SCALE[fmt])


def test_sample_bytes(fx):
    L = fx.lib()
    assert [L.fxrx_iq_sample_bytes(f) for f in (0, 1, 2, 3, -1, 99)] == [8, 4, 2, 0, 0, 0]


@pytest.mark.parametrize("fmt", [ri.IQ_SC16, ri.IQ_SC8])
def test_convert_host_equals_numpy_on_every_value(fx, fmt):
    L = fx.lib()
    info = np.iinfo(ri.DTYPE[fmt])
    v = np.arange(info.min, info.max + 1).astype(ri.DTYPE[fmt])
    q = np.stack([np.concatenate([v, v[::-1]]), np.concatenate([v[::-1], v])], axis=1)      # every value in both components
    q = np.ascontiguousarray(q)
    for scale in (ri.DEFAULT_SCALE[fmt], 1.0 / 3.0e4, 0.0123456789):
        out = np.full(len(q), np.nan, np.complex64)
        assert L.fxrx_iq_convert_host(fmt, C.c_float(scale), q.ctypes.data, len(q), out.ctypes.data) == 0
        want = ri.to_float(q, scale)
        assert np.array_equal(out.view(np.uint32), want.view(np.uint32)), scale
        assert np.array_equal(fx.iq_convert(q, scale=scale).view(np.uint32), want.view(np.uint32))
    assert set(np.unique(q[:, 0])) == set(v) and set(np.unique(q[:, 1])) == set(v)


def test_convert_host_fc32_copies_and_bad_arguments(fx):
    L = fx.lib()
    x = (np.arange(10, dtype=np.float32) * np.float32(0.37)).view(np.complex64)
    out = np.zeros(5, np.complex64)
    assert L.fxrx_iq_convert_host(0, C.c_float(1.0), x.ctypes.data, 5, out.ctypes.data) == 0
    assert np.array_equal(out.view(np.uint32), x.view(np.uint32))
    q = np.zeros((4, 2), np.int16); o = np.zeros(4, np.complex64)
    assert L.fxrx_iq_convert_host(3, C.c_float(1.0), q.ctypes.data, 4, o.ctypes.data) == -1         # FXRX_ERR_ARG
    assert L.fxrx_iq_convert_host(-1, C.c_float(1.0), q.ctypes.data, 4, o.ctypes.data) == -1
    assert L.fxrx_iq_convert_host(1, C.c_float(1.0), None, 4, o.ctypes.data) == -1
    assert L.fxrx_iq_convert_host(1, C.c_float(1.0), q.ctypes.data, 4, None) == -1
    assert L.fxrx_iq_convert_host(1, C.c_float(1.0), None, 0, None) == 0                             # nothing to do
    assert L.fxrx_set_iq_scale(None, 1, C.c_float(1.0)) == -1


def test_reference_quantiser_rules():
    x = np.array([0.5 + 1.5j, 2.5 - 0.5j, -1.5 - 2.5j, complex(np.nan, 1e9), complex(-np.inf, np.inf), 127.49 + 127.5j, -128.5 - 129j], np.complex64)
    q, sat = ri.quantize(x, ri.IQ_SC8, 1.0)
    assert q.tolist() == [[0, 2], [2, 0], [-2, -2], [0, 127], [-128, 127], [127, 127], [-128, -128]]      # ties to even, NaN -> 0
    assert sat == 1 + 2 + 1 + 1                                  # 1e9 | -inf, +inf | 127.5 -> 128 | -129 (-128.5 -> -128 is in range)


@pytest.mark.parametrize("fmt", [ri.IQ_SC16, ri.IQ_SC8])
def test_quantised_capture_is_decodable_by_the_oracle(fx, oracle, fmt):
    """The GPU tests' inputs, before anyone spends GPU time on them: every injected frame found with a valid, correct payload."""
    from parity_util import oracle_frames
    x, injected = capture(fx)
    assert len(injected) == 3
    q, sat = quantised(x, fmt)
    assert sat == 0, "clipping at 1/4 full scale"
    y = ri.to_float(q, 1.0 / (RMS_OF_FULL_SCALE * ri.FULL_SCALE[fmt]))                  # back to unit power
    fr = oracle_frames(oracle, y)
    assert len(fr) == len(injected)
    for f, (_, pl) in zip(fr, injected):
        assert f.header_valid and f.payload_valid and f.payload == pl
    # and at the default scale (signal at 1/4 amplitude): the receiver is gain invariant
    fr = oracle_frames(oracle, ri.to_float(q))
    assert [f.payload for f in fr if f.payload_valid] == [pl for _, pl in injected]


def test_rx_dispatch_by_dtype_and_shape(fx):
    """(n, 2) int16 -> FXRX_IQ_SC16, (n, 2) int8 -> FXRX_IQ_SC8, everything else the float way (no device involved)."""
    m = fx.marshal_streams
    q16 = np.arange(20, dtype=np.int16).reshape(10, 2); q8 = np.arange(14, dtype=np.int8).reshape(7, 2)
    keep, ptrs, counts, on_device, fmt = m([q16, q16[:3]])
    assert (fmt, on_device, counts) == (fx.IQ_SC16, False, [10, 3]) and ptrs[0] == keep[0].ctypes.data and keep[0].dtype == np.int16
    keep, ptrs, counts, on_device, fmt = m([q8])
    assert (fmt, on_device, counts) == (fx.IQ_SC8, False, [7]) and keep[0].dtype == np.int8
    keep, ptrs, counts, on_device, fmt = m([q16[::2]])                                   # a strided view is made contiguous
    assert fmt == fx.IQ_SC16 and counts == [5] and keep[0].flags["C_CONTIGUOUS"] and np.array_equal(keep[0], q16[::2])
    x = np.zeros(9, np.complex64)
    keep, ptrs, counts, on_device, fmt = m([x])
    assert (fmt, on_device, counts) == (fx.IQ_FC32, False, [9]) and keep[0].dtype == np.complex64
    for other in (np.zeros(9, np.complex128), np.zeros(9, np.int16), np.zeros((9, 2), np.int32), np.zeros((9, 2), np.float32)[:, 0]):
        keep, _, counts, _, fmt = m([other])                                              # as before: cast to complex64
        assert fmt == fx.IQ_FC32 and keep[0].dtype == np.complex64 and counts == [9]
    with pytest.raises(ValueError):
        m([q16, q8])
    with pytest.raises(ValueError):
        m([q16, x])
    assert fx._ffi.lib().fxrx_submit_fmt.argtypes[-1] is C.c_int and fx._ffi.lib().fxrx_process_fmt.restype is C.c_int
