"""numpy statement of integer IQ in both directions, from the definitions in include/fxrx.h.

Receive side: a sample is re = (float)i_re * scale, im = (float)i_im * scale -- one exact int -> binary32 conversion and
one binary32 multiply.  Generator side: q = saturate(rint(x * inv_scale)) per component, round half to even, NaN -> 0."""
import numpy as np

IQ_FC32, IQ_SC16, IQ_SC8 = 0, 1, 2
DTYPE = {IQ_SC16: np.int16, IQ_SC8: np.int8}
DEFAULT_SCALE = {IQ_SC16: 1.0 / 32768.0, IQ_SC8: 1.0 / 128.0}
FULL_SCALE = {IQ_SC16: 32768.0, IQ_SC8: 128.0}


def to_float(q, scale=None, fmt=None):
    """(n, 2) int16 / int8 -> complex64."""
    q = np.ascontiguousarray(q)
    fmt = (IQ_SC16 if q.dtype == np.int16 else IQ_SC8) if fmt is None else fmt
    assert q.dtype == DTYPE[fmt] and q.ndim == 2 and q.shape[1] == 2
    scale = DEFAULT_SCALE[fmt] if scale is None else scale
    f = q.astype(np.float32) * np.float32(scale)
    return np.ascontiguousarray(f).view(np.complex64).reshape(-1)


def quantize(x, fmt, inv_scale):
    """complex64 -> ((n, 2) int16 / int8, number of clamped components)."""
    f = np.ascontiguousarray(x, dtype=np.complex64).view(np.float32).reshape(-1, 2)
    info = np.iinfo(DTYPE[fmt])
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.rint(f * np.float32(inv_scale))
    saturated = int(np.count_nonzero((r > info.max) | (r < info.min)))
    r = np.where(np.isnan(r), np.float32(0.0), np.clip(r, info.min, info.max))
    return r.astype(DTYPE[fmt]), saturated
