"""fx_txenc_kernel / fx_txgen_kernel (TxContext.generate), the host generator (FrameGen) and the synthetic sources built on
them against tests/ref_framegen.py, the float64 statement of the frame generator, on the frames of tests/framegen_cases.py.
Bound: ref_framegen.sample_tol(dt) per sample component (derived there); lengths and the zeros around the frames exactly."""
import numpy as np
import pytest

import framegen_cases as FC
import ref_framegen as G

pytestmark = pytest.mark.gpu

TWO_PI = 6.283185307179586


@pytest.fixture(scope="module")
def refs():
    return FC.reference_frames()


def _generate(fx):
    """(samples of the whole case list in one TxContext.generate into a zeroed buffer, [(offset, frame_len)])"""
    import torch
    tx = fx.TxContext()
    lay, total = FC.layout(lambda c: tx.frame_len(FC.tx_desc(c)))
    out = torch.zeros(total, dtype=torch.complex64, device="cuda")
    torch.cuda.synchronize()
    tx.generate([FC.tx_desc(c, off) for off, c in lay], out.data_ptr(), out.numel())
    y = out.cpu().numpy()
    lens = [tx.frame_len(FC.tx_desc(c)) for _, c in lay]
    tx.close()
    return y, [(off, n) for (off, _), n in zip(lay, lens)]


@pytest.fixture(scope="module")
def gpu_encoded(fx):
    return _generate(fx)


def _check_frames(y, spans, refs):
    """every frame against the reference, zeros elsewhere; returns (worst error, its case)"""
    worst, who, bad = 0.0, None, []
    covered = np.zeros(len(y), bool)
    for (off, n), c, ref in zip(spans, FC.cases(), refs):
        assert n == len(ref), (c["tag"], n, len(ref))
        e = G.compare(ref, y[off:off + n])
        if not e <= G.sample_tol(c["dt"]):
            bad.append((c["tag"], c["mod"], c["fec0"], c["fec1"], c["check"], len(c["payload"]), c["dt"], e))
        if e >= worst:
            worst, who = e, c
        covered[off:off + n] = True
    assert not bad, bad[:10]
    assert not np.any(y[~covered].view(np.uint32)), "samples outside the frames are not exactly zero"
    return worst, who


def test_batched_generator_gpu_encoding(gpu_encoded, refs):
    y, spans = gpu_encoded
    assert {off % 2 for off, _ in spans} == {0, 1}
    worst, c = _check_frames(y, spans, refs)
    print("\nreference vs fxtx_generate: %d frames, worst sample error %.3g (%s mod %d fec %d/%d check %d n %d dt %g)" % (
        len(spans), worst, c["tag"], c["mod"], c["fec0"], c["fec1"], c["check"], len(c["payload"]), c["dt"]))
    assert 4.0 * worst <= min(G.sample_tol(d) for d in G.DTS)
    m = G.MEASURED["gpu"]                           # the recorded figure is this run's, rounded up: it cannot drift
    assert 0.5 * m <= worst <= m, ("ref_framegen.MEASURED['gpu'] is not this run's", worst)


def test_batched_generator_host_encoding(fx, gpu_encoded, refs, monkeypatch):
    monkeypatch.setenv("FXTX_HOST_ENCODE", "1")
    y, spans = _generate(fx)
    _check_frames(y, spans, refs)
    assert spans == gpu_encoded[1] and np.array_equal(y.view(np.uint32), gpu_encoded[0].view(np.uint32))


def test_single_frame_generator(fx, refs):
    cs = FC.cases()
    worst = 0.0
    for i in FC.subset(60):
        c = cs[i]
        g = fx.FrameGen(c["mod"], c["fec0"], c["fec1"], c["check"])
        got = g.frame(c["payload"], header=c["header"], dt=c["dt"])
        g.close()
        e = G.compare(refs[i], got)
        assert e <= G.sample_tol(c["dt"]), (i, c["tag"], c["mod"], c["fec0"], c["fec1"], len(got), len(refs[i]), e)
        worst = max(worst, e)
    print("\nreference vs FrameGen: 60 frames, worst sample error %.3g" % worst)


@pytest.mark.parametrize("mod,fec0,fec1,check,plen,delay", [(2, 11, 1, 5, 100, 0.25), (29, 16, 7, 6, 150, -0.37), (11, 1, 27, 3, 61, 0.0)])
def test_synth_stream_frames_are_the_references(fx, mod, fec0, fec1, check, plen, delay):
    """synth_stream at cfo = phase = 0 (its rotation is then exactly 1) and snr_db = 300: sigma = 7e-16, and 8 sigma is
    allowed on top of the sample bound (the noise draw is Gaussian)."""
    n, gap, lead = 9000, 77, 11
    x, frames = fx.synth_stream(n, stream_id=5, mod=mod, fec0=fec0, fec1=fec1, check=check, payload_len=plen, gap=gap, snr_db=300.0,
                                cfo=0.0, phase=0.0, delay=delay, lead=lead)
    assert len(frames) >= 2 and frames[0][0] == lead
    ref = np.zeros(n, np.complex128)
    for p, pl in frames:
        f = G.frame(np.frombuffer(pl, np.uint8), mod, fec0, fec1, check, dt=delay)
        ref[p:p + len(f)] = f
    assert frames[1][0] == lead + G.frame_len(plen, mod, fec0, fec1, check) + gap
    assert G.compare(ref, x) <= G.sample_tol(delay) + 8.0 * np.sqrt(0.5e-30)


def _units(rad):
    """fxtx_apply_channel's rounding of an angle (passed as float32) to a 32-bit phase (tests/test_gpu_channel_range.py)"""
    return int(np.rint(float(np.float32(rad)) * (4294967296.0 / TWO_PI))) % (1 << 32)


def test_synth_streams_device_frames_are_the_references(fx):
    """synth_streams_device at snr_db = 300 (sigma = 7e-16): each stream is the reference's frames at the reported offsets,
    turned by the stream's carrier (the channel draws are MT19937(0xC0FFEE + id): cfo, phase, delay; angles on the channel's
    32-bit grid).  Bound: the sample bound plus the device channel's own 1e-6 |x| (test_device_channel_rotation_against_float64)."""
    props = {40: dict(mod=2, fec0=11, fec1=1, check=5, payload_len=90), 41: dict(mod=28, fec0=17, fec1=10, check=6, payload_len=131),
             42: dict(mod=10, fec0=1, fec1=1, check=1, payload_len=64)}
    n, gap = 8000, 33
    out, injected = fx.synth_streams_device(3, n, first_stream_id=40, props=lambda sid: props[sid], gap=gap, snr_db=300.0)
    y = out.cpu().numpy()
    idx = np.arange(n)
    for s, sid in enumerate(sorted(props)):
        p = props[sid]
        crng = np.random.RandomState((0xC0FFEE + sid) & 0x7FFFFFFF)
        cfo, phase, delay = crng.uniform(-0.05, 0.05), crng.uniform(-np.pi, np.pi), crng.uniform(-0.5, 0.5)
        assert len(injected[s]) >= 2
        ref = np.zeros(n, np.complex128)
        for off, pl in injected[s]:
            assert len(pl) == p["payload_len"]
            f = G.frame(np.frombuffer(pl, np.uint8), p["mod"], p["fec0"], p["fec1"], p["check"], dt=delay)
            ref[off:off + len(f)] = f
        assert injected[s][1][0] == G.frame_len(p["payload_len"], p["mod"], p["fec0"], p["fec1"], p["check"]) + gap
        ang = ((_units(phase) + _units(cfo) * idx) % (1 << 32)).astype(np.float64) * (TWO_PI / 4294967296.0)
        ref = ref * np.exp(1j * ang)
        tol = G.sample_tol(delay) + 1e-6 * float(np.abs(ref).max()) + 8.0 * np.sqrt(0.5e-30)
        e = G.compare(ref, y[s])
        print("stream %d: worst sample error %.3g (bound %.3g)" % (sid, e, tol))
        assert e <= tol, (sid, e, tol)
