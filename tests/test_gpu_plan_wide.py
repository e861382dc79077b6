"""The one-workgroup plan kernel at each width FXRX_PLAN_THREADS may ask for (256, 512, 1024: fx_planfused_kernel<NT>, a tile of 2048 frames
as 8 or 4 consecutive frames a thread, whose records are loaded two frames at a time before the two frames' jobs and host records are
stored).  There are instances for 256 and 512 threads; 1024 has none (a thread's 128 registers do not hold a frame's job and record:
DESIGN.md section 6, wide-workgroup log), the library keeps its default width when asked for it, and the case stays so that an instance
added later is covered.

Every case runs once per width and is compared field for field, and in the counters that come out of the plan header, with the pair in one
workgroup (FXRX_PLAN_FUSED=0) and over two (FXRX_PLAN_GRID=2) -- run once per case and shared by the widths -- and the payloads with what
was sent.  Frame counts: 511 / 512 / 513 and 1023 / 1024 / 1025 are the edges between one and two, and two and three, frames a thread at
512 threads (the last thread's last frame missing; at 1025 a batch of two frames ends and a batch of one follows), and between two / three
and four / five frames at 256; 2047 / 2048 / 2049 are the tile's edge: the last one is a second tile of one frame behind a counting sweep."""
import numpy as np
import pytest

from test_gpu_plan_fused import COUNTERS, CONV_V27, _same, _build, _noise
from test_gpu_plan_onewg import PSK4, PSK8, QAM16, FEC_NONE, GOLAY, RS_M8, GAP, _frame_len, _fit, _run

WIDTHS = (256, 512, 1024)
PAIR = ({"FXRX_PLAN_FUSED": "0"}, {"FXRX_PLAN_GRID": "2"})
COUNTS = (0, 1, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049)
_PAIR_RUNS = {}


def _wide(monkeypatch, width, runner):
    monkeypatch.setenv("FXRX_PLAN_THREADS", str(width))
    return runner({"FXRX_PLAN_FUSED": "1"})


def _against_pair(monkeypatch, case, width, runner):
    """runner(env) -> (frames, counters).  The pair's two runs of `case` are made once; returns this width's frames and counters."""
    if case not in _PAIR_RUNS:
        monkeypatch.delenv("FXRX_PLAN_THREADS", raising=False)
        a, b = (runner(env) for env in PAIR)
        _same(a[0], b[0])
        assert a[1] == b[1]
        _PAIR_RUNS[case] = a
    ref, ref_cnt = _PAIR_RUNS[case]
    got, cnt = _wide(monkeypatch, width, runner)
    _same(ref, got)
    assert cnt == ref_cnt, (width, cnt, ref_cnt)
    return got, cnt


def _sent(specs, seed, corrupt=()):
    """the payloads _build(fx, specs, n, seed, corrupt=corrupt) drew, in frame order"""
    rng = np.random.RandomState(seed)
    out = []
    for i, (_, _, _, plen) in enumerate(specs):
        out.append(rng.randint(0, 256, plen).astype(np.uint8).tobytes())
        if i in corrupt:
            rng.choice([-1.0, 1.0], 300); rng.choice([-1.0, 1.0], 300)
    return out


@pytest.fixture(scope="module")
def short_frames(fx):
    """2049 of the shortest frames there are (1-byte payloads) back to back, from the device-side generator"""
    import torch
    step = _frame_len(fx, (PSK4, CONV_V27, FEC_NONE, 1)) + GAP
    xd, injected = fx.synth_streams_device(1, max(COUNTS) * step, first_stream_id=78, payload_len=1, gap=GAP)
    torch.cuda.synchronize()
    assert len(injected[0]) == max(COUNTS)
    return xd[0], injected[0], step


@pytest.mark.gpu
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("count", COUNTS)
def test_frame_counts_at_every_width(fx, monkeypatch, short_frames, count, width):
    """One block: 4000 quiet samples, `count` whole frames, 4000 quiet samples."""
    import torch
    xd, injected, step = short_frames
    quiet = torch.zeros(4000, dtype=torch.complex64, device=xd.device)
    x = torch.cat([quiet, xd[:count * step], quiet]).contiguous()
    torch.cuda.synchronize()
    blocks = [[(x.data_ptr(), x.numel())]]
    got, cnt = _against_pair(monkeypatch, ("count", count), width, lambda env: _run(fx, monkeypatch, env, blocks, on_device=True))
    assert len(got) == count
    assert all(g["payload_valid"] and g["payload"] == pl for g, (_, pl) in zip(got, injected))
    assert (cnt["payload_symbols"] > 0) == (count > 0) and (cnt["vb_blocks"] > 0) == (count > 0)


@pytest.mark.gpu
@pytest.mark.parametrize("width", WIDTHS)
def test_every_list_and_padding_run_in_one_block(fx, monkeypatch, width):
    """The block of test_gpu_plan_onewg.py's case of the same name: three modulation classes, batch-path frames, a Reed-Solomon frame, frames
    without an inner convolutional code, and two frames whose header fails."""
    specs = [(PSK4, CONV_V27, FEC_NONE, 200), (QAM16, CONV_V27, FEC_NONE, 333), (PSK8, CONV_V27, FEC_NONE, 64), (PSK4, CONV_V27, RS_M8, 150),
             (PSK4, CONV_V27, FEC_NONE, 90), (QAM16, FEC_NONE, FEC_NONE, 120), (PSK8, FEC_NONE, GOLAY, 77), (PSK4, CONV_V27, FEC_NONE, 1),
             (QAM16, CONV_V27, FEC_NONE, 500), (PSK8, CONV_V27, FEC_NONE, 17), (PSK4, CONV_V27, FEC_NONE, 31)]
    corrupt = (4, 9)
    x = _build(fx, specs, _fit(fx, specs), 31, corrupt=corrupt)
    blocks = [[(x.ctypes.data, len(x))]]
    got, cnt = _against_pair(monkeypatch, "every list", width, lambda env: _run(fx, monkeypatch, env, blocks, want_framesyms=True))
    assert len(got) == len(specs) and [i for i, g in enumerate(got) if not g["header_valid"]] == list(corrupt)
    for i, (g, pl) in enumerate(zip(got, _sent(specs, 31, corrupt))):
        assert i in corrupt or (g["payload_valid"] and g["payload"] == pl), i
    ok = [g for g in got if g["header_valid"]]
    assert {g["mod_scheme"] for g in ok} == {PSK4, PSK8, QAM16}
    assert any(g["fec1"] == RS_M8 for g in ok) and any(g["fec0"] == FEC_NONE for g in ok) and cnt["vb_blocks"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("width", WIDTHS)
def test_three_streams_with_none_one_and_several_frames(fx, monkeypatch, width):
    n = 60_000
    spec1, spec2 = [(PSK4, CONV_V27, FEC_NONE, 300)], [(PSK4, CONV_V27, FEC_NONE, 40), (QAM16, CONV_V27, FEC_NONE, 64)] * 3
    xs = [_noise(n, 41), _build(fx, spec1, n, 42), _build(fx, spec2, n, 43)]
    blocks = [[(x.ctypes.data, len(x)) for x in xs]]
    got, _ = _against_pair(monkeypatch, "three streams", width, lambda env: _run(fx, monkeypatch, env, blocks, want_framesyms=True))
    assert [sum(1 for g in got if g["stream"] == s) for s in range(3)] == [0, 1, 6]
    sent = _sent(spec1, 42) + _sent(spec2, 43)
    assert all(g["payload_valid"] and g["payload"] == pl for g, pl in zip(got, sent))


@pytest.mark.gpu
@pytest.mark.parametrize("width", WIDTHS)
def test_detector_mode_block(fx, monkeypatch, width):
    """detect = 1: no frame has a payload stage, every list is empty, and every detection still gets its record."""
    xs = [_build(fx, [(PSK4, CONV_V27, FEC_NONE, 64)] * 5, 40_000, 51), _noise(40_000, 52), _build(fx, [(QAM16, CONV_V27, FEC_NONE, 10)] * 3, 40_000, 53)]
    blocks = [[(x.ctypes.data, len(x)) for x in xs]]
    got, cnt = _against_pair(monkeypatch, "detector", width, lambda env: _run(fx, monkeypatch, env, blocks, mode=fx.MODE_DETECTOR, threshold=0.45))
    assert cnt["payload_symbols"] == 0 and cnt["vb_blocks"] == 0
    assert sum(1 for g in got if g["stream"] == 0) >= 5 and sum(1 for g in got if g["stream"] == 2) >= 3 and all(g["stream"] != 1 for g in got)
