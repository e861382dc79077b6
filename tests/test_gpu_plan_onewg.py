"""The one-workgroup plan kernel (fx_planfused_kernel: sizes of all frames of a tile in one round of loads, one scan per tile, counts and
list cursors in LDS, item runs written 16 lanes per frame) at the smallest shapes where it can go wrong, each laid out three ways as in
test_gpu_plan_fused.py -- the kernel itself, the two-kernel path in one workgroup (FXRX_PLAN_FUSED=0) and over two workgroups
(FXRX_PLAN_GRID=2) -- and compared field for field between the three, in the plan header's counters, and with the CPU oracle.

A thread owns ceil(frames / 256) consecutive frames of a tile, so 255 / 256 / 257 frames are the edge between one and two frames per
thread with the last thread's second frame missing; 16 frames share a round of the item writes.

Not covered here: the rule that demotes frames at the end of the trellis arena.  No knob shrinks the arena (it is priced from the block's
samples), so no case is added; the traffic-built overflow (LONG_TRELLIS of shift_cases.py, run by test_gpu_traffic_shift.py) goes through this kernel."""
import numpy as np
import pytest

from parity_util import oracle_frames, compare_frames
from test_gpu_plan_fused import MODES, COUNTERS, CONV_V27, _same, _build, _noise, _three_ways

PSK4, PSK8, QAM16, FEC_NONE, GOLAY, RS_M8 = 2, 3, 27, 1, 7, 27
GAP = 256


def _frame_len(fx, spec):
    mod, fec0, fec1, plen = spec
    g = fx.FrameGen(mod, fec0, fec1, fx.CRC_24)
    n = len(g.frame(np.zeros(plen, np.uint8), dt=0.1))
    g.close()
    return n


def _fit(fx, specs):
    """samples a stream needs for one frame per spec as _build lays them out, and a tail of noise"""
    lens = {s: _frame_len(fx, s) for s in set(specs)}
    return 300 + sum(lens[s] + GAP for s in specs) + 4000


def _build_alike(fx, spec, count, seed, snr_db=20.0):
    """_build for `count` frames of one kind, from one generator (a generator per frame costs more than the frame)"""
    mod, fec0, fec1, plen = spec
    rng = np.random.RandomState(seed)
    g = fx.FrameGen(mod, fec0, fec1, fx.CRC_24)
    frames = [np.array(g.frame(rng.randint(0, 256, plen).astype(np.uint8), dt=0.1), np.complex64) for _ in range(count)]
    g.close()
    n = 300 + sum(len(fr) + GAP for fr in frames) + 4000
    x = np.zeros(n, np.complex64)
    p = 300
    for fr in frames:
        x[p:p + len(fr)] = fr
        p += len(fr) + GAP
    x *= np.exp(1j * (0.01 * np.arange(n, dtype=np.float64) + 0.3)).astype(np.complex64)
    x += np.float32(np.sqrt(0.5 * 10.0 ** (-snr_db / 10.0))) * rng.standard_normal(2 * n).astype(np.float32).view(np.complex64)
    return x


@pytest.mark.gpu
@pytest.mark.parametrize("count", [0, 1, 255, 256, 257])
def test_frame_counts_around_one_frame_per_thread(fx, oracle, monkeypatch, count):
    """1-byte payloads (the shortest frames there are) keep the 257-frame stream at some 400 k samples."""
    x = _build_alike(fx, (PSK4, CONV_V27, FEC_NONE, 1), count, 20 + count) if count else _noise(60_000, 20)
    got, cnt = _three_ways(fx, oracle, monkeypatch, [x])
    assert len(got) == count and all(g["payload_valid"] for g in got)
    assert (cnt["payload_symbols"] > 0) == (count > 0) and (cnt["vb_blocks"] > 0) == (count > 0)


@pytest.mark.gpu
def test_every_list_and_padding_run_in_one_block(fx, oracle, monkeypatch):
    """Three modulation classes; batch-path frames, a Reed-Solomon frame (its own decode list), frames without an inner convolutional
    code (the plain list, no trellis items), and two frames whose header fails (jobs and records with pad_ = 0 / nsym = 0, in no list)."""
    specs = [(PSK4, CONV_V27, FEC_NONE, 200), (QAM16, CONV_V27, FEC_NONE, 333), (PSK8, CONV_V27, FEC_NONE, 64), (PSK4, CONV_V27, RS_M8, 150),
             (PSK4, CONV_V27, FEC_NONE, 90), (QAM16, FEC_NONE, FEC_NONE, 120), (PSK8, FEC_NONE, GOLAY, 77), (PSK4, CONV_V27, FEC_NONE, 1),
             (QAM16, CONV_V27, FEC_NONE, 500), (PSK8, CONV_V27, FEC_NONE, 17), (PSK4, CONV_V27, FEC_NONE, 31)]
    got, cnt = _three_ways(fx, oracle, monkeypatch, [_build(fx, specs, _fit(fx, specs), 31, corrupt=(4, 9))])
    assert len(got) == len(specs) and sum(1 for g in got if not g["header_valid"]) == 2
    ok = [g for g in got if g["header_valid"]]
    assert {g["mod_scheme"] for g in ok} == {PSK4, PSK8, QAM16} and all(g["payload_valid"] for g in ok)
    assert any(g["fec1"] == RS_M8 for g in ok) and any(g["fec0"] == FEC_NONE for g in ok) and cnt["vb_blocks"] > 0


@pytest.mark.gpu
def test_three_streams_with_none_one_and_several_frames(fx, oracle, monkeypatch):
    n = 60_000
    xs = [_noise(n, 41), _build(fx, [(PSK4, CONV_V27, FEC_NONE, 300)], n, 42), _build(fx, [(PSK4, CONV_V27, FEC_NONE, 40), (QAM16, CONV_V27, FEC_NONE, 64)] * 3, n, 43)]
    got, _ = _three_ways(fx, oracle, monkeypatch, xs)
    assert [sum(1 for g in got if g["stream"] == s) for s in range(3)] == [0, 1, 6] and all(g["payload_valid"] for g in got)


def _run(fx, monkeypatch, env, blocks, depth=1, on_device=False, **ctx_args):
    """As _run of test_gpu_plan_fused.py, for any kind of context; blocks hold (address, samples) per stream."""
    for k in ("FXRX_PLAN_FUSED", "FXRX_PLAN_GRID"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ctx = fx.RxContext(len(blocks[0]), **ctx_args)
    ctx.set_depth(depth)
    got, cnt, inflight = [], dict.fromkeys(COUNTERS, 0), 0

    def collect():
        got.extend(ctx.results(ctx.collect_raw()))
        tm = ctx.timing()
        for k in COUNTERS:
            cnt[k] += tm[k]
    for b in blocks:
        if inflight == depth:
            collect(); inflight -= 1
        ctx.submit_raw([p for p, _ in b], [n for _, n in b], on_device); inflight += 1
    while inflight:
        collect(); inflight -= 1
    ctx.close()
    return got, cnt


@pytest.mark.gpu
def test_detector_mode_writes_records_and_empty_lists(fx, oracle, monkeypatch):
    """detect = 1: no frame has a payload stage, every list is empty, and every detection still gets its record."""
    xs = [_build(fx, [(PSK4, CONV_V27, FEC_NONE, 64)] * 5, 40_000, 51), _noise(40_000, 52), _build(fx, [(QAM16, CONV_V27, FEC_NONE, 10)] * 3, 40_000, 53)]
    blocks = [[(x.ctypes.data, len(x)) for x in xs]]
    runs = [_run(fx, monkeypatch, env, blocks, mode=fx.MODE_DETECTOR, threshold=0.45) for _, env in MODES]
    ref, ref_cnt = runs[0]
    for got, cnt in runs[1:]:
        _same(ref, got)
        assert cnt == ref_cnt
    assert ref_cnt["payload_symbols"] == 0 and ref_cnt["vb_blocks"] == 0
    for s, x in enumerate(xs):
        od, mine = oracle.Detector(0.45).run(x), [g for g in ref if g["stream"] == s]
        assert [d["pos"] for d in od] == [g["start"] for g in mine] and [d["offset"] for d in od] == [g["cfo_bin"] for g in mine]
    assert sum(1 for g in ref if g["stream"] == 0) >= 5 and sum(1 for g in ref if g["stream"] == 2) >= 3


@pytest.fixture(scope="module")
def long_stream(fx):
    """One stream from the device-side generator (2100 frames on the CPU take far longer than a few seconds): 20 k samples without a
    frame, then minimal frames back to back.  Returns the device tensor, the injected payloads and the length of a frame with its gap."""
    import torch
    step = _frame_len(fx, (PSK4, CONV_V27, FEC_NONE, 1)) + GAP
    quiet, n = 20_000, 2100 * step + 9 * 8 * step
    xd, injected = fx.synth_streams_device(1, n, first_stream_id=77, payload_len=1, gap=GAP)
    x = torch.cat([torch.zeros(quiet, dtype=torch.complex64, device=xd.device), xd[0]]).contiguous()
    torch.cuda.synchronize()
    return x, [(p + quiet, pl) for p, pl in injected[0]], step, quiet


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [1, 3])
def test_more_than_a_tile_in_one_workgroup_and_both_paths_in_one_context(fx, monkeypatch, long_stream, depth):
    """Ten blocks of a continuing stream: a quiet one, eight frames, more than 2048 frames, then seven blocks of eight frames.  The grid comes
    from the frame count of the block collected last, so without any knob the long block meets ONE workgroup (counting sweep, two tiles),
    the first block submitted after its collection is planned by the pair over two workgroups, and the blocks after that by one again: in
    a context of depth + 1 slots the pair takes over a slot (workspace, walk header) that the one-workgroup kernel left, and hands it back.
    Compared with the pair throughout (FXRX_PLAN_FUSED=0, FXRX_PLAN_GRID=2) and with the payloads that were sent; the oracle would take
    minutes over three million samples."""
    x, injected, step, quiet = long_stream
    cuts = [0, quiet, quiet + 8 * step, quiet + (8 + 2100) * step] + [quiet + (8 + 2100 + 8 * k) * step for k in range(1, 8)]
    cuts[-1] = x.numel()
    blocks = [[(x.data_ptr() + 8 * a, b - a)] for a, b in zip(cuts[:-1], cuts[1:])]
    assert len(blocks) == 10 and cuts[3] - cuts[2] == 2100 * step
    runs = [_run(fx, monkeypatch, env, blocks, depth, on_device=True) for _, env in MODES]
    ref, ref_cnt = runs[0]
    for got, cnt in runs[1:]:
        _same(ref, got)
        assert cnt == ref_cnt
    assert len(ref) == len(injected) > 2048 + 8 * 8
    assert all(g["payload_valid"] and g["payload"] == pl for g, (_, pl) in zip(ref, injected))
