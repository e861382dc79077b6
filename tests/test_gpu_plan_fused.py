"""The plan stage as ONE launch (fx_planfused_kernel: both passes in a single workgroup, taken when one workgroup plans the block)
against the two launches it replaces (FXRX_PLAN_FUSED=0) and against the two-kernel path over two workgroups, whose second
one goes through the look-back (FXRX_PLAN_GRID=2).  The three must lay the payload stage out identically: every case compares
the decoded frames field for field between the three runs and with the CPU oracle, and the counters that come out of the plan
stage's header (walk jobs, payload symbols, trellis work items)."""
import numpy as np
import pytest

from parity_util import oracle_frames, compare_frames

CONV_V27 = 11
MODES = (("fused", {"FXRX_PLAN_FUSED": "1"}), ("two launches", {"FXRX_PLAN_FUSED": "0"}), ("two workgroups", {"FXRX_PLAN_GRID": "2"}))
COUNTERS = ("walk_jobs", "payload_symbols", "vb_blocks")


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


def _build(fx, specs, n, seed, snr_db=20.0, corrupt=()):
    """A stream of n samples holding one frame per (mod, fec0, fec1, payload_len) of specs, 256-sample gaps, CFO / phase / AWGN;
    the frames whose index is in `corrupt` have their header symbols overwritten (the header check fails: no payload stage)."""
    rng = np.random.RandomState(seed)
    x = np.zeros(n, np.complex64)
    p = 300
    for i, (mod, fec0, fec1, plen) in enumerate(specs):
        g = fx.FrameGen(mod, fec0, fec1, fx.CRC_24)
        fr = np.array(g.frame(rng.randint(0, 256, plen).astype(np.uint8), dt=0.1), np.complex64)
        g.close()
        if i in corrupt:
            fr[200:500] = ((rng.choice([-1.0, 1.0], 300) + 1j * rng.choice([-1.0, 1.0], 300)) / np.sqrt(2.0)).astype(np.complex64)
        assert p + len(fr) <= n, "stream too short for its frames"
        x[p:p + len(fr)] = fr
        p += len(fr) + 256
    x *= np.exp(1j * (0.01 * np.arange(n, dtype=np.float64) + 0.3)).astype(np.complex64)
    x += np.float32(np.sqrt(0.5 * 10.0 ** (-snr_db / 10.0))) * rng.standard_normal(2 * n).astype(np.float32).view(np.complex64)
    return x


def _noise(n, seed):
    return (np.float32(0.1) * np.random.RandomState(seed).standard_normal(2 * n).astype(np.float32).view(np.complex64)).copy()


def _run(fx, monkeypatch, env, blocks, depth=1):
    """blocks: consecutive blocks of continuing streams, each a list with one array per stream.  Returns the frames of all blocks
    and the plan counters summed over them."""
    for k in ("FXRX_PLAN_FUSED", "FXRX_PLAN_GRID"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ctx = fx.RxContext(len(blocks[0]), want_framesyms=True)
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
        ctx.submit_raw([a.ctypes.data for a in b], [len(a) for a in b], False); inflight += 1
    while inflight:
        collect(); inflight -= 1
    ctx.close()
    return got, cnt


def _three_ways(fx, oracle, monkeypatch, streams, blocks=None, depth=1):
    """streams: the whole streams (what the oracle receives); blocks: how they are fed (default: one block)."""
    blocks = [streams] if blocks is None else blocks
    runs = [(name, _run(fx, monkeypatch, env, blocks, depth)) for name, env in MODES]
    (_, (ref, ref_cnt)) = runs[0]
    for name, (got, cnt) in runs[1:]:
        _same(ref, got)
        assert cnt == ref_cnt, (name, cnt, ref_cnt)
    for s, x in enumerate(streams):
        compare_frames(oracle_frames(oracle, x), [g for g in ref if g["stream"] == s])
    return ref, ref_cnt


@pytest.mark.gpu
def test_noise_only(fx, oracle, monkeypatch):
    got, cnt = _three_ways(fx, oracle, monkeypatch, [_noise(150_000, 1)])
    assert got == [] and cnt["payload_symbols"] == 0 and cnt["vb_blocks"] == 0


@pytest.mark.gpu
def test_exactly_one_frame(fx, oracle, monkeypatch):
    got, cnt = _three_ways(fx, oracle, monkeypatch, [_build(fx, [(2, CONV_V27, 1, 1024)], 40_000, 2)])
    assert len(got) == 1 and got[0]["payload_valid"] and cnt["payload_symbols"] > 0


@pytest.mark.gpu
def test_65_short_frames(fx, oracle, monkeypatch):
    """65 frames of one class: its PLL list is one full wave and one frame in a second wave, the other 63 slots padding."""
    got, _ = _three_ways(fx, oracle, monkeypatch, [_build(fx, [(2, CONV_V27, 1, 16)] * 65, 90_000, 3)])
    assert len(got) == 65 and all(g["payload_valid"] for g in got)


@pytest.mark.gpu
def test_mixed_classes_and_a_failed_header(fx, oracle, monkeypatch):
    """PSK4 and QAM16 frames in one block (two PLL classes, each padded to whole waves) around a frame whose header fails (it
    gets a job without a payload stage: pad_ == 0, in no list)."""
    specs = [(2, CONV_V27, 1, 1024), (27, CONV_V27, 1, 700), (2, CONV_V27, 1, 300), (27, CONV_V27, 1, 64), (2, CONV_V27, 1, 1024),
             (27, CONV_V27, 1, 1024), (2, CONV_V27, 1, 40), (27, CONV_V27, 1, 333)]
    got, _ = _three_ways(fx, oracle, monkeypatch, [_build(fx, specs, 150_000, 4, corrupt=(2,))])
    assert len(got) == len(specs)
    assert sum(1 for g in got if not g["header_valid"]) == 1
    assert {g["mod_scheme"] for g in got if g["header_valid"]} == {2, 27}
    assert all(g["payload_valid"] for g in got if g["header_valid"])


@pytest.mark.gpu
def test_three_streams_middle_one_without_frames(fx, oracle, monkeypatch):
    xs = [_build(fx, [(2, CONV_V27, 1, 1024)] * 4, 80_000, 5), _noise(80_000, 6), _build(fx, [(2, CONV_V27, 1, 500)] * 6, 80_000, 7)]
    got, _ = _three_ways(fx, oracle, monkeypatch, xs)
    assert [sum(1 for g in got if g["stream"] == s) for s in range(3)] == [4, 0, 6]


@pytest.mark.gpu
def test_two_blocks_of_a_continuing_stream_in_flight(fx, oracle, monkeypatch):
    x = _build(fx, [(2, CONV_V27, 1, 1024)] * 8, 150_000, 8)
    got, _ = _three_ways(fx, oracle, monkeypatch, [x], blocks=[[x[:75_000]], [x[75_000:]]], depth=2)
    assert len(got) == 8 and all(g["payload_valid"] for g in got)
