"""Who writes a frame's run of trellis items (gr-liquiddsp_amd/csrc/fx_kernels.hip: vb_item, vb_write_run).  The plan stage only
hands every batch-path frame its run of slots; the frame's own wave of fx_vbpre_kernel writes the run -- frame and block for a frame
that needs the trellis, "off" for one it has decoded itself -- and a slot no wave has reached holds what an earlier block left, which
vb_item must find off or equal to this block's layout.

Every case decodes its streams with the batch Viterbi path and with FXRX_BATCH_VITERBI=0 (viterbi27 in the lean decoder, which uses
no item list): every field of every record and every payload byte must be equal, and a payload that passes its check must be the one
that was sent.  Streams come from synth_stream, 300 000 samples at the most; every block starts its streams afresh (reset), so a
block's result does not depend on the blocks before it -- which is what the stale-slot cases check.

Trellis blocks are 192 steps here (the host's choice for traffic this light): a frame of k = payload + 3 (CRC-24) bytes has
ceil((8 k + 6) / 192) of them, fx_fecdims.h: v27_steps.  1-byte payloads: one block; 1520 bytes: 64; 1540 bytes: 65 (a run that
crosses the wave's 64 lanes); 1024 bytes: 43.

The frame counts 1, 511, 512, 513 and 2049 through the one-workgroup kernel at both widths against the pair are the cases of
tests/test_gpu_plan_wide.py (test_frame_counts_at_every_width), which the plan kernels changed here pass unchanged; no copy of them
is added.

Not covered: a frame demoted at the end of the arena.  No knob shrinks the arena (vb_cap is priced from the block's samples), so the
sub-case is left out; the traffic-built overflow of test_gpu_traffic_shift.py (LONG_TRELLIS) goes through the changed kernels."""
import numpy as np
import pytest

from test_gpu_plan_fused import _same, _noise

PSK4, QAM16 = 2, 27
CONV_V27, CONV_V27P23, CONV_V27P34 = 11, 15, 16
VB_BLK = 192
KNOBS = ("FXRX_BATCH_VITERBI", "FXRX_VB_CLEAN", "FXRX_PLAN_FUSED", "FXRX_PLAN_THREADS", "FXRX_PLAN_GRID", "FXRX_VB_DEBUG", "FXRX_VB_BLK", "FXRX_VB_EARLY_TAIL")
COUNTERS = ("vb_blocks", "vb_repairs", "vb_fallbacks", "vb_clean")
LEAN = {"FXRX_BATCH_VITERBI": "0"}
PLAN_PATHS = [("0", "256"), ("0", "512"), ("1", "256"), ("1", "512")]      # (FXRX_PLAN_FUSED, FXRX_PLAN_THREADS)
_CACHE = {}


def _nblk(payload_len):
    return (8 * (payload_len + 3) + 6 + VB_BLK - 1) // VB_BLK


def _decode(fx, monkeypatch, env, blocks):
    """blocks: a list of blocks, each a list with one array per stream, fed to ONE context back to back, every block from freshly
    reset streams (the context keeps its arenas, its slots and what it knows of the last block's traffic).  Returns, per block,
    (frames, counters), and the context's late_stats at the end."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ctx = fx.RxContext(len(blocks[0]), want_framesyms=True)
    out = []
    for b in blocks:
        ctx.reset()
        got = ctx.process(list(b))
        tm = ctx.timing()
        out.append((got, {k: tm[k] for k in COUNTERS}))
    late = dict(zip(ctx.LATE_REASONS, ctx.late_stats()[:6]))
    ctx.close()
    return out, late


def _alone(fx, monkeypatch, key, env, block):
    """one block in a fresh context, decoded once per (case, knobs) and shared"""
    k = (key, tuple(sorted(env.items())))
    if k not in _CACHE:
        _CACHE[k] = _decode(fx, monkeypatch, env, [block])[0][0]
    return _CACHE[k]


def _check_sent(frames, sent_by_stream, all_decode=()):
    """a payload that passes its check is one its stream sent; the streams of all_decode deliver every frame, in order"""
    for s, sent in enumerate(sent_by_stream):
        mine = [g for g in frames if g["stream"] == s]
        pool = {pl for _, pl in sent}
        for g in mine:
            assert not g["payload_valid"] or g["payload"] in pool, (s, g["start"])
        if s in all_decode:
            assert len(mine) == len(sent) and all(g["payload_valid"] and g["payload"] == pl for g, (_, pl) in zip(mine, sent)), s


def _against_lean(fx, monkeypatch, key, block, sent, env=None, all_decode=()):
    """the block alone under env (default knobs: the batch path) against the lean decoder; returns (frames, counters)"""
    got, cnt = _alone(fx, monkeypatch, key, env or {}, block)
    ref, ref_cnt = _alone(fx, monkeypatch, key, LEAN, block)
    _same(ref, got)
    assert ref_cnt["vb_blocks"] == 0
    _check_sent(got, sent, all_decode)
    return got, cnt


def _batch_frames(frames):
    return [g for g in frames if g["header_valid"] and g["fec0"] in (CONV_V27, CONV_V27P23, CONV_V27P34)]


# ---- the streams (made once per session) ----
def _stream(fx, key, n, **kw):
    if ("stream", key) not in _CACHE:
        _CACHE[("stream", key)] = fx.synth_stream(n, **kw)
    return _CACHE[("stream", key)]


def _r12_3db(fx):
    return _stream(fx, "r12_3db", 300_000, stream_id=2100, mod=PSK4, fec0=CONV_V27, payload_len=1024, snr_db=3.0)


def _r12_9db(fx):
    """Es/N0 = 9 dB: a raw bit error rate of some 2e-3 over 16444 coded bits a frame -- no frame is a codeword as received, and the trellis corrects them"""
    return _stream(fx, "r12_9db", 300_000, stream_id=2101, mod=PSK4, fec0=CONV_V27, payload_len=1024, snr_db=9.0)


def _r12_20db(fx):
    return _stream(fx, "r12_20db", 300_000, stream_id=2102, mod=PSK4, fec0=CONV_V27, payload_len=1024, snr_db=20.0)


def _r34_12db(fx):
    return _stream(fx, "r34_12db", 300_000, stream_id=2103, mod=QAM16, fec0=CONV_V27P34, payload_len=1024, snr_db=12.0)


def _r23_6db(fx):
    return _stream(fx, "r23_6db", 200_000, stream_id=2104, mod=PSK4, fec0=CONV_V27P23, payload_len=300, snr_db=6.0)


def _mixed_block(fx):
    """case 1's stream beside a clean one and a dirty one of the same code: clean and dirty runs in one code class of one block"""
    streams = [_r12_3db(fx), _r12_20db(fx), _r12_9db(fx)]
    return [x for x, _ in streams], [inj for _, inj in streams]


# ---- 1. mixed clean and dirty frames in one block ----
@pytest.mark.gpu
def test_r12_at_3db(fx, monkeypatch):
    """PSK4 r1/2, 1024-byte payloads, Es/N0 = 3 dB: frames fail the codeword check and take the trellis.  Fewer trellis blocks run than
    the block has item slots (the slots of clean frames and of the class padding are off)."""
    x, inj = _r12_3db(fx)
    got, cnt = _against_lean(fx, monkeypatch, "r12_3db", [x], [inj])
    n = len(_batch_frames(got))
    ran = (n - cnt["vb_clean"]) * _nblk(1024)
    print("frames %d of %d sent, batch %d, clean %d, items %d, trellis blocks %d, repairs %d, fallbacks %d" % (
        len(got), len(inj), n, cnt["vb_clean"], cnt["vb_blocks"], ran, cnt["vb_repairs"], cnt["vb_fallbacks"]))
    assert n > 0 and cnt["vb_blocks"] > 0 and cnt["vb_clean"] < n
    assert 0 < ran < cnt["vb_blocks"]


@pytest.mark.gpu
def test_clean_and_dirty_frames_in_one_block(fx, monkeypatch):
    """The 3 dB stream, a 20 dB stream (every frame clean) and a 9 dB stream (none) of the same code in one block: both kinds occur."""
    xs, inj = _mixed_block(fx)
    got, cnt = _against_lean(fx, monkeypatch, "mixed", xs, inj, all_decode=(1,))
    n = len(_batch_frames(got))
    n_clean_stream = sum(1 for g in got if g["stream"] == 1)
    print("batch frames %d, clean %d, items %d" % (n, cnt["vb_clean"], cnt["vb_blocks"]))
    assert n_clean_stream == len(inj[1]) > 0 and any(g["payload_valid"] for g in got if g["stream"] == 2)
    assert n_clean_stream <= cnt["vb_clean"] < n
    assert cnt["vb_blocks"] > 0 and (n - cnt["vb_clean"]) * _nblk(1024) < cnt["vb_blocks"]


# ---- 2. a punctured code: no frame is clean ----
@pytest.mark.gpu
def test_punctured_code_is_never_clean(fx, monkeypatch):
    """QAM16 r3/4 at 12 dB, and the same stream with the codeword check off: every run is written as trellis items either way."""
    x, inj = _r34_12db(fx)
    got, cnt = _against_lean(fx, monkeypatch, "r34", [x], [inj])
    off, off_cnt = _against_lean(fx, monkeypatch, "r34", [x], [inj], env={"FXRX_VB_CLEAN": "0"})
    _same(got, off)
    assert cnt == off_cnt and cnt["vb_clean"] == 0 and cnt["vb_blocks"] > 0
    assert len(_batch_frames(got)) > 0 and any(g["payload_valid"] for g in got)


# ---- 3. both plan paths, both widths ----
@pytest.mark.gpu
@pytest.mark.parametrize("fused,threads", PLAN_PATHS)
@pytest.mark.parametrize("case", ["r12_3db", "mixed", "r34", "r34 check off"])
def test_plan_paths_agree(fx, monkeypatch, case, fused, threads):
    """The pair (FXRX_PLAN_FUSED=0) and the one-workgroup kernel at 256 and 512 threads hand out the same runs: outputs equal to the
    lean decoder's, counters equal to the default path's."""
    if case == "r12_3db":
        key, block, inj = "r12_3db", [_r12_3db(fx)[0]], [_r12_3db(fx)[1]]
    elif case == "mixed":
        key = "mixed"; block, inj = _mixed_block(fx)
    else:
        key, block, inj = "r34", [_r34_12db(fx)[0]], [_r34_12db(fx)[1]]
    base = {"FXRX_VB_CLEAN": "0"} if case.endswith("check off") else {}
    _, ref_cnt = _against_lean(fx, monkeypatch, key, block, inj, env=base)
    _, cnt = _against_lean(fx, monkeypatch, key, block, inj, env=dict(base, FXRX_PLAN_FUSED=fused, FXRX_PLAN_THREADS=threads))
    assert cnt == ref_cnt, (cnt, ref_cnt)


# ---- 4. stale slots ----
def _layout_blocks(fx):
    """A: 14 streams of 2045-byte frames (8 a stream, 86 trellis blocks a frame) at 4 dB and 20 dB alternately.  B: the same context's 14
    streams with a few short frames of a punctured code in the first and a few of rate 1/2 in the second, noise in the rest."""
    if "layouts" not in _CACHE:
        a = [_stream(fx, "long%d" % s, 300_000, stream_id=2200 + s, mod=PSK4, fec0=CONV_V27, payload_len=2045, snr_db=4.0 if s % 2 else 20.0) for s in range(14)]
        b = [_stream(fx, "shortp", 14_000, stream_id=2300, mod=QAM16, fec0=CONV_V27P34, payload_len=100, snr_db=14.0),
             _stream(fx, "shortr", 14_000, stream_id=2301, mod=PSK4, fec0=CONV_V27, payload_len=40, snr_db=20.0)]
        b += [(_noise(4096, 2310 + s), []) for s in range(12)]
        _CACHE["layouts"] = ([x for x, _ in a], [i for _, i in a]), ([x for x, _ in b], [i for _, i in b])
    return _CACHE["layouts"]


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["ABBAAB", "BAAB"])
def test_stale_slots_between_blocks_of_different_layouts(fx, monkeypatch, order):
    """One context, blocks back to back, nothing reset but the streams.  A context at depth 1 rotates two sets of arenas, so the orders
    give each set A behind B and B behind A.  After B the tail's grids follow B's traffic -- at most 1.5 x its frames + 64 waves of
    fx_vbpre_kernel, 1.5 x its items + 1024 item slots (fx_traffic.h) -- and do not cover A: runs of A stay unwritten until
    finish_decode, and the trellis kernels launched with the chain meet whatever the set held before.  The first block of a context is
    the other kind: its set has never been written.  Every block must give what it gives alone in a fresh context."""
    (xa, ia), (xb, ib) = _layout_blocks(fx)
    alone = {"A": _against_lean(fx, monkeypatch, "layout A", xa, ia, all_decode=tuple(range(0, 14, 2))),
             "B": _against_lean(fx, monkeypatch, "layout B", xb, ib, all_decode=(1,))}
    na, nb = len(_batch_frames(alone["A"][0])), len(_batch_frames(alone["B"][0]))
    print("A: %d batch frames, %s; B: %d batch frames, %s" % (na, alone["A"][1], nb, alone["B"][1]))
    assert nb > 0 and na > nb + nb // 2 + 64 and alone["A"][1]["vb_blocks"] > alone["B"][1]["vb_blocks"] * 3 // 2 + 1024
    assert 0 < alone["A"][1]["vb_clean"] < na
    runs, late = _decode(fx, monkeypatch, {}, [{"A": xa, "B": xb}[c] for c in order])
    for i, (c, (got, cnt)) in enumerate(zip(order, runs)):
        _same(alone[c][0], got)
        assert cnt == alone[c][1], (i, c, cnt, alone[c][1])
    print("late work:", late)
    assert late["more_batch_frames"] > 0 and late["more_batch_items"] > 0


# ---- 5. the smallest shapes ----
@pytest.mark.gpu
@pytest.mark.parametrize("check", ["1", "0"])
@pytest.mark.parametrize("payload_len,nblk", [(1, 1), (1520, 64), (1540, 65)])
def test_smallest_runs(fx, monkeypatch, payload_len, nblk, check):
    """A run of a single trellis block, of 64 (the wave's lanes exactly) and of 65 (one slot on a second round); at 20 dB the frames are
    clean and the run is written off, with the check off the same frames write their items and take the trellis."""
    assert _nblk(payload_len) == nblk
    x, inj = _stream(fx, "small%d" % payload_len, 60_000, stream_id=2400 + nblk, mod=PSK4, fec0=CONV_V27, payload_len=payload_len, snr_db=20.0)
    got, cnt = _against_lean(fx, monkeypatch, "small%d" % payload_len, [x], [inj], env={"FXRX_VB_CLEAN": check}, all_decode=(0,))
    assert len(got) == len(inj) > 0
    assert cnt["vb_clean"] == (len(got) if check == "1" else 0)
    assert cnt["vb_blocks"] == (len(got) * nblk + 127) // 128 * 128 and cnt["vb_fallbacks"] == 0


# ---- 6. two streams, one clean and one dirty, of different code classes ----
@pytest.mark.gpu
@pytest.mark.parametrize("fused", ["1", "0"])
def test_two_code_classes_clean_and_dirty(fx, monkeypatch, fused):
    """Rate 1/2 at 20 dB (clean) and punctured rate 2/3 at 6 dB (never clean): two code classes, each padded to whole waves, the first
    one's runs written off and the second one's as items."""
    (x0, i0), (x1, i1) = _r12_20db(fx), _r23_6db(fx)
    got, cnt = _against_lean(fx, monkeypatch, "two classes", [x0, x1], [i0, i1], env={"FXRX_PLAN_FUSED": fused}, all_decode=(0,))
    n0 = sum(1 for g in got if g["stream"] == 0)
    n1 = sum(1 for g in _batch_frames(got) if g["stream"] == 1)
    assert n0 == len(i0) and cnt["vb_clean"] == n0 and n1 > 0
    pad = lambda v: (v + 127) // 128 * 128
    assert cnt["vb_blocks"] == pad(n0 * _nblk(1024)) + pad(n1 * _nblk(300))
