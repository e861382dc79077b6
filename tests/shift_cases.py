"""Block sequences whose traffic the block before did not announce, as data (tests/test_ref_shift.py, tests/test_gpu_traffic_shift.py).

A block's kernel chain is enqueued before the host knows what the block holds, so its grids -- and whether some kernels are launched at
all -- follow what the last collected block held.  A block that outgrows them is completed when it is collected (finish_decode, six
reasons: RxContext.LATE_REASONS), or, for the trellis arena, has frames taken off the batch Viterbi path by the plan kernel.  Every
case below is a list of blocks made of fx.synth_stream pieces and is named by the transition it makes; `checks` states that transition
as inequalities between the class counts of consecutive blocks, which tests/test_ref_shift.py proves from the CPU oracle's frames, and
`expect` names the reasons that must act at a block (depth 1).

The inequalities carry margins that do not come from the host's sizing rules: "jump" is at least four times the count of the block
before plus 200 frames (plus 2048 for trellis work items), so that a retuned rule does not silently empty a case.

A piece holds whole frames and ends with TAIL samples of noise, so every frame completes in the block it starts in and a block's
frames are the same whether its streams continue (`cont`) or every block is an independent capture (`reset`).
"""
import functools
import importlib

import numpy as np

import ref_decode as R

TAIL = 600              # noise behind a piece's last frame: less than the shortest frame (a header alone is 630 samples)
JUMP_FRAMES, JUMP_ITEMS, JUMP_FACTOR = 200, 2048, 4

# ---- which decoder a frame goes to: the rule of plan_sizes / plan_key (fx_kernels.hip), restated as a table of
# (soft decisions, family of fec0, family of fec1) with the families conv (K = 7 convolutional), rs (Reed-Solomon) and other (none, block codes)
CLASS = {
    (0, "conv", "other"): "batch", (0, "conv", "conv"): "plain", (0, "conv", "rs"): "rs",
    (0, "rs", "other"): "rs", (0, "rs", "conv"): "rs", (0, "rs", "rs"): "rs",
    (0, "other", "other"): "plain", (0, "other", "conv"): "plain", (0, "other", "rs"): "rs",
    (1, "conv", "other"): "plain", (1, "conv", "conv"): "plain", (1, "conv", "rs"): "rs",
    (1, "rs", "other"): "rs", (1, "rs", "conv"): "rs", (1, "rs", "rs"): "rs",
    (1, "other", "other"): "plain", (1, "other", "conv"): "plain", (1, "other", "rs"): "rs",
}


def family(fec):
    return "conv" if fec in R.CONV else "rs" if fec == R.FEC_RS else "other"


def frame_class(fec0, fec1, soft=0):
    return CLASS[(soft, family(fec0), family(fec1))]


def trellis_steps(n, check):
    """trellis steps of a frame of n payload bytes under a K = 7 code: 8 bits a byte of payload and check, 6 tail bits"""
    return 8 * R.packet_dims(n, check, R.FEC_NONE, R.FEC_NONE)[0] + 6


def counts(frames, vb_blk=None):
    """class counts of a block from (header_valid, fec0, fec1, check, payload length) tuples; `items`: trellis blocks of vb_blk steps"""
    c = dict(frames=len(frames), valid=0, plain=0, batch=0, rs=0, items=0, steps=0)
    for hv, f0, f1, chk, n in frames:
        if not hv:
            continue
        c["valid"] += 1
        k = frame_class(f0, f1)
        c[k] += 1
        if k == "batch":
            s = trellis_steps(n, chk)
            c["steps"] += s
            c["items"] += -(-s // vb_blk) if vb_blk else 0
    return c


def P(frames, sid, mod=R.PSK4, fec0=R.FEC_V27, fec1=R.FEC_NONE, check=R.CRC_24, n=1024, gap=0, snr=20.0, lead=0):
    return dict(frames=frames, sid=sid, mod=mod, fec0=fec0, fec1=fec1, check=check, n=n, gap=gap, snr=snr, lead=lead)


def silence(samples, sid):
    return dict(frames=0, sid=sid, samples=samples, snr=20.0)


def short(sid, per, fec0=R.FEC_V27, snr=25.0):
    """4 * per frames of 0, 5, 11 and 16 payload bytes with no gap, in four modulations"""
    return [P(per, sid + i, mod=m, fec0=fec0, n=n, snr=snr) for i, (m, n) in enumerate(((R.QAM64, 0), (R.QAM16, 5), (R.PSK8, 11), (R.PSK4, 16)))]


_fx = None


def fx():
    global _fx
    if _fx is None:
        _fx = importlib.import_module("gr-liquiddsp_amd")
    return _fx


def frame_len(p):
    return int(fx().lib().fxrx_gen_frame_len(p["mod"], p["check"], p["fec0"], p["fec1"], p["n"]))


def piece_len(p):
    if not p["frames"]:
        return p["samples"]
    return p["lead"] + p["frames"] * (frame_len(p) + p["gap"]) - p["gap"] + TAIL


def make_piece(p):
    if not p["frames"]:
        rng = np.random.RandomState(p["sid"])
        return (np.float32(np.sqrt(0.5 * 10.0 ** (-p["snr"] / 10.0))) * rng.standard_normal(2 * p["samples"]).astype(np.float32)).view(np.complex64)
    x, inj = fx().synth_stream(piece_len(p), stream_id=p["sid"], mod=p["mod"], fec0=p["fec0"], fec1=p["fec1"], check=p["check"], payload_len=p["n"],
                               gap=p["gap"], snr_db=p["snr"], lead=p["lead"])
    assert len(inj) == p["frames"], (p, len(inj))
    return x


# ---- the long frame of LONG_TRELLIS: the smallest payload whose trellis blocks (of 128 steps) exceed 4 x those of the block before + 2048
VB_BLK_FORCED = 128
_D_SHORT = dict(frames=20, n=16)
_d_items0 = _D_SHORT["frames"] * -(-trellis_steps(_D_SHORT["n"], R.CRC_24) // VB_BLK_FORCED)
D_LONG = next(n for n in range(1, 65536) if -(-trellis_steps(n, R.CRC_24) // VB_BLK_FORCED) > JUMP_FACTOR * _d_items0 + JUMP_ITEMS)

# ---- the block of ARENA: frames of QAM64 under the rate-7/8 code (2.6 trellis steps per sample), as many as it takes for the trellis
# blocks to exceed 1.5 steps per sample of the block -- what the arena is priced at (fx_host.cpp: vb_cap) -- by more than 2048 blocks
ARENA_N = 8000


def arena_frames():
    p = P(1, 0, mod=R.QAM64, fec0=R.FEC_V27P78, n=ARENA_N)
    per = -(-trellis_steps(ARENA_N, R.CRC_24) // VB_BLK_FORCED)
    for k in range(1, 200):
        samples = piece_len(dict(p, frames=k))
        if k * per * VB_BLK_FORCED > samples + samples // 2 + (JUMP_ITEMS + 64) * VB_BLK_FORCED:
            return k
    raise AssertionError("no overflow shape")


V27x = lambda k, sid, **kw: P(k, sid, **kw)          # 1024-byte QPSK rate-1/2 frames (18.7 k samples each)

# name -> dict(env, mode, blocks[b][stream] = [pieces], checks = [(block, key, kind)], expect = {block: [reasons]}, shifted = blocks decoded by the
# numpy reference).  kinds: zero | some | from_zero (0 before, some now) | jump | jump_items | one (exactly one) | over32
CASES = {
    "nothing -> plain -> 4x plain": dict(
        blocks=[[[V27x(5, 9000)]],
                [[V27x(4, 9001), P(1, 9002, mod=R.QAM16, fec0=R.FEC_H74, n=64)]],
                [[V27x(1, 9003)] + short(9010, 51, fec0=R.FEC_H74)]],
        checks=[(0, "plain", "zero"), (1, "plain", "from_zero"), (1, "plain", "one"), (2, "plain", "jump")],
        expect={1: ["more_plain"], 2: ["more_plain"]}),
    "nothing -> RS -> nothing -> RS": dict(
        blocks=[[[V27x(3, 9020)]],
                [[V27x(3, 9021), P(1, 9022, mod=R.QAM16, fec0=R.FEC_RS, n=219)]],           # (one such frame: whatever the hint's fading rule, a single RS-free block takes it to zero)
                [[V27x(3, 9023)]],
                [[V27x(3, 9024), P(3, 9025, mod=R.QAM16, fec0=R.FEC_RS, n=443)]]],
        checks=[(0, "rs", "zero"), (1, "rs", "from_zero"), (1, "rs", "one"), (2, "rs", "zero"), (3, "rs", "from_zero")],
        expect={1: ["more_rs"], 3: ["more_rs"]}),
    "few -> many batch frames": dict(
        blocks=[[[silence(40_000, 9030), V27x(1, 9031)]],
                [short(9040, 51)]],
        checks=[(1, "batch", "jump")],
        expect={1: ["more_batch_frames"]}, device=True),
    "small -> one long trellis": dict(
        env=dict(FXRX_VB_BLK=VB_BLK_FORCED),
        # (the short frames are punctured, never clean: the trellis kernels stay in the next block's chain, and it is their grid that is outgrown)
        blocks=[[[silence(40_000, 9050), P(_D_SHORT["frames"], 9051, mod=R.QAM16, fec0=R.FEC_V27P23, n=_D_SHORT["n"])]],
                [[P(1, 9052, mod=R.QAM64, n=D_LONG, snr=25.0)]]],
        checks=[(1, "items", "jump_items")],
        expect={1: ["more_batch_items"]}),
    "fallbacks beyond the launch": dict(
        env=dict(FXRX_VB_DEBUG=2, FXRX_VB_BLK=VB_BLK_FORCED),
        blocks=[[[P(20, 9060 + s, mod=R.QAM16, fec0=R.FEC_H128, n=300)] for s in range(3)],
                # (QAM16 at 6 dB: trellis blocks whose warm-up does not arrive at the true metrics, the only source of handed-back frames; 51 frames
                # of 19 work items, within what a block after none is launched with)
                [[P(17, 9064 + s, mod=R.QAM16, n=300, snr=6.0)] for s in range(3)]],
        checks=[(0, "batch", "zero"), (1, "batch", "over32")],
        expect={1: ["more_fb"]}),
    "dense -> silent -> dense": dict(
        blocks=[[short(9070, 51)], [[silence(60_000, 9075)]], [short(9076, 51)]],
        checks=[(1, "frames", "zero"), (2, "batch", "jump")],
        expect={2: ["more_batch_frames"]}),
    "hard mix -> all formats at once": dict(
        blocks=[[[V27x(2, 9080), P(3, 9081, mod=R.QAM16, fec0=R.FEC_V27P23, n=600)], [P(3, 9082, mod=R.PSK8, fec0=R.FEC_V27P34, n=700), silence(20_000, 9083)]],
                [[P(3, 9084, mod=R.PSK2, fec0=R.FEC_NONE, n=100, snr=25.0), P(3, 9085, mod=R.PSK4, n=300, snr=25.0), P(3, 9086, mod=R.PSK8, fec0=R.FEC_V27P34, n=300, snr=25.0),
                  P(3, 9087, mod=R.PSK16, fec0=R.FEC_H74, n=200, snr=28.0), P(3, 9088, mod=R.DPSK2, fec0=R.FEC_H128, n=100, snr=25.0), P(3, 9089, mod=R.DPSK4, fec0=R.FEC_GOLAY, n=200, snr=25.0)],
                 [P(3, 9090, mod=R.DPSK8, fec0=R.FEC_SD22, n=200, snr=28.0), P(3, 9091, mod=R.ASK4, fec0=R.FEC_V27, fec1=R.FEC_SD39, n=200, snr=25.0), P(3, 9092, mod=R.QAM16, fec0=R.FEC_RS, n=443, snr=25.0),
                  P(3, 9093, mod=R.QAM32, fec0=R.FEC_V27, fec1=R.FEC_RS, n=300, snr=28.0), P(3, 9094, mod=R.QAM64, fec0=R.FEC_SD72, fec1=R.FEC_V27, n=300, snr=30.0)]]],
        checks=[(0, "plain", "zero"), (0, "rs", "zero"), (1, "plain", "from_zero"), (1, "rs", "from_zero")],
        expect={1: ["more_plain", "more_rs"]}, device=True),
    "clean -> noisy": dict(
        # (frames that arrive as codewords leave the trellis kernels out of the next chain; QAM16 at 9 dB never does)
        blocks=[[[V27x(3, 9120)]], [[P(6, 9121, mod=R.QAM16, n=600, snr=9.0), silence(20_000, 9122)]]],
        checks=[(0, "batch", "some"), (1, "batch", "some"), (0, "plain", "zero"), (1, "plain", "zero")],
        expect={1: ["late_trellis"]}),
    "detector: few -> many detections": dict(
        detector=True,
        blocks=[[[silence(20_000, 9100), V27x(2, 9101)]], [short(9102, 52)]],
        checks=[(1, "frames", "jump")],
        expect={}),
}
ARENA = "arena overflow"
ALL_MODS_CASE = "hard mix -> all formats at once"


def arena_case():
    return dict(env=dict(FXRX_VB_BLK=VB_BLK_FORCED), blocks=[[[P(arena_frames(), 9110, mod=R.QAM64, fec0=R.FEC_V27P78, n=ARENA_N, snr=30.0)]]], checks=[(0, "items", "arena")], expect={})


def case(name):
    return arena_case() if name == ARENA else CASES[name]


@functools.lru_cache(maxsize=None)
def build(name):
    """blocks[b][s]: the samples of stream s in block b (built once, never modified)"""
    out = []
    for blk in case(name)["blocks"]:
        row = []
        for pieces in blk:
            x = np.concatenate([make_piece(p) for p in pieces])
            x.setflags(write=False)
            row.append(x)
        out.append(row)
    return out


def block_ranges(blocks, s):
    """[lo, hi) of every block within stream s, continuing"""
    e = np.cumsum([0] + [len(b[s]) for b in blocks])
    return list(zip(e[:-1], e[1:]))


@functools.lru_cache(maxsize=None)
def oracle(name, form, repeat=1):
    """The CPU oracle's frames (detector mode: detections), [block][stream] -> list.  form `reset`: every block of every stream alone;
    `cont`: each stream in one pass over its blocks (`repeat` times over), a frame belonging to the block it starts in -- a piece ends with
    TAIL samples of noise, so that is the block that delivers it.  Positions count from the last reset."""
    import oracle_ffi as O
    from parity_util import oracle_frames
    c = case(name)
    blocks = build(name) * repeat

    def run(x):
        if c.get("detector"):
            d = O.Detector(threshold=0.45)
            r = d.run(np.ascontiguousarray(x)); d.close()
            return r
        return oracle_frames(O, np.ascontiguousarray(x))

    start = (lambda f: f["pos"]) if c.get("detector") else (lambda f: f.info["start"])
    ns = len(blocks[0])
    if form == "reset":
        return [[run(b[s]) for s in range(ns)] for b in blocks]
    out = [[[] for _ in range(ns)] for _ in blocks]
    for s in range(ns):
        fr = run(np.concatenate([b[s] for b in blocks]))
        rng = block_ranges(blocks, s)
        for f in fr:
            k = next(i for i, (lo, hi) in enumerate(rng) if lo <= start(f) + 256 < hi)
            out[k][s].append(f)
    return out


def block_counts(name, form):
    """per block, counts() over all streams of the oracle's frames"""
    c = case(name)
    vb = int(c.get("env", {}).get("FXRX_VB_BLK", 0)) or None
    res = []
    for blk in oracle(name, form):
        fr = [f for per_stream in blk for f in per_stream]
        if c.get("detector"):
            res.append(dict(frames=len(fr)))
        else:
            res.append(counts([(f.header_valid, f.fec0, f.fec1, f.check, len(f.payload)) for f in fr], vb))
    return res
