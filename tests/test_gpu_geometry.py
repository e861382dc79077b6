"""Launch geometry is placement only: whatever the waves per workgroup, workgroups per CU, segment taper, decoder choice or the
number of CUs the host plans for (FXRX_DEBUG_CUS), a block's frames are bit-identical to the default run's -- which is held to the
CPU oracle.  `-m gpu`.

On the 256-CU chip the small shapes of the other suites land in one branch of every decision keyed on the CU count (automatic segment
length and taper, trellis block length, packed trellis lanes, hops per verification run); FXRX_DEBUG_CUS=1, 8, 32 takes the others.
Each setting is shown to have changed something where the library offers a view of it: the walk-job count, the hops per walk job
under a taper, the trellis block length."""
import numpy as np
import pytest

import ref_decode as R
import ref_detect as rd
import shift_cases as SC
from parity_util import compare_frames, oracle_frames
from test_gpu_traffic_shift import same

pytestmark = pytest.mark.gpu

THR = 0.45
# (mod, fec0, fec1, payload bytes, SNR): all 11 modulations, and every code family on one side or the other
FORMATS = [(R.PSK2, R.FEC_NONE, R.FEC_NONE, 150, 25.0), (R.PSK4, R.FEC_V27, R.FEC_NONE, 1024, 20.0), (R.PSK8, R.FEC_V27P34, R.FEC_NONE, 700, 25.0),
           (R.PSK16, R.FEC_H74, R.FEC_NONE, 400, 28.0), (R.DPSK2, R.FEC_H128, R.FEC_NONE, 150, 25.0), (R.DPSK4, R.FEC_GOLAY, R.FEC_NONE, 300, 25.0),
           (R.DPSK8, R.FEC_SD22, R.FEC_NONE, 400, 28.0), (R.ASK4, R.FEC_V27, R.FEC_SD39, 300, 25.0), (R.QAM16, R.FEC_RS, R.FEC_NONE, 700, 25.0),
           (R.QAM32, R.FEC_V27, R.FEC_RS, 600, 28.0), (R.QAM64, R.FEC_V27P78, R.FEC_SD72, 1500, 30.0), (R.QAM16, R.FEC_V27, R.FEC_NONE, 600, 9.0)]
KNOBS = ("FXRX_PLL_WAVES", "FXRX_DEC_WAVES", "FXRX_WALK_PER_CU", "FXRX_VERIFY_PER_CU", "FXRX_SKIP_SEEK", "FXRX_MF_PER_CU", "FXRX_TAPER", "FXRX_BATCH_VITERBI",
         "FXRX_INCHAIN_REPAIR", "FXRX_DEBUG_CUS", "FXRX_VB_BLK", "FXRX_VB_DEBUG", "FXRX_TAIL_GANG")


@pytest.fixture(scope="module")
def flex_set(fx):
    """3 streams of about 150 k samples (the last format, QAM16 at 9 dB: frames that are not clean, so the trellis kernels run)"""
    xs = []
    for s in range(3):
        specs = [SC.P(1, 9200 + i, mod=m, fec0=f0, fec1=f1, n=n, snr=snr) for i, (m, f0, f1, n, snr) in enumerate(FORMATS) if i % 3 == s]
        xs.append(np.concatenate([SC.make_piece(dict(p, frames=max(2, 37_500 // SC.frame_len(p)))) for p in specs]))      # (four formats a stream, equal shares)
    assert all(120_000 <= len(x) <= 200_000 for x in xs), [len(x) for x in xs]
    return xs


@pytest.fixture(scope="module")
def det_set(fx):
    return [np.ascontiguousarray(fx.synth_stream(64_000, stream_id=9300 + s, payload_len=40 + 10 * s)[0]) for s in range(8)]


def run(fx, monkeypatch, xs, env, detect=False, depth=1, blocks=1):
    """-> (frames per block, timing() of the last block, hops per walk job of the last block)"""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    ctx = fx.RxContext(len(xs), mode=fx.MODE_DETECTOR, threshold=THR) if detect else fx.RxContext(len(xs), want_framesyms=True)
    ctx.set_depth(depth)
    out, inflight = [], 0
    for _ in range(blocks):
        if inflight == depth:
            out.append(ctx.results(ctx.collect_raw())); inflight -= 1
        ctx.reset()
        ctx.submit_raw([x.ctypes.data for x in xs], [len(x) for x in xs], False); inflight += 1
    while inflight:
        out.append(ctx.results(ctx.collect_raw())); inflight -= 1
    tm = ctx.timing()
    words = np.zeros(6 * 4096, np.uint32)
    nj = fx.lib().fxrx_debug_walk_jobs(ctx.h, words.ctypes.data, 4096)
    assert nj >= 0
    ctx.close()
    return out, tm, words.reshape(-1, 6)[:nj, 4].copy()


@pytest.fixture(scope="module")
def flex_default(fx, oracle, flex_set):
    mp = pytest.MonkeyPatch()
    out, tm, hops = run(fx, mp, flex_set, {})
    mp.undo()
    mods, fams = set(), set()
    for s, x in enumerate(flex_set):
        of = oracle_frames(oracle, x)
        compare_frames(of, [g for g in out[0] if g["stream"] == s])
        mods |= {f.mod_scheme for f in of if f.header_valid}
        fams |= {SC.family(f.fec0) for f in of if f.header_valid} | {SC.family(f.fec1) for f in of if f.header_valid}
    assert mods == set(R.PAYLOAD_MODS) and fams == {"conv", "rs", "other"}
    assert tm["vb_blocks"] > 0 and tm["vb_clean"] > 0 and tm["frames"] >= 50
    return out[0], tm, hops


@pytest.fixture(scope="module")
def det_default(fx, oracle, det_set):
    mp = pytest.MonkeyPatch()
    out, tm, hops = run(fx, mp, det_set, {}, detect=True)
    mp.undo()
    for s, x in enumerate(det_set):
        d = oracle.Detector(threshold=THR)
        od = d.run(x); d.close()
        mine = [g for g in out[0] if g["stream"] == s]
        assert [q["pos"] for q in od] == [g["start"] for g in mine] and len(od) >= 20
        assert all(rd.parity_ok(q, g)[0] for q, g in zip(od, mine))
    return out[0], tm, hops


FLEX_ENVS = [dict(FXRX_PLL_WAVES=1), dict(FXRX_PLL_WAVES=4), dict(FXRX_DEC_WAVES=1), dict(FXRX_DEC_WAVES=8), dict(FXRX_WALK_PER_CU=1), dict(FXRX_WALK_PER_CU=8),
             dict(FXRX_VERIFY_PER_CU=1, FXRX_SKIP_SEEK=1), dict(FXRX_VERIFY_PER_CU=64, FXRX_SKIP_SEEK=1), dict(FXRX_MF_PER_CU=1), dict(FXRX_MF_PER_CU=64),
             dict(FXRX_TAPER=0.5), dict(FXRX_TAPER=0.95), dict(FXRX_BATCH_VITERBI=0), dict(FXRX_INCHAIN_REPAIR=0), dict(FXRX_INCHAIN_REPAIR=2)]
_id = lambda e: ",".join("%s=%s" % (k[5:], v) for k, v in e.items())


@pytest.mark.parametrize("env", FLEX_ENVS, ids=_id)
def test_flex_rx_knobs(fx, monkeypatch, flex_set, flex_default, env):
    out, tm, hops = run(fx, monkeypatch, flex_set, env)
    same(flex_default[0], out[0])
    if "FXRX_BATCH_VITERBI" in env:
        assert tm["vb_blocks"] == 0 and flex_default[1]["vb_blocks"] > 0
    if "FXRX_TAPER" in env or "FXRX_WALK_PER_CU" in env:
        print("\n%s: walk jobs %d (default %d)" % (env, tm["walk_jobs"], flex_default[1]["walk_jobs"]))


@pytest.mark.parametrize("depth", [1, 4])
@pytest.mark.parametrize("cus", [1, 8, 32])
def test_flex_rx_planned_for_fewer_cus(fx, monkeypatch, flex_set, flex_default, cus, depth):
    """depth 4: the set five times over as independent captures, four in flight, tails ganged"""
    out, tm, hops = run(fx, monkeypatch, flex_set, dict(FXRX_DEBUG_CUS=cus), depth=depth, blocks=5 if depth == 4 else 1)
    for got in out:
        same(flex_default[0], got)
    print("\nCUs %d depth %d: walk jobs %d (default %d)" % (cus, depth, tm["walk_jobs"], flex_default[1]["walk_jobs"]))
    if cus == 1:
        assert tm["walk_jobs"] != flex_default[1]["walk_jobs"]


DET_RUNS = [(e, 1) for e in (dict(FXRX_TAPER=0.5), dict(FXRX_TAPER=0.95), dict(FXRX_WALK_PER_CU=1), dict(FXRX_WALK_PER_CU=8))] + \
           [(dict(FXRX_DEBUG_CUS=n), d) for n in (1, 8, 32) for d in (1, 4)]


@pytest.mark.parametrize("env,depth", DET_RUNS, ids=lambda v: _id(v) if isinstance(v, dict) else "depth%d" % v)
def test_detector_knobs(fx, monkeypatch, det_set, det_default, env, depth):
    out, tm, hops = run(fx, monkeypatch, det_set, env, detect=True, depth=depth, blocks=5 if depth == 4 else 1)
    for got in out:
        same(det_default[0], got)
    # a stream's two walk jobs, first over second, by the hops they took (256 samples a hop; a walker runs on past its segment to
    # the next detection, a frame of 5 to 6 hops away at the most: a fifth of the shorter segment under the steepest taper)
    def ratio(h):
        r = h[0::2].astype(float) / np.maximum(h[1::2], 1)
        return r.min(), r.max()
    print("\n%s depth %d: walk jobs %d (default %d), hops per job %s (default %s)" % (env, depth, tm["walk_jobs"], det_default[1]["walk_jobs"], hops.tolist(), det_default[2].tolist()))
    if env.get("FXRX_DEBUG_CUS") == 1:
        assert tm["walk_jobs"] != det_default[1]["walk_jobs"]
    if "FXRX_TAPER" in env:
        # two segments a stream: 32768 and 31232 samples by default, the integral of the line (1 + t) -> (1 - t) cut at its middle under a taper
        t = env["FXRX_TAPER"]
        want = (0.5 * (1 + t) - 0.25 * t) / (1.0 - (0.5 * (1 + t) - 0.25 * t))
        assert tm["walk_jobs"] == det_default[1]["walk_jobs"] == 2 * len(det_set)
        assert ratio(det_default[2])[1] <= 1.25 * 32768 / 31232 and ratio(hops)[0] >= 0.8 * want, (ratio(det_default[2]), ratio(hops), want)


def test_trellis_block_length_follows_the_traffic(fx, oracle, monkeypatch):
    """Planned for one CU, two continuing blocks of QAM64 rate-1/2 frames, the second with more of them: the first one's trellis
    steps ask for blocks longer than the shortest (192 steps), and the second block is cut into those -- n_vb_items says so."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("FXRX_DEBUG_CUS", "1")
    n = 1024
    blocks = [SC.make_piece(SC.P(k, 9400 + i, mod=R.QAM64, n=n, snr=25.0)) for i, k in enumerate((16, 24))]
    steps = SC.trellis_steps(n, R.CRC_24)
    ctx = fx.RxContext(1, want_framesyms=True)
    got, items = [], []
    for x in blocks:
        got += ctx.process([x])
        items.append(ctx.late_stats()[9])
    ctx.close()
    compare_frames(oracle_frames(oracle, np.concatenate(blocks)), got)
    print("\ntrellis work items per block %s for %s steps" % (items, [16 * steps, 24 * steps]))
    assert 16 * steps / items[0] <= 192 < 24 * steps / items[1], items
