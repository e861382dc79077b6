"""Clean frames finish in fx_vbpre_kernel (their tail -- de-whitening, CRC, payload and record to the host -- runs where the
codeword check has just written the message), and the trellis kernels join a block's chain only while the traffic has frames
for them; a block that meets such a frame without them is completed when it is collected (late_decodes).  Every case is run
with the early tail on and off (FXRX_VB_EARLY_TAIL=0: tail in fx_vbfinish_kernel, trellis launched with every block), the two
must give identical frames, and the frames are those of the CPU oracle."""
import numpy as np
import pytest

from parity_util import oracle_frames, compare_frames

CONV_V27, CONV_V27P23, HAMMING74 = 11, 15, 4


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


def _run(fx, monkeypatch, early, blocks, depth=1, reset=True):
    """blocks: a list of blocks, each a list with one array per stream; reset: every block is an independent capture.
    Returns (frames per block, timing() per block)."""
    monkeypatch.setenv("FXRX_VB_EARLY_TAIL", "1" if early else "0")
    ctx = fx.RxContext(len(blocks[0]), want_framesyms=True)
    ctx.set_depth(depth)
    res, tms, inflight = [], [], 0

    def collect():
        res.append(ctx.results(ctx.collect_raw())); tms.append(ctx.timing())
    for b in blocks:
        if inflight == depth:
            collect(); inflight -= 1
        if reset:
            ctx.reset()
        ctx.submit_raw([a.ctypes.data for a in b], [len(a) for a in b], False); inflight += 1
    while inflight:
        collect(); inflight -= 1
    ctx.close()
    return res, tms


def _both(fx, monkeypatch, blocks, **kw):
    on, tm_on = _run(fx, monkeypatch, True, blocks, **kw)
    off, tm_off = _run(fx, monkeypatch, False, blocks, **kw)
    assert len(on) == len(off)
    for a, b in zip(on, off):
        _same(a, b)
    assert all(t["trellis_launched"] == 1 for t in tm_off)
    return on, tm_on, tm_off


@pytest.mark.gpu
def test_all_clean_blocks_need_one_decode_launch(fx, oracle, monkeypatch):
    x, injected = fx.synth_stream(150_000, stream_id=1500)
    assert len(injected) == 8
    on, tm, _ = _both(fx, monkeypatch, [[x]] * 3)
    ref = oracle_frames(oracle, x)
    for got in on:
        compare_frames(ref, got)
        assert all(g["payload_valid"] and g["payload"] == pl for g, (_, pl) in zip(got, injected))
    assert tm[0]["trellis_launched"] == 1                                     # nothing known about the traffic yet
    for t in tm[1:]:
        assert t["trellis_launched"] == 0 and t["late_decodes"] == tm[0]["late_decodes"] and t["vb_clean"] == len(injected)


@pytest.mark.gpu
def test_never_clean_frames_keep_the_trellis_in_the_chain(fx, oracle, monkeypatch):
    """A punctured inner code (rate 2/3: no codeword check), and rate-1/2 packets of 6 KB coded (beyond the front part's LDS
    buffer: no check either)."""
    xa, ia = fx.synth_stream(120_000, stream_id=1510, fec0=CONV_V27P23, payload_len=600)
    xb, ib = fx.synth_stream(120_000, stream_id=1511, payload_len=3000)
    assert len(ia) >= 2 and len(ib) >= 2
    on, tm, _ = _both(fx, monkeypatch, [[xa, xb]] * 3)
    refs = [oracle_frames(oracle, xa), oracle_frames(oracle, xb)]
    for got in on:
        for s in range(2):
            compare_frames(refs[s], [g for g in got if g["stream"] == s])
        assert all(g["payload_valid"] for g in got)
    for t in tm:
        assert t["trellis_launched"] == 1 and t["vb_clean"] == 0
        assert t["late_decodes"] == tm[0]["late_decodes"]


@pytest.mark.gpu
def test_outer_block_code_over_a_clean_inner_code(fx, oracle, monkeypatch):
    x, injected = fx.synth_stream(150_000, stream_id=1520, fec1=HAMMING74, payload_len=500)
    assert len(injected) >= 4
    on, tm, _ = _both(fx, monkeypatch, [[x]] * 2)
    ref = oracle_frames(oracle, x)
    for got in on:
        compare_frames(ref, got)
        assert all(g["payload_valid"] and g["payload"] == pl and g["fec1"] == HAMMING74 for g, (_, pl) in zip(got, injected))
    assert tm[1]["trellis_launched"] == 0 and tm[1]["vb_clean"] == len(injected) and tm[1]["late_decodes"] == tm[0]["late_decodes"]


@pytest.fixture(scope="module")
def noisy_case(fx, oracle):
    """A 20 dB and a 5 dB capture (fixed seeds) with their oracle frames; at 5 dB the raw bit error rate is about 4e-2, so no
    1024-byte frame arrives as a codeword, while the Viterbi decoder still mends them."""
    xc, ic = fx.synth_stream(150_000, stream_id=1530)
    xn, inn = fx.synth_stream(150_000, stream_id=1531, snr_db=5.0)
    oc, on = oracle_frames(oracle, xc), oracle_frames(oracle, xn)
    assert len(oc) == len(ic) and all(f.payload_valid for f in oc)
    assert sum(1 for f in on if f.header_valid) >= 4
    return xc, xn, oc, on


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [4, 1])
def test_stream_turning_noisy(fx, noisy_case, monkeypatch, depth):
    xc, xn, oc, on_ = noisy_case
    n0, n_noisy, total = 6, 2, 32
    kinds = [n0 <= i < n0 + n_noisy for i in range(total)]
    blocks = [[xn if k else xc] for k in kinds]
    on, tm, tm_off = _both(fx, monkeypatch, blocks, depth=depth)
    for got, k in zip(on, kinds):
        compare_frames(on_ if k else oc, got)
    # the noisy blocks hold frames that are not codewords
    n_batch = sum(1 for f in on_ if f.header_valid)
    assert all(tm[i]["vb_clean"] < n_batch for i in range(n0, n0 + n_noisy))
    assert all(tm[i]["vb_clean"] == len(oc) for i in range(total) if not kinds[i])
    # blocks in flight without the trellis kernels pay one late decode each -- at most `depth` of them
    rise = tm[-1]["late_decodes"] - tm[n0 - 1]["late_decodes"]
    assert 1 <= rise <= depth, rise
    assert tm[n0 - 1]["late_decodes"] == tm[0]["late_decodes"] and tm[n0 - 1]["trellis_launched"] == 0
    assert tm_off[-1]["late_decodes"] == tm_off[0]["late_decodes"]
    # the first block submitted after the first noisy one was collected has them in its chain again, and so have those behind it
    assert tm[n0 + depth]["trellis_launched"] == 1 and tm[n0 + depth + 1]["trellis_launched"] == 1
    assert tm[n0 + depth]["late_decodes"] == tm[n0 + depth + 1]["late_decodes"] == tm[-1]["late_decodes"]
    # ... and after a while without such frames they are left out again
    assert tm[-1]["trellis_launched"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("dbg", [1, 2])
def test_forced_wrong_guesses_and_unrepaired_handovers(fx, oracle, monkeypatch, dbg):
    """FXRX_VB_DEBUG 1 (wrong traceback guesses) and 2 (hand-overs left unrepaired: frames go back to the wave-per-frame decoder)
    on the continuing streams of test_gpu_vb_clean.py's case of the same kind: clean (14 dB) and trellis (4 dB) frames mixed,
    blocks of 100 k samples, three in flight."""
    xa = fx.synth_stream(900_000, stream_id=1400, payload_len=500, snr_db=14.0)[0]
    xb = fx.synth_stream(900_000, stream_id=1401, payload_len=800, snr_db=4.0)[0]
    monkeypatch.setenv("FXRX_VB_DEBUG", str(dbg))
    blocks = [[xa[i:i + 100_000], xb[i:i + 100_000]] for i in range(0, len(xa), 100_000)]
    on, tm, _ = _both(fx, monkeypatch, blocks, depth=3, reset=False)
    got = [g for blk in on for g in blk]
    assert sum(t["vb_clean"] for t in tm) > 0
    for s, x in enumerate((xa, xb)):
        compare_frames(oracle_frames(oracle, x), [g for g in got if g["stream"] == s])
