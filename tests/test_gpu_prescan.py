"""The pre-lock scan of the speculative segments' first hops ahead of their walkers (fx_prescan_kernel, FXRX_PRESCAN, DESIGN.md
section 2.1).  Every case runs the same input twice, with FXRX_PRESCAN=0 and =1: the two runs agree frame for frame and field
for field (evm_sum bit for bit, payloads and carrier-recovered symbols included), and they are the CPU oracle's frames.
fxrx_debug_prescan_stats says what the walkers did with the scan's table.  `-m gpu`."""
import numpy as np
import pytest

import cut_cases as CC
import ref_detect as rd
from parity_util import compare_frames, oracle_frames

pytestmark = pytest.mark.gpu

HOP, NFFT, S_LEN, CHUNK = 256, 512, 156, 16


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


def _run(fx, monkeypatch, blocks, on, hops=None, depth=1, **cfg):
    """blocks: a list of blocks, each a list with one array per stream.  Returns (frames of all blocks in order of delivery,
    timing() per block, prescan_stats() per block)."""
    monkeypatch.setenv("FXRX_PRESCAN", "1" if on else "0")
    if hops is None:
        monkeypatch.delenv("FXRX_PRESCAN_HOPS", raising=False)
    else:
        monkeypatch.setenv("FXRX_PRESCAN_HOPS", str(hops))
    ctx = fx.RxContext(len(blocks[0]), want_framesyms=True, **cfg)
    ctx.set_depth(depth)
    got, tms, stats, inflight = [], [], [], 0

    def collect():
        got.extend(ctx.results(ctx.collect_raw())); tms.append(ctx.timing()); stats.append(ctx.prescan_stats())
    for b in blocks:
        if inflight == depth:
            collect(); inflight -= 1
        ctx.submit_raw([a.ctypes.data for a in b], [len(a) for a in b], False); inflight += 1
    while inflight:
        collect(); inflight -= 1
    ctx.close()
    return got, tms, stats


def _both(fx, monkeypatch, blocks, refs, hops=None, **kw):
    """Off and on; identical, and the oracle's (refs: its frames per stream).  Returns (off, on) as _run gives them."""
    off = _run(fx, monkeypatch, blocks, False, hops, **kw)
    on = _run(fx, monkeypatch, blocks, True, hops, **kw)
    assert all(s == (0, 0, 0) for s in off[2]), off[2]
    _same(off[0], on[0])
    for s, ref in enumerate(refs):
        compare_frames(ref, [g for g in on[0] if g["stream"] == s])
    return off, on


@pytest.fixture(scope="module")
def clean(fx, oracle):
    """One 20 dB stream of short frames (computed once, never changed): the array, where its frames were put, the oracle's frames."""
    x, injected = fx.synth_stream(300_000, stream_id=1601, payload_len=200)
    ref = oracle_frames(oracle, x)
    assert len(ref) == len(injected) >= 40 and all(f.payload_valid for f in ref)
    return x, injected, ref


def _frame_len(injected):
    return injected[1][0] - injected[0][0] - 256


SEGS = [4096, 8192, 20000, 65536]


@pytest.mark.parametrize("seg", SEGS)
def test_fixed_segment_lengths(fx, clean, monkeypatch, seg):
    x, injected, ref = clean
    _, on = _both(fx, monkeypatch, [[x]], [ref], segment_len=seg)
    print("segment %d: prescan stats %r, hops_cheap %d" % (seg, on[2][0], on[1][0]["hops_cheap"]))
    assert on[2][0][0] == on[1][0]["walk_jobs"] - 1 and on[2][0][1] + on[2][0][2] == on[2][0][0]


def test_segment_starts_at_every_position_of_a_frame(fx, clean, monkeypatch):
    """The second segment starts exactly on a frame's first sample, 1 and 255 samples before it, 1 sample after it, inside its
    header, and in the gap behind it (the other boundaries fall where they fall)."""
    x, injected, ref = clean
    p = injected[5][0]
    flen = _frame_len(injected)
    for name, start in (("on the first sample", p), ("1 before", p - 1), ("255 before", p - 255), ("1 after", p + 1), ("in the header", p + 400),
                        ("in the gap", p + flen + 100)):
        _, on = _both(fx, monkeypatch, [[x]], [ref], segment_len=start)
        print("segment start %s (%d): stats %r" % (name, start, on[2][0]))


def test_lags_at_the_ends_of_the_accepted_range(fx, clean, monkeypatch):
    """The second segment starts d samples in front of a frame's aligned start a0.  Hop 0 -- zeros below the floor -- holds the
    preamble at lag 256 + d (accepted below 356: d < 100), hop 1 at lag d, hop 2 at lag d - 256: the values put it below lag 8 and
    at or above lag 512 - 156 - 12 = 344 of the hop that sees it first, just inside and just outside the range, and one
    sample in front of the floor."""
    x, injected, ref = clean
    a0 = ref[6].info["start"]
    for d in (-1, 0, 1, 4, 7, 88, 92, 99, 100, 101, 107, 255, 256, 263, 344, 350, 355, 356, 357, 363, 511, 512, 600):
        _, on = _both(fx, monkeypatch, [[x]], [ref], segment_len=a0 - d)
        print("a0 - %d: stats %r" % (d, on[2][0]))


def _far_segment(ref, n, lo, hi, clear_hops):
    """A segment length whose every boundary has no frame start within clear_hops hops behind it (nor a hop in front of it)."""
    starts = np.array([f.info["start"] for f in ref])
    for seg in range(lo, hi):
        b = np.arange(seg, n - seg // 2, seg)
        d = starts[None, :] - b[:, None]
        if not np.any((d > -2 * HOP) & (d < (clear_hops + 2) * HOP)):
            return seg
    raise AssertionError("no such segment length")


def test_k_too_short_and_k_zero(fx, clean, monkeypatch):
    """FXRX_PRESCAN_HOPS=4 and no frame start within six hops of a segment start: every job falls back at hop 4.  =0: no scan."""
    x, injected, ref = clean
    assert _frame_len(injected) > 8 * HOP
    seg = _far_segment(ref, len(x), 30_000, 60_000, 4)
    _, on = _both(fx, monkeypatch, [[x]], [ref], hops=4, segment_len=seg)
    jobs = on[1][0]["walk_jobs"]
    assert jobs >= 4 and on[2][0] == (jobs - 1, 0, jobs - 1), (seg, on[2][0], jobs)
    off, on = _both(fx, monkeypatch, [[x]], [ref], hops=0, segment_len=seg)
    assert on[2][0] == (0, 0, 0) and on[1][0]["hops_cheap"] == off[1][0]["hops_cheap"] and on[1][0]["walk_jobs"] == jobs


def test_k_longer_than_the_segment_and_the_data(fx, clean, monkeypatch):
    """Segments of 4096 samples (16 hops) with 128 hops asked for; a block length that is no multiple of 256; a last segment that
    ends one, three and five hops (and a few samples) behind its start's grid."""
    x, injected, ref = clean
    for n in (len(x) - 77, 4096 * 40 + 2048 + 300, 4096 * 40 + 2048 + 3 * HOP + 1, 4096 * 40 + 2048 + 5 * HOP - 1):
        xr = np.ascontiguousarray(x[:n])
        r = [f for f in ref if f.info["start"] + _frame_len(injected) + 2 * NFFT < n]
        off = _run(fx, monkeypatch, [[xr]], False, 128, segment_len=4096)
        on = _run(fx, monkeypatch, [[xr]], True, 128, segment_len=4096)
        _same(off[0], on[0])
        assert len(on[0]) >= len(r)
        compare_frames(r, on[0][:len(r)])
        print("n = %d: stats %r" % (n, on[2][0]))


def _template(oracle):
    return rd.build_template(oracle.table("fxr_preamble_pn", 64), oracle.table("fxr_tx_taps", 29, complex_=False))


def test_false_candidates(fx, oracle, monkeypatch):
    """Noise only; noise with bursts of the preamble at a carrier offset of 1.5 rad/sample, five times what the exact detector's
    sweep covers (24 bins of 2 pi / 512 = 0.29): the differential correlator does not see the offset and fires (0.72 of the
    energy against its threshold of 0.06), the exact detector stays silent; and the same at 0.6 rad/sample, where the exact
    detector still fires in a window of little else and the header is invalid."""
    rng = np.random.RandomState(1602)
    n = 200_000
    noise = (0.05 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
    _, on = _both(fx, monkeypatch, [[noise]], [[]], segment_len=8192)
    assert on[2][0][0] > 0
    s = _template(oracle)
    at = list(range(9000, n - 2000, 8192))                       # some 800 samples behind every segment start
    for cfo, silent in ((1.5, True), (0.6, False)):
        x = noise.copy()
        for p in at:
            x[p:p + S_LEN] += (s * np.exp(1j * cfo * np.arange(S_LEN))).astype(np.complex64)
        ref = oracle_frames(oracle, x)
        if silent:
            assert ref == []
            for p in at[:3]:
                assert rd.walk(x[p - 300:p + 700], s, 0.5)[0] is None      # the exact detector, on the float64 reference
        else:
            assert len(ref) >= len(at) // 2 and not any(f.header_valid for f in ref)
        _, on = _both(fx, monkeypatch, [[x]], [ref], segment_len=8192)
        print("bursts at %.1f rad/sample: stats %r" % (cfo, on[2][0]))
        assert on[2][0][1] >= len(at) // 2, "the bursts did not fire the differential correlator: the case proves nothing"


def test_low_snr_with_repairs(fx, oracle, monkeypatch):
    x = fx.synth_stream(400_000, stream_id=1541, snr_db=4.0, payload_len=800, return_payloads=False)
    ref = oracle_frames(oracle, x)
    off, on = _both(fx, monkeypatch, [[x]], [ref], segment_len=8192)
    print("repairs off %d on %d, stats %r" % (off[1][0]["repairs"], on[1][0]["repairs"], on[2][0]))
    assert off[1][0]["repairs"] > 0, "no hand-off miss in the run with the switch off: the case proves nothing"


@pytest.fixture(scope="module")
def pair(fx, oracle):
    xs = CC.pair_streams(fx, 400_000)
    return xs, [oracle_frames(oracle, x) for x in xs]


@pytest.mark.parametrize("depth", [3, 8])
def test_continuing_streams(fx, pair, monkeypatch, depth):
    """The recorded pair 1540 / 1541 as continuing blocks of 100 000 samples, default segments and tail gang."""
    xs, refs = pair
    blocks = [[x[i:i + CC.PAIR["block"]] for x in xs] for i in range(0, len(xs[0]), CC.PAIR["block"])]
    _, on = _both(fx, monkeypatch, blocks, refs, depth=depth)
    assert all(s[0] > 0 for s in on[2]), on[2]


def test_two_streams_of_different_lengths(fx, clean, pair, monkeypatch):
    x, injected, ref = clean
    xs, refs = pair
    short = np.ascontiguousarray(xs[0][:123_457])
    r = [f for f in refs[0] if f.info["start"] + CC.PAIR["frame_len"][0] + 2 * NFFT < len(short)]
    off = _run(fx, monkeypatch, [[x, short]], False, segment_len=16384)
    on = _run(fx, monkeypatch, [[x, short]], True, segment_len=16384)
    _same(off[0], on[0])
    compare_frames(ref, [g for g in on[0] if g["stream"] == 0])
    got1 = [g for g in on[0] if g["stream"] == 1]
    compare_frames(r, got1[:len(r)])


def test_the_scan_is_used(fx, clean, monkeypatch):
    """Every speculative job with a frame start within K hops of its segment start takes its candidate from the table.  The count is
    per block, not per job, and `near` is narrower than "a frame start within K hops": it counts only the jobs whose preamble lies
    wholly inside the scanned hops' new halves (first sample at or behind the segment start, last sample inside hop K - 1), the ones
    that cannot miss; with this capture every job is one of them, so `took` must be every job and none may fall back.
    Cheap hops: the walker adds h + 1 for a hit at hop h, where the switch-off run counts whole rounds of four (4 ceil((h + 1) / 4)),
    and behind the candidate the two runs are the same walk: the block's count is at most the switch-off run's."""
    x, injected, ref = clean
    seg, K = 20_000, 32
    starts = np.array([f.info["start"] for f in ref])
    bounds = list(range(seg, len(x) - seg // 2, seg))
    # a preamble wholly inside the scanned hops' new halves: its first sample at or behind the segment start, its last inside hop K - 1
    near = sum(1 for b in bounds if np.any((starts >= b) & (starts + S_LEN <= b + K * HOP)))
    off, on = _both(fx, monkeypatch, [[x]], [ref], hops=K, segment_len=seg)
    jobs, took, fell = on[2][0]
    print("jobs %d took %d fell back %d, %d with a frame start inside the scanned hops; hops_cheap off %d on %d" % (jobs, took, fell, near, off[1][0]["hops_cheap"], on[1][0]["hops_cheap"]))
    assert jobs == len(bounds) and took + fell == jobs
    assert near == jobs, "a segment of this capture has no whole preamble inside its scanned hops: the case is not what it was built to be"
    assert took == jobs and fell == 0
    assert on[1][0]["hops_cheap"] <= off[1][0]["hops_cheap"]
