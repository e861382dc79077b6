"""The front plan on the device: a block is cut into exactly the walk jobs the plain statement of the rules (tests/frontplan_ref.py)
gives for this chip's CU count, and where the cuts fall changes nothing that is received.  `-m gpu`.

Two streams of 64 000 and 40 000 samples a block, three consecutive blocks without a reset (the second and third continue: an
8192-sample first segment for the true walker, frames that straddle the block edges), at depth 1 and with all three in flight at
depth 4, in flex_rx and in detector mode, at the default segment length and at segment_len = 8192; one detector case under
FXRX_TAPER=0.75.  After each collect fxrx_debug_walk_jobs gives the block's job count; every block's frames are identical, field by
field, to those of the same blocks received with segment_len = 2^20 -- one job per stream, no speculative segment."""
import numpy as np
import pytest
import torch

import frontplan_ref as R
from test_gpu_traffic_shift import same

pytestmark = pytest.mark.gpu

THR = 0.45
BLOCK = (64_000, 40_000)
N_BLOCKS = 3
KNOBS = ("FXRX_TAPER", "FXRX_WALK_PER_CU", "FXRX_DEBUG_CUS", "FXRX_PRESCAN", "FXRX_PRESCAN_HOPS")


@pytest.fixture(scope="module")
def blocks(fx):
    """[block][stream] -> samples"""
    xs = [np.ascontiguousarray(fx.synth_stream(N_BLOCKS * n, stream_id=9500 + s, payload_len=300 + 100 * s)[0]) for s, n in enumerate(BLOCK)]
    return [[np.ascontiguousarray(x[b * n:(b + 1) * n]) for x, n in zip(xs, BLOCK)] for b in range(N_BLOCKS)]


def receive(fx, blocks, detect, depth, segment_len):
    """-> (frames, walk jobs) of every block"""
    ctx = fx.RxContext(len(BLOCK), mode=fx.MODE_DETECTOR, threshold=THR, segment_len=segment_len) if detect else fx.RxContext(len(BLOCK), segment_len=segment_len)
    ctx.set_depth(depth)
    out, pending = [], 0
    words = np.zeros(6 * 4096, np.uint32)

    def collect():
        frames = ctx.results(ctx.collect_raw())
        nj = fx.lib().fxrx_debug_walk_jobs(ctx.h, words.ctypes.data, 4096)
        out.append((frames, nj))

    for xs in blocks:
        if pending == depth:
            collect(); pending -= 1
        ctx.submit_raw([x.ctypes.data for x in xs], [len(x) for x in xs], False); pending += 1
    while pending:
        collect(); pending -= 1
    ctx.close()
    return out


@pytest.fixture(scope="module")
def one_job_per_stream(fx, blocks):
    mp = pytest.MonkeyPatch()
    for k in KNOBS:
        mp.delenv(k, raising=False)
    ref = {detect: receive(fx, blocks, detect, 1, 1 << 20) for detect in (False, True)}
    mp.undo()
    for detect in ref:
        assert [nj for _, nj in ref[detect]] == [len(BLOCK)] * N_BLOCKS
        assert all(len(frames) >= 8 for frames, _ in ref[detect]), [len(frames) for frames, _ in ref[detect]]
    return ref


def jobs_by_rule(detect, depth, segment_len, taper, block):
    k = R.DEFAULT._replace(detect=int(detect), depth=depth, n_cus=torch.cuda.get_device_properties(0).multi_processor_count, segment_len=segment_len, taper=taper)
    seg = R.segment_len(sum(BLOCK), k)
    t = R.choose_taper(sum(BLOCK), seg, k)
    return sum(len(R.cut_stream(n, int(block > 0), 0, seg, t, int(detect))) for n in BLOCK)


CASES = [(detect, depth, seg, None) for detect in (False, True) for depth in (1, 4) for seg in (0, 8192)] + [(True, 1, 8192, 0.75)]


@pytest.mark.parametrize("detect,depth,segment_len,taper", CASES, ids=lambda v: str(v))
def test_blocks_are_cut_by_the_rule_and_receive_the_same(fx, monkeypatch, blocks, one_job_per_stream, detect, depth, segment_len, taper):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    if taper is not None:
        monkeypatch.setenv("FXRX_TAPER", str(taper))
    got = receive(fx, blocks, detect, depth, segment_len)
    want_jobs = [jobs_by_rule(detect, depth, segment_len, -1.0 if taper is None else taper, b) for b in range(N_BLOCKS)]
    print("\nwalk jobs %s, by the rule %s; frames %s" % ([nj for _, nj in got], want_jobs, [len(f) for f, _ in got]))
    assert [nj for _, nj in got] == want_jobs
    if segment_len == 8192:
        assert min(want_jobs) > 2 * len(BLOCK)             # (the case does cut its streams)
    for (frames, _), (ref, _) in zip(got, one_job_per_stream[detect]):
        same(ref, frames)
