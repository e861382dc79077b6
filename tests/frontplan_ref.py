"""A plain statement of the sizing rules of a block's front -- segment length, taper, pre-lock scan depth, the cut of a stream into
walk jobs, and the capacities of tables and arenas --, written from the host runtime's enqueue_block as it stood before the rules
moved to gr-liquiddsp_amd/csrc/fx_frontplan.h: one loop over the streams with running totals, as that function had it.
tests/test_frontplan.py compares the header with it value by value; tests/test_gpu_frontplan.py takes the job count from it."""
from collections import namedtuple

import numpy as np

HOP, CHUNK, REPAIR_CAP = 256, 16, 256
U32 = 0xFFFFFFFF

Knobs = namedtuple("Knobs", "detect depth n_cus walk_per_cu segment_len taper prescan prescan_hops batch_viterbi soft_decision vb_blk_force")
Traffic = namedtuple("Traffic", "frames samples vb_steps")
DEFAULT = Knobs(detect=0, depth=1, n_cus=256, walk_per_cu=2, segment_len=0, taper=-1.0, prescan=0, prescan_hops=-1, batch_viterbi=1,
                soft_decision=0, vb_blk_force=0)


def frames_cap(samples, detect):
    """one frame per 600 samples (a detection per hop in detector mode), plus 8"""
    return samples // (256 if detect else 600) + 8


def seg_frames_cap(samples, detect):
    return min(frames_cap(samples, detect), 4000)


def segment_len(tot, k):
    seg = k.segment_len
    if seg == 0:
        slots = k.n_cus * k.walk_per_cu
        if k.depth > 1 and not k.detect:
            seg = tot // max(max(1, k.n_cus), min(slots, 6 * slots // k.depth))
        elif tot // slots < 131072:
            seg = tot // (slots - slots // 16)
        else:
            seg = max(tot // (4 * slots), 65536)
        seg = min(max(seg, 32768), 1 << 20)
    return max(seg, 4096)


def choose_taper(tot, seg, k):
    if k.taper >= 0:
        return float(np.float32(k.taper))
    return 0.75 if k.detect and tot // seg > 4 * k.n_cus else 0.0


def prescan_hops(t, k):
    if not k.prescan or k.detect:
        return 0
    if k.prescan_hops >= 0:
        return k.prescan_hops
    K = min(128, max(16, t.samples // t.frames // HOP + 2)) if t.frames else 64
    return (K + CHUNK - 1) // CHUNK * CHUNK


def prescan_words(K):
    return (K + CHUNK - 1) // CHUNK


def taper_span(n, cont, seg):
    """(p_t, k_t): the taper covers [p_t, n) in k_t pieces"""
    seg0 = min(seg, 8192) if cont else seg
    p_t = min(n, seg0) if cont else 0
    return p_t, max(1, ((n - p_t) + seg // 2) // seg)


def cut_stream(n, cont, carry_bound, seg, taper, detect):
    """the stream's walk jobs as (start, stop, max_frames, first)"""
    seg0 = min(seg, 8192) if cont else seg
    p_t, k_t = taper_span(n, cont, seg)
    if not taper > 0:
        k_t = 0
    cuts, p, first, i_t = [], 0, True, 0
    while first or p < n:
        stop = min(n, p + (seg0 if first else seg))
        if n - stop < seg // 2:
            stop = n
        if k_t > 1 and p >= p_t:
            u = float(i_t + 1) / float(k_t)
            e = p_t + int(float(n - p_t) * (u * (1.0 + taper) - taper * u * u))
            stop = n if i_t + 1 >= k_t else min(n, max(p + 4096, e & ~255))
            i_t += 1
        cuts.append((p, stop, seg_frames_cap(stop - p + (carry_bound if first and cont else 0), detect), first))
        p, first = stop, False
        if p >= n:
            break
    return cuts


def launch_order(cuts, cont):
    """the speculative jobs under a taper: longest first, equal lengths in their order"""
    return sorted((i for i, c in enumerate(cuts) if not (c[3] and cont)), key=lambda i: -(cuts[i][1] - cuts[i][0]))


def trellis_block(t, k):
    if k.detect or k.soft_decision or not k.batch_viterbi:
        return 0
    want_items = 64 * 4 * k.n_cus * 6
    blk = min(4096, max(192, ((t.vb_steps // want_items + 63) // 64) * 64))
    return k.vb_blk_force if k.vb_blk_force else blk


def size_trellis(span, vb_steps, blk):
    """(work items, decision words, per-item records) of the batch Viterbi arenas"""
    if not blk:
        return 128, 0, 128
    steps_cap = min(max(span + span // 2, vb_steps + vb_steps // 4), 4 * span)
    vb_cap = ((steps_cap // blk + 2048 + 127) & ~127) & U32
    return vb_cap, max(vb_cap * blk, steps_cap + 2176 * 4096), max(vb_cap, steps_cap // 192 + 2176)


def window_slots(frames, chain_slots, forced):
    return min(chain_slots, forced) if forced else min(chain_slots, max(0, frames + frames // 2 + 64))


def front_plan(streams, t, k):
    """streams: (n, cont, carry_bound) each.  Everything the block's front is sized by, as a dict"""
    tot = sum(n for n, _, _ in streams)
    seg = segment_len(tot, k)
    taper = choose_taper(tot, seg, k)
    frame_slots = chain_slots = n_total = carry_total = n_jobs = 0
    per_stream = []
    for n, cont, cb in streams:
        cuts, bases = cut_stream(n, cont, cb, seg, taper, k.detect), []
        for c in cuts:
            bases.append(frame_slots)
            frame_slots = (frame_slots + c[2]) & U32
        chain_cap = ((n + (cb if cont else 0)) // (256 if k.detect else 600) + 8) & U32
        per_stream.append(dict(first_job=n_jobs, cuts=cuts, frame_base=bases, chain_base=chain_slots, chain_cap=chain_cap))
        chain_slots = (chain_slots + chain_cap) & U32
        n_jobs += len(cuts)
        n_total += n
        carry_total += cb if cont else 0
    for s in per_stream:
        s["repair_base"] = frame_slots
        frame_slots = (frame_slots + REPAIR_CAP) & U32
    span = n_total + carry_total
    blk = trellis_block(t, k)
    p = dict(seg=seg, taper=taper, ps_hops=prescan_hops(t, k), n_jobs=n_jobs, streams=per_stream, frame_slots=frame_slots, chain_slots=chain_slots,
             run_cap=min(span // HOP + 2 * n_jobs + 1024, 0x7FFFFFFF), mf_cap=min(span // 2 // 1024 + chain_slots + 16, 0x7FFFFFFF),
             sym_cap=span // 2 + 8 * chain_slots + 64, byte_cap=(span // 2) * 3 // 4 + 48 * chain_slots + 64,
             dw_cap=0 if k.detect else (span // 2) * 6 + 200 * chain_slots + 64, out_cap=(span // 2) * 3 // 4 + 16 * chain_slots + 64,
             vb_blk=blk, vb=size_trellis(span, t.vb_steps, blk))
    p["too_large"] = int(p["sym_cap"] >= 1 << 32 or p["dw_cap"] >= 1 << 32)
    return p
