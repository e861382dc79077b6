"""The sizing rules of a block's front (gr-liquiddsp_amd/csrc/fx_frontplan.h: segment length, taper, pre-lock scan depth, the cut of
every stream into walk jobs, frame-table, chain-table and arena capacities) against tests/frontplan_ref.py, a plain statement of the
same rules written from the host runtime before they moved to the header.  The header is compiled into a small host-only driver
(tests/cpp/frontplan_check.cpp) with g++ under AddressSanitizer and UndefinedBehaviorSanitizer, which prints every value of every
function for the cases this module writes; every line must agree, and the properties the runtime relies on are asserted from what
the driver printed, for every case:

* a stream's cuts tile [0, n) in order, exactly one of them is `first`, and every stream has a job;
* an interior boundary of a tapered stream is a multiple of 256 and at least 4096 past its start;
* no untapered segment is shorter than half the segment length, except the first of a continuing stream (8192 samples by rule) and
  the only segment of a stream (a stream shorter than half a segment has nothing to be folded into);
* frame_base values are disjoint and ascend, the repair slots lie behind all job slots and end the table;
* the chain regions are contiguous and their capacities add up to chain_slots;
* the batch Viterbi allocations are the same at 192 and at 4096 steps per trellis block (a change of block length does not reallocate);
* the same inputs give the same plan twice (what a replay relies on).

Cases: the small rules on the full product of their inputs; the cut on every stream length x fresh / continuing x carry bound x
segment length x taper x mode; whole plans on the full product of modes and knobs (flex / detector, depth 1 / 4 / 12, 8 / 256 CUs,
segment_len 0 / 4096 / 8192 / 65536, taper -1 / 0 / 0.75, five pre-lock scan settings) x one, two and eight streams, the batch
Viterbi inputs (vb_steps x vb_blk_force x soft_decision x batch_viterbi: 24 settings) taken in turn.  Plans with the 40-Msample
stream run on a part of the knobs (the cut itself has that length at every segment length), and one 1.5-Gsample stream shows the
32-bit verdict."""
import itertools
import os
import subprocess

import frontplan_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")

LENGTHS = [0, 1, 255, 4095, 4096, 12_288, 40_000, 64_000, 1_000_000, 40_000_000]
CARRY = [0, 20_000]
SEGS = [0, 4096, 8192, 65536]
PRESCAN = [(0, -1, None), (1, -1, 0), (1, -1, 37), (1, 0, 37), (1, 24, 37)]      # prescan, prescan_hops, frames of the last block
VB = list(itertools.product([0, 5_000_000, 10**12], [0, 192], [0, 1], [1, 0]))   # vb_steps (the last far above 4 x span), force, soft, batch


def knob_grid():
    for detect, depth, n_cus, seg, taper, ps in itertools.product([0, 1], [1, 4, 12], [8, 256], SEGS, [-1.0, 0.0, 0.75], PRESCAN):
        yield R.DEFAULT._replace(detect=detect, depth=depth, n_cus=n_cus, segment_len=seg, taper=taper, prescan=ps[0], prescan_hops=ps[1]), ps[2] or 0


def stream_sets():
    """(streams, with the 40-Msample stream?)"""
    for n in LENGTHS:
        yield [(n, 0, 0)], n == 40_000_000
        for cb in CARRY:
            yield [(n, 1, cb)], n == 40_000_000
    yield [(64_000, 0, 0), (40_000, 1, 20_000)], False
    yield [(1_000_000, 1, 0), (0, 0, 0)], False
    yield [(40_000, 1, 20_000), (64_000, 1, 0)], False
    yield [(n, i % 2, CARRY[i // 2 % 2]) for i, n in enumerate(LENGTHS[:8])], False
    yield [(n, 1 - i % 2, CARRY[1 - i // 2 % 2]) for i, n in enumerate(reversed(LENGTHS[:9]))][:8], False
    yield [(n, i % 2, 20_000) for i, n in enumerate([40_000_000, 1, 1_000_000, 0, 64_000, 4095, 12_288, 255])], True


def ktext(k):
    return " ".join(str(v) for v in k)


def cuts_text(cuts):
    return "".join(" %d:%d:%d:%d" % c for c in cuts)


def make_cases():
    """(case line, expected answer lines, what the property checks need)"""
    cases = []
    for samples, detect in itertools.product(LENGTHS + [600, 2_399_400, 1_023_999], [0, 1]):
        cases.append(("cap %d %d" % (samples, detect), ["cap %d %d" % (R.frames_cap(samples, detect), R.seg_frames_cap(samples, detect))], None))
    totals = sorted({sum(n for n, _, _ in s) for s, _ in stream_sets()})
    seen = set()
    for (k, frames), tot in itertools.product(knob_grid(), totals):
        key = (k.detect, k.depth, k.n_cus, k.segment_len, k.taper, tot)
        if key in seen:
            continue
        seen.add(key)
        seg = R.segment_len(tot, k)
        cases.append(("seg %s %d" % (ktext(k), tot), ["seg %d" % seg], None))
        cases.append(("tap %s %d %d" % (ktext(k), tot, seg), ["tap %.9g" % R.choose_taper(tot, seg, k)], None))
    for detect, ps, samples in itertools.product([0, 1], PRESCAN, [0, 64_000, 1_000_000, 40_000_000]):
        for frames in ([0] if ps[2] is None else [0, 1, ps[2], 4000]):
            k, t = R.DEFAULT._replace(detect=detect, prescan=ps[0], prescan_hops=ps[1]), R.Traffic(frames, samples, 0)
            K = R.prescan_hops(t, k)
            cases.append(("ps %s %d %d" % (ktext(k), frames, samples), ["ps %d %d" % (K, R.prescan_words(K))], None))
    for n, cont, cb, seg, taper, detect in itertools.product(LENGTHS, [0, 1], CARRY, [4096, 8192, 32768, 65536, 1 << 20], [0.0, 0.75], [0, 1]):
        cuts = R.cut_stream(n, cont, cb, seg, taper, detect)
        cases.append(("cut %d %d %d %d %s %d" % (n, cont, cb, seg, taper, detect),
                      ["cut %d%s order%s" % (len(cuts), cuts_text(cuts), "".join(" %d" % i for i in R.launch_order(cuts, cont)))],
                      dict(kind="cut", streams=[(n, cont, cb)], seg=seg, taper=taper)))
    for (steps, force, soft, batch), detect, n_cus, span in itertools.product(VB, [0, 1], [8, 256], [0, 1, 104_000, 1_020_000, 40_020_000]):
        k, t = R.DEFAULT._replace(detect=detect, n_cus=n_cus, vb_blk_force=force, soft_decision=soft, batch_viterbi=batch), R.Traffic(0, 0, steps)
        blk = R.trellis_block(t, k)
        vals = (blk,) + R.size_trellis(span, steps, blk) + R.size_trellis(span, steps, 192) + R.size_trellis(span, steps, 4096)
        cases.append(("vb %s %d %d" % (ktext(k), steps, span), ["vb " + " ".join(str(v) for v in vals)], dict(kind="vb")))
    for frames, slots, forced in itertools.product([0, 1, 37, 4000], [8, 100, 5000], [0, 1, 64, 10**6]):
        cases.append(("win %d %d %d" % (frames, slots, forced), ["win %d" % R.window_slots(frames, slots, forced)], None))
    turn = itertools.cycle(VB)
    plans = [(k, frames, s) for (k, frames), (s, big) in itertools.product(knob_grid(), stream_sets())
             if not big or (k.segment_len in (0, 65536) and k.prescan == 0) or (k.depth == 1 and k.n_cus == 256 and k.taper < 0 and k.prescan == 0)]
    plans += [(R.DEFAULT._replace(detect=d, segment_len=1 << 20), 0, [(1_500_000_000, 1, 20_000)]) for d in (0, 1)]
    for k, frames, streams in plans:
        steps, force, soft, batch = next(turn)
        k = k._replace(vb_blk_force=force, soft_decision=soft, batch_viterbi=batch)
        t = R.Traffic(frames, 1_000_000, steps)
        p = R.front_plan(streams, t, k)
        want = ["plan seg %d taper %.9g ps %d jobs %d repair_cap %d caps %d %d %d %d %d %d %d %d %d %d %d %d too_large %d same 1" % (
            p["seg"], p["taper"], p["ps_hops"], p["n_jobs"], R.REPAIR_CAP, p["frame_slots"], p["chain_slots"], p["run_cap"], p["mf_cap"],
            p["sym_cap"], p["byte_cap"], p["dw_cap"], p["out_cap"], p["vb_blk"], *p["vb"], p["too_large"])]
        for s in p["streams"]:
            want.append("stream %d %d %d %d %d cuts%s frame_base%s" % (s["first_job"], len(s["cuts"]), s["chain_base"], s["chain_cap"], s["repair_base"],
                                                                       cuts_text(s["cuts"]), "".join(" %d" % b for b in s["frame_base"])))
        cases.append(("plan %s %d %d %d %d %s" % (ktext(k), t.frames, t.samples, t.vb_steps, len(streams), " ".join("%d %d %d" % s for s in streams)),
                      want, dict(kind="plan", streams=streams)))
    return cases


def parse_cuts(fields):
    return [tuple(int(v) for v in f.split(":")) for f in fields]


def check_cuts(cuts, n, cont, seg, taper, where):
    assert len(cuts) >= 1 and cuts[0][0] == 0 and cuts[-1][1] == n, where
    assert all(a[1] == b[0] for a, b in zip(cuts, cuts[1:])) and all(c[0] < c[1] for c in cuts if n), where
    assert [c[3] for c in cuts] == [1] + [0] * (len(cuts) - 1), where
    p_t, k_t = R.taper_span(n, cont, seg)
    tapered = taper > 0 and k_t > 1
    for start, stop, _, first in cuts:
        if tapered and start >= p_t:
            assert stop == n or (stop % 256 == 0 and stop - start >= 4096), (where, start, stop)
        elif not (first and cont) and len(cuts) > 1:
            assert stop - start >= seg // 2, (where, start, stop)


def check_properties(case, got, info):
    f = got[0].split()
    if info["kind"] == "vb":
        assert f[6:8] == f[9:11], (case, got)              # decision words and per-item records: the same at 192 and at 4096 steps a block
        return
    if info["kind"] == "cut":
        (n, cont, _), = info["streams"]
        check_cuts(parse_cuts(f[2:f.index("order")]), n, cont, info["seg"], info["taper"], case)
        return
    seg, taper, frame_slots, chain_slots = int(f[2]), float(f[4]), int(f[12]), int(f[13])
    assert f[-1] == "1" and f[-2] == "same", case
    assert len(got) == 1 + len(info["streams"]), case
    slot_end = chain_end = job_end = 0
    repairs = []
    for (n, cont, _), line in zip(info["streams"], got[1:]):
        g = line.split()
        first_job, n_jobs, chain_base, chain_cap, repair_base = (int(v) for v in g[1:6])
        cuts, bases = parse_cuts(g[7:g.index("frame_base")]), [int(v) for v in g[g.index("frame_base") + 1:]]
        assert n_jobs == len(cuts) == len(bases) >= 1 and first_job == job_end, case
        check_cuts(cuts, n, cont, seg, taper, case)
        for c, b in zip(cuts, bases):
            assert b >= slot_end, (case, b, slot_end)
            slot_end = b + c[2]
        assert chain_base == chain_end, case
        chain_end += chain_cap
        job_end += n_jobs
        repairs.append(repair_base)
    assert job_end == int(f[8]) and chain_end == chain_slots, case
    for r in repairs:
        assert r >= slot_end, (case, r, slot_end)
        slot_end = r + int(f[10])
    assert slot_end == frame_slots, case


def test_frontplan_header_against_plain_rules(tmp_path):
    exe, path = str(tmp_path / "frontplan_check"), str(tmp_path / "cases.txt")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__"] + SAN +
                          ["-o", exe, os.path.join(ROOT, "tests", "cpp", "frontplan_check.cpp")])
    cases = make_cases()
    with open(path, "w") as f:
        f.write("".join(c[0] + "\n" for c in cases))
    r = subprocess.run([exe, path], capture_output=True, text=True, env=ENV, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    lines = r.stdout.splitlines()
    assert lines[-1] == "%d cases" % len(cases)
    at = 0
    kinds = set()
    for case, want, info in cases:
        got = lines[at:at + len(want)]
        at += len(want)
        assert got == want, (case, [(g[:300], w[:300]) for g, w in zip(got, want) if g != w][:3])
        if info:
            check_properties(case, got, info)
            kinds.add(info["kind"])
    assert at == len(lines) - 1 and kinds == {"cut", "vb", "plan"}
    assert any(w[0].endswith("too_large 1 same 1") for _, w, _ in cases)
