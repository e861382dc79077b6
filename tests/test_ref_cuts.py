"""The captures and cut layouts of tests/cut_cases.py on the CPU: "the one-pass result" is a statement about the stream, not
about how it is fed.
  a. every capture is clear of the reference's margins and its frames come out in their declared roles;
  b. the oracle fed piece by piece at every layout's cuts (one handle, Sync.execute per piece) equals the oracle fed whole,
     field for field and symbol bit for bit, and the reference under ref_stream.compare;
  c. the pair of streams DESIGN.md section 6 recorded (ids 1540 / 1541): what the oracle delivers, whole and in two pieces;
  d. negative controls: wrongly cut receivers built from the reference must differ from it on the layout each names."""
import numpy as np
import pytest

import cut_cases as CC
import ref_stream as S
from stream_cases import check_roles

_W = {}


def _world(oracle, cap):
    if cap["name"] not in _W:
        x = CC.build(cap)
        ref, unc = S.receive(x, cap["threshold"])
        s = oracle.Sync(threshold=cap["threshold"])
        whole = list(s.execute(x))
        s.close()
        _W[cap["name"]] = (x, ref, unc, whole)
    return _W[cap["name"]]


def _piecewise(oracle, x, cuts, threshold=0.5):
    s = oracle.Sync(threshold=threshold)
    e = [0] + list(cuts) + [len(x)]
    for a, b in zip(e[:-1], e[1:]):
        s.execute(x[a:b])
    out = list(s.frames)
    s.close()
    return out


def _oracle_differences(a, b):
    """two lists of oracle frames, every field: list of strings"""
    if len(a) != len(b):
        return ["%d vs %d frames" % (len(a), len(b))]
    bad = []
    for f, g in zip(a, b):
        for k in ("header20", "header_valid", "payload", "payload_valid", "mod_scheme", "mod_bps", "check", "fec0", "fec1"):
            if getattr(f, k) != getattr(g, k):
                bad.append("frame at %d: %s" % (f.info["start"], k))
        for k, v in f.info.items():
            if np.float32(v).tobytes() != np.float32(g.info[k]).tobytes() if isinstance(v, float) else v != g.info[k]:
                bad.append("frame at %d: %s %r vs %r" % (f.info["start"], k, v, g.info[k]))
        if f.framesyms.tobytes() != g.framesyms.tobytes():
            bad.append("frame at %d: symbols" % f.info["start"])
    return bad


# ---------------------------------------------------------------------------------------------------- a. the captures
@pytest.mark.parametrize("cap", CC.CAPTURES, ids=lambda c: c["name"])
def test_captures_are_certain_and_in_their_roles(oracle, cap):
    x, ref, unc, whole = _world(oracle, cap)
    assert not unc, unc
    assert not check_roles(cap, ref, len(x)), check_roles(cap, ref, len(x))
    for kw in (dict(equalizer=True), dict(soft_header=True)):           # the options tests/test_gpu_cuts.py runs
        assert not S.receive(x, cap["threshold"], **kw)[1], kw
    assert not S.detect(x, cap["threshold"])[1]
    names = [n for n, _ in CC.layouts(cap)]
    assert {CC.ZERO_BLOCK, CC.THREE_CUTS, "frame 0: a-512", "frame 0: a+156", "frame 0: header symbol 230 +1", "frame 0: resume"} <= set(names)
    assert len(CC.many_blocks(cap["total"])) == 71


def test_the_qpsk_capture_holds_what_it_promises(oracle):
    q0, q1, q2 = CC.QPSK["frames"]
    assert CC.npay(q0) > 1025 and q1["at"] == q0["at"] + CC.length(q0) and q2["at"] == q1["at"] + CC.length(q1) + 257
    names = dict(CC.layouts(CC.QPSK))
    assert names["between the zero-gap frames 0 and 1"] == [q1["at"]]
    for j in (7, 8, 9, 1023, 1024, 1025, CC.npay(q0) - 1):
        assert "frame 0: payload symbol %d" % j in names
    ref = _world(oracle, CC.QPSK)[1]
    assert names["frame 0: last sample"] == [ref[0]["last"]] and names["frame 0: resume"] == [ref[0]["last"] + 1]      # the geometry is the reference's


# ---------------------------------------------------------------------------------------------------- b. the oracle, piecewise
@pytest.mark.parametrize("cap", CC.CAPTURES, ids=lambda c: c["name"])
def test_oracle_piecewise_equals_oracle_whole_and_the_reference(oracle, cap):
    x, ref, unc, whole = _world(oracle, cap)
    worst = {}
    bad = S.compare(ref, [S.view_oracle(f) for f in whole], x, worst=worst)
    assert not bad, bad
    for name, cuts in CC.layouts(cap) + [("72 blocks", CC.many_blocks(cap["total"]))]:
        d = _oracle_differences(whole, _piecewise(oracle, x, cuts, cap["threshold"]))
        assert not d, (cap["name"], name, cuts, d[:4])


# ---------------------------------------------------------------------------------------------------- c. the recorded pair
def test_recorded_pair_oracle_facts(fx, oracle):
    """(synth_stream goes through the library's FrameGen: the fx fixture builds it where it is missing)"""
    P = CC.PAIR
    for s, x in enumerate(CC.pair_streams(fx, 2 * P["block"])):
        q = oracle.Sync()
        whole = list(q.execute(x))
        q.close()
        found, valid = P["oracle_first_200k"][s]
        assert (len(whole), sum(f.payload_valid for f in whole)) == (found, valid), s
        starts = [f.info["start"] for f in whole]
        cross = P["straddler"] if s == 0 else P["neighbour_straddler"]
        assert cross in starts and cross < P["block"] < cross + P["frame_len"][s]
        if s == 0:
            assert starts[starts.index(cross) + 1] == P["next_start"] and whole[starts.index(cross)].payload_valid
        assert not _oracle_differences(whole, _piecewise(oracle, x, [P["block"]], None)), s


# ---------------------------------------------------------------------------------------------------- d. negative controls
def _summary(frames):
    return [(f["start"], bool(f["header_valid"]), bytes(f["header"]), f.get("payload"), f.get("payload_valid")) for f in frames]


def _blocks(x, cuts):
    e = [0] + list(cuts) + [len(x)]
    return list(zip(e[:-1], e[1:]))


def _fresh_detector_every_block(x, cuts):
    """the tail dropped at a cut"""
    out = []
    for a, b in _blocks(x, cuts):
        out += [dict(f, start=f["start"] + a) for f in S.receive(x[a:b], 0.5)[0]]
    return out


def _positions_not_advanced(x, cuts):
    """the tail kept, but a frame found in the carried tail is placed as if the tail started where the block does"""
    ref = S.receive(x, 0.5)[0]
    out = []
    for f in ref:
        blk = next(a for a, b in _blocks(x, cuts) if a <= f["last"] < b)            # the block that delivers it
        out.append(dict(f, start=f["start"] if f["start"] >= blk else f["start"] + (blk - f["floor"])))
    return out


def _zero_block_resets(x, cuts):
    """a block of no samples resets the stream"""
    out, a0 = [], 0
    bl = _blocks(x, cuts)
    for i, (a, b) in enumerate(bl):
        if (a == b and a > 0) or i == len(bl) - 1:
            end = b
            out += [dict(f, start=f["start"] + a0) for f in S.receive(x[a0:end], 0.5)[0]]
            a0 = end
    return out


@pytest.mark.parametrize("mutant,layout,spared", [(_fresh_detector_every_block, CC.MID_PAYLOAD, "frame 0: a-512"),
                                                   (_positions_not_advanced, CC.MID_PAYLOAD, "frame 0: a-512"),
                                                   (_zero_block_resets, CC.ZERO_BLOCK, CC.THREE_CUTS)])
def test_wrongly_cut_receivers_fail(oracle, mutant, layout, spared):
    x, ref, _, _ = _world(oracle, CC.QPSK)
    lay = dict(CC.layouts(CC.QPSK))
    assert _summary(mutant(x, lay[layout])) != _summary(ref), "the mutant passes on '%s'" % layout
    assert _summary(mutant(x, lay[spared])) == _summary(ref), "the mutant fails where its defect does not apply ('%s')" % spared
