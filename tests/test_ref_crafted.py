"""The crafted received words of tests/crafted_cases.py, without a GPU: each case is what its name says (error weights, tied
metrics, tie positions against the trellis block edges, metric spreads, Reed-Solomon error counts and places); the numpy
reference and the oracle's packet decoder agree on every crafted packet, hard and soft; and the oracle receiver, fed the
crafted IQ, finds every frame, accepts every header and demaps exactly the crafted word -- the condition under which
tests/test_gpu_crafted_decode.py may judge the kernels by these frames."""
import collections
import ctypes as C

import numpy as np
import pytest

import crafted_cases as CC
import ref_decode as R
from parity_util import oracle_frames


def inner_word(c):
    """what fec0's decoder reads: the packet through the de-interleavers and the (clean) outer decoder"""
    k, l0, l1 = R.packet_dims(c["n"], c["check"], c["fec0"], c["fec1"])
    return R.interleave(R.fec_decode(c["fec1"], R.interleave(c["pkt"], decode=True), l0), decode=True)


def ref_of(c):
    """(payload, valid), fec0 metric of a case, from the module-wide reference"""
    for (x, cs), (out, met) in zip(CC.streams(), CC.reference()):
        for i, d in enumerate(cs):
            if d is c:
                return out[i], met[i]
    raise KeyError(c["name"])


def test_case_list_shape():
    cs = CC.cases()
    assert dict(collections.Counter(c["family"] for c in cs)) == CC.FAMILY_COUNTS
    assert len({c["name"] for c in cs}) == len(cs)
    assert all(c["gap"] >= CC.GAP for c in cs)
    assert {c["mod"] for c in cs} == {R.PSK2, R.PSK4, R.QAM16}
    assert sum(len(s[1]) for s in CC.streams()) == len(cs)
    for fam in ("single", "burst", "tie", "tail", "garbage", "short", "outer"):
        assert {c["fec0"] for c in CC.of_family(fam)} == set(R.CONV), fam
    assert {c["fec1"] for c in CC.of_family("outer")} == {R.FEC_GOLAY, R.FEC_SD72, R.FEC_RS}
    ks = lambda fam: {c["n"] + R.crc_len(c["check"]) for c in CC.of_family(fam)}
    assert ks("single") == {1, 2, 16} and ks("burst") == {32} and ks("tie") == {48, 49} and ks("garbage") == {48, 1100} and ks("short") == {0, 1, 2}
    assert {1, 222, 223, 224, 446, 447} <= {c["n"] + R.crc_len(c["check"]) for c in CC.of_family("rs") if c["fec0"] == R.FEC_RS}


@pytest.mark.parametrize("fs", R.CONV)
def test_metric_spread(fs):
    """the recorded worst spreads are the search's; all stay under the six-step bound, and doubled under the kernels' stated
    bound; the garbage words hold what the table says"""
    pat, held, held_any, start = CC.spread_search(fs)
    assert (pat, held, start) == CC.SPREAD[fs] and held == held_any
    assert held <= start <= CC.SPREAD_BOUND and 2 * start < CC.KERNEL_BOUND_DOUBLED
    for c in CC.of_family("garbage"):
        if c["fec0"] != fs:
            continue
        k = c["n"] + R.crc_len(c["check"])
        if k > 48 and not c["name"].endswith(("spread", "zeros")):
            continue                                            # (8806 reference steps each: "ones" and "complement" are checked at k = 48 only, for time)
        sp = CC.spread_of(fs, inner_word(c), k)
        assert sp <= start, (c["name"], sp)
        if c["name"].endswith(("spread", "zeros")):
            assert sp >= held, (c["name"], sp, held)


def test_single_burst_tail_short_error_weights():
    """flips: coded bits (pad bits not counted) in which the inner word differs from the true codeword"""
    n_pad = 0
    for c in CC.of_family("single", "burst", "tail", "short", "outer"):
        if c.get("flips") is None:
            continue
        fs = c["fec0"]
        k = len(c["truth"])
        nb = CC.coded_bits(fs, k)
        d = R.bits_of(inner_word(c) ^ R.fec_encode(fs, c["truth"]))
        assert int(d[:nb].sum()) == c["flips"], c["name"]
        pad = int(d[nb:].sum())
        if "pad" in c["name"]:
            assert pad >= 1 and c["flips"] == 0, c["name"]
            n_pad += 1
        else:
            assert pad == 0, c["name"]
        if c["family"] == "burst":
            where = np.nonzero(d)[0]
            assert where[-1] - where[0] + 1 == c["flips"]
            if " start " in c["name"]: assert where[0] == 0
            if " end " in c["name"]: assert where[-1] == nb - 1
        (payload, valid), metric = ref_of(c)
        assert metric <= c["flips"]
    assert n_pad >= 7 * 3
    # single: every position of the first two periods, the last max(2 P, 6) steps and the pad bits
    for fs in R.CONV:
        for k in (1, 2, 16):
            got = {int(c["name"].split("bit")[1].split()[0]) for c in CC.of_family("single") if c["fec0"] == fs and len(c["truth"]) == k}
            P, tot = CC.period(fs), 8 * R.fec_enc_len(fs, k)
            want = set(range(min(2 * CC.bits_before(fs, P), tot))) | set(range(CC.bits_before(fs, CC.steps_of(k) - max(2 * P, 6)), tot))
            assert got == want, (fs, k)


def test_ties_are_ties_at_the_block_edges():
    """both codewords have the same metric against the received word; the reference's maximum-likelihood metric is not above
    it, and equals it at rate 1/2, where the pair's distance is the code's free distance (the punctured codes' ties are counted:
    most are maximum-likelihood too); the divergence steps are the block edges, the warm-up lengths and both ends"""
    free_rates, by = collections.Counter(), collections.defaultdict(set)
    for c in CC.of_family("tie", "outer"):
        if "tie" not in c:
            continue
        fs, word = c["fec0"], inner_word(c)
        bits = R.bits_of(word)
        ma, mb = R.conv_metric(fs, c["truth"], bits, 1), R.conv_metric(fs, c["other"], bits, 1)
        half = sum(d // 2 for _, _, d, _ in c["tie"])
        assert all(d % 2 == 0 and d >= 2 for _, _, d, _ in c["tie"])
        assert ma == mb == half, (c["name"], ma, mb, half)
        assert not np.array_equal(c["truth"], c["other"])
        (payload, valid), metric = ref_of(c)
        assert metric <= half
        if fs == R.FEC_V27:                                     # d = 10 is the code's free distance: nothing is nearer than d / 2
            assert all(d == 10 for _, _, d, _ in c["tie"]) and metric == half, c["name"]
        free_rates[fs] += int(metric == half)
        # the two messages differ from the divergence step on and nowhere before
        first = int(np.nonzero(R.bits_of(c["truth"] ^ c["other"]))[0][0])
        assert first == c["tie"][0][0]
        if c["family"] == "tie" and len(c["tie"]) == 1:
            by[(fs, len(c["truth"]))].add(c["tie"][0][0])
    for fs in R.CONV:
        for k in CC.TIE_K:
            want = {0}
            for B in CC.BLOCKS:
                want |= {B - 65, B - 64, B - 1, B, B + 1, B + 63, B + 64, B + 96, B + 128}
            assert want <= by[(fs, k)], (fs, k, sorted(want - by[(fs, k)]))
            last = max(by[(fs, k)])
            assert 8 * k - 16 < last <= 8 * k - 1                      # its difference path ends in the flush steps
            assert CC.steps_of(k) % 8 == 6 and all(B < 8 * k for B in CC.BLOCKS)
    two = [c for c in CC.of_family("tie") if len(c["tie"]) == 2]
    assert len(two) >= 14 and all(c["tie"][0][0] // B != c["tie"][1][0] // B for c in two for B in CC.BLOCKS if c["tie"][0][0] == B - 30)
    print("\nties whose pair is maximum-likelihood, per rate:", {CC.RATE[f]: n for f, n in free_rates.items()})
    assert all(free_rates[fs] >= 20 for fs in R.CONV)


def test_tails_and_clean_codewords():
    """non-zero tail: a valid code sequence (metric 0 against the unterminated encoder) that no zero-tailed message matches;
    pad bits set / last coded bit: metric 0 / 1.  The rate-1/2 cases counted as clean are exactly those whose coded bits
    re-encode from the decoded message."""
    for c in CC.of_family("tail"):
        (payload, valid), metric = ref_of(c)
        if "nonzero tail" in c["name"]:
            assert metric > 0, c["name"]
        elif "pad bits" in c["name"]:
            assert metric == 0 and valid and not np.array_equal(inner_word(c), R.fec_encode(c["fec0"], c["truth"]))
        else:
            assert metric == 1 and valid
    n_clean = 0
    for (x, cs), (out, met) in zip(CC.streams(), CC.reference()):
        for c, (payload, valid), m in zip(cs, out, met):
            if c["fec0"] != R.FEC_V27 or not CC.on_batch_path(c):
                continue
            k = c["n"] + R.crc_len(c["check"])
            dec = R.fec_decode(R.FEC_V27, inner_word(c), k)
            nb = CC.coded_bits(R.FEC_V27, k)
            same = np.array_equal(R.conv_encode_bits(R.FEC_V27, dec), R.bits_of(inner_word(c))[:nb])
            assert same == (m == 0), c["name"]
            n_clean += int(same)
    assert n_clean == sum(CC.clean_count(cs, met) for (x, cs), (out, met) in zip(CC.streams(), CC.reference())) > 10


def test_reed_solomon_cases():
    seen = collections.Counter()
    for c in CC.of_family("rs"):
        errs = c["rs_errors"]
        nb, N = errs.shape
        dl = N - 32
        w = (errs != 0).sum(axis=1)
        if c["rs_count"] is not None:
            assert (w == c["rs_count"]).all(), c["name"]
            if " data " in c["name"]: assert not errs[:, dl:].any()
            if " parity " in c["name"]: assert not errs[:, :dl].any()
            if " ends " in c["name"] and c["rs_count"] >= 2: assert errs[:, 0].all() and errs[:, -1].all()
            if " ends " in c["name"] and c["rs_count"] == 1: assert ((errs[:, 0] != 0) | (errs[:, -1] != 0)).all()
            assert set(np.unique(errs)) <= {0, 0x01} or set(np.unique(errs)) <= {0, 0xff}
            seen[(c["fec0"] == R.FEC_RS, c["rs_count"])] += 1
            seen[(c["fec0"] == R.FEC_RS, c["rs_count"], c["name"].split()[-2])] += 1
            if " ends " in c["name"] and c["rs_count"] == 1 and nb == 1:
                seen[(c["fec0"] == R.FEC_RS, "lone error at the", "last" if errs[0, -1] else "first")] += 1
        rx = (c["rs_codeword"].reshape(nb, N) ^ errs)
        fixed = [R.rs_decode_block(b)[1] for b in rx]
        (payload, valid), _ = ref_of(c)
        truth = R.scramble(c["truth"])[:c["n"]].tobytes()
        if c["rs_count"] is not None and c["rs_count"] <= 16:
            assert fixed == [c["rs_count"]] * nb and payload == truth and valid, c["name"]
        elif c["rs_count"] == 17:
            assert fixed == [-1] * nb, (c["name"], fixed)                    # 17 random errors: no codeword within 16
        elif "all-zero" in c["name"]:
            assert not rx.any() and fixed == [0] * nb                       # the zero word is a codeword
            seen[(c["fec0"] == R.FEC_RS, "zero", nb)] += 1
        elif "other codeword" in c["name"]:
            assert (w >= 17).all() and fixed == [15] * nb
            assert all(np.array_equal(R.rs_decode_block(b)[0], o) for b, o in zip(rx, c["rs_other"].reshape(nb, N)))
            if c["fec0"] == R.FEC_RS:                               # (over V27 the inner decoder may repair the other codeword's byte)
                assert payload != truth
            seen[(c["fec0"] == R.FEC_RS, "other")] += 1
        else:
            bad = int(c["name"].split("block ")[1].split()[0])
            assert nb >= 3 and 0 < bad < nb - 1 and fixed == [-1 if b == bad else 0 for b in range(nb)]
            seen[(c["fec0"] == R.FEC_RS, "beyond")] += 1
    for fec0 in (True, False):                                              # both roles: as fec0, and as fec1 over V27
        for count in (0, 1, 8, 15, 16, 17):
            assert seen[(fec0, count)] >= 1, (fec0, count)
            for where in ("data", "parity", "ends") if count else ("ends",):
                assert seen[(fec0, count, where)] >= 1, (fec0, count, where)
        assert seen[(fec0, "other")] >= 3 and seen[(fec0, "beyond")] >= 2
        assert all(seen[(fec0, "zero", nb)] >= 1 for nb in (1, 2, 3)) if not fec0 else all(seen[(fec0, "zero", nb)] >= 1 for nb in (1, 3))
        assert seen[(fec0, "lone error at the", "first")] >= 1 and seen[(fec0, "lone error at the", "last")] >= 1


@pytest.fixture(scope="module")
def L(oracle):
    L = oracle.lib()
    L.fxr_packet_decode_soft.restype = C.c_int
    L.fxr_packet_decode_soft.argtypes = [C.c_uint, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    return L


def test_reference_and_oracle_packet_decoders_agree(L):
    """every crafted packet: ref_decode.packet_decode = fxr_packet_decode and, on soft inputs 0 / 255 of the crafted bits,
    ref_decode.packet_decode_soft = fxr_packet_decode_soft; the batched reference is the unbatched one"""
    n_checked = 0
    for (x, cs), (out, met) in zip(CC.streams(), CC.reference()):
        softs = [(R.bits_of(c["pkt"]) * 255).astype(np.uint8) for c in cs]
        sout, _ = CC.decode_batch(cs, softs, soft=True)
        for i, (c, (payload, valid), (spayload, svalid)) in enumerate(zip(cs, out, sout)):
            n, args = c["n"], (c["n"], c["check"], c["fec0"], c["fec1"])
            pkt = np.concatenate([c["pkt"], np.zeros(8, np.uint8)])
            buf = np.zeros(n + 16, np.uint8)
            ok = L.fxr_packet_decode(*args, pkt.ctypes.data, buf.ctypes.data)
            assert (buf[:n].tobytes(), int(ok)) == (payload, valid), ("hard", c["name"])
            soft = np.concatenate([softs[i], np.zeros(64, np.uint8)])
            buf = np.zeros(n + 16, np.uint8)
            ok = L.fxr_packet_decode_soft(*args, soft.ctypes.data, buf.ctypes.data)
            assert (buf[:n].tobytes(), int(ok)) == (spayload, svalid), ("soft", c["name"])
            if i % 5 == 0 and n < 1000:
                assert R.packet_decode(c["pkt"], *args) == (payload, valid), c["name"]
                assert R.packet_decode_soft(softs[i], *args) == (spayload, svalid), c["name"]
            n_checked += 1
    assert n_checked == len(CC.cases())


def test_oracle_receiver_delivers_every_crafted_word(oracle):
    """the condition: on the crafted IQ the oracle receiver finds every frame where it was put, every header is valid and
    states the case's properties, and its symbols demap -- by the reference's nearest-point rule, far from any boundary -- to
    exactly the crafted word; its payload is the reference's.  No frame is excluded."""
    worst = 1.0
    for (x, cs), (out, met) in zip(CC.streams(), CC.reference()):
        lay, total = CC.layout(cs)
        assert total == len(x)
        of = oracle_frames(oracle, x)
        assert len(of) == len(cs), (cs[0]["family"], len(of), len(cs))
        for f, (off, c), (payload, valid) in zip(of, lay, out):
            assert f.header_valid, c["name"]
            assert (f.mod_scheme, f.check, f.fec0, f.fec1, len(f.payload)) == (c["mod"], c["check"], c["fec0"], c["fec1"], c["n"]), c["name"]
            assert abs(f.info["start"] - off) <= 64, (c["name"], f.info["start"], off)
            lab, margin = R.demap_hard(c["mod"], f.framesyms)
            assert np.array_equal(lab, CC.crafted_labels(c)), c["name"]
            if len(margin):
                worst = min(worst, float(margin.min()))
            assert (f.payload, f.payload_valid) == (payload, valid), c["name"]
    print("\nsmallest decision margin over all crafted symbols: %.3f" % worst)
    assert worst > 0.1
