"""The bound on f and the soft hand-over of soft-decision Reed-Solomon decoding (fxrx_config.soft_rs_fmax, soft_rs_chain) without a GPU:
the numpy reference (tests/ref_rs_chain.py) on the crafted blocks and packets (tests/rs_chain_cases.py); its identities with
ref_rs_soft, with ref_decode's hard decoder and with the hard hand-over; four wrong decoders, each caught by a named case; and the
rule as the decode kernel states it (gr-liquiddsp_amd/csrc/fx_rsgmd.h), run serially by a host-only driver
(tests/cpp/rschain_check.cpp, g++ with the address and undefined-behaviour sanitizers), against the reference bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ref_decode as rd
import ref_rs_chain as rc
import ref_rs_soft as rs
import rs_chain_cases as K
import rs_soft_cases as K0

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = K.block_cases()
PACKETS = K.all_packet_cases()


# ---------------------------------------------------------------------------------------------------- the crafted cases
@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_block_case_is_what_its_name_says(c):
    out, f, so, cand, ok, cost = K.block_result(c)
    fm = c["fmax"]
    h = rs.hard_bytes(c["soft"])
    within = [i for i in range(fm // 2 + 1) if ok[i]]
    # the rule: the least cost among the candidates of f <= fmax, ties to the smallest f; none: h, 255
    if within:
        best = min((int(cost[i]), i) for i in within)
        assert f == 2 * best[1] and (out == cand[best[1]]).all()
        assert (so == np.unpackbits(out) * 255).all()
    else:
        assert f == rc.NO_F and (out == h).all() and (so == c["soft"]).all()
    if c["chosen"] is not None:
        assert f == c["chosen"]
    name = c["name"]
    if name.startswith("won_at_f_equal_fmax"):
        # (a smaller f may have a candidate of its own, a far codeword at a higher cost -- N = 255, f = 28 --, but none reaches the sent one)
        assert f == fm and (out == c["sent"]).all() and not any(ok[i] and (cand[i] == c["sent"]).all() for i in range(fm // 2))
    if name.startswith("only_candidates_above_fmax"):
        first = int(name.split("first_at_")[1].split("_")[0])
        assert not ok[:fm // 2 + 1].any() and ok[first // 2] and (cand[first // 2] == c["sent"]).all() and first > fm
        assert not any(ok[i] and (cand[i] == c["sent"]).all() for i in range(first // 2))
    if "unbounded" in c:
        full, f32 = K.block_result(c, 32)[:2]
        assert f32 != rc.NO_F and f32 > fm and (full != out).any() and not (out == c["sent"]).all()
        assert (full == c["sent"]).all() == (c["unbounded"] == "sent")
    if "other" in c:                                    # the bounded winner is the near codeword, the unbounded one the sent
        assert (out == c["other"]).all() and f == 0 and any(ok[i] and cost[i] < cost[0] for i in range(fm // 2 + 1, 17))
    if c.get("far"):
        assert not ok[:9].any()                         # nothing up to f = 16
        assert (f == rc.NO_F) == (not ok[:fm // 2 + 1].any())
        if fm <= 16:
            assert f == rc.NO_F
        assert ((c["soft"] != 0) & (c["soft"] != 255)).mean() > 0.9     # pass-through is distinguishable from re-hardening
    if c.get("mid"):
        assert set(np.unique(c["soft"])) == {127, 128} and f == rc.NO_F
    if name.startswith("codeword_as_received"):
        assert not rd.rs_syndromes(h[None]).any() and f == 0


@pytest.mark.parametrize("p", PACKETS, ids=[p["name"] for p in PACKETS])
def test_packet_case_is_what_its_name_says(p):
    n = p["n"]
    nb, dl = rd.rs_dims(n)
    chosen = []
    so = rc.rs_stage_soft_out(p["soft"], n, p["fmax"], chosen)
    assert tuple(chosen) == p["chosen"] and len(so) == 8 * n
    hard = rc.rs_stage_hard_out(p["soft"], n, p["fmax"])
    s = p["soft"].reshape(nb, 8 * (dl + 32))
    for b, f in enumerate(chosen):
        ln = min(dl, n - b * dl)
        seg = so[8 * b * dl:8 * (b * dl + ln)]
        if f == rc.NO_F:
            assert (seg == s[b, :8 * ln]).all() and ((seg != 0) & (seg != 255)).mean() > 0.9
        else:
            assert (seg == np.unpackbits(hard[b * dl:b * dl + ln]) * 255).all()
    if "padded" in p["name"]:
        assert nb * dl == n + 1 and s[1, 8 * (dl - 1):8 * dl].any()    # the pad position has soft values of its own, none of them emitted


# ---------------------------------------------------------------------------------------------------- identities
def test_fmax_32_is_the_unbounded_rule():
    for n in K.SIZES:
        nb, dl = rd.rs_dims(n)
        soft, tr, _ = K.packet_set(n)
        blocks, f = rs.rs_decode_soft_blocks(soft.reshape(-1, 8 * (dl + 32)))
        hard, so, chosen = K.packet_reference(n, 32)
        assert (chosen.ravel() == f).all() and (f != rc.NO_F).all()
        assert (hard == blocks[:, :dl].reshape(len(soft), nb * dl)[:, :n]).all()
    for c in K0.cases():                                # and on every case of rs_soft_cases
        tr = {}
        blocks, f = rs.rs_decode_soft_blocks(c["soft"][None], tr)
        b32, f32 = rc.bounded_from_trace(tr, 32)
        assert (b32 == blocks).all() and (f32 == f).all()


def test_fmax_0_is_the_hard_decoder():
    for c in list(CASES) + list(K0.cases()):
        blocks, f = rc.rs_blocks_bounded(c["soft"][None], 0)
        want, fixed = rd.rs_decode_block(rs.hard_bytes(c["soft"]))
        assert (blocks[0] == want).all() and (int(f[0]) == 0) == (fixed >= 0) and int(f[0]) in (0, rc.NO_F), c["name"]
    for n in (224, 225):
        soft = K.packet_set(n)[0]
        hard = K.packet_reference(n, 0)[0]
        for i in range(0, len(soft), 7):
            assert (hard[i] == rd.fec_decode(rd.FEC_RS, rs.hard_bytes(soft[i]), n)).all()


def _packet(rng, n, fec0, wrong, weak_margin):
    """a packet of n payload bytes, fec1 Reed-Solomon: channel soft values with `wrong` weak wrong bytes in every Reed-Solomon block"""
    msg = rng.randint(0, 256, n).astype(np.uint8)
    trace = {}
    rd.packet_encode(msg, rd.CRC_32, fec0, rd.FEC_RS, trace)
    cw1 = trace["cw1"].copy()
    nb, dl = rd.rs_dims(len(trace["cw0"]))
    soft = K0.strong(cw1)
    for b in range(nb):
        for j in b * (dl + 32) + rng.permutation(dl + 32)[:wrong]:
            soft[8 * j:8 * j + 8] = np.where(soft[8 * j:8 * j + 8] > 127, (255 - weak_margin) // 2, (255 + weak_margin) // 2)
    return msg, rd.interleave_soft(soft, len(cw1), decode=False)


def test_chain_with_every_block_accepted_is_the_hard_hand_over():
    """the soft-input Viterbi decoder on 0 / 255 is the hard one"""
    rng = np.random.RandomState(21)
    for fec0, n, wrong in ((rd.FEC_V27, 64, 10), (rd.FEC_V27P34, 64, 20), (rd.FEC_V27, 300, 12), (rd.FEC_V27P78, 300, 24)):
        msg, chan = _packet(rng, n, fec0, wrong, 15)
        for fmax in (24, 32):
            on = rc.packet_decode_rs_chain(chan, n, rd.CRC_32, fec0, rd.FEC_RS, fmax, True)
            off = rc.packet_decode_rs_chain(chan, n, rd.CRC_32, fec0, rd.FEC_RS, fmax, False)
            assert on == off == (msg.tobytes(), 1)
    # not accepted blocks only: random values, every block far
    for fec0, n in ((rd.FEC_V27, 64), (rd.FEC_V27P23, 300)):
        l1 = rd.packet_dims(n, rd.CRC_32, fec0, rd.FEC_RS)[2]
        chan = rng.randint(0, 256, 8 * l1).astype(np.uint8)
        assert rc.packet_decode_rs_chain(chan, n, rd.CRC_32, fec0, rd.FEC_RS, 32, True) == rs.packet_decode_soft_rs(chan, n, rd.CRC_32, fec0, rd.FEC_RS)


def test_the_options_act_only_on_reed_solomon_before_a_convolutional_code():
    rng = np.random.RandomState(22)
    n = 40
    for fec0, fec1 in ((rd.FEC_NONE, rd.FEC_RS), (rd.FEC_RS, rd.FEC_NONE), (rd.FEC_GOLAY, rd.FEC_RS), (rd.FEC_V27, rd.FEC_H74), (rd.FEC_V27, rd.FEC_NONE)):
        l1 = rd.packet_dims(n, rd.CRC_32, fec0, fec1)[2]
        chan = rng.randint(0, 256, 8 * l1).astype(np.uint8)
        for fmax in (0, 16, 32):
            assert rc.packet_decode_rs_chain(chan, n, rd.CRC_32, fec0, fec1, fmax, True) == rc.packet_decode_rs_chain(chan, n, rd.CRC_32, fec0, fec1, fmax, False)
        assert rc.packet_decode_rs_chain(chan, n, rd.CRC_32, fec0, fec1, 32, True) == rs.packet_decode_soft_rs(chan, n, rd.CRC_32, fec0, fec1)


def test_given_up_block_reaches_the_soft_viterbi_decoder():
    """Reed-Solomon over V27, 40 weak wrong bytes in the block, more than any f reaches, every one with all eight bits weakly wrong:
    the hard hand-over gives fec0 320 wrong bits, the soft hand-over at fmax = 16 gives it 320 weak ones among strong right ones"""
    rng = np.random.RandomState(23)
    msg, chan = _packet(rng, 64, rd.FEC_V27, 40, 9)
    args = (chan, 64, rd.CRC_32, rd.FEC_V27, rd.FEC_RS)
    assert rc.packet_decode_rs_chain(*args, 16, False)[1] == 0
    assert rc.packet_decode_rs_chain(*args, 16, True) == (msg.tobytes(), 1)
    assert rd.packet_decode_soft(*args)[1] == 0


def test_noisy_packets_hold_both_classes_at_fmax_16():
    for n in K.SIZES:
        acc, gone = K.noisy_shares(n)
        print("n = %-3d  accepted %.2f  given up %.2f" % (n, acc, gone))
        assert acc >= 0.1 and gone >= 0.1


# ---------------------------------------------------------------------------------------------------- four wrong decoders
def _stage(soft, n, fmax, bound=True, accepted="c", given_up="s", pad=False):
    """the stage's soft output, with switches for the four mistakes"""
    nb, dl = rd.rs_dims(n)
    s = np.asarray(soft, np.uint8).reshape(nb, 8 * (dl + 32))
    blocks, f = rc.rs_blocks_bounded(s, fmax if bound else 32)
    h = rs.hard_bytes(s)
    out = []
    for b in range(nb):
        if f[b] != rc.NO_F:
            o = np.unpackbits(blocks[b] if accepted == "c" else h[b]) * 255
        else:
            o = s[b] if given_up == "s" else np.unpackbits(h[b]) * 255
        out.append(o[:8 * (dl if pad else min(dl, n - b * dl))])
    return np.concatenate(out).astype(np.uint8)


WRONG = [("bound_ignored", dict(bound=False), "accepted_then_given_up_n224"),
         ("accepted_block_emits_the_received_bits", dict(accepted="h"), "accepted_at_f_16_then_given_up_n446"),
         ("given_up_block_emits_hard_decisions", dict(given_up="h"), "given_up_then_accepted_n224"),
         ("pad_positions_emitted", dict(pad=True), "accepted_then_given_up_padded_last_block_n225")]


@pytest.mark.parametrize("name,kw,case", WRONG, ids=[w[0] for w in WRONG])
def test_wrong_decoder_fails_on_a_named_case(name, kw, case):
    p = next(p for p in PACKETS if p["name"] == case)
    want = rc.rs_stage_soft_out(p["soft"], p["n"], p["fmax"])
    assert (_stage(p["soft"], p["n"], p["fmax"]) == want).all()                # the switches off: the rule
    got = _stage(p["soft"], p["n"], p["fmax"], **kw)
    assert len(got) != len(want) or (got != want).any()
    for q in PACKETS:                                                           # and no other switch is needed to pass the others' cases
        if name == "pad_positions_emitted" and "padded" not in q["name"]:
            assert (_stage(q["soft"], q["n"], q["fmax"], **kw) == rc.rs_stage_soft_out(q["soft"], q["n"], q["fmax"])).all()


# ---------------------------------------------------------------------------------------------------- the kernel's rule on the host
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rschain") / "rschain_check")
    subprocess.check_call(["g++", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "rschain_check.cpp")])

    def run(soft, n, fmax, chain, tmp):
        soft = np.ascontiguousarray(soft, np.uint8)
        nb = rd.rs_dims(n)[0]
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        with open(fin, "wb") as f:
            f.write(np.array([n, len(soft), fmax, chain], np.uint32).tobytes())
            f.write(soft.tobytes())
        subprocess.check_call([exe, fin, fout])
        ol = 8 * n if chain else n
        o = np.fromfile(fout, np.uint8).reshape(len(soft), ol + nb)
        return o[:, :ol], o[:, ol:]
    return run


@pytest.mark.parametrize("n", K.SIZES)
def test_kernel_rule_on_the_host_matches_the_reference(driver, tmp_path, n):
    soft, _, ncraft = K.packet_set(n)
    soft = soft[:ncraft + 40]                                                   # every crafted packet and 40 noisy ones
    for fmax in K.FMAX:
        hard, so, chosen = K.packet_reference(n, fmax)
        for chain, want in ((0, hard), (1, so)):
            got, gf = driver(soft, n, fmax, chain, str(tmp_path))
            assert (gf == chosen[:len(soft)]).all(), (n, fmax, chain)
            assert (got == want[:len(soft)]).all(), (n, fmax, chain)


# ---------------------------------------------------------------------------------------------------- the library (these fail without the feature)
def test_library_exports_the_entry_points(fx):
    L = fx.lib()
    for name in ("fxrx_debug_rs_chain", "fxrx_sync_set_soft_rs_fmax", "fxrx_sync_set_soft_rs_chain"):
        assert hasattr(L, name) and name in fx._ffi.EXPORTS
    assert hasattr(L, "fx_launch_rschain")
    F = fx._ffi
    assert issubclass(F.ConfigRsChain, F.ConfigRs) and [n for n, _ in F.ConfigRsChain._fields_] == ["soft_rs_fmax", "soft_rs_chain"]
    assert F.ConfigRsChain.soft_rs_fmax.offset == C.sizeof(F.ConfigRs) and C.sizeof(F.ConfigRsChain) == C.sizeof(F.ConfigRs) + 2 * C.sizeof(C.c_int)
    assert L.fxrx_sync_set_soft_rs_fmax(None, 1) == -1 and L.fxrx_sync_set_soft_rs_chain(None, 1) == -1
    buf = (C.c_ubyte * 4096)()
    assert L.fxrx_debug_rs_chain(0, 1, 16, 0, buf, buf, buf) == -1          # bad arguments are refused before any device is looked for
    assert L.fxrx_debug_rs_chain(4, 1, 16, 1, None, buf, buf) == -1
    assert L.fxrx_debug_rs_chain(4, 1, 16, 1, buf, None, buf) == -1
    assert L.fxrx_debug_rs_chain(4, 1, 16, 1, buf, buf, None) == -1
    assert L.fxrx_debug_rs_chain(4, 1, 15, 0, buf, buf, buf) == -1          # an odd bound
    assert L.fxrx_debug_rs_chain(4, 1, 34, 0, buf, buf, buf) == -1
    assert L.fxrx_debug_rs_chain(4, 1, -2, 0, buf, buf, buf) == -1
    assert L.fxrx_debug_rs_chain((1 << 18) + 1, 1, 16, 0, buf, buf, buf) == -1


# (soft_rs, soft_rs_fmax, soft_rs_chain) fxrx_create refuses, and the option its text names
BAD = [((0, 0, 1), b"soft_rs_chain"), ((0, 17, 0), b"soft_rs_fmax"), ((1, 16, 0), b"soft_rs_fmax"), ((1, 35, 0), b"soft_rs_fmax"), ((1, -1, 1), b"soft_rs_fmax"),
       ((1, 2, 1), b"soft_rs_fmax")]


@pytest.mark.parametrize("fields,text", BAD, ids=["chain_without_soft_rs", "fmax_without_soft_rs", "odd_bound_15", "bound_34", "negative", "odd_bound_1"])
def test_create_refuses_bad_combinations(fx, fields, text):
    L = fx.lib()
    cfg = fx._ffi.ConfigRsChain(0, 0, 1, 0.0, 0, 0, 0, 1, 0, 0, 0, *fields)
    assert not L.fxrx_create(cfg)
    err = L.fxrx_last_error()
    assert text in err and b"FXRX_ERR_ARG" in err
