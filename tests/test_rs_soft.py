"""Soft-decision Reed-Solomon decoding (fxrx_config.soft_rs) without a GPU: the numpy reference (tests/ref_rs_soft.py) on the crafted
blocks (tests/rs_soft_cases.py), against ref_decode's hard decoder, and the decode kernel's own trial (gr-liquiddsp_amd/csrc/
fx_rsgmd.h), run serially by a host-only driver (tests/cpp/rsgmd_check.cpp, g++), against the reference bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ref_decode as rd
import ref_rs_soft as rs
import rs_soft_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = K.cases()


def _ref(c):
    blocks, f, tr = K.reference()[c["N"]]
    i = [x["name"] for x in K.of_length(c["N"])].index(c["name"])
    return blocks[i], int(f[i]), tr["cand"][:, i], tr["ok"][:, i], tr["cost"][:, i]


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_case_is_what_its_name_says(c):
    out, f, cand, ok, cost = _ref(c)
    reaches = [bool(o) and (cd == c["sent"]).all() for cd, o in zip(cand, ok)]
    if c["expect"] == "sent":
        assert (out == c["sent"]).all() and f != rs.NO_F
    else:
        assert not (out == c["sent"]).all()
    if "hard_ok" in c:
        assert reaches[0] == c["hard_ok"]
    if "chosen" in c:
        assert f == c["chosen"]
    if "other" in c:                                   # two f give different codewords
        hits = {tuple(cd) for cd, o in zip(cand, ok) if o}
        assert tuple(c["other"]) in hits and tuple(c["sent"]) in hits
        assert bool(ok[0]) and (cand[0] == c["other"]).all()
    if c["name"].startswith("cost_tie"):
        fa = next(i for i, r in enumerate(reaches) if r)
        assert cost[fa] == cost[0] and fa > 0 and not (cand[fa] == cand[0]).all()
    if c.get("far"):
        assert not ok[:9].any() and ok[16] and f != rs.NO_F and not (out == rs.hard_bytes(c["soft"])).all()
    if c["name"].startswith(("equal_0_255", "boundary_127_128")):
        assert (rs.erasure_order(c["soft"]) == np.arange(c["N"])).all()
        assert reaches == [False] * 4 + [True] * 13 and len(set(int(x) for x in cost[4:])) == 1
    # the winner is the least cost among the candidates, ties to the smallest f
    best = min((int(d), i) for i, (d, o) in enumerate(zip(cost, ok)) if o)
    assert f == 2 * best[1] and (out == cand[best[1]]).all()


def test_the_f0_candidate_is_the_hard_decoder():
    for c in CASES:
        _, _, cand, ok, _ = _ref(c)
        want, fixed = rd.rs_decode_block(rs.hard_bytes(c["soft"]))
        assert bool(ok[0]) == (fixed >= 0), c["name"]
        assert (cand[0] == want).all(), c["name"]


def test_reliability_and_order():
    soft = np.full(8 * 40, 255, np.uint8)
    soft[8 * 7 + 3], soft[8 * 9], soft[8 * 2 + 7], soft[8 * 30] = 128, 127, 0, 200
    rho = rs.byte_reliability(soft)
    assert rho[7] == 1 and rho[9] == 1 and rho[2] == 255 and rho[30] == 145 and rho[0] == 255
    assert list(rs.erasure_order(soft)[:4]) == [7, 9, 30, 0]
    assert rs.hard_bytes(soft)[7] == 0xff and rs.hard_bytes(soft)[9] == 0x7f and rs.hard_bytes(soft)[2] == 0xfe


def test_erasures_alone_up_to_32():
    rng = np.random.RandomState(5)
    cw = K.codeword(rng, 60)
    pos = rng.permutation(60)[:33]
    h = cw.copy()
    h[pos] ^= rng.randint(1, 256, 33).astype(np.uint8)
    c, ok = rs.rs_decode_erasures(h, pos[:32])
    assert not ok or not (c == cw).all()                  # one error outside 32 erasures: radius 0
    h[pos[32]] = cw[pos[32]]
    c, ok = rs.rs_decode_erasures(h, pos[:32])
    assert ok and (c == cw).all()


def test_packet_decoder_with_soft_rs_off_is_packet_decode_soft():
    rng = np.random.RandomState(9)
    for fec0, fec1 in ((rd.FEC_NONE, rd.FEC_RS), (rd.FEC_V27, rd.FEC_RS), (rd.FEC_RS, rd.FEC_NONE), (rd.FEC_V27, rd.FEC_H74)):
        n = 40
        l1 = rd.packet_dims(n, rd.CRC_32, fec0, fec1)[2]
        soft = rng.randint(0, 256, 8 * l1).astype(np.uint8)
        assert rs.packet_decode_soft_rs(soft, n, rd.CRC_32, fec0, fec1, soft_rs=False) == rd.packet_decode_soft(soft, n, rd.CRC_32, fec0, fec1)
    soft = rng.randint(0, 256, 8 * rd.packet_dims(40, rd.CRC_32, rd.FEC_V27, rd.FEC_H74)[2]).astype(np.uint8)
    assert rs.packet_decode_soft_rs(soft, 40, rd.CRC_32, rd.FEC_V27, rd.FEC_H74) == rd.packet_decode_soft(soft, 40, rd.CRC_32, rd.FEC_V27, rd.FEC_H74)


def test_packet_decoder_recovers_what_the_hard_chain_loses():
    """24 weak wrong bytes (every bit on the wrong side, near the middle) in the Reed-Solomon block of a packet: invalid by hard
    decisions -- 192 wrong bits are beyond the Viterbi decoder behind it, too --, valid with soft_rs"""
    rng = np.random.RandomState(11)
    for fec0 in (rd.FEC_NONE, rd.FEC_V27):
        msg = rng.randint(0, 256, 64).astype(np.uint8)
        trace = {}
        pkt = rd.packet_encode(msg, rd.CRC_32, fec0, rd.FEC_RS, trace)
        cw1 = trace["cw1"].copy()
        soft = K.strong(cw1)
        for j in rng.permutation(len(cw1))[:24]:
            soft[8 * j:8 * j + 8] = np.where(soft[8 * j:8 * j + 8] > 127, 120, 135)
        chan = rd.interleave_soft(soft, len(cw1), decode=False)
        assert rd.packet_decode_soft(chan, 64, rd.CRC_32, fec0, rd.FEC_RS)[1] == 0
        assert rs.packet_decode_soft_rs(chan, 64, rd.CRC_32, fec0, rd.FEC_RS) == (msg.tobytes(), 1)


# ---------------------------------------------------------------------------------------------------- the kernel's trial on the host
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rsgmd") / "rsgmd_check")
    subprocess.check_call(["g++", "-O2", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "rsgmd_check.cpp")])

    def run(soft, N, tmp):
        soft = np.ascontiguousarray(soft, np.uint8)
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        with open(fin, "wb") as f:
            f.write(np.array([N, len(soft)], np.uint32).tobytes())
            f.write(soft.tobytes())
        subprocess.check_call([exe, fin, fout])
        o = np.fromfile(fout, np.uint8).reshape(len(soft), N + 1)
        return o[:, :N], o[:, N]
    return run


@pytest.mark.parametrize("N", K.block_lengths())
def test_kernel_trial_on_the_host_matches_the_reference(driver, tmp_path, N):
    blocks, f, _ = K.reference()[N]
    got, gf = driver(np.stack([c["soft"] for c in K.of_length(N)]), N, str(tmp_path))
    assert (got == blocks).all() and (gf == f).all()
    n = {33: 1, 144: 224, 255: 223}[N]
    soft, dec, f = K.packet_reference(n, 150, 4000 + n)
    nb, dl = rd.rs_dims(n)
    got, gf = driver(soft.reshape(-1, 8 * N), N, str(tmp_path))
    assert (got[:, :dl].reshape(len(soft), nb * dl)[:, :n] == dec).all() and (gf.reshape(len(soft), nb) == f).all()
    assert 0.2 < (gf[len(K.of_length(N)) * nb:] == 0).mean() < 0.9          # the noise level sits at the hard decoder's limit


# ---------------------------------------------------------------------------------------------------- the library (these fail without the feature)
def test_library_exports_the_soft_rs_entry_points(fx):
    L = fx.lib()
    for name in ("fxrx_debug_rs_soft", "fxrx_sync_set_soft_rs"):
        assert hasattr(L, name) and name in fx._ffi.EXPORTS
    assert hasattr(L, "fx_launch_rssoft")
    F = fx._ffi
    assert issubclass(F.ConfigRs, F.ConfigChain) and [n for n, _ in F.ConfigRs._fields_] == ["soft_rs"]
    assert F.ConfigRs.soft_rs.offset == C.sizeof(F.ConfigChain) and C.sizeof(F.ConfigRs) == C.sizeof(F.ConfigChain) + C.sizeof(C.c_int)
    assert L.fxrx_sync_set_soft_rs(None, 1) == -1
    buf = (C.c_ubyte * 4096)()
    assert L.fxrx_debug_rs_soft(0, 1, buf, buf, buf) == -1          # bad arguments are refused before any device is looked for
    assert L.fxrx_debug_rs_soft(4, 1, None, buf, buf) == -1
    assert L.fxrx_debug_rs_soft(4, 1, buf, None, buf) == -1
    assert L.fxrx_debug_rs_soft(4, 1, buf, buf, None) == -1
    assert L.fxrx_debug_rs_soft((1 << 18) + 1, 1, buf, buf, buf) == -1       # (a stage of a 65535-byte frame is up to 131 080 bytes: taken)


@pytest.mark.parametrize("mode,soft", [(0, 0), (1, 1), (1, 0)], ids=["no_soft_decision", "detector", "detector_hard"])
def test_soft_rs_needs_soft_decision_and_flex_rx(fx, mode, soft):
    L = fx.lib()
    cfg = fx._ffi.ConfigRs(0, mode, 1, 0.0, 0, 0, 0, soft, 0, 0, 0, 1)
    assert not L.fxrx_create(cfg)
    assert b"soft_rs" in L.fxrx_last_error()


# ---------------------------------------------------------------------------------------------------- the crafted frames
@pytest.mark.parametrize("fec0", [rd.FEC_NONE, rd.FEC_V27], ids=["rs_alone", "rs_over_v27"])
def test_crafted_frame_demaps_to_the_crafted_word_rejected_hard_accepted_soft(fec0):
    """ref_framegen -> ref_sync (float64) -> ref_decode.demap_soft: behind the soft de-interleaver the hard word is the crafted one,
    its 24 wrong bytes are the 24 least reliable of the block, the hard chain rejects it and the soft rule returns the payload"""
    import ref_framegen as G
    import ref_sync
    c = K.frame_case(fec0)
    k, l0, l1 = c["dims"]
    x = np.concatenate([c["x"], np.zeros(64, np.complex128)])
    out = ref_sync.sync(x, 1, 0.0, 1.0, 0.0, 0.0, G.tables())
    assert out["header_valid"] and not out["short"]
    assert out["props"] == dict(payload_len=K.FRAME_N, ms=rd.PSK4, check=rd.CRC_32, fec0=fec0, fec1=rd.FEC_RS)
    soft = rd.soft_to_channel(rd.demap_soft(rd.PSK4, out["r"]), l1)
    v = rd.interleave_soft(soft, l1, decode=True)
    assert (rs.hard_bytes(v) == c["word"]).all()
    assert len(c["wrong"]) == K.FRAME_WRONG and sorted(rs.erasure_order(v)[:K.FRAME_WRONG]) == c["wrong"]
    rho = rs.byte_reliability(v)
    print("fec0 %d: rho of the wrong bytes %d..%d, of the others %d..%d" % (fec0, rho[c["wrong"]].min(), rho[c["wrong"]].max(),
                                                                          np.delete(rho, c["wrong"]).min(), np.delete(rho, c["wrong"]).max()))
    assert rd.rs_decode_block(c["word"])[1] == -1                                  # the hard decoder gives up
    got, valid = rd.packet_decode_soft(soft, K.FRAME_N, rd.CRC_32, fec0, rd.FEC_RS)
    assert valid == 0 and got != c["payload"]
    chosen = []
    assert (rs.rs_decode_soft(v, l0, chosen) == c["sent"][:l0]).all()
    assert len(chosen) == 1 and 16 <= chosen[0] <= 24                # 24 - f wrong bytes outside E_f, radius (32 - f) / 2: from f = 16 on
    assert rs.packet_decode_soft_rs(soft, K.FRAME_N, rd.CRC_32, fec0, rd.FEC_RS) == (c["payload"], 1)
