"""tests/ref_framegen.py (the float64 frame generator and the tables' definitions) against the oracle, against the other
references, and closed on itself.  CPU only.

  1  the tables from their definitions against the oracle's float32 tables: p/n and pilots exactly, taps within 1 float32 ulp
  2  ref_detect.build_template fed from either source
  3  every frame of tests/framegen_cases.py against oracle.gen_frame, within ref_framegen.sample_tol(dt)
  4  compose_header inverts ref_sync.parse_header
  5  each negative control misses the oracle's frame by at least 1000 x the bound
  6  frame -> ref_sync.sync with ref_framegen.tables() -> ref_decode: no oracle and no product in the signal path
"""
import numpy as np
import pytest

import framegen_cases as FC
import ref_decode as R
import ref_detect as rd
import ref_framegen as G
import ref_header_soft as RH
import ref_sync as rs


def _ulps(ref64, got32):
    got32 = np.asarray(got32, np.float32)
    return float((np.abs(got32.astype(np.float64) - ref64) / np.spacing(np.abs(got32)).astype(np.float64)).max())


def _oracle_frame(oracle, c):
    return oracle.gen_frame(c["payload"], mod=c["mod"], fec0=c["fec0"], fec1=c["fec1"], check=c["check"], header=c["header"], dt=c["dt"])


def _name(c):
    return "%s mod %d fec %d/%d check %d n %d dt %g header %s" % (c["tag"], c["mod"], c["fec0"], c["fec1"], c["check"], len(c["payload"]),
                                                                   c["dt"], "set" if c["header"] is not None else "none")


# ---------------------------------------------------------------------------------------------------- 1. tables
def test_msequence_is_liquids():
    """m = 7, g = 0x89: x^7 + x^3 + 1 (period 127, 64 ones); the first bits by hand: v = 1, taps 0x44 -> 0 until the one reaches
    bit 2 (the third step emits 1)."""
    b = G.msequence(7, 0x0089, 1, 254)
    assert list(b[:8]) == [0, 0, 1, 0, 0, 1, 1, 0]
    assert np.array_equal(b[:127], b[127:]) and int(b[:127].sum()) == 64
    assert not any(np.array_equal(b[:127], np.roll(b[:127], s)) for s in range(1, 127))
    p = G.msequence(4, 0x13, 1, 30)
    assert np.array_equal(p[:15], p[15:]) and int(p[:15].sum()) == 8


def test_tables_from_definitions_equal_the_oracles(oracle):
    assert np.array_equal(G.preamble().astype(np.complex64), oracle.table("fxr_preamble_pn", G.PN_LEN))
    assert np.array_equal(G.pilots().astype(np.complex64), oracle.table("fxr_pilots", G.N_PILOTS))
    worst = dict(tx=_ulps(G.tx_taps(), oracle.table("fxr_tx_taps", 29, complex_=False)),
                 proto=_ulps(G.mf_proto(), oracle.table("fxr_mf_proto", 897, complex_=False)),
                 eq=_ulps(G.eq_init(), oracle.eq_init_taps()))
    for dt in G.DTS:
        h = np.empty(29, np.float32)
        oracle.lib().fxr_firdes_arkaiser(G.K, G.M_SPAN, np.float32(0.3), np.float32(dt), h.ctypes.data)
        worst["dt %g" % dt] = _ulps(G.tx_taps(dt), h)
    print("\ntables: worst difference in float32 ulps of the entry:", {k: round(v, 3) for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), worst
    tb = rs.Tables.from_reference()
    to = rs.Tables.from_oracle(oracle)
    assert np.array_equal(tb.pn.astype(np.complex64), to.pn.astype(np.complex64)) and len(tb.proto) == len(to.proto)


def test_detector_template_from_either_source(oracle):
    ref = rd.build_template(G.preamble(), G.tx_taps())
    orc = rd.build_template(oracle.table("fxr_preamble_pn", G.PN_LEN), oracle.table("fxr_tx_taps", 29, complex_=False))
    assert G.compare(ref, orc) <= G.sample_tol(0.0)
    assert G.compare(ref, oracle.table("fxr_template", len(ref))) <= G.sample_tol(0.0)


# ---------------------------------------------------------------------------------------------------- 3. frames
def test_case_list_holds_what_it_promises():
    cs = FC.cases()
    assert 450 <= len(cs) <= 600
    assert {(c["mod"], c["fec0"]) for c in cs if c["fec1"] == R.FEC_NONE} >= {(m, f) for m in FC.MODS for f in FC.CODES}
    assert {(c["fec0"], c["fec1"]) for c in cs} >= {(a, b) for a in (R.FEC_V27, R.FEC_V27P34) for b in R.BLOCK + (R.FEC_RS,)} | {(R.FEC_RS, R.FEC_V27)}
    assert {c["check"] for c in cs} == set(FC.CHECKS) and {len(c["payload"]) for c in cs} >= {0, 1, 2}
    k = lambda c: len(c["payload"]) + R.crc_len(c["check"])
    for f in (R.FEC_GOLAY, R.FEC_H128):
        assert {k(c) % 3 for c in cs if c["fec0"] == f} == {0, 1, 2}
    for f in (R.FEC_SD22, R.FEC_SD39, R.FEC_SD72):
        assert {k(c) % 8 for c in cs if c["fec0"] == f} == set(range(8))
    assert {k(c) for c in cs if c["fec0"] == R.FEC_RS} >= {222, 223, 224, 446, 447}
    npay = lambda c: G.num_payload_symbols(len(c["payload"]), c["mod"], c["fec0"], c["fec1"], c["check"])
    for m in R.DPSK:                                              # both sides of every 64-symbol carry
        got = {npay(c) for c in cs if c["mod"] == m}
        assert got >= {x for x in FC.DPSK_COUNTS if FC.reachable(m, x)} and {64, 128} <= got
        assert any(x < 64 for x in got) and any(64 < x < 128 for x in got) and any(x > 128 for x in got)
    assert not any(FC.reachable(R.DPSK2, x) or FC.reachable(R.DPSK4, x) for x in (63, 65, 129))       # 8 l1 = 0 mod 4
    assert {FC.HEAD + npay(c) for c in cs} >= set(FC.TILE_NSYM) | {FC.HEAD}
    for m in (R.PSK8, R.QAM32, R.QAM64):
        assert any(8 * R.packet_dims(len(c["payload"]), c["check"], c["fec0"], c["fec1"])[2] % R.bps(m) for c in cs if c["mod"] == m)
    lay, _ = FC.layout(FC.ref_len)
    assert {off % 2 for off, _ in lay} == {0, 1} and {c["gap"] for c in cs} >= {0, 1}
    for d in G.DTS:
        assert {c["header"] is not None for c in cs if c["dt"] == d} == {False, True}
    sub = [cs[i] for i in FC.subset()]
    assert len(sub) == 60 and {c["mod"] for c in sub} == set(FC.MODS) and {c["dt"] for c in sub} == set(G.DTS)
    assert {c["fec0"] for c in sub} == set(FC.CODES) and {c["fec1"] for c in sub} >= set(R.BLOCK + (R.FEC_RS, R.FEC_V27))


def test_every_frame_against_the_oracle(oracle):
    """lengths equal, every sample component within sample_tol(dt); the worst error is ref_framegen.MEASURED['oracle']"""
    worst, who, bad = 0.0, None, []
    for c, ref in zip(FC.cases(), FC.reference_frames()):
        got = _oracle_frame(oracle, c)
        assert len(got) == len(ref) == FC.ref_len(c), _name(c)
        e = G.compare(ref, got)
        if not e <= G.sample_tol(c["dt"]):
            bad.append((_name(c), e))
        if e > worst:
            worst, who = e, c
    print("\nreference vs oracle: %d frames, worst sample error %.3g (%s); bounds %.3g .. %.3g" % (
        len(FC.cases()), worst, _name(who), min(map(G.sample_tol, G.DTS)), max(map(G.sample_tol, G.DTS))))
    assert not bad, bad[:10]
    assert 4.0 * worst <= min(G.sample_tol(d) for d in G.DTS)
    m = G.MEASURED["oracle"]                        # the recorded figure is this run's, rounded up: it cannot drift
    assert 0.5 * m <= worst <= m, ("ref_framegen.MEASURED['oracle'] is not this run's", worst)
    assert 4.0 * G.MEASURED["gpu"] <= min(G.sample_tol(d) for d in G.DTS)


# ---------------------------------------------------------------------------------------------------- 4. header
def test_compose_header_inverts_parse_header():
    rng = np.random.default_rng(7)
    for _ in range(40):
        f = dict(payload_len=int(rng.integers(0, 65536)), ms=int(rng.choice(R.PAYLOAD_MODS)), check=int(rng.integers(1, 7)),
                 fec0=int(rng.choice(R.ALL_FEC)), fec1=int(rng.choice(R.ALL_FEC)))
        user = rng.integers(0, 256, 14, dtype=np.uint8)
        hdr = G.compose_header(user, f["payload_len"], f["ms"], f["check"], f["fec0"], f["fec1"])
        ok, dec, p = rs.parse_header(RH.header_encode(hdr))
        assert ok and p == f and bytes(dec[:14]) == user.tobytes() and bytes(dec) == hdr.tobytes()
    assert bytes(G.compose_header(None, 5, R.PSK4, R.CRC_24, R.FEC_V27, R.FEC_NONE)[:14]) == bytes(14)


# ---------------------------------------------------------------------------------------------------- 5. negative controls
def _first(pred):
    return next(c for c in FC.cases() if pred(c))


def _npay(c):
    return G.num_payload_symbols(len(c["payload"]), c["mod"], c["fec0"], c["fec1"], c["check"])


CONTROLS = {
    "DPSK sum restarted at symbol 64": (dict(dpsk_restart=64), lambda c: c["mod"] == R.DPSK8 and _npay(c) > 64),
    "pilots one position late": (dict(pilot_shift=1), lambda c: True),
    "dt negated": (dict(dt_sign=-1), lambda c: c["dt"] == -0.37),
    "taps shifted by one": (dict(tap_shift=1), lambda c: True),
    "QAM32 split 2+3": (dict(qam32_split=(2, 3)), lambda c: c["mod"] == R.QAM32 and _npay(c) > 16),
    "payload words LSB first": (dict(lsb_first=True), lambda c: c["mod"] == R.QAM16 and _npay(c) > 16),
}


@pytest.mark.parametrize("name", sorted(CONTROLS))
def test_negative_controls_miss_the_oracle(oracle, name):
    """each wrong reading misses the oracle's frame by at least 1000 x the bound, on a frame that can show it"""
    mut, pred = CONTROLS[name]
    c = _first(pred)
    got = _oracle_frame(oracle, c)
    assert G.compare(FC.ref_frame(c), got) <= G.sample_tol(c["dt"])
    e = G.compare(FC.ref_frame(c, **mut), got)
    print("\n%s: %s off by %.3g = %.0f x the bound" % (name, _name(c), e, e / G.sample_tol(c["dt"])))
    assert e >= 1000.0 * G.sample_tol(c["dt"])


# ---------------------------------------------------------------------------------------------------- 6. closure
@pytest.mark.parametrize("dt", [0.0, 0.3, -0.37])
def test_references_close_on_themselves(dt):
    """ref_framegen.frame -> ref_sync.sync (tables from ref_framegen.tables()) -> ref_decode, noise-free, one frame per
    modulation, V27 + CRC-24: header fields and payload bytes exact.
    CONVENTION (found by trial, then explained): the generator's dt is an advance, tau = -dt.  For tau > 0 and for tau < 0 the
    aligned sample 0 is the frame's first sample.  tau = 0 exactly falls under ref_sync's `tau <= 0` rule, whose grid is one
    sample early while its branch floor(32 (1 + 0)) mod 32 wraps to 0: there the aligned sample 0 is the frame's SECOND sample
    (start = 1), the same instants as (start = 0, tau = +0)."""
    tb = G.tables()
    rng = np.random.default_rng(11)
    worst = -np.inf
    for ms in R.PAYLOAD_MODS:
        payload = rng.integers(0, 256, 40, dtype=np.uint8)
        user = rng.integers(0, 256, 14, dtype=np.uint8)
        x = np.concatenate([G.frame(payload, ms, R.FEC_V27, R.FEC_NONE, R.CRC_24, header=user, dt=dt), np.zeros(64, np.complex128)])
        tau = -float(np.float32(dt))
        out = rs.sync(x, 1 if tau == 0.0 else 0, tau, 1.0, 0.0, 0.0, tb)
        assert out["header_valid"] and not out["short"], (ms, dt)
        assert out["props"] == dict(payload_len=40, ms=ms, check=R.CRC_24, fec0=R.FEC_V27, fec1=R.FEC_NONE)
        assert out["header"][:14] == user.tobytes()
        l1 = R.packet_dims(40, R.CRC_24, R.FEC_V27, R.FEC_NONE)[2]
        got, valid = R.packet_decode(R.symbols_to_bytes(ms, out["labels"], l1), 40, R.CRC_24, R.FEC_V27, R.FEC_NONE)
        assert valid and got == payload.tobytes(), (ms, dt)
        sent = G.payload_points(payload, ms, R.CRC_24, R.FEC_V27, R.FEC_NONE)
        evm = 10.0 * np.log10(np.mean(np.abs(out["r"] - sent) ** 2))
        worst = max(worst, evm)
        print("closure dt %+.2f mod %2d: payload EVM %.1f dB" % (dt, ms, evm))
    print("closure dt %+.2f: worst payload EVM %.1f dB" % (dt, worst))
