"""The HIP payload decode path against the plain numpy reference of tests/ref_decode.py -- not against the oracle, which
shares the decoders' construction with the kernels (a bug common to both passes every parity test).

Traffic: synth_stream cases whose SNRs put every decoder near its limit (convolutional codes near their thresholds, block
codes at and past their correction radius, Reed-Solomon blocks with 9-16 and more byte errors), payload lengths that hit the
codes' tails.  For every header-valid frame:
  * hard decisions: the reference decoded from the GPU's own carrier-recovered symbols (framesyms) gives the GPU's payload
    bytes and validity exactly (frames with a symbol within TIE of a decision boundary are excluded and counted);
  * soft decisions: the GPU's soft bytes are within 1 of the reference soft demapper on framesyms, and the reference's soft
    chain run on those bytes gives the GPU's payload and validity exactly.
Each decode path (clean-frame short cut on / off, batch Viterbi block lengths, forced repairs / retraces / fallbacks, the
Reed-Solomon instance, the soft instance) is compared with the reference, and the timing counters show that it ran.  Coverage
floors -- counted from the true payloads re-encoded against the GPU's hard decisions -- keep the traffic from being kind."""
import collections

import numpy as np
import pytest

import ref_decode as R

pytestmark = pytest.mark.gpu

# decision margin (distance to the runner-up point minus distance to the nearest) below which a symbol's hard decision may
# legitimately differ: PSK sectors come from a polynomial atan2 (errors up to ~1e-6 rad), ASK / QAM levels from one float32
# multiply-add and a floor
TIE = {m: 1e-5 for m in (R.PSK2, R.PSK4, R.PSK8, R.PSK16) + R.DPSK}
TIE_GRID = 2e-6

# (mod, fec0, fec1, check, payload_len, snr_db): each decoder near its limit
CASES = [
    (R.QAM16, R.FEC_V27, R.FEC_NONE, R.CRC_24, 300, 9.0),
    (R.PSK4, R.FEC_V27, R.FEC_NONE, R.CRC_24, 200, 3.0),
    (R.PSK8, R.FEC_V27, R.FEC_NONE, R.CRC_16, 150, 8.0),
    (R.QAM16, R.FEC_V27P23, R.FEC_NONE, R.CRC_24, 200, 11.0),
    (R.PSK8, R.FEC_V27P34, R.FEC_NONE, R.CRC_24, 150, 11.0),
    (R.PSK4, R.FEC_V27P45, R.FEC_NONE, R.CRC_32, 100, 6.5),
    (R.QAM16, R.FEC_V27P56, R.FEC_NONE, R.CRC_24, 120, 14.0),
    (R.PSK8, R.FEC_V27P67, R.FEC_NONE, R.CRC_8, 90, 12.5),
    (R.QAM16, R.FEC_V27P78, R.FEC_NONE, R.CRC_24, 80, 15.0),
    (R.PSK4, R.FEC_V27, R.FEC_NONE, R.CRC_24, 400, 14.0),                 # clean frames: the short cut
    # block codes as fec0, lengths k = n + crc with k mod 3 = 0, 1, 2 (Golay, Hamming(12,8)) and k mod 2, 4, 8 (SECDED)
    (R.QAM16, R.FEC_GOLAY, R.FEC_NONE, R.CRC_24, 297, 10.5),
    (R.QAM16, R.FEC_GOLAY, R.FEC_NONE, R.CRC_24, 298, 10.0),
    (R.QAM64, R.FEC_GOLAY, R.FEC_NONE, R.CRC_16, 300, 17.5),
    (R.QAM16, R.FEC_H128, R.FEC_NONE, R.CRC_24, 100, 14.0),
    (R.QAM16, R.FEC_H128, R.FEC_NONE, R.CRC_24, 101, 14.0),
    (R.PSK8, R.FEC_H128, R.FEC_NONE, R.CRC_32, 101, 13.0),
    (R.QAM16, R.FEC_H74, R.FEC_NONE, R.CRC_24, 121, 14.0),
    (R.PSK16, R.FEC_H84, R.FEC_NONE, R.CRC_24, 80, 18.0),
    (R.QAM16, R.FEC_SD22, R.FEC_NONE, R.CRC_24, 120, 16.0),
    (R.QAM16, R.FEC_SD22, R.FEC_NONE, R.CRC_24, 121, 16.0),
    (R.QAM16, R.FEC_SD39, R.FEC_NONE, R.CRC_24, 122, 16.0),
    (R.QAM16, R.FEC_SD39, R.FEC_NONE, R.CRC_32, 123, 16.0),
    (R.QAM16, R.FEC_SD72, R.FEC_NONE, R.CRC_24, 125, 17.0),
    (R.QAM64, R.FEC_SD72, R.FEC_NONE, R.CRC_8, 131, 20.0),
    # block codes as fec1 under a convolutional fec0
    (R.QAM16, R.FEC_V27, R.FEC_GOLAY, R.CRC_24, 120, 9.0),
    (R.QAM16, R.FEC_V27, R.FEC_H74, R.CRC_24, 100, 9.5),
    (R.PSK8, R.FEC_V27P23, R.FEC_H84, R.CRC_24, 90, 9.0),
    (R.QAM16, R.FEC_V27, R.FEC_H128, R.CRC_16, 110, 9.5),
    (R.QAM16, R.FEC_V27, R.FEC_SD22, R.CRC_24, 100, 9.5),
    (R.QAM16, R.FEC_V27P34, R.FEC_SD39, R.CRC_24, 90, 12.0),
    (R.QAM16, R.FEC_V27, R.FEC_SD72, R.CRC_24, 100, 9.5),
    # Reed-Solomon: fec0 alone with 1, 2, 3+ blocks and unequal fill, and next to V27 on either side
    (R.QAM16, R.FEC_RS, R.FEC_NONE, R.CRC_24, 219, 12.0),
    (R.QAM16, R.FEC_RS, R.FEC_NONE, R.CRC_24, 221, 12.0),
    (R.QAM16, R.FEC_RS, R.FEC_NONE, R.CRC_32, 443, 12.0),
    (R.QAM64, R.FEC_RS, R.FEC_NONE, R.CRC_24, 444, 19.0),
    (R.QAM16, R.FEC_RS, R.FEC_NONE, R.CRC_24, 700, 12.0),
    (R.QAM16, R.FEC_V27, R.FEC_RS, R.CRC_24, 100, 9.0),
    (R.QAM16, R.FEC_RS, R.FEC_V27, R.CRC_24, 300, 9.0),
    # differential PSK and ASK
    (R.DPSK4, R.FEC_V27, R.FEC_NONE, R.CRC_24, 150, 6.5),
    (R.DPSK8, R.FEC_H128, R.FEC_NONE, R.CRC_24, 60, 13.0),
    (R.ASK4, R.FEC_V27, R.FEC_NONE, R.CRC_24, 100, 9.5),
    (R.ASK4, R.FEC_GOLAY, R.FEC_SD39, R.CRC_24, 60, 11.0),
]
STREAM_LEN = 400_000
# about half of what the traffic reached when the floors were set (the CPU oracle's symbols are bit-identical to the GPU's)
FLOORS = {"golay words, 3 errors": 600, "golay words, >= 4 errors": 350, "secded blocks, 2 errors": 1800,
          "rs blocks, 9-16 errors": 300, "rs blocks, 16 errors": 10, "rs blocks, >= 17 errors": 120,
          "viterbi corrected at >= 2% BER": 350, "viterbi ML output wrong": 35}


def _traffic(fx):
    xs, inj = [], []
    for i, (m, f0, f1, chk, n, snr) in enumerate(CASES):
        x, fr = fx.synth_stream(STREAM_LEN, stream_id=4200 + i, mod=m, fec0=f0, fec1=f1, check=chk, payload_len=n, snr_db=snr)
        xs.append(x)
        inj.append(fr)
    return xs, inj


def _match(g, injected):
    """the injected payload of a received frame: the injected frame starting nearest to it (frames are >= 800 samples apart)"""
    best = min(injected, key=lambda pf: abs(pf[0] - g["start"]), default=None)
    return np.frombuffer(best[1], np.uint8) if best is not None and abs(best[0] - g["start"]) < 400 else None


class Ref:
    """the reference's view of one frame, from its carrier-recovered symbols"""

    def __init__(self, g):
        self.n, self.check, self.fec0, self.fec1, self.ms = len(g["payload"]), g["check"], g["fec0"], g["fec1"], g["mod_scheme"]
        self.k, self.l0, self.l1 = R.packet_dims(self.n, self.check, self.fec0, self.fec1)
        self.syms = g["framesyms"]
        assert len(self.syms) == R.num_symbols(self.ms, self.l1)
        self.labels, margin = R.demap_hard(self.ms, self.syms)
        self.tie = bool(len(margin) and margin.min() < TIE.get(self.ms, TIE_GRID))
        self.pkt = R.symbols_to_bytes(self.ms, self.labels, self.l1)
        self.trace = {}
        self.payload, self.valid = R.packet_decode(self.pkt, self.n, self.check, self.fec0, self.fec1, self.trace)
        self.soft = R.soft_to_channel(R.demap_soft(self.ms, self.syms, self.labels), self.l1)

    def soft_decode(self, soft_bits):
        return R.packet_decode_soft(soft_bits, self.n, self.check, self.fec0, self.fec1)


def _word_errors(fs, got, want, n):
    """per-codeword bit errors (byte errors for RS) of a stage's received codeword bytes against the true ones"""
    got, want = np.asarray(got, np.uint8), np.asarray(want, np.uint8)
    if fs in (R.FEC_H74, R.FEC_H128, R.FEC_GOLAY):
        k, w, _ = R.code_table(fs)
        nb = (8 * n + k - 1) // k
        return R.popcount(R.words_of(R.bits_of(got ^ want)[:nb * w], w))
    if fs == R.FEC_H84:
        return R.popcount(got ^ want)
    if fs in R.SECDED:
        return np.unpackbits(R.secded_blocks(fs, got, n) ^ R.secded_blocks(fs, want, n), axis=1).sum(axis=1)
    nb, dl = R.rs_dims(n)
    return (got.reshape(nb, dl + 32) != want.reshape(nb, dl + 32)).sum(axis=1)


def _coverage(ref, truth, cov):
    """count what the traffic reached, per stage, from the true payload re-encoded"""
    tr = {}
    R.packet_encode(truth, ref.check, ref.fec0, ref.fec1, tr)
    right = ref.payload == truth.tobytes() and ref.valid
    stages = ((ref.fec1, ref.trace["in1"], tr["cw1"], ref.l0, np.array_equal(ref.trace["out1"], R.interleave(tr["cw0"]))),
              (ref.fec0, ref.trace["in0"], tr["cw0"], ref.k, right))
    for fs, got, want, n, ok in stages:
        if fs == R.FEC_NONE:
            continue
        if fs in R.CONV:
            ber = float(R.bits_of(got ^ want).mean())
            cov["viterbi frames"] += 1
            cov["viterbi frames with channel errors"] += int(ber > 0)
            cov["viterbi corrected at >= 2% BER"] += int(ok and ber >= 0.02)
            cov["viterbi ML output wrong"] += int(not ok)
            continue
        e = _word_errors(fs, got, want, n)
        if fs == R.FEC_GOLAY:
            cov["golay words, 3 errors"] += int((e == 3).sum())
            cov["golay words, >= 4 errors"] += int((e >= 4).sum())
        elif fs in R.SECDED:
            cov["secded blocks, 1 error"] += int((e == 1).sum())
            cov["secded blocks, 2 errors"] += int((e == 2).sum())
        elif fs == R.FEC_RS:
            cov["rs blocks, 9-16 errors"] += int(((e >= 9) & (e <= 16)).sum())
            cov["rs blocks, 16 errors"] += int((e == 16).sum())
            cov["rs blocks, >= 17 errors"] += int((e >= 17).sum())
        else:
            name = {R.FEC_H74: "h74", R.FEC_H84: "h84", R.FEC_H128: "h128"}[fs]
            cov[name + " words, 1 error"] += int((e == 1).sum())
            cov[name + " words, >= 2 errors"] += int((e >= 2).sum())


def _run(fx, monkeypatch, xs, env, soft=False):
    for k in ("FXRX_VB_CLEAN", "FXRX_VB_BLK", "FXRX_VB_DEBUG"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    ctx = fx.RxContext(len(xs), want_framesyms=True, soft_decision=soft)
    got = ctx.process(xs)
    tm = ctx.timing()
    ctx.close()
    return got, tm


@pytest.fixture(scope="module")
def traffic(fx):
    return _traffic(fx)


@pytest.fixture(scope="module")
def reference(fx, traffic):
    """the default hard-decision run and the reference's view of each of its header-valid frames (keyed by stream, start)"""
    mp = pytest.MonkeyPatch()
    got, tm = _run(fx, mp, traffic[0], {})
    mp.undo()
    return got, tm, {(g["stream"], g["start"]): Ref(g) for g in got if g["header_valid"]}


def _compare_hard(got, refs, cases=CASES):
    n, excluded, bad = 0, 0, []
    for g in got:
        if not g["header_valid"]:
            continue
        r = refs[(g["stream"], g["start"])]
        assert np.array_equal(g["framesyms"].view(np.uint32), r.syms.view(np.uint32)), "framesyms differ between runs"
        n += 1
        if r.tie:
            excluded += 1
            continue
        if (g["payload"], g["payload_valid"]) != (r.payload, r.valid):
            bad.append((g["stream"], g["start"], cases[g["stream"]][:3], g["payload_valid"], r.valid))
    assert not bad, "payloads differ from the reference (stream, start, case, gpu valid, ref valid): %s" % bad[:10]
    assert excluded < 0.01 * n, (excluded, n)
    return n, excluded


def test_hard_decode_and_coverage(traffic, reference):
    """default path: every header-valid frame equals the reference; the traffic reaches every decoder's edges"""
    _, inj = traffic
    got, tm, refs = reference
    n, excluded = _compare_hard(got, refs)
    cov, per_case = collections.Counter(), collections.Counter()
    for g in got:
        if not g["header_valid"]:
            continue
        per_case[g["stream"]] += 1
        truth = _match(g, inj[g["stream"]])
        if truth is not None and len(truth) == len(g["payload"]):
            _coverage(refs[(g["stream"], g["start"])], truth, cov)
            cov["frames with truth"] += 1
            cov["payloads invalid"] += int(not g["payload_valid"])
    print("\nframes compared %d, excluded (tie) %d, timing %s" % (n, excluded, {k: tm[k] for k in ("vb_clean", "vb_blocks", "vb_repairs", "vb_fallbacks")}))
    print("header-valid frames per case:", dict(per_case))
    print("coverage:")
    for k in sorted(cov):
        print("  %-34s %8d   floor %s" % (k, cov[k], FLOORS.get(k)))
    assert all(per_case[i] > 0 for i in range(len(CASES))), "a case lost every header: %s" % dict(per_case)
    for k, f in FLOORS.items():
        assert cov[k] >= f, (k, cov[k], f)
    assert tm["vb_clean"] > 0 and tm["vb_blocks"] > 0


@pytest.mark.parametrize("env", [dict(FXRX_VB_CLEAN=0), dict(FXRX_VB_BLK=128), dict(FXRX_VB_BLK=448),
                                 dict(FXRX_VB_DEBUG=1), dict(FXRX_VB_DEBUG=2, FXRX_VB_BLK=128)],
                         ids=["clean0", "blk128", "blk448", "debug1", "debug2"])
def test_hard_decode_paths(fx, monkeypatch, traffic, reference, env):
    """the same traffic down each batch-Viterbi path: still the reference's payloads, and the path ran"""
    got, tm = _run(fx, monkeypatch, traffic[0], env)
    _compare_hard(got, reference[2])
    print("timing", {k: tm[k] for k in ("vb_clean", "vb_blocks", "vb_repairs", "vb_fallbacks")})
    assert tm["vb_blocks"] > 0
    assert (tm["vb_clean"] == 0) if env.get("FXRX_VB_CLEAN") == 0 else (tm["vb_clean"] > 0)
    if env.get("FXRX_VB_DEBUG") == 1:
        assert tm["vb_repairs"] + tm["vb_fallbacks"] > 0
    if env.get("FXRX_VB_DEBUG") == 2:
        assert tm["vb_fallbacks"] > 0


def _compare_soft(got, refs, cases=CASES):
    n, excluded, bad, off = 0, 0, [], 0
    for g in got:
        if not g["header_valid"]:
            continue
        r = refs[(g["stream"], g["start"])]
        assert np.array_equal(g["framesyms"].view(np.uint32), r.syms.view(np.uint32))
        n += 1
        if r.tie:
            excluded += 1
            continue
        sb = g["soft_bits"]
        assert sb is not None and len(sb) == 8 * r.l1
        d = np.abs(sb.astype(np.int64) - r.soft.astype(np.int64))
        assert d.max() <= 1, (g["stream"], cases[g["stream"]][:3], int(d.max()))
        off += int((d == 1).sum())
        if (g["payload"], g["payload_valid"]) != r.soft_decode(sb):
            bad.append((g["stream"], g["start"], cases[g["stream"]][:3]))
    assert not bad, bad[:10]
    assert excluded < 0.01 * n
    return n, excluded, off


def test_soft_decode(fx, monkeypatch, traffic, reference):
    """soft instance: soft bytes within 1 of the reference demapper; the reference soft chain on the GPU's soft bytes gives
    the GPU's payloads and validity"""
    got, tm = _run(fx, monkeypatch, traffic[0], {}, soft=True)
    n, excluded, off = _compare_soft(got, reference[2])
    print("\nsoft frames compared %d, excluded %d, soft bytes off by one %d, vb_blocks %d" % (n, excluded, off, tm["vb_blocks"]))
    assert tm["vb_blocks"] == 0                     # soft decisions run on the wave-per-frame decoder


MAXLEN_CASES = [(R.QAM16, R.FEC_V27, R.FEC_NONE, R.CRC_24, 12.0), (R.QAM16, R.FEC_RS, R.FEC_V27, R.CRC_32, 10.5)]


@pytest.mark.parametrize("soft", [False, True], ids=["hard", "soft"])
def test_maximum_length_with_errors(fx, monkeypatch, soft):
    """65535-byte payloads at SNRs where the hard decisions carry errors that the codes still correct: V27 alone (524 294
    trellis steps, the batch path when hard) and Reed-Solomon (294 blocks) outside V27"""
    xs, inj = [], []
    for i, (m, f0, f1, chk, snr) in enumerate(MAXLEN_CASES):
        g = fx.FrameGen(m, f0, f1, chk)
        n = len(g.frame(np.zeros(65535, np.uint8)))
        g.close()
        x, fr = fx.synth_stream(n + 2000, stream_id=4300 + i, mod=m, fec0=f0, fec1=f1, check=chk, payload_len=65535, snr_db=snr, lead=500)
        assert len(fr) == 1
        xs.append(x)
        inj.append(fr)
    got, tm = _run(fx, monkeypatch, xs, {}, soft=soft)
    assert len(got) == 2 and all(g["header_valid"] and len(g["payload"]) == 65535 for g in got)
    cov = collections.Counter()
    for g in got:
        r = Ref(g)
        assert not r.tie
        assert (g["payload"], g["payload_valid"]) == (r.soft_decode(g["soft_bits"]) if soft else (r.payload, r.valid))
        truth = np.frombuffer(inj[g["stream"]][0][1], np.uint8)
        _coverage(r, truth, cov)
        assert g["payload_valid"] and g["payload"] == truth.tobytes()
    print("\n", dict(cov), {k: tm[k] for k in ("vb_clean", "vb_blocks", "vb_repairs", "vb_fallbacks")})
    assert cov["viterbi frames"] == 2 and cov["viterbi frames with channel errors"] == 2
    if not soft:
        assert tm["vb_blocks"] > 0 and tm["vb_clean"] == 0


# The LDS staging size of the one-wave decode workgroups: mirrors DEC_LDS in csrc/fx_kernels.hip.  fx_vbpre_kernel (batch Viterbi
# path) keeps a packet in LDS when both coded lengths + 32 fit, deinterleave_staged (wave-per-frame path) when the length + 16 does.
LDS_STAGE = 4608
# (fec0, fec1, snr_db, slack, the payload lengths the rule gives: the last two whose packet fits, the first two that do not).
# QAM16, CRC_24; SNRs: those of QAM16 with the same fec0 in CASES (V27 alone, V27 over a Hamming code, a Hamming code alone)
LDS_EDGES = [
    (R.FEC_V27, R.FEC_NONE, 9.0, 32, [2283, 2284, 2285, 2286]),           # l = 2 k + 2: 4576 is the last that fits
    (R.FEC_V27, R.FEC_H84, 9.5, 32, None),                                # l1 = 2 l0 straddles the limit while l0 fits
    (R.FEC_H84, R.FEC_NONE, 14.0, 16, [2292, 2293, 2294, 2295]),          # l = 2 k: 4592 is the last that fits
]


def _lds_edge_cases():
    cases = []
    for f0, f1, snr, slack, want in LDS_EDGES:
        last = max(n for n in range(1, 4096) if R.packet_dims(n, R.CRC_24, f0, f1)[2] + slack <= LDS_STAGE)
        ns = [last - 1, last, last + 1, last + 2]
        assert want is None or ns == want, (ns, want)
        for i, n in enumerate(ns):
            k, l0, l1 = R.packet_dims(n, R.CRC_24, f0, f1)
            assert k == n + 3
            assert (l1 + slack <= LDS_STAGE) == (i < 2), (n, l1)
            if f1 != R.FEC_NONE:
                assert l0 + 32 <= LDS_STAGE, (n, l0)                          # (fx_vbpre_kernel's rule is on both lengths: here l1 alone decides)
            cases.append((R.QAM16, f0, f1, R.CRC_24, n, snr))
    assert R.packet_dims(2284, R.CRC_24, R.FEC_V27, R.FEC_NONE)[2] == 4576 and R.packet_dims(2293, R.CRC_24, R.FEC_H84, R.FEC_NONE)[2] == 4592
    return cases


def test_lds_fit_boundaries(fx, monkeypatch):
    """one frame per stream at the payload lengths either side of each LDS-fit rule, with channel errors: the batch path's front
    kernel (default and without the clean-frame short cut) and the wave-per-frame decoder, hard and soft, against the reference"""
    cases = _lds_edge_cases()
    xs, inj = [], []
    for i, (m, f0, f1, chk, n, snr) in enumerate(cases):
        g = fx.FrameGen(m, f0, f1, chk)
        flen = len(g.frame(np.zeros(n, np.uint8)))
        g.close()
        x, fr = fx.synth_stream(flen + 2000, stream_id=4400 + i, mod=m, fec0=f0, fec1=f1, check=chk, payload_len=n, snr_db=snr, lead=500)
        assert len(fr) == 1
        xs.append(x)
        inj.append(fr)
    got, tm = _run(fx, monkeypatch, xs, {})
    assert [g["stream"] for g in got] == list(range(len(cases)))
    assert all(g["header_valid"] and len(g["payload"]) == c[4] and (g["fec0"], g["fec1"]) == c[1:3] for g, c in zip(got, cases))
    refs = {(g["stream"], g["start"]): Ref(g) for g in got}
    assert not any(r.tie for r in refs.values()), "a frame would be excluded as a tie: choose another stream_id"
    cov = collections.Counter()
    for g in got:
        _coverage(refs[(g["stream"], g["start"])], np.frombuffer(inj[g["stream"]][0][1], np.uint8), cov)
    print("\n", dict(cov), "valid payloads %d of %d" % (sum(g["payload_valid"] for g in got), len(got)))
    assert cov["viterbi frames with channel errors"] == 8 and cov["h84 words, 1 error"] > 0
    assert _compare_hard(got, refs, cases) == (len(cases), 0)
    assert tm["vb_blocks"] > 0
    got, tm = _run(fx, monkeypatch, xs, dict(FXRX_VB_CLEAN=0))
    assert _compare_hard(got, refs, cases) == (len(cases), 0)
    assert tm["vb_blocks"] > 0 and tm["vb_clean"] == 0
    got, tm = _run(fx, monkeypatch, xs, {}, soft=True)
    assert _compare_soft(got, refs, cases)[:2] == (len(cases), 0)
    assert tm["vb_blocks"] == 0
