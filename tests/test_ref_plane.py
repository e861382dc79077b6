"""The plane frames of tests/plane_cases.py, without a GPU: each case is what it says -- the oracle receiver delivers exactly
the crafted frames, ties are rare, the far frames reach every clamp of the grid schemes from beyond the outermost level, every
PSK sector is decided from far off its centre, soft values saturate at both ends and in between at every bit position, the
second work item of 1024 symbols and the padded last symbol exist -- and the numpy reference and the oracle agree on every
symbol, hard and soft.  This is the condition under which tests/test_gpu_plane.py may judge the kernels by these frames; a
later edit that makes the cases kinder fails here."""
import numpy as np
import pytest

import plane_cases as PC
import ref_decode as R
from parity_util import oracle_frames


@pytest.fixture(scope="module")
def runs(oracle):
    """per stream: (cases, the oracle receiver's frames hard, soft)"""
    return [(cs, oracle_frames(oracle, x), oracle_frames(oracle, x, soft=True)) for x, cs in PC.streams()]


@pytest.fixture(scope="module")
def views(runs):
    """per stream, per case: ref_decode's view of the oracle's symbols"""
    return [[PC.View(c, f.framesyms) for c, f in zip(cs, hard)] for cs, hard, _ in runs]


def test_case_list_shape():
    st = PC.streams()
    assert [cs[0]["mod"] for _, cs in st] == list(R.PAYLOAD_MODS)
    assert len({len(x) for x, _ in st}) == 1 and len(st[0][0]) < 20_000 and all(x.dtype == np.complex64 and not x.flags.writeable for x, _ in st)
    for x, cs in st:
        ms, k = cs[0]["mod"], R.bps(cs[0]["mod"])
        assert [c["kind"] for c in cs] == list(PC.KINDS) and all(c["gap"] >= 300 for c in cs)
        assert all((c["check"], c["fec0"], c["fec1"]) == (R.CRC_NONE, R.FEC_NONE, R.FEC_NONE) for c in cs)
        assert all(R.packet_dims(c["n"], c["check"], c["fec0"], c["fec1"])[2] == c["n"] for c in cs)
        plane, far, tiny = cs
        assert 1025 <= plane["nsym"] <= 2047
        assert plane["padded"] == (k in (3, 5, 6)) == ((8 * plane["n"]) % k != 0)            # the padded last symbol exists
        assert far["nsym"] == (352 if ms == R.QAM64 else 256) and far["listed"] >= 3 * (1 << k) and far["factors"] == PC.FAR_FACTORS[ms]
        assert tiny["n"] == 1 and tiny["nsym"] == -(-8 // k)
        rad = PC.SPREAD * np.abs(R.constellation(ms)[0]).max()
        p = plane["points"]
        assert R.demap_hard(ms, p[:PC.SETTLE])[1].min() > 0.1                                   # settling points are true points
        assert max(np.abs(p.real).max(), np.abs(p.imag).max()) <= rad and np.abs(p[PC.SETTLE + PC.RAYS:]).max() > 0.8 * rad
    assert sum(len(cs) for _, cs in st) == 33


def test_oracle_receiver_delivers_exactly_the_crafted_frames(runs):
    """in order, where they were put, header valid and stating the case's properties, no extra detection; hard and soft runs
    see the same symbols"""
    for cs, hard, soft in runs:
        lay, _ = PC.layout(cs)
        for of in (hard, soft):
            assert len(of) == len(cs), (cs[0]["mod"], len(of))
            for f, (off, c) in zip(of, lay):
                assert f.header_valid, c["name"]
                assert (f.mod_scheme, f.check, f.fec0, f.fec1, len(f.payload), len(f.framesyms)) == (c["mod"], c["check"], c["fec0"], c["fec1"], c["n"], c["nsym"]), c["name"]
                assert abs(f.info["start"] - off) <= 64, (c["name"], f.info["start"], off)
        for a, b in zip(hard, soft):
            assert np.array_equal(a.framesyms.view(np.uint32), b.framesyms.view(np.uint32))
            assert b.soft is not None and len(b.soft) == 8 * len(b.payload)


def test_ties_are_rare_and_the_second_work_item_is_judged(runs, views):
    print()
    lo, hi = 9.0, 0.0
    for (cs, _, _), vs in zip(runs, views):
        ms = cs[0]["mod"]
        ties, total = sum(int(v.tie.sum()) for v in vs), sum(len(v.r) for v in vs)
        lo, hi = min(lo, min(np.abs(v.r).min() for v in vs)), max(hi, max(np.abs(v.r).max() for v in vs))
        print("scheme %2d: %4d symbols, %d ties (%.2f %%), per frame %s" % (ms, total, ties, 100.0 * ties / total, [int(v.tie.sum()) for v in vs]))
        assert ties <= PC.TIE_CAP * total, (ms, ties, total)
        assert ties == PC.MEASURED_TIES[ms], (ms, ties)
        plane = vs[0]
        assert len(plane.r) > 1024 and int((~plane.tie[1024:]).sum()) >= 0.9 * (len(plane.r) - 1024)
        if R.bps(ms) in (3, 5, 6):
            assert (8 * cs[0]["n"]) % R.bps(ms) != 0 and not plane.tie[-1], "the padded last symbol is a tie: choose another seed"
    print("received |r|: %.4f .. %.2f" % (lo, hi))
    assert lo < 0.05 and hi > 8.0


@pytest.mark.parametrize("ms", PC.GRID)
def test_far_frames_reach_every_clamp(runs, views, ms):
    """the hard labels of non-tie symbols include each outermost level, on both sides of both axes, decided from a received
    coordinate beyond that level -- and beyond it by 2, 4 and 8 level spacings (within a third of a spacing)"""
    s = R.PAYLOAD_MODS.index(ms)
    v = views[s][1]
    al, Li, Lq = PC.axes(ms)
    ii, iq = PC.level_indices(ms, v.labels)
    for coord, idx, L in ((v.r.real, ii, Li), (v.r.imag, iq, Lq)):
        if L == 1:
            continue
        edge = (L - 1) * al
        for side, level in ((1.0, L - 1), (-1.0, 0)):
            beyond = (side * coord - edge) / (2.0 * al)
            for f in PC.FAR_FACTORS[ms]:
                hit = ~v.tie & (np.abs(beyond - f) < 1.0 / 3.0)
                assert hit.sum() >= 2 and (idx[hit] == level).all(), (ms, side, f, int(hit.sum()))
    # and the plane frame, less far out
    p = views[s][0]
    ii, iq = PC.level_indices(ms, p.labels)
    assert (~p.tie & (ii == Li - 1) & (p.r.real > (Li - 1) * al)).any() and (~p.tie & (ii == 0) & (p.r.real < -(Li - 1) * al)).any()


@pytest.mark.parametrize("ms", PC.PSK)
def test_every_sector_is_decided_from_far_off_its_centre(views, ms):
    s = R.PAYLOAD_MODS.index(ms)
    M = 1 << R.bps(ms)
    pts = R.constellation(ms)[0]
    v = views[s][0]
    off = np.abs(np.angle(v.r * np.conj(pts[v.index])))
    assert off.max() <= np.pi / M + 1e-9
    far = ~v.tie & (off > 0.25 * 2.0 * np.pi / M)
    assert set(v.index[far].tolist()) == set(range(M)), ms
    if ms in R.DPSK:                                            # every step of the running index, too
        assert set(v.labels[~v.tie].tolist()) == set(range(M))


def test_soft_values_saturate_both_ways_at_every_bit(runs):
    for cs, _, soft in runs:
        ms, k = cs[0]["mod"], R.bps(cs[0]["mod"])
        if ms in R.DPSK:
            assert all(set(np.unique(f.soft)) <= {0, 255} for f in soft)
            continue
        for b in range(k):
            col = np.concatenate([f.soft[:len(f.soft) // k * k].reshape(-1, k)[:, b] for f in soft])     # (whole symbols)
            assert (col == 0).any() and ((col > 1) & (col < 254)).any(), (ms, b)
            if (ms, b) == (R.ASK4, 1):
                # the one bit that cannot reach 255: the inner levels +-1/sqrt(5) carry the 1, and midway between them d0 - d1 =
                # (3^2 - 1^2) / 5 = 1.6 is as large as it gets: 127 + 16 x 1.2 x 4 x 1.6 = 249.88
                assert col.max() == 250, int(col.max())
            else:
                assert (col == 255).any(), (ms, b)
        far = soft[1].soft.reshape(-1, k)[PC.SETTLE:]
        assert ((far == 0) | (far == 255)).mean() > 0.75, ms           # most far symbols saturate (16-PSK times 2 does not, at its low bits)


def test_reference_and_oracle_agree_on_every_symbol(runs, views):
    """hard labels equal on non-tie symbols; soft bytes within 1 of ref_decode.demap_soft and equal away from rounding ties
    (test_demappers_match_oracle_over_the_plane's criterion); the hard payload is the reference's packet decode of the
    labels (the oracle's own at tie symbols), the soft payload and validity the reference's soft chain on the oracle's soft bytes"""
    n_sym = n_off = n_differ = 0
    for (cs, hard, soft), vs in zip(runs, views):
        for c, fh, fs, v in zip(cs, hard, soft, vs):
            ms, k, n = c["mod"], v.k, c["n"]
            ob, ex = PC.payload_label_bits(ms, fh.payload, n)
            bad = np.nonzero(((ob != v.bits) & ex & ~v.tie[:, None]).any(axis=1))[0]
            assert not len(bad), "%s: symbol %d at %s: oracle %s, reference %s" % (c["name"], bad[0], v.r[bad[0]], ob[bad[0]], v.bits[bad[0]])
            assert (fh.payload, fh.payload_valid) == v.payload_of(np.where(ex, v.labels_with(ob), 0)), c["name"]
            want, exact = v.soft(np.where(ex, ob, v.bits))
            want, exact = want.ravel()[:8 * n].astype(int), exact.ravel()[:8 * n]
            d = np.abs(fs.soft.astype(int) - want)
            if ms in R.DPSK:
                assert not d.any(), c["name"]
            else:
                i = int(d.argmax())
                assert d.max() <= 1 and not d[exact].any(), "%s: soft value %d (symbol %d at %s): oracle %d, reference %d" % (
                    c["name"], i, i // k, v.r[i // k], fs.soft[i], want[i])
            n_off += int((d == 1).sum())
            assert (fs.payload, fs.payload_valid) == v.soft_decode(fs.soft), c["name"]
            n_differ += int(fs.payload != fh.payload)
            n_sym += len(v.r)
    print("\n%d symbols, %d soft bytes off by one, %d frames whose soft payload is not the hard one" % (n_sym, n_off, n_differ))
    assert n_differ >= 5                                        # (a soft byte of 127 decodes as 0 where the hard label may be 1)


def test_guard_streams(oracle):
    """the two variants differ in the last symbol alone (and what its pulse leaves on the ones before), and there in the soft value of the first bit the packet does not hold"""
    g = PC.guard_streams()
    assert [c["mod"] for c in g["cases"]] == list(PC.GUARD_MODS)
    for xa, xb, c, bit in zip(g["a"], g["b"], g["cases"], g["bit"]):
        (fa,), (fb,) = oracle_frames(oracle, xa, soft=True), oracle_frames(oracle, xb, soft=True)
        k = R.bps(c["mod"])
        assert fa.header_valid and fb.header_valid and len(fa.framesyms) == len(fb.framesyms) == c["nsym"] and bit == 8 - k * (c["nsym"] - 1) < k
        assert np.abs(fa.framesyms[:-1] - fb.framesyms[:-1]).max() < 0.02                       # (the pulses' overlap alone)
        va, vb = PC.View(c, fa.framesyms), PC.View(c, fb.framesyms)
        assert int(vb.soft()[0][-1, bit]) - int(va.soft()[0][-1, bit]) > 100, c["name"]
