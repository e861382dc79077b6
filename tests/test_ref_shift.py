"""Every case of tests/shift_cases.py is what its name says, proved on the CPU from the oracle's frames: per block, the class counts
(which decoder a frame goes to -- shift_cases.CLASS --, trellis work items) satisfy the case's inequalities against the block before,
for continuing streams and for independent captures alike.  Without this the GPU tests of tests/test_gpu_traffic_shift.py could pass
on traffic that never leaves the launched grids.  No GPU."""
import pytest

import ref_decode as R
import shift_cases as SC

NAMES = list(SC.CASES) + [SC.ARENA]


def test_class_table_covers_every_code_pair():
    fecs = (R.FEC_NONE, R.FEC_RS) + R.CONV + R.BLOCK
    for soft in (0, 1):
        for f0 in fecs:
            for f1 in fecs:
                k = SC.frame_class(f0, f1, soft)
                assert k in ("plain", "batch", "rs")
                # the batch path: hard decisions, a convolutional fec0, fec1 neither convolutional nor Reed-Solomon; Reed-Solomon on either side otherwise
                want = "batch" if (not soft and f0 in R.CONV and f1 not in R.CONV and f1 != R.FEC_RS) else "rs" if R.FEC_RS in (f0, f1) else "plain"
                assert k == want, (soft, f0, f1)


@pytest.mark.parametrize("form", ["cont", "reset"])
@pytest.mark.parametrize("name", NAMES)
def test_case_is_what_its_name_says(fx, oracle, name, form):
    c = SC.case(name)
    blocks = SC.build(name)
    cnt = SC.block_counts(name, form)
    print("\n%s (%s): samples %s, counts %s" % (name, form, [[len(x) for x in b] for b in blocks], cnt))
    assert 1 <= len(blocks[0]) <= 3
    for b, key, kind in c["checks"]:
        now, before = cnt[b][key], (cnt[b - 1][key] if b else 0)
        if kind == "zero":
            assert now == 0, (b, key, now)
        elif kind == "some":
            assert now > 0, (b, key, now)
        elif kind == "from_zero":
            assert before == 0 and now > 0, (b, key, before, now)
        elif kind == "one":
            assert now == 1, (b, key, now)
        elif kind == "jump":
            assert now >= SC.JUMP_FACTOR * before + SC.JUMP_FRAMES, (b, key, before, now)
        elif kind == "jump_items":
            assert now > SC.JUMP_FACTOR * before + SC.JUMP_ITEMS, (b, key, before, now)
        elif kind == "over32":
            assert now > 32, (b, key, now)
        elif kind == "arena":
            # trellis steps beyond 1.5 per sample of the block by more than the 2048 spare work items, and no smaller frame count does it
            samples = sum(len(x) for x in blocks[b])
            per = now // cnt[b]["batch"]
            assert now * SC.VB_BLK_FORCED > samples + samples // 2 + SC.JUMP_ITEMS * SC.VB_BLK_FORCED, (now, samples)
            assert cnt[b]["batch"] == SC.arena_frames() == cnt[b]["frames"] and cnt[b]["plain"] == 0 and now == per * cnt[b]["batch"]
        else:
            raise AssertionError(kind)
    if not c.get("detector"):
        # every frame that was sent is found with a valid header (the counts above are of what the receiver sees, not of what was sent)
        sent = [sum(p["frames"] for pieces in blk for p in pieces) for blk in c["blocks"]]
        noisy = any(p["snr"] < 12.0 for blk in c["blocks"] for pieces in blk for p in pieces)
        for b, n in enumerate(sent):
            assert cnt[b]["valid"] == n or (noisy and 0.7 * n <= cnt[b]["valid"] <= n), (b, n, cnt[b])
    # blocks of 60 k to 120 k samples per stream, but for the cases whose transition takes more (dense short frames, the long trellis, the arena)
    assert all(len(x) <= 420_000 for b in blocks for x in b)


def test_all_formats_block_holds_every_modulation_and_code_family(fx, oracle):
    blk = SC.oracle(SC.ALL_MODS_CASE, "reset")[1]
    fr = [f for s in blk for f in s if f.header_valid]
    assert {f.mod_scheme for f in fr} == set(R.PAYLOAD_MODS)
    fam = lambda f: "none" if f == R.FEC_NONE else "v27" if f == R.FEC_V27 else "punctured" if f in R.CONV else "rs" if f == R.FEC_RS else \
        "hamming" if f in (R.FEC_H74, R.FEC_H84, R.FEC_H128) else "golay" if f == R.FEC_GOLAY else "secded"
    assert {fam(f.fec0) for f in fr} | {fam(f.fec1) for f in fr} == {"none", "v27", "punctured", "rs", "hamming", "golay", "secded"}
    assert all(f.payload_valid for f in fr)
