"""The full-length cases of tests/soft_scale_cases.py without a GPU: every case is what its name says, from the numpy references
alone (tests/ref_block_soft.py, ref_block_siso.py, ref_rs_soft.py), and three wrong decoders disagree with the references on the
cases named here.

  counts     a case's lengths come from ref_decode.packet_dims for a 65535-byte payload with CRC-32; its codewords, rounds of 64
             lanes and Reed-Solomon blocks are those of a full-length frame (Golay behind V27: 87 387 codewords
             in 1366 rounds; Reed-Solomon: 294 and 588 blocks, the last block of either with fewer message bytes than dl).
  coverage   conditions, not measurements.  Per soft-block packet the soft decoder's message differs from the hard decoder's on
             the hard word in a codeword of the first round, of the last round, and of a round beyond the one that holds the
             129th codeword.  Per Reed-Solomon packet at least half the blocks have a non-zero syndrome and every third of the
             packet has a block won by a candidate with f > 0.
  controls   a soft-output decoder run in place without the barrier between a round's reads and writes; a Reed-Solomon decoder
             with the previous block's erasure order; a soft-block decoder whose codeword index wraps at 2^16."""
import numpy as np
import pytest

import ref_decode as R
import ref_block_soft as B
import ref_rs_soft as RS
import siso_cases as SK
import soft_scale_cases as K


# ---------------------------------------------------------------------------------------------------- the lengths
def test_lengths_are_those_of_a_full_length_packet():
    d = K.stage_lengths()
    assert d["k"] == 65535 + 4 and K.MOST_PUNCTURED == R.FEC_V27P78
    assert d["l0_v27"] == R.fec_enc_len(R.FEC_V27, d["k"]) == (2 * (8 * d["k"] + 6) + 7) // 8
    assert d["l0_punct"] == R.fec_enc_len(R.FEC_V27P78, d["k"]) and d["k"] < d["l0_punct"] < d["l0_v27"]
    assert all(R.fec_enc_len(f, d["k"]) >= d["l0_punct"] for f in R.CONV)
    assert len(K.BLOCK_CASES) == 4 * len(B.SOFT_BLOCK) and len(set(K.BLOCK_CASES)) == len(K.BLOCK_CASES)
    # Golay: 43 693 codewords in 683 rounds at n = k, twice that behind V27
    assert (SK.ncw(R.FEC_GOLAY, d["k"]), K.rounds_of(R.FEC_GOLAY, d["k"])) == (43693, 683)
    assert (SK.ncw(R.FEC_GOLAY, d["l0_v27"]), K.rounds_of(R.FEC_GOLAY, d["l0_v27"])) == (87387, 1366)


@pytest.mark.parametrize("fs", B.SOFT_BLOCK)
def test_short_length_ends_short(fs):
    n, d = K.short_length(fs), K.stage_lengths()
    assert d["l0_punct"] < n < d["l0_v27"] and n not in (d["k"], d["l0_v27"], d["l0_punct"])
    if fs == R.FEC_GOLAY:
        k, w, ncw, el = R._packed_dims(fs, n)
        assert 8 * n - k * (ncw - 1) == 4                              # the last codeword carries four message bits
    elif fs in R.SECDED:
        nd = R.SECDED[fs][0]
        assert n % nd == 1 and R.fec_enc_len(fs, n) == (n // nd) * (nd + 1) + 2           # a last block of parity and one data byte
    else:
        assert 0 < SK.ncw(fs, n) % K.LANES < K.LANES                   # Hamming: the last round is partial
    assert K.rounds_of(fs, n) > 129


# ---------------------------------------------------------------------------------------------------- soft-block packets
@pytest.mark.parametrize("c", K.BLOCK_CASES, ids=K.case_id)
def test_block_case_makes_the_soft_decoder_work_in_every_part(c):
    fs, n = c
    ref = K.block_reference(fs, n)
    el = R.fec_enc_len(fs, n)
    assert ref["soft"].shape == (K.PACKETS, 8 * el) and ref["dec"].shape == ref["hard"].shape == (K.PACKETS, n)
    assert ref["siso"].shape == (K.PACKETS, 8 * n)
    assert K.rounds_of(fs, n) == -(-SK.ncw(fs, n) // 64) > 3
    # the soft outputs' signs are the soft decoder's message
    assert (np.packbits(ref["siso"] > 127, axis=1) == ref["dec"]).all()
    for p, lanes in enumerate(K.lanes_that_differ(fs, ref["dec"], ref["hard"])):
        first, last, far = K.round_coverage(fs, n, lanes)
        print("%s packet %d: soft != hard in %d of %d codewords; first round %d, last round %d, beyond the 129th %d" % (
            K.case_id(c), p, len(lanes), SK.ncw(fs, n), first, last, far))
        assert first >= 1 and last >= 1 and far >= 1, (K.case_id(c), p, first, last, far)
    assert (ref["dec"][0] != ref["dec"][1]).any()                      # two packets, not one twice


# ---------------------------------------------------------------------------------------------------- Reed-Solomon packets
@pytest.mark.parametrize("n", K.RS_CASES)
def test_rs_case_makes_the_soft_decoder_work_in_every_part(n):
    d = K.stage_lengths()
    nb, dl = R.rs_dims(n)
    assert (nb, dl) == {d["k"]: (294, 223), d["l0_v27"]: (588, 223)}[n]
    last_len = n - (nb - 1) * dl
    assert last_len == {d["k"]: 200, d["l0_v27"]: 179}[n] and last_len < dl       # the last block is padded: len < dl in the kernel's loop
    ref = K.rs_reference(n)
    assert ref["soft"].shape == (K.PACKETS, 8 * nb * (dl + 32)) and ref["dec"].shape == (K.PACKETS, n) and ref["f"].shape == (K.PACKETS, nb)
    for p in range(K.PACKETS):
        share, thirds = K.rs_coverage(ref["f"][p], ref["dirty"][p])
        print("n=%d packet %d: %.0f %% of the blocks with a non-zero syndrome, blocks won by f > 0 per third %s, f histogram %s" % (
            n, p, 100 * share, thirds, np.bincount(ref["f"][p] // 2, minlength=17).tolist()))
        assert share >= 0.5 and min(thirds) >= 1
        assert (ref["f"][p] != RS.NO_F).all() and (ref["f"][p][~ref["dirty"][p]] == 0).all()


# ---------------------------------------------------------------------------------------------------- negative controls
CONTROL_SISO = (R.FEC_GOLAY, K.stage_lengths()["l0_v27"])
CONTROL_RS = K.stage_lengths()["l0_v27"]
CONTROL_WRAP = (R.FEC_GOLAY, K.stage_lengths()["l0_v27"])


def test_control_siso_in_place_without_the_barrier_is_caught():
    fs, n = CONTROL_SISO
    ref = K.block_reference(fs, n)
    for p in range(K.PACKETS):
        wrong = K.siso_in_place_without_the_round_barrier(fs, ref["soft"][p], n)
        bad = np.nonzero(wrong != ref["siso"][p])[0]
        assert len(bad) > 0 and bad.max() // K.message_bits(fs) < K.LANES           # the first round's codewords, nothing later
        # in the order in which the kernel's rounds follow each other, in place is the reference
        assert (K.siso_ascending_in_place(fs, ref["soft"][p], n) == ref["siso"][p]).all()


def test_control_rs_with_a_stale_erasure_order_is_caught():
    n = CONTROL_RS
    ref = K.rs_reference(n)
    dec, f, _ = K.rs_with_the_previous_blocks_erasure_order(ref["soft"], n)
    for p in range(K.PACKETS):
        assert (dec[p] != ref["dec"][p]).any() and (f[p] != ref["f"][p]).any()
        assert f[p][0] == ref["f"][p][0]                               # (a packet's first block has no block before it)


def test_control_soft_block_with_a_16_bit_index_is_caught():
    fs, n = CONTROL_WRAP
    assert SK.ncw(fs, n) > 1 << 16
    ref = K.block_reference(fs, n)
    wrong = K.soft_block_with_a_16_bit_group_index(fs, ref["soft"], n)
    for p, lanes in enumerate(K.lanes_that_differ(fs, wrong, ref["dec"])):
        assert len(lanes) > 0 and lanes.min() >= 1 << 16, p
    # and a case below 2^16 codewords cannot tell: which is why the case above is named
    fs, n = R.FEC_GOLAY, K.stage_lengths()["k"]
    assert SK.ncw(fs, n) <= 1 << 16
    assert (K.soft_block_with_a_16_bit_group_index(fs, K.block_reference(fs, n)["soft"], n) == K.block_reference(fs, n)["dec"]).all()
