"""Bounded soft-decision Reed-Solomon decoding and its soft hand-over (fxrx_config.soft_rs_fmax, soft_rs_chain), the reference in
numpy, on top of tests/ref_rs_soft.py, whose trace (candidate, ok and cost per f) gives the bounded winner.  The rules (DESIGN.md
section 8), per block of N = dl + 32 bytes:

  fmax (even, 0 .. 32): soft_rs's rule with the trials f = 0, 2, ..., fmax only -- the winner is the least D among them, ties to the
    smallest f.  No candidate among them: the block is given up on, passed on as received (the hard bytes h), chosen f = 255.
    fmax = 32 is soft_rs's rule, fmax = 0 the bounded-distance hard decoder.
  soft hand-over (fec1 Reed-Solomon, fec0 convolutional): with len the data bytes the block really carries, the stage emits 8 len
    values, MSB first, in byte order: a block with a winner c emits c_bit ? 255 : 0 for its data bits, a block given up on its
    channel values s unchanged; parity and pad positions are not emitted.  The 8 l0 values pass the soft de-interleaver and the
    soft-input Viterbi decoder, as behind FEC_NONE."""
import numpy as np

import ref_decode as rd
import ref_rs_soft as rs

NO_F = rs.NO_F


def bounded_from_trace(tr, fmax):
    """the bounded winner from ref_rs_soft's trace: (blocks (B, N), chosen (B,), 255 = none)"""
    assert fmax % 2 == 0 and 0 <= fmax <= 32
    h = tr["hard"]
    best, chosen = h.copy(), np.full(len(h), NO_F, np.int64)
    best_cost = np.full(len(h), np.iinfo(np.int64).max)
    for i, f in enumerate(rs.F_LIST):
        if f > fmax:
            break
        better = tr["ok"][i] & (tr["cost"][i] < best_cost)
        best[better], best_cost[better], chosen[better] = tr["cand"][i][better], tr["cost"][i][better], f
    return best, chosen.astype(np.uint8)


def rs_blocks_bounded(soft, fmax, trace=None):
    """soft (B, 8 N) -> (blocks (B, N) after decoding under the bound, chosen f (B,), 255 for a block given up on)"""
    tr = {} if trace is None else trace
    if "cand" not in tr:
        rs.rs_decode_soft_blocks(soft, tr)
    return bounded_from_trace(tr, fmax)


def blocks_soft_out(soft, blocks, chosen):
    """the soft form of whole blocks: (B, 8 N): 0 / 255 of the winner, or the block's own values where there is none"""
    soft = np.asarray(soft, np.uint8)
    hardened = (np.unpackbits(np.asarray(blocks, np.uint8), axis=-1) * 255).astype(np.uint8)
    return np.where((np.asarray(chosen) == NO_F)[:, None], soft, hardened)


def _cut(per_block, n, unit):
    """(nb, >= unit dl) per-block rows -> the packet's first unit n entries: data positions only, no pad"""
    nb, dl = rd.rs_dims(n)
    return per_block[:, :unit * dl].reshape(-1)[:unit * n].copy()


def rs_stage_hard_out(soft, n, fmax, chosen=None):
    """one packet: 8 fec_enc_len(RS, n) soft values (codeword order) -> n message bytes under the bound"""
    nb, dl = rd.rs_dims(n)
    blocks, f = rs_blocks_bounded(np.asarray(soft, np.uint8)[:8 * nb * (dl + 32)].reshape(nb, 8 * (dl + 32)), fmax)
    if chosen is not None:
        chosen.extend(int(x) for x in f)
    return _cut(blocks, n, 1)


def rs_stage_soft_out(soft, n, fmax, chosen=None):
    """one packet: 8 fec_enc_len(RS, n) soft values (codeword order) -> 8 n soft values by the hand-over rule"""
    nb, dl = rd.rs_dims(n)
    s = np.asarray(soft, np.uint8)[:8 * nb * (dl + 32)].reshape(nb, 8 * (dl + 32))
    blocks, f = rs_blocks_bounded(s, fmax)
    if chosen is not None:
        chosen.extend(int(x) for x in f)
    return _cut(blocks_soft_out(s, blocks, f), n, 8)


def chain_acts(fec0, fec1, chain):
    return bool(chain) and fec1 == rd.FEC_RS and fec0 in rd.CONV


def packet_decode_rs_chain(soft, n, check, fec0, fec1, fmax=32, chain=False):
    """ref_rs_soft.packet_decode_soft_rs under the bound fmax and, where fec1 is Reed-Solomon and fec0 convolutional, with the soft
    hand-over.  Where the options do not act this is packet_decode_soft_rs / ref_decode.packet_decode_soft."""
    k, l0, l1 = rd.packet_dims(n, check, fec0, fec1)
    rs_stage = fec1 == rd.FEC_RS or (fec1 == rd.FEC_NONE and fec0 == rd.FEC_RS)
    if not rs_stage:
        return rd.packet_decode_soft(soft, n, check, fec0, fec1)
    if fmax == 32 and not chain_acts(fec0, fec1, chain):
        return rs.packet_decode_soft_rs(soft, n, check, fec0, fec1)
    v = rd.interleave_soft(np.asarray(soft, np.uint8)[:8 * l1], l1, decode=True)
    if fec1 == rd.FEC_NONE:
        b0 = rs_stage_hard_out(rd.interleave_soft(v, l0, decode=True), k, fmax)
    elif chain_acts(fec0, fec1, chain):
        v0 = rd.interleave_soft(rs_stage_soft_out(v, l0, fmax), l0, decode=True)
        b0 = rd.viterbi(fec0, v0[None], k, 255)[0][0]
    else:
        b0 = rd.fec_decode(fec0, rd.interleave(rs_stage_hard_out(v, l0, fmax), decode=True), k)
    return rd._finish(b0, n, check)
