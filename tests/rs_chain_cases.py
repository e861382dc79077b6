"""Crafted Reed-Solomon blocks and packets for the bound on f and the soft hand-over (fxrx_config.soft_rs_fmax, soft_rs_chain; the rules:
tests/ref_rs_chain.py), each named for what it is, and seeded noisy packets.  Built from rs_soft_cases' builders.

A block case is a dict: name, N, soft (8 N values), sent, fmax (the bound under which the name holds) and what holds there:
  chosen      the bounded winner's f (255: given up on);
  unbounded   'sent' where the unbounded rule (fmax = 32) returns the sent codeword although the bounded one gives up or differs,
              'other' where it "corrects" the block to another codeword.
A packet case is a dict: name, n, soft (8 fec_enc_len(RS, n) values), fmax, chosen (one per block).

Sizes: rs_soft_cases.SIZES -- 1, 223, 224 and 446 message bytes: N = 33, N = 255, 2 x 144, 2 x 255 -- and 225: 2 x 145, whose last block
carries 112 data bytes and one pad byte.  (None of the four sizes above has a pad: 224 = 2 x 112 and 446 = 2 x 223.  225 is the
smallest two-block size with one.)

Noisy packets: rs_soft_cases' noise levels (N = 145 takes N = 144's), at which the hard decoder finds about half of the blocks.
Shares at fmax = 16 over the noisy blocks of packet_set(n), by the reference (test_rs_chain.py asserts at least 10 % each):
  n = 1    accepted 0.73  given up 0.27        n = 223  accepted 0.30  given up 0.70
  n = 224  accepted 0.26  given up 0.74        n = 225  accepted 0.20  given up 0.80
  n = 446  accepted 0.28  given up 0.72"""
import functools

import numpy as np

import ref_decode as rd
import ref_rs_chain as rc
import ref_rs_soft as rs
import rs_soft_cases as K

SIZES = K.SIZES + (225,)
FMAX = (0, 2, 16, 30, 32)
COUNT = {1: 300, 223: 120, 224: 80, 225: 80, 446: 60}      # noisy packets per size: 740 blocks in all
SIGMA = {**K.SIGMA, 145: K.SIGMA[144]}


def block_lengths():
    return sorted({rd.rs_dims(n)[1] + 32 for n in SIZES})


def _bounded(base, name, fmax, chosen, **kw):
    return dict(name="%s_N%d" % (name, base["N"]), N=base["N"], soft=base["soft"], sent=base["sent"], fmax=fmax, chosen=chosen, **kw)


@functools.lru_cache(None)
def block_cases():
    """errors_and_weak(e, w): e strong and w weak wrong bytes, the weak ones the least reliable: the sent codeword is first reached at
    f = 2 (e + w) - 32 (w >= that f), and every larger f ties with it."""
    rng = np.random.RandomState(3255)
    out = []
    for N in block_lengths():
        for e, w, f in ((15, 2, 2), (8, 16, 16), (1, 30, 30)):
            out.append(_bounded(K.errors_and_weak(rng, N, e, w), "won_at_f_equal_fmax_%d" % f, f, f))
        out.append(_bounded(K.errors_and_weak(rng, N, 8, 16), "only_candidates_above_fmax_2_first_at_16_given_up", 2, 255, unbounded="sent"))
        # (N = 33 has one data byte and 256 codewords: with 31 of 33 bytes wrong the unbounded winner is a cheaper codeword than the sent one)
        out.append(_bounded(K.errors_and_weak(rng, N, 1, 30), "only_candidates_above_fmax_16_first_at_30_given_up", 16, 255, unbounded="sent" if N > 33 else "other"))
        # hard decoder: the near codeword B; f = 4 reaches the sent one at less cost
        tc = K.two_codewords(rng, N, False)
        out.append(_bounded(tc, "candidate_at_f_0_cheaper_one_above_fmax_2", 2, 0, unbounded="sent", other=tc["other"]))
        far = K.far_word(rng, N)
        for f in (0, 16, 30):
            out.append(_bounded(far, "word_far_from_every_codeword_fmax_%d" % f, f, None, far=True))
        # every soft value 127 / 128, 20 wrong bytes, first reached at f = 8: given up on at fmax = 2, values far from 0 / 255
        out.append(_bounded(K.equal_reliabilities(rng, N, True), "given_up_every_soft_value_127_or_128", 2, 255, unbounded="sent", mid=True))
        out.append(_bounded(K.clean(rng, N), "codeword_as_received_is_its_own_f_0_candidate", 0, 0))
    return tuple(out)


def of_length(N):
    return [c for c in block_cases() if c["N"] == N]


@functools.lru_cache(None)
def block_reference():
    """per block length: ref_rs_soft's trace on that length's cases, computed once"""
    out = {}
    for N in block_lengths():
        tr = {}
        rs.rs_decode_soft_blocks(np.stack([c["soft"] for c in of_length(N)]), tr)
        out[N] = tr
    return out


def block_result(c, fmax=None):
    """(block, chosen, soft form of the block, cand, ok, cost) of case c under fmax (default: its own)"""
    tr = block_reference()[c["N"]]
    i = [x["name"] for x in of_length(c["N"])].index(c["name"])
    blocks, chosen = rc.bounded_from_trace(tr, c["fmax"] if fmax is None else fmax)
    so = rc.blocks_soft_out(c["soft"][None], blocks[i:i + 1], chosen[i:i + 1])[0]
    return blocks[i], int(chosen[i]), so, tr["cand"][:, i], tr["ok"][:, i], tr["cost"][:, i]


# ---------------------------------------------------------------------------------------------------- packets
def _by_name(N, start):
    return next(c for c in of_length(N) if c["name"].startswith(start))


@functools.lru_cache(None)
def packet_cases(n):
    """named packets of n message bytes (two-block sizes): one block accepted and one given up on, in both orders, at fmax = 16"""
    nb, dl = rd.rs_dims(n)
    if nb != 2:
        return ()
    N = dl + 32
    good, far, mid = _by_name(N, "codeword_as_received"), _by_name(N, "word_far_from_every_codeword_fmax_16"), _by_name(N, "won_at_f_equal_fmax_16")
    pad = "_padded_last_block" if nb * dl != n else ""
    return (dict(name="accepted_then_given_up%s_n%d" % (pad, n), n=n, soft=np.concatenate([good["soft"], far["soft"]]), fmax=16, chosen=(0, 255)),
            dict(name="given_up_then_accepted%s_n%d" % (pad, n), n=n, soft=np.concatenate([far["soft"], good["soft"]]), fmax=16, chosen=(255, 0)),
            dict(name="accepted_at_f_16_then_given_up%s_n%d" % (pad, n), n=n, soft=np.concatenate([mid["soft"], far["soft"]]), fmax=16, chosen=(16, 255)))


def all_packet_cases():
    return [p for n in SIZES for p in packet_cases(n)]


def noisy_packets(n, count, seed):
    """rs_soft_cases.noisy_packets with N = 145 added: (messages (count, n), soft (count, 8 fec_enc_len))"""
    rng = np.random.RandomState(seed)
    nb, dl = rd.rs_dims(n)
    msg = rng.randint(0, 256, (count, n)).astype(np.uint8)
    enc = np.stack([rd.fec_encode(rd.FEC_RS, m) for m in msg])
    bits = np.unpackbits(enc, axis=1).astype(np.float64)
    sigma = np.asarray(SIGMA[dl + 32])[rng.randint(0, len(SIGMA[dl + 32]), (count, 1))]
    y = (2.0 * bits - 1.0) + sigma * rng.standard_normal(bits.shape)
    return msg, np.clip(np.round(127.5 + 100.0 * y), 0, 255).astype(np.uint8)


def case_packets(n):
    """the named packets, then the crafted blocks of the packet's block length as packets: every block of a packet a case, in rotation"""
    nb, dl = rd.rs_dims(n)
    cs = of_length(dl + 32)
    rot = [np.concatenate([cs[(i + b) % len(cs)]["soft"] for b in range(nb)]) for i in range(len(cs))]
    return np.stack([p["soft"] for p in packet_cases(n)] + rot)


@functools.lru_cache(None)
def packet_set(n):
    """(soft (P, 8 fec_enc_len), trace of ref_rs_soft over its P nb blocks, number of crafted packets): the crafted packets of size n
    followed by COUNT[n] noisy ones; the reference's 17 trials run once, every fmax is read from their trace"""
    nb, dl = rd.rs_dims(n)
    crafted = case_packets(n)
    soft = np.ascontiguousarray(np.concatenate([crafted, noisy_packets(n, COUNT[n], 5100 + n)[1]]))
    tr = {}
    rs.rs_decode_soft_blocks(soft.reshape(-1, 8 * (dl + 32)), tr)
    soft.setflags(write=False)
    return soft, tr, len(crafted)


@functools.lru_cache(None)
def packet_reference(n, fmax):
    """(hard output (P, n), soft output (P, 8 n), chosen f (P, nb)) of packet_set(n) under fmax, by the reference"""
    nb, dl = rd.rs_dims(n)
    soft, tr, _ = packet_set(n)
    blocks, chosen = rc.bounded_from_trace(tr, fmax)
    P = len(soft)
    hard = blocks[:, :dl].reshape(P, nb * dl)[:, :n].copy()
    so = rc.blocks_soft_out(soft.reshape(-1, 8 * (dl + 32)), blocks, chosen)[:, :8 * dl].reshape(P, 8 * nb * dl)[:, :8 * n].copy()
    chosen = chosen.reshape(P, nb)
    for a in (hard, so, chosen):
        a.setflags(write=False)
    return hard, so, chosen


def noisy_shares(n, fmax=16):
    """(accepted, given up) shares of the noisy blocks of packet_set(n) under fmax"""
    nb = rd.rs_dims(n)[0]
    chosen = packet_reference(n, fmax)[2][packet_set(n)[2]:]
    return float((chosen != rc.NO_F).mean()), float((chosen == rc.NO_F).mean())
