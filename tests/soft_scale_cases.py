"""Inputs of the soft payload decoders at the sizes of a full-length frame (tests/test_soft_scale.py, tests/test_gpu_soft_scale.py):
seeded packets of soft values in codeword bit order whose lengths are a stage's sizes for a 65535-byte payload with CRC-32, taken
from ref_decode.packet_dims; the references of tests/ref_block_soft.py, ref_block_siso.py and ref_rs_soft.py on them, computed once;
and three wrong decoders, small wrappers round the references, that the cases must tell from the right ones.

A case is (code, n): n message bytes of the stage.  Per soft-block code (ref_block_soft.SOFT_BLOCK) the lengths are
  k         the packet and its CRC: the stage behind no inner code;
  l0 / V27  fec0's output behind the rate-1/2 code;
  l0 / P78  behind the most punctured convolutional code of the menu;
  short     the largest n below l0 / V27 that ends short: Golay -- a last codeword with four message bits; SECDED -- a last block of
            one data byte.  Hamming codewords are never short (4 or 8 message bits each): their fourth length is the largest one
            below l0 / V27 that leaves the last round of 64 lanes partial.
Reed-Solomon: n = k (294 blocks of 255) and n = l0 / V27 (588 blocks); the last block of either carries fewer message bytes than dl.

Two packets per case, so that the second packet's offset into the input and output arrays is exercised: packet 0 is uniform noise,
packet 1 noise around a codeword near the decoders' limit (siso_cases' kinds 3 and 4, the latter louder; Reed-Solomon: rs_soft_cases' Gaussian noise
at SIGMA[255], packet 0 with every seventh block uniform noise).  No case's reference takes 20 s here, so no case was halved.

The kernels work in rounds of 64 lanes, one codeword (SECDED: block) a lane; `rounds` below speaks of those."""
import functools

import numpy as np

import ref_decode as R
import ref_block_soft as B
import ref_block_siso as S
import ref_rs_soft as RS
import rs_soft_cases as RK
import siso_cases as SK

PAYLOAD = 65535
CHECK = R.CRC_32
PACKETS = 2
LANES = 64
MOST_PUNCTURED = min(R.CONV, key=lambda f: R.fec_enc_len(f, PAYLOAD + R.crc_len(CHECK)))


@functools.lru_cache(None)
def stage_lengths():
    """{'k', 'l0_v27', 'l0_punct'}: a stage's message bytes for the full-length payload"""
    k, l0, _ = R.packet_dims(PAYLOAD, CHECK, R.FEC_V27, R.FEC_NONE)
    return dict(k=k, l0_v27=l0, l0_punct=R.packet_dims(PAYLOAD, CHECK, MOST_PUNCTURED, R.FEC_NONE)[1])


def message_bits(fs):
    """message bits of one lane's work: a codeword, or a whole SECDED block"""
    return 8 * R.SECDED[fs][0] if fs in R.SECDED else R.code_table(fs)[0]


def ends_short(fs, n):
    if fs == R.FEC_GOLAY:
        return 8 * n % 12 == 4
    if fs in R.SECDED:
        return n % R.SECDED[fs][0] == 1
    return SK.ncw(fs, n) % LANES != 0


@functools.lru_cache(None)
def short_length(fs):
    n = stage_lengths()["l0_v27"] - 1
    while not ends_short(fs, n):
        n -= 1
    return n


def block_lengths(fs):
    d = stage_lengths()
    return (d["k"], d["l0_v27"], d["l0_punct"], short_length(fs))


BLOCK_CASES = tuple((fs, n) for fs in B.SOFT_BLOCK for n in block_lengths(fs))
RS_CASES = (stage_lengths()["k"], stage_lengths()["l0_v27"])


def case_id(c):
    return "fec%d_n%d" % c


def rounds_of(fs, n):
    return -(-SK.ncw(fs, n) // LANES)


# ---------------------------------------------------------------------------------------------------- packets
def lane_width(fs):
    """soft values of one lane's work: a codeword, or a whole SECDED block (parity byte and data)"""
    return 8 * (R.SECDED[fs][0] + 1) if fs in R.SECDED else R.code_table(fs)[1]


def from_round(fs, soft, n, r):
    """the packets from round r on, as packets of their own: (soft values, message bytes)"""
    g = r * LANES
    return np.asarray(soft)[:, g * lane_width(fs):], n - g * message_bits(fs) // 8


def hard_decode(fs, soft, n):
    """the hard decoder on the hard word of the soft values: (P, n) bytes.  Golay by ref_block_soft.golay_hard (its syndrome table;
    ref_decode.fec_decode's search over all codewords, the same rule, takes ten seconds a packet at this length)"""
    if fs != R.FEC_GOLAY:
        return B.block_decode_hard(fs, hard_input(soft), n)
    k, w, nb, _ = R._packed_dims(fs, n)
    y = (np.asarray(soft)[:, :nb * w] > 127).astype(np.uint8)
    d = B.golay_hard(y.reshape(-1, w))[0]
    return np.packbits(R.bits_of_words(d, k).reshape(len(y), nb * k)[:, :8 * n], axis=1)


def _edge_rounds_differ(fs, soft, n):
    """whether, in every packet, soft and hard decoding differ in a codeword of the first round and in one of the last"""
    first = min(n, LANES * message_bits(fs) // 8)
    last_soft, last_n = from_round(fs, soft, n, rounds_of(fs, n) - 1)
    for sv, m in ((soft, first), (last_soft, last_n)):
        if not all(len(l) for l in lanes_that_differ(fs, B.block_decode_soft(fs, sv, m), hard_decode(fs, sv, m))):
            return False
    return True


NOISE = 180                                    # packet 1: a codeword's 0 / 255 plus uniform noise of this amplitude: 15 % of the hard bits wrong


def block_packets(fs, n):
    """(PACKETS, 8 fec_enc_len(fs, n)) soft values: packet 0 uniform noise, packet 1 noise around a codeword.  The last round of a
    case may hold one codeword only, so the seed is the first of the case's series with which the coverage conditions of
    tests/test_soft_scale.py hold in the first and the last round (looked at on those two rounds alone; the test asserts all)"""
    msg = np.random.RandomState(31000 + 97 * fs + n % 1009).randint(0, 256, n).astype(np.uint8)
    bits = np.unpackbits(R.fec_encode(fs, msg)).astype(np.int64)
    for attempt in range(64):
        rng = np.random.RandomState(32000 + 97 * fs + n % 1009 + 7919 * attempt)
        unif = rng.randint(0, 256, bits.shape)
        near = np.clip(bits * 255 + rng.randint(-NOISE, NOISE + 1, bits.shape), 0, 255)
        soft = np.ascontiguousarray(np.stack([unif, near]).astype(np.uint8))
        if _edge_rounds_differ(fs, soft, n):
            return soft
    raise AssertionError("no seed for %s" % case_id((fs, n)))


def rs_packets(n):
    """(PACKETS, 8 fec_enc_len(RS, n)) soft values at the noise of rs_soft_cases.SIGMA; every seventh block of packet 0 is uniform noise"""
    nb, dl = R.rs_dims(n)
    soft = RK.noisy_packets(n, PACKETS, 52000 + n % 1009)[1].copy()
    rng = np.random.RandomState(53000 + n % 1009)
    blocks = soft[0].reshape(nb, 8 * (dl + 32))
    blocks[3::7] = rng.randint(0, 256, blocks[3::7].shape)
    return np.ascontiguousarray(soft)


# ---------------------------------------------------------------------------------------------------- references, once per case
def _frozen(**kw):
    for v in kw.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return kw


def hard_input(soft):
    """the hard word of soft values, as coded bytes"""
    return np.packbits((np.asarray(soft) > 127).astype(np.uint8), axis=-1)


@functools.lru_cache(None)
def block_reference(fs, n):
    """dict: soft (the packets), dec (PACKETS, n) of ref_block_soft, hard (PACKETS, n) of ref_decode's hard decoder on the hard word,
    siso (PACKETS, 8 n) of ref_block_siso"""
    soft = block_packets(fs, n)
    return _frozen(soft=soft, dec=B.block_decode_soft(fs, soft, n), hard=hard_decode(fs, soft, n),
                   siso=S.block_decode_siso(fs, soft, n))


@functools.lru_cache(None)
def rs_reference(n):
    """dict: soft, dec (PACKETS, n), f (PACKETS, nb) the chosen f, dirty (PACKETS, nb) blocks whose hard word is no codeword"""
    nb, dl = R.rs_dims(n)
    soft = rs_packets(n)
    dec, f, dirty = rs_decode_packets(soft, n)
    return _frozen(soft=soft, dec=dec, f=f, dirty=dirty)


def rs_decode_packets(soft, n, order_of=None):
    """ref_rs_soft on packets of n message bytes: (dec (P, n), chosen f (P, nb), dirty (P, nb)).  order_of: a wrong decoder's
    erasure order, a function of the true one (P nb, N)"""
    nb, dl = R.rs_dims(n)
    soft = np.asarray(soft, np.uint8)
    v = soft[:, :8 * nb * (dl + 32)].reshape(-1, 8 * (dl + 32))
    blocks, f = RS.rs_decode_soft_blocks(v) if order_of is None else _rs_with_order(v, order_of(RS.erasure_order(v)))
    dec = blocks[:, :dl].reshape(len(soft), nb * dl)[:, :n].copy()
    dirty = R.rs_syndromes(RS.hard_bytes(v)).any(axis=1)
    return dec, f.reshape(len(soft), nb).copy(), dirty.reshape(len(soft), nb)


# ---------------------------------------------------------------------------------------------------- coverage
def lanes_that_differ(fs, a, b):
    """per packet, the indices of the codewords (SECDED: blocks) on whose message bits the decoded bytes a and b differ"""
    diff = np.unpackbits(np.asarray(a, np.uint8) ^ np.asarray(b, np.uint8), axis=-1)
    return [np.unique(np.nonzero(d)[0] // message_bits(fs)) for d in diff.reshape(-1, diff.shape[-1])]


def round_coverage(fs, n, lanes):
    """of codeword indices: (in the first round, in the last round, in a round beyond the one that holds the 129th codeword and
    before the last) -- counts"""
    r = np.asarray(lanes) // LANES
    last = rounds_of(fs, n) - 1
    return int((r == 0).sum()), int((r == last).sum()), int(((r > 128 // LANES) & (r < last)).sum())


def rs_coverage(f, dirty):
    """one packet's chosen f and dirty flags (nb,): (share of blocks with a non-zero syndrome, blocks won by f > 0 in each third)"""
    nb = len(f)
    third = np.arange(nb) * 3 // nb
    return float(np.mean(dirty)), tuple(int(((f > 0) & (third == t)).sum()) for t in range(3))


# ---------------------------------------------------------------------------------------------------- wrong decoders
def siso_in_place_without_the_round_barrier(fs, soft, n):
    """block_decode_siso in place, S -> S, as a kernel without the barrier between a round's reads and its writes could run it:
    the lanes of a round one after the other, the highest first, each writing its message over the arena before the next lane
    reads its codeword.  Message g lies where codeword g / 2 (rate-1/2 codes) was: in the first round that lane has not read yet.
    (In ascending order nothing goes wrong: message g ends where codeword g + 1 begins or before -- ascending_in_place.)"""
    return _siso_in_place(fs, soft, n, descending=True)


def siso_ascending_in_place(fs, soft, n):
    """the same in place, every lane after the one before it: the order in which the kernel's rounds follow each other"""
    return _siso_in_place(fs, soft, n, descending=False)


def _siso_in_place(fs, soft, n, descending):
    assert fs in (R.FEC_H84, R.FEC_H128, R.FEC_GOLAY)          # (whole words per codeword: enough for a control)
    k, w, _ = R.code_table(fs)
    ncw = SK.ncw(fs, n)
    arena = np.zeros(max(ncw * w, 8 * R.fec_enc_len(fs, n)), np.uint8)
    arena[:8 * R.fec_enc_len(fs, n)] = np.asarray(soft, np.uint8)[:8 * R.fec_enc_len(fs, n)]
    one = (lambda s: S.golay_siso(s)) if fs == R.FEC_GOLAY else (lambda s: S.ml_siso(fs, s))
    r0 = 0
    while r0 < ncw and k * (r0 + LANES) > w * r0:              # rounds whose messages land on codewords of the same round
        lanes = range(r0, min(r0 + LANES, ncw))
        for g in (reversed(lanes) if descending else lanes):
            arena[k * g:k * g + k] = one(arena[w * g:w * g + w][None])[0]
        r0 += LANES
    if r0 < ncw:                                               # the rest: no lane's message reaches a codeword of its round or a later one
        arena[k * r0:k * ncw] = one(arena[w * r0:w * ncw].reshape(-1, w).copy()).ravel()
    return arena[:8 * n].copy()


def rs_with_the_previous_blocks_erasure_order(soft, n):
    """rs_decode_packets with a stale `era`: block b erases the positions block b - 1 chose (a packet's first block: its own)"""
    nb = R.rs_dims(n)[0]

    def stale(order):
        out = np.roll(order, 1, axis=0)
        out[::nb] = order[::nb]
        return out
    return rs_decode_packets(soft, n, stale)


def _rs_with_order(v, order):
    """ref_rs_soft.rs_decode_soft_blocks with the erasure order given"""
    h = RS.hard_bytes(v)
    best, best_cost = h.copy(), np.full(len(h), np.iinfo(np.int64).max)
    chosen = np.full(len(h), RS.NO_F, np.int64)
    for f in RS.F_LIST:
        c, ok = RS.rs_decode_erasures_batch(h, order[:, :f])
        d = RS.cost(v, c, h)
        better = ok & (d < best_cost)
        best[better], best_cost[better], chosen[better] = c[better], d[better], f
    return best, chosen.astype(np.uint8)


def soft_block_with_a_16_bit_group_index(fs, soft, n):
    """block_decode_soft whose codeword index wraps at 2^16: codeword g is decoded from the soft values of codeword g mod 65536"""
    assert fs in (R.FEC_H84, R.FEC_H128, R.FEC_GOLAY)
    w, ncw = R.code_table(fs)[1], SK.ncw(fs, n)
    soft = np.array(soft, np.uint8)
    words = soft[:, :ncw * w].reshape(len(soft), ncw, w)
    soft[:, :ncw * w] = words[:, np.arange(ncw) & 0xffff].reshape(len(soft), ncw * w)
    return B.block_decode_soft(fs, soft, n)
