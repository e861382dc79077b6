"""Crafted received words for the payload decoders: one list of named cases, each a noise-free frame whose payload symbols
carry a coded packet corrupted on purpose.  tests/test_ref_crafted.py proves (no GPU) that each case is what its name says and
that the numpy reference and the oracle agree on it; tests/test_gpu_crafted_decode.py puts the same frames in front of every
Viterbi and Reed-Solomon implementation of the library, through the whole receive path.

A case is (name, mod, fec0, fec1, check, n, pkt): the header states (n, mod, check, fec0, fec1) and the payload symbols are the
labels of pkt, the l1 channel bytes.  pkt is built from the word the decoder under test is to receive:
    inner word r0 (l0 bytes, what fec0's decoder reads)   pkt = interleave(fec_encode(fec1, interleave(r0)))   (fec1 clean)
    outer word r1 (l1 bytes, what fec1's decoder reads)   pkt = interleave(r1)
so that the receive side's de-interleavers (and a clean outer decoder) hand the decoder exactly r0 / r1.  k = n + crc bytes is
the inner message (scrambled payload + CRC), Tn = 8 k + 6 the trellis steps of a convolutional fec0.

Families and frames (FAMILY_COUNTS, asserted in test_ref_crafted.py):
    single    507   one flipped coded bit at every position of the first two and the last two puncturing periods -- the last
                    max(2 P, 6) steps, so all six flush steps, and the pad bits behind the last coded bit; k = 1, 2, 16; 7 rates
    burst     252   runs of 1 .. 12 flipped bits at the start, the middle and the end of the word; k = 32; 7 rates
    tie       226   message m and a neighbour m' = m ^ e (e a low-weight difference of at most 8 bits, found by search with
                    the reference encoder: the smallest EVEN codeword distance at that puncturing phase); every second one of the
                    differing coded bits is flipped, so both codewords are d / 2 from the received word.  Divergence at step
                    t in {0, B-65, B-64, B-1, B, B+1, B+63, B+64, B+96, B+128, last message step with an even distance} for
                    B = 128 and 192 (the trellis block edge, the warm-ups of 64 / 96 / 128 steps, the traceback warm-up of 64);
                    k = 48 and 49 (390 and 398 steps); and per rate and k two ties in neighbouring blocks.  At rate 1/2 d = 10
                    is the code's free distance and the tied pair is maximum-likelihood; of the punctured codes' ties most are.
    tail       63   per rate and k = 2, 16, 33 (or the next k whose last byte has pad bits): the code sequence of a message
                    whose six tail bits are not zero; a clean codeword with every pad bit set; a clean codeword with an error in the last transmitted coded bit
    garbage    56   all-zero word, all-one word, the complement of a codeword, and the worst-spread pattern (below) repeated;
                    k = 1100 (8806 steps: FXRX_VB_BLK=4096 makes blocks of 4096 steps plus warm-up) and k = 48; 7 rates
    short      42   k = 0 (check none, n = 0: the six flush steps alone), 1 and 2, clean and with one error; 7 rates
    outer     252   tie words (t = 0, 63, 127, 128, 129, 191, 192, 256) and burst words (start, middle, end) at k = 48 inside
                    fec1 = Golay(24,12) and SECDED(72,64) (batch path) and Reed-Solomon (not); 7 rates
    rs        168   Reed-Solomon as fec0 (k = 1, 222, 223, 224, 446, 447) and as fec1 over V27 (the RS message is V27's 2 k + 2
                    bytes, always even: 2, 222, 224, 446), in both roles: 0, 1, 8, 15, 16, 17 errors per block; in the data
                    only, in the 32 parity bytes only, spread with the first and the last transmitted byte among them (a lone
                    error at either); error values 0x01 and 0xFF; all-zero blocks (1, 2 or 3 of them); another codeword c' plus
                    15 errors ("17 errors that are 15 from another codeword"); one block beyond repair between clean ones

Carriers: PSK4 and QAM16 in turns, PSK2 for every 9th convolutional case.  All three meet the condition of test_ref_crafted.py
(the oracle receiver finds every frame, accepts every header and demaps exactly the crafted word); none had to be removed.

Worst spread max(pm) - min(pm) of the reference's path metrics in ref_decode.viterbi (hard decisions, cost 1 per differing
bit, start in state 0), searched over all 2^16 patterns of 16 coded bits, repeated (spread_search, re-derived by
test_ref_crafted.py against SPREAD): "held" at steps 32 and later, when the start state is forgotten, "start" at steps 6 and
later (the largest values sit at step 6: states the start state reaches only through six ones).
    rate    1/2  2/3  3/4  4/5  5/6  6/7  7/8
    held      8    5    4    4    4    4    4
    start     9    7    6    6    6    6    5
The all-zero and the all-one word are among the patterns that hold the largest spread; the garbage family's "spread" word is the
first pattern with both bit values that holds it too.  A K = 7 trellis reaches every state from every state in six steps of
at most two bits each, so 12 bounds every spread.  The batch kernels keep doubled metrics (18 at most here, 24 by the bound)
and state "metric differences stay below 256" (fx_kernels.hip, above vb2_butterfly; vb_save_vec clamps at 255): the
measured spreads are more than ten times below the stated bound.  No finding.

Everything here is deterministic (seeded) and computed once per process; the arrays handed out must not be modified."""
import functools

import numpy as np

import ref_decode as R
import ref_framegen as G

GAP = 300                                   # silent samples between frames (at least)
GAPS = (300, 301, 303, 300, 305, 302, 311)  # odd and even offsets, as framegen_cases.layout
LEAD = 333
BLOCKS = (128, 192)                         # trellis block lengths the tie positions are placed against (FXRX_VB_BLK=128, the default 192)
TIE_K = (48, 49)
BATCH_FEC1 = (R.FEC_NONE,) + R.BLOCK        # outer codes that keep a convolutional fec0 on the batch path
CHECKS = (R.CRC_NONE, R.CRC_CHECKSUM, R.CRC_8, R.CRC_16, R.CRC_24, R.CRC_32)
RATE = {R.FEC_V27: "1/2", R.FEC_V27P23: "2/3", R.FEC_V27P34: "3/4", R.FEC_V27P45: "4/5", R.FEC_V27P56: "5/6", R.FEC_V27P67: "6/7",
        R.FEC_V27P78: "7/8"}
# per rate: (the first pattern with both bit values that holds the largest spread, held, start), see spread_search()
SPREAD = {R.FEC_V27: (0x013e, 8, 9), R.FEC_V27P23: (0x000b, 5, 7), R.FEC_V27P34: (0x0003, 4, 6), R.FEC_V27P45: (0x0001, 4, 6),
          R.FEC_V27P56: (0x0003, 4, 6), R.FEC_V27P67: (0x0003, 4, 6), R.FEC_V27P78: (0x0003, 4, 5)}
SPREAD_BOUND = 12                           # six steps of at most two coded bits
KERNEL_BOUND_DOUBLED = 256                  # "metric differences stay below 256", in the kernels' doubled units
FAMILY_COUNTS = dict(single=507, burst=252, tie=226, tail=63, garbage=56, short=42, outer=252, rs=168)


def period(fs):
    return len(R.PUNCTURE[fs][0])


def steps_of(k):
    return 8 * k + 6


def coded_bits(fs, k):
    """coded bits of a k-byte message (without the pad bits of the last byte)"""
    return int(R._conv_mask(fs, steps_of(k)).sum())


def bits_before(fs, t):
    """coded bits before trellis step t"""
    return int(R._conv_mask(fs, t).sum()) if t > 0 else 0


def pick_check(k, i):
    """a check whose key fits into k bytes, in turns"""
    fits = [c for c in CHECKS if R.crc_len(c) <= k]
    return fits[i % len(fits)]


def inner_message(payload, check):
    """the k bytes fec0 encodes: payload and key, scrambled"""
    payload = np.asarray(payload, np.uint8)
    cl, key = R.crc_len(check), R.crc_key(check, payload)
    return R.scramble(np.concatenate([payload, np.array([(key >> (8 * (cl - 1 - i))) & 0xff for i in range(cl)], np.uint8)]))


def channel_from_inner(r0, fec1):
    return R.interleave(R.fec_encode(fec1, R.interleave(np.asarray(r0, np.uint8))))


def channel_from_outer(r1):
    return R.interleave(np.asarray(r1, np.uint8))


def flip_bits(word, positions):
    b = R.bits_of(word)
    b[np.asarray(list(positions), np.int64)] ^= 1
    return np.packbits(b)


def code_sequence(fs, bits):
    """coded bits of an arbitrary input bit sequence, one trellis step per bit, no tail appended (the encoder's definition
    again: ref_decode.conv_encode_bits appends six zeros to whole bytes)"""
    u = np.asarray(bits, np.uint8)
    n = len(u)
    up = np.concatenate([np.zeros(6, np.uint8), u])
    out = np.zeros((n, 2), np.uint8)
    for g, poly in enumerate(R.CONV_POLYS):
        for j in range(7):
            if poly >> j & 1:
                out[:, g] ^= up[6 - j:6 - j + n]
    return out[R._conv_mask(fs, n)]


# ---------------------------------------------------------------------------------------------------- spread search
def spread_search(fs, steps=112):
    """Over all 2^16 patterns of 16 coded bits, repeated: the largest max(pm) - min(pm) that the reference's add-compare-select
    (ref_decode.viterbi's costs, predecessors and start state) reaches at steps 6 .. `steps` - 1.  112 steps hold every
    rate's joint period of pattern and puncturing (8, 32, 12, 64, 40, 96, 14 steps) at least once behind the first six.
    Returns (pattern, held, held_any, start): the first pattern with both bit values whose spread at steps 32 and later is the
    largest of such patterns, that spread, the largest spread at steps 32 and later of any pattern, the largest at steps 6
    and later of any pattern."""
    pats = np.arange(1 << 16, dtype=np.int64)
    mask = R._conv_mask(fs, steps)
    pm = np.full((1 << 16, 64), 1000, np.int16)            # ref_decode.viterbi's start: state 0 (the others out of reach)
    pm[:, 0] = 0
    worst, held = np.zeros(1 << 16, np.int16), np.zeros(1 << 16, np.int16)
    pos = 0
    for t in range(steps):
        c0 = np.zeros((1 << 16, 2), np.int16)               # cost of expecting 0 at A / B
        for g in range(2):
            if mask[t, g]:
                c0[:, g] = (pats >> (15 - pos % 16)) & 1
                pos += 1
        c1 = np.where(mask[t][None, :], 1 - c0, 0).astype(np.int16)
        bm = np.stack([c0[:, 0] + c0[:, 1], c0[:, 0] + c1[:, 1], c1[:, 0] + c0[:, 1], c1[:, 0] + c1[:, 1]], axis=1)
        m0 = pm[:, R._P0] + bm[:, R._C0]
        m1 = pm[:, R._P1] + bm[:, R._C1]
        pm = np.minimum(m0, m1)
        pm -= pm.min(axis=1, keepdims=True)
        if t >= 6:                                          # (every state has been reached)
            worst = np.maximum(worst, pm.max(axis=1))
        if t >= 32:                                         # (the start state is forgotten)
            held = np.maximum(held, pm.max(axis=1))
    mixed = held[1:0xffff]                                  # (0x0000 and 0xffff are the garbage family's zeros and ones)
    pat = 1 + int(np.nonzero(mixed == mixed.max())[0][0])
    return pat, int(held[pat]), int(held.max()), int(worst.max())


def spread_of(fs, word, k):
    """the largest spread of the reference's metrics over the steps of one received word (from step 6 on: before that not
    every state has been reached from the start state)"""
    sp = []
    R.viterbi(fs, R.bits_of(word)[None], k, 1, spread=sp)
    return int(max(sp[6:])) if len(sp) > 6 else 0


# ---------------------------------------------------------------------------------------------------- tie search
@functools.lru_cache(None)
def _difference_weights(fs, phase):
    """{e: codeword distance} for every message difference e of at most 8 bits (first bit set: e in [128, 256) read MSB
    first) that starts at a trellis step congruent to phase modulo the puncturing period"""
    out = {}
    for e in range(128, 256):
        m = np.zeros(24 + 8, np.uint8)
        m[phase:phase + 8] = [(e >> (7 - i)) & 1 for i in range(8)]
        out[e] = int(code_sequence(fs, m).sum())
    return out


def _e_len(e):
    return 8 - ((e & -e).bit_length() - 1)          # bits from the first to the last set one


def find_neighbour(fs, t, k):
    """the difference e (8 bits, MSB first, starting at step t) with the smallest even codeword distance that fits into the
    message, then the smallest length, then the smallest value; None if no difference that fits has an even distance.
    Returns (e, distance, free: whether that distance is the smallest of ALL differences that fit, even or odd)."""
    w = _difference_weights(fs, t % period(fs))
    fit = [e for e in w if t + _e_len(e) <= 8 * k]
    even = [e for e in fit if w[e] % 2 == 0]
    if not even:
        return None
    e = min(even, key=lambda e: (w[e], _e_len(e), e))
    return e, w[e], w[e] == min(w[x] for x in fit)


def tie_word(fs, m, ts):
    """received word with a tie at every divergence step of ts: (word, m', [(t, e, d, free)])"""
    k = len(m)
    mb = R.bits_of(m)
    cw = R.conv_encode_bits(fs, m)
    rx, m2, info = cw.copy(), mb.copy(), []
    for t in ts:
        e, d, free = find_neighbour(fs, t, k)
        eb = np.zeros(len(mb), np.uint8)
        eb[t:t + 8] = [(e >> (7 - i)) & 1 for i in range(8)][:len(mb) - t]
        diff = np.nonzero(cw ^ R.conv_encode_bits(fs, np.packbits(mb ^ eb)))[0]
        assert len(diff) == d
        rx[diff[0::2]] ^= 1
        m2 ^= eb
        info.append((t, e, d, free))
    return R.bytes_of(rx, R.fec_enc_len(fs, k)), np.packbits(m2), info


def tie_steps(k):
    """divergence steps of the tie family for a k-byte message: block edges, warm-up lengths, both ends"""
    ts = {0}
    for B in BLOCKS:
        ts |= {B - 65, B - 64, B - 1, B, B + 1, B + 63, B + 64, B + 96, B + 128}
    return sorted(t for t in ts if t < 8 * k - 8)


def last_tie_step(fs, k):
    """the last message step at which a difference with an even distance still fits (its path then ends in the flush steps)"""
    for t in range(8 * k - 1, 8 * k - 16, -1):
        if find_neighbour(fs, t, k) is not None:
            return t
    raise AssertionError((fs, k))


# ---------------------------------------------------------------------------------------------------- the list
def _build():
    rng = np.random.default_rng(20261019)
    cases = []

    def carrier(i, conv=True):
        if conv and i % 9 == 4:
            return R.PSK2
        return (R.PSK4, R.QAM16)[i % 2]

    def add(family, name, fec0, fec1, check, n, pkt, conv=True, **meta):
        k, l0, l1 = R.packet_dims(n, check, fec0, fec1)
        pkt = np.asarray(pkt, np.uint8)
        assert len(pkt) == l1, (name, len(pkt), l1)
        pkt.setflags(write=False)
        i = len(cases)
        cases.append(dict(family=family, name="%s/%s" % (family, name), mod=carrier(i, conv), fec0=fec0, fec1=fec1, check=check, n=n,
                          pkt=pkt, gap=GAPS[i % len(GAPS)], **meta))

    def message(k, i):
        check = pick_check(k, i)
        n = k - R.crc_len(check)
        return check, n, inner_message(rng.integers(0, 256, n, dtype=np.uint8), check)

    def add_inner(family, name, fs, fec1, check, n, r0, **meta):
        add(family, name, fs, fec1, check, n, channel_from_inner(r0, fec1), **meta)

    j = 0
    # ---- single
    for fs in R.CONV:
        P = period(fs)
        for k in (1, 2, 16):
            check, n, m = message(k, j); j += 1
            cw = R.fec_encode(fs, m)
            nb, tot = coded_bits(fs, k), 8 * len(cw)
            first = range(min(2 * bits_before(fs, P), tot))
            last = range(bits_before(fs, steps_of(k) - max(2 * P, 6)), tot)
            for pos in sorted(set(first) | set(last)):
                add_inner("single", "r%s k%d bit%d%s" % (RATE[fs], k, pos, " pad" if pos >= nb else ""), fs, R.FEC_NONE, check, n,
                          flip_bits(cw, [pos]), flips=1 if pos < nb else 0, truth=m)
    # ---- burst
    for fs in R.CONV:
        k = 32
        check, n, m = message(k, j); j += 1
        cw = R.fec_encode(fs, m)
        nb = coded_bits(fs, k)
        for run in range(1, 13):
            for where, at in (("start", 0), ("middle", nb // 2 - run // 2), ("end", nb - run)):
                add_inner("burst", "r%s %s run%d" % (RATE[fs], where, run), fs, R.FEC_NONE, check, n, flip_bits(cw, range(at, at + run)),
                          flips=run, truth=m)
    # ---- tie
    for fs in R.CONV:
        for k in TIE_K:
            for t in tie_steps(k) + [last_tie_step(fs, k)]:
                check, n, m = message(k, j); j += 1
                r0, m2, info = tie_word(fs, m, [t])
                add_inner("tie", "r%s k%d t%d" % (RATE[fs], k, t), fs, R.FEC_NONE, check, n, r0, tie=info, truth=m, other=m2)
            for B in BLOCKS:                                   # two ties in neighbouring blocks
                if fs == R.FEC_V27 or (B == 128) == (k == 48):
                    check, n, m = message(k, j); j += 1
                    ts = [B - 30, B + 70]
                    r0, m2, info = tie_word(fs, m, ts)
                    add_inner("tie", "r%s k%d two t%d t%d" % (RATE[fs], k, ts[0], ts[1]), fs, R.FEC_NONE, check, n, r0, tie=info, truth=m, other=m2)
    # ---- tail
    for fs in R.CONV:
        for k in (2, 16, 33):
            while coded_bits(fs, k) % 8 == 0:                 # (a length whose last byte has pad bits)
                k += 1
            check, n, m = message(k, j); j += 1
            cw = R.fec_encode(fs, m)
            nb, l0 = coded_bits(fs, k), len(cw)
            tailbits = np.concatenate([R.bits_of(m), np.array([1, 0, 1, 1, 0, 1], np.uint8)])
            add_inner("tail", "r%s k%d nonzero tail" % (RATE[fs], k), fs, R.FEC_NONE, check, n, R.bytes_of(code_sequence(fs, tailbits), l0),
                      flips=None, truth=m)
            add_inner("tail", "r%s k%d pad bits set" % (RATE[fs], k), fs, R.FEC_NONE, check, n, flip_bits(cw, range(nb, 8 * l0)), flips=0, truth=m)
            add_inner("tail", "r%s k%d last coded bit" % (RATE[fs], k), fs, R.FEC_NONE, check, n, flip_bits(cw, [nb - 1]), flips=1, truth=m)
    # ---- garbage
    for fs in R.CONV:
        for k in (1100, 48):
            check, n, m = message(k, j); j += 1
            cw = R.fec_encode(fs, m)
            l0 = len(cw)
            pat = SPREAD[fs][0]
            rep = np.resize(np.array([(pat >> (15 - i)) & 1 for i in range(16)], np.uint8), 8 * l0)
            for name, r0 in (("zeros", np.zeros(l0, np.uint8)), ("ones", np.full(l0, 0xff, np.uint8)), ("complement", cw ^ 0xff),
                             ("spread", np.packbits(rep))):
                add_inner("garbage", "r%s k%d %s" % (RATE[fs], k, name), fs, R.FEC_NONE, check, n, r0, truth=m)
    # ---- short
    for fs in R.CONV:
        for k in (0, 1, 2):
            check, n, m = message(k, j); j += 1
            cw = R.fec_encode(fs, m)
            add_inner("short", "r%s k%d clean" % (RATE[fs], k), fs, R.FEC_NONE, check, n, cw, flips=0, truth=m)
            add_inner("short", "r%s k%d one error" % (RATE[fs], k), fs, R.FEC_NONE, check, n, flip_bits(cw, [min(3, coded_bits(fs, k) - 1)]),
                      flips=1, truth=m)
    # ---- outer: tie and burst words inside an outer code
    for fec1 in (R.FEC_GOLAY, R.FEC_SD72, R.FEC_RS):
        for fs in R.CONV:
            k = 48
            for t in (0, 63, 127, 128, 129, 191, 192, 256):
                check, n, m = message(k, j); j += 1
                r0, m2, info = tie_word(fs, m, [t])
                add_inner("outer", "r%s %d tie t%d" % (RATE[fs], fec1, t), fs, fec1, check, n, r0, tie=info, truth=m, other=m2)
            check, n, m = message(k, j); j += 1
            cw = R.fec_encode(fs, m)
            nb = coded_bits(fs, k)
            for where, at, run in (("start", 0, 5), ("middle", nb // 2, 12), ("end", nb - 7, 7), ("end", nb - 1, 1)):
                add_inner("outer", "r%s %d burst %s run%d" % (RATE[fs], fec1, where, run), fs, fec1, check, n, flip_bits(cw, range(at, at + run)),
                          flips=run, truth=m)
    # ---- Reed-Solomon
    def rs_block_errors(dl, count, where, value, seed, pick=0):
        """positions and values of `count` byte errors in a block of dl + 32 bytes; where = "ends": the first and the last
        transmitted byte among them (a lone error: the first byte for pick 0, the last for pick 1)"""
        r = np.random.default_rng(seed)
        N = dl + 32
        if where == "data":
            pool = np.arange(dl)
        elif where == "parity":
            pool = np.arange(dl, N)
        else:
            pool = np.arange(N)
        if count > len(pool):
            return None
        pos = r.choice(pool, count, replace=False)
        if where == "ends" and count >= 1:
            rest = [p for p in pos if p not in (0, N - 1)]
            pos = np.array(([0, N - 1] if count >= 2 else [(0, N - 1)[pick % 2]]) + rest[:max(0, count - 2)], np.int64)
        err = np.zeros(N, np.uint8)
        err[pos] = value
        return err

    def add_rs(name, as_fec1, k, make_rx, **meta):
        """One Reed-Solomon case: fec0 = RS on a k-byte message (fec1 none), or fec1 = RS over V27 on a k-byte message (the RS
        message is V27's 2 k + 2 bytes).  make_rx(cw) -> received blocks, both (nb, dl + 32)."""
        nonlocal j
        check, n, m = message(k, j); j += 1
        if as_fec1:
            tr = {}
            R.packet_encode(R.scramble(m)[:n], check, R.FEC_V27, R.FEC_RS, tr)
            cw = tr["cw1"]
        else:
            cw = R.fec_encode(R.FEC_RS, m)
        nb, dl = R.rs_dims(R.fec_enc_len(R.FEC_V27, k) if as_fec1 else k)
        cw2 = cw.reshape(nb, dl + 32)
        rx = np.asarray(make_rx(cw2), np.uint8)
        assert rx.shape == cw2.shape
        if as_fec1:
            add("rs", "over V27 " + name, R.FEC_V27, R.FEC_RS, check, n, channel_from_outer(rx.ravel()), conv=False, truth=m,
                rs_errors=rx ^ cw2, rs_codeword=cw, **meta)
        else:
            add("rs", "fec0 " + name, R.FEC_RS, R.FEC_NONE, check, n, channel_from_inner(rx.ravel(), R.FEC_NONE), conv=False, truth=m,
                rs_errors=rx ^ cw2, rs_codeword=cw, **meta)

    seed = lone = 0
    for as_fec1, ks in ((False, (1, 222, 223, 224, 446, 447)), (True, (0, 110, 111, 222))):
        for k in ks:
            rs_n = R.fec_enc_len(R.FEC_V27, k) if as_fec1 else k
            nb, dl = R.rs_dims(rs_n)
            for count in (0, 1, 8, 15, 16, 17):
                for where in (("ends",) if count == 0 else ("data", "parity", "ends")):
                    value = (0x01, 0xff)[seed % 2]
                    blocks = [rs_block_errors(dl, count, where, value, seed * 8 + b, pick=lone + b) for b in range(nb)]
                    seed += 1
                    lone += int(count == 1 and where == "ends")      # (lone errors take the first and the last byte in turns)
                    if any(b is None for b in blocks):
                        continue
                    add_rs("n%d %d errors %s %02x" % (rs_n, count, where, value), as_fec1, k, lambda cw, e=np.stack(blocks): cw ^ e, rs_count=count)
    # the special words, in both roles (over V27 the RS message is 2 k + 2 bytes: k = 0, 222, 300 -> 1, 2, 3 blocks)
    for as_fec1, ks in ((False, (1, 223, 447)), (True, (0, 222, 300))):        # an all-zero received block (every block of the packet)
        for k in ks:
            rs_n = R.fec_enc_len(R.FEC_V27, k) if as_fec1 else k
            add_rs("n%d all-zero blocks" % rs_n, as_fec1, k, lambda cw: np.zeros_like(cw), rs_count=None)
    for as_fec1, ks in ((False, (222, 223, 447)), (True, (110, 222, 300))):    # 15 errors from ANOTHER codeword: 17 or more from the one sent
        for k in ks:
            rs_n = R.fec_enc_len(R.FEC_V27, k) if as_fec1 else k
            nb, dl = R.rs_dims(rs_n)
            errs = np.stack([rs_block_errors(dl, 15, "all", 0xff, 9000 + seed + b) for b in range(nb)])
            seed += 1
            hold = {}

            def other_plus_15(cw, errs=errs, dl=dl, hold=hold):
                d2 = cw[:, :dl].copy()
                d2[:, 0] ^= 0x5a                                    # another message -> a codeword at distance >= 33
                hold["other"] = R.rs_encode_blocks(d2)
                return hold["other"] ^ errs
            add_rs("n%d other codeword + 15" % rs_n, as_fec1, k, other_plus_15, rs_count=None)
            cases[-1]["rs_other"] = hold["other"].ravel()
    for as_fec1, kb in ((False, ((447, 1), (700, 2))), (True, ((300, 1), (400, 2)))):   # one block beyond repair between clean ones
        for k, bad in kb:
            rs_n = R.fec_enc_len(R.FEC_V27, k) if as_fec1 else k
            nb, dl = R.rs_dims(rs_n)
            errs = np.zeros((nb, dl + 32), np.uint8)
            errs[bad] = rs_block_errors(dl, 40, "all", 0x01, 777 + k)
            add_rs("n%d block %d of %d beyond repair" % (rs_n, bad, nb), as_fec1, k, lambda cw, e=errs: cw ^ e, rs_count=None)
    return cases


@functools.lru_cache(None)
def cases():
    return _build()


def families():
    return tuple(FAMILY_COUNTS)


def of_family(*fams):
    return [c for c in cases() if c["family"] in fams]


# ---------------------------------------------------------------------------------------------------- frames and streams
def frame(c):
    """the case's frame, complex128: the header of (n, mod, check, fec0, fec1), the payload symbols of pkt's labels, the pulse of
    ref_framegen.frame at dt = 0"""
    words = G.payload_words(c["pkt"], R.bps(c["mod"]))
    pts = G._points_of_labels(c["mod"], words)
    x = G.frame_symbols(np.zeros(c["n"], np.uint8), c["mod"], c["fec0"], c["fec1"], c["check"], points=pts)
    up = np.zeros(G.K * len(x), np.complex128)
    up[::G.K] = x
    return np.convolve(up, G.tx_taps(0.0))[:G.K * len(x)]


def layout(cs):
    """[(offset, case)] back to back with each case's gap (>= 300 samples) behind it, and the total length"""
    out, off = [], LEAD
    for c in cs:
        out.append((off, c))
        off += G.frame_len(c["n"], c["mod"], c["fec0"], c["fec1"], c["check"]) + c["gap"]
    return out, off + 700


STREAMS = (("single",), ("burst",), ("tie",), ("tail", "short"), ("garbage",), ("outer",), ("rs",))


@functools.lru_cache(None)
def streams():
    """one complex64 stream per entry of STREAMS: (samples, [case, ...] in order of appearance)"""
    out = []
    for fams in STREAMS:
        cs = of_family(*fams)
        lay, total = layout(cs)
        x = np.zeros(total, np.complex128)
        for off, c in lay:
            f = frame(c)
            x[off:off + len(f)] = f
        x = x.astype(np.complex64)
        x.setflags(write=False)
        out.append((x, cs))
    return out


def stream_of(*fams):
    return next(i for i, f in enumerate(STREAMS) if f == fams)


def crafted_labels(c):
    """the labels the receiver's demapper must give for the case's payload symbols"""
    return G.payload_words(c["pkt"], R.bps(c["mod"]))


# ---------------------------------------------------------------------------------------------------- batched reference decode
def decode_batch(cs, chans, soft=False):
    """ref_decode.packet_decode (soft: packet_decode_soft) of every case's channel input -- chans[i]: l1 bytes, soft: 8 l1 soft
    values -- with the convolutional fec0 decodes of equal shape run as one ref_decode.viterbi call.  Returns
    ([(payload, valid)], [fec0's final metric or None])."""
    out, metric, groups = [None] * len(cs), [None] * len(cs), {}
    hard = lambda s: np.packbits((np.asarray(s) > 127).astype(np.uint8))
    for i, (c, ch) in enumerate(zip(cs, chans)):
        n, check, fec0, fec1 = c["n"], c["check"], c["fec0"], c["fec1"]
        k, l0, l1 = R.packet_dims(n, check, fec0, fec1)
        if fec0 not in R.CONV or fec1 in R.CONV:
            out[i] = R.packet_decode_soft(ch, n, check, fec0, fec1) if soft else R.packet_decode(ch, n, check, fec0, fec1)
            continue
        if soft:
            v = R.interleave_soft(np.asarray(ch, np.uint8)[:8 * l1], l1, decode=True)
            if fec1 == R.FEC_NONE:
                groups.setdefault((fec0, k, 255), []).append((i, R.interleave_soft(v, l0, decode=True).astype(np.int64)))
                continue
            in1 = hard(v)
        else:
            in1 = R.interleave(np.asarray(ch, np.uint8)[:l1], decode=True)
        in0 = R.interleave(R.fec_decode(fec1, in1, l0), decode=True)
        groups.setdefault((fec0, k, 1), []).append((i, R.bits_of(in0).astype(np.int64)))
    for (fs, k, vmax), members in groups.items():
        dec, met = R.viterbi(fs, np.stack([v for _, v in members]), k, vmax)
        for (i, _), d, mt in zip(members, dec, met):
            out[i] = R._finish(d, cs[i]["n"], cs[i]["check"])
            metric[i] = int(mt)
    return out, metric


@functools.lru_cache(None)
def reference():
    """per stream: ([(payload, valid)] of the crafted packets by the reference's hard-decision chain, [fec0 metric or None])"""
    return tuple(decode_batch(cs, [c["pkt"] for c in cs]) for _, cs in streams())


def on_batch_path(c):
    return c["fec0"] in R.CONV and c["fec1"] in BATCH_FEC1


def clean_count(cs, metrics):
    """rate-1/2 cases on the batch path whose inner word is, as received, the codeword of a zero-tailed message: the
    reference's maximum-likelihood metric is 0 (pad bits are not coded bits and do not count)"""
    return sum(1 for c, m in zip(cs, metrics) if c["fec0"] == R.FEC_V27 and on_batch_path(c) and m == 0)
