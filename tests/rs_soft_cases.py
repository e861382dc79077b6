"""Crafted Reed-Solomon blocks for soft-decision decoding (fxrx_config.soft_rs; the rule: tests/ref_rs_soft.py), each named for what it
is, and seeded random packets.  A case is a dict: name, N, soft (8 N soft values, codeword order), sent (the codeword), expect:
  'sent'      the rule's output is the sent codeword;
  'not_sent'  it is not (too much is wrong);
and optionally hard_ok (whether the f = 0 candidate, the hard decoder, finds the sent codeword), chosen (the winning f), other (a
second codeword some f must reach).

Soft values: a byte is strong (every bit 0 / 255, margin 255) unless stated; a weak byte has one bit, or where it is wrong every
bit, at margin m < 255 (s = (255 +- m) / 2), which is its reliability rho.  Wrong bytes differ from the sent codeword in one to eight bits.

Note on 'no candidate': at f = 32 the rule's radius is 0 outside 32 erased positions, and any N - 32 positions of an MDS code are an
information set, so the f = 32 candidate always exists: the rule never passes a word on as received.  (Large f have candidates on
most random words too: at f = 30 two redundant symbols are left against one error.)  The far-word cases therefore assert that the
small f, the hard decoder among them, have no candidate, that f = 32 has one, and that the output is not the word received."""
import functools

import numpy as np

import ref_decode as rd
import ref_rs_soft as rs

SIZES = (1, 223, 224, 446)            # message bytes: N = 33; N = 255; two blocks of N = 144; two blocks of N = 255


def block_lengths():
    return sorted({rd.rs_dims(n)[1] + 32 for n in SIZES})


def strong(cw):
    """soft values of the bytes cw at full confidence"""
    return (np.unpackbits(np.asarray(cw, np.uint8)) * 255).astype(np.uint8)


def set_margin(soft, j, bit, m):
    """bit `bit` (0 = MSB) of byte j keeps its hard value at margin m (odd)"""
    i = 8 * j + bit
    soft[i] = (255 + m) // 2 if soft[i] > 127 else (255 - m) // 2


def codeword(rng, N):
    return rd.rs_encode_blocks(rng.randint(0, 256, (1, N - 32)))[0]


def _case(name, soft, sent, expect, **kw):
    return dict(name=name, N=len(sent), soft=np.asarray(soft, np.uint8), sent=np.asarray(sent, np.uint8), expect=expect, **kw)


def errors_and_weak(rng, N, e, w, name=None):
    """e strong wrong bytes (margin 255) and w weak wrong bytes (every bit at margin 1: the least reliable of the block); the correct
    bytes have one bit at margin 253, so that erasures beyond the weak bytes fall on correct bytes before they fall on wrong ones"""
    cw = codeword(rng, N)
    pos = rng.permutation(N)[:e + w]
    h = cw.copy()
    h[pos] ^= rng.randint(1, 256, e + w).astype(np.uint8)
    soft = strong(h)
    for j in np.setdiff1d(np.arange(N), pos):
        set_margin(soft, j, int(rng.randint(8)), 253)
    for j in pos[e:]:
        for b in range(8):
            set_margin(soft, j, b, 1)
    ok = 2 * e + w <= 32
    return _case(name or "%d_errors_%d_weak_wrong_N%d" % (e, w, N), soft, cw, "sent" if ok else "not_sent", hard_ok=e + w <= 16)


def wrong_not_least_reliable(rng, N):
    """10 wrong bytes at margin 101, 16 correct bytes weaker than that: erasing costs radius, the hard decoder's candidate wins"""
    cw = codeword(rng, N)
    pos = rng.permutation(N)[:26]
    h = cw.copy()
    h[pos[:10]] ^= rng.randint(1, 256, 10).astype(np.uint8)
    soft = strong(h)
    for j in pos[:10]:
        for b in range(8):
            set_margin(soft, j, b, 101)
    for i, j in enumerate(pos[10:]):
        set_margin(soft, j, int(rng.randint(8)), 2 * i + 1)
    return _case("wrong_bytes_not_the_least_reliable_N%d" % N, soft, cw, "sent", hard_ok=True, chosen=0)


def equal_reliabilities(rng, N, boundary):
    """every margin equal (0 / 255, or 127 / 128 at the boundary): the order is the index; bytes 0 .. 19 wrong: f = 8 is the first f
    that reaches the sent codeword (12 errors outside E_8, radius 12), and every larger f ties with it"""
    cw = codeword(rng, N)
    h = cw.copy()
    h[:20] ^= rng.randint(1, 256, 20).astype(np.uint8)
    soft = strong(h)
    if boundary:
        soft = np.where(soft > 127, 128, 127).astype(np.uint8)
    return _case("%s_everywhere_20_wrong_N%d" % ("boundary_127_128" if boundary else "equal_0_255", N), soft, cw, "sent", hard_ok=False, chosen=8)


def two_codewords(rng, N, tie):
    """sent A and B = A + a weight-33 codeword on the positions P; the word is B on 18 of P (weak there) and A on the other 15 (strong):
    15 from B, 18 from A.  The hard decoder gives B; with the weak positions erased A is reached, at less cost.  tie: margins chosen
    so that D(A) = D(B); the smaller f -- B's -- wins."""
    while True:
        A = codeword(rng, N)
        P = rng.permutation(N)[:33]
        unit = np.zeros(N, np.uint8)
        unit[P[0]] = int(rng.randint(1, 256))
        Cw, ok = rs.rs_decode_erasures(unit, P[1:])
        assert ok and Cw[P[0]] == unit[P[0]]
        if np.count_nonzero(Cw) != 33:
            continue
        B = A ^ Cw
        h = A.copy()
        h[P[:18]] = B[P[:18]]
        kA = int(np.unpackbits(h ^ A).sum())
        kB = int(np.unpackbits(h ^ B).sum())
        if not tie or (kA % 2 == kB % 2 and 0 < kA - 18 <= 5 * kB - 18 <= 255 * (kA - 18)):
            break
    soft = strong(h)
    if not tie:
        for i, j in enumerate(P[:18]):
            for b in range(8):
                set_margin(soft, j, b, 2 * i + 1)
        return _case("15_from_one_codeword_soft_values_favour_the_far_one_N%d" % N, soft, A, "sent", hard_ok=False, other=B)
    # D(B) = 5 kB: the bits of the 15 strong-side bytes where B differs, at margin 5 (rho = 5).  D(A): one differing bit per weak byte at
    # margin 1 (rho = 1), the other kA - 18 differing bits share 5 kB - 18 in odd margins
    for j in P[18:]:
        for b in np.nonzero(np.unpackbits((h ^ B)[j:j + 1]))[0]:
            set_margin(soft, j, int(b), 5)
    rest, todo = 5 * kB - 18, kA - 18
    for j in P[:18]:
        bits = np.nonzero(np.unpackbits((h ^ A)[j:j + 1]))[0]
        set_margin(soft, j, int(bits[0]), 1)
        for b in bits[1:]:
            m = min(255, rest - (todo - 1))             # (odd: rest and todo keep the same parity)
            set_margin(soft, j, int(b), m)
            rest, todo = rest - m, todo - 1
    assert rest == 0 and todo == 0
    return _case("cost_tie_between_two_codewords_N%d" % N, soft, A, "not_sent", hard_ok=False, other=B, chosen=0)


def far_word(rng, N):
    """random bytes at random margins: far from every codeword"""
    soft = rng.randint(0, 256, 8 * N).astype(np.uint8)
    return _case("word_far_from_every_codeword_N%d" % N, soft, codeword(rng, N), "not_sent", hard_ok=False, far=True)


def clean(rng, N):
    cw = codeword(rng, N)
    soft = strong(cw)
    for j in rng.permutation(N)[:20]:
        set_margin(soft, j, int(rng.randint(8)), 2 * int(rng.randint(60)) + 1)
    return _case("clean_word_N%d" % N, soft, cw, "sent", hard_ok=True, chosen=0)


@functools.lru_cache(None)
def cases():
    rng = np.random.RandomState(2255)
    out = []
    for N in block_lengths():
        for e, w in ((16, 0), (12, 8), (4, 24), (0, 32), (12, 7), (14, 3), (0, 17), (0, 25), (2, 28)):
            out.append(errors_and_weak(rng, N, e, w))
        for e, w in ((16, 1), (13, 7), (5, 23), (17, 0)) + (((0, 33),) if N >= 33 else ()):
            out.append(errors_and_weak(rng, N, e, w))
        out += [wrong_not_least_reliable(rng, N), equal_reliabilities(rng, N, False), equal_reliabilities(rng, N, True),
                two_codewords(rng, N, False), two_codewords(rng, N, True), far_word(rng, N), clean(rng, N)]
    return tuple(out)


def of_length(N):
    return [c for c in cases() if c["N"] == N]


@functools.lru_cache(None)
def reference():
    """per block length: (blocks after decoding, chosen f, trace) of ref_rs_soft on that length's cases, computed once"""
    out = {}
    for N in block_lengths():
        tr = {}
        blocks, f = rs.rs_decode_soft_blocks(np.stack([c["soft"] for c in of_length(N)]), tr)
        blocks.setflags(write=False), f.setflags(write=False)
        out[N] = (blocks, f, tr)
    return out


# ---------------------------------------------------------------------------------------------------- packets
# noise on the soft values at which about half of the blocks decode (bit error rates of roughly 22 wrong bytes a block)
SIGMA = {33: (0.6, 0.7, 0.8, 0.9), 144: (0.45, 0.5, 0.55), 255: (0.40, 0.43, 0.46, 0.5)}


def noisy_packets(n, count, seed):
    """count packets of n message bytes: (messages (count, n), soft (count, 8 fec_enc_len))"""
    rng = np.random.RandomState(seed)
    nb, dl = rd.rs_dims(n)
    msg = rng.randint(0, 256, (count, n)).astype(np.uint8)
    enc = np.stack([rd.fec_encode(rd.FEC_RS, m) for m in msg])
    bits = np.unpackbits(enc, axis=1).astype(np.float64)
    sigma = np.asarray(SIGMA[dl + 32])[rng.randint(0, len(SIGMA[dl + 32]), (count, 1))]
    y = (2.0 * bits - 1.0) + sigma * rng.standard_normal(bits.shape)
    return msg, np.clip(np.round(127.5 + 100.0 * y), 0, 255).astype(np.uint8)


def case_packets(n):
    """the crafted blocks of the packet's block length as packets of n message bytes: every block of a packet a case, in rotation"""
    nb, dl = rd.rs_dims(n)
    cs = of_length(dl + 32)
    return np.stack([np.concatenate([cs[(i + b) % len(cs)]["soft"] for b in range(nb)]) for i in range(len(cs))])


@functools.lru_cache(None)
def packet_reference(n, count, seed):
    """(soft, decoded (count, n), chosen f (count, nb)) of the crafted packets followed by `count` noisy ones, by the reference, once"""
    nb, dl = rd.rs_dims(n)
    soft = np.ascontiguousarray(np.concatenate([case_packets(n), noisy_packets(n, count, seed)[1]]))
    blocks, f = rs.rs_decode_soft_blocks(soft.reshape(-1, 8 * (dl + 32)))
    dec = blocks[:, :dl].reshape(len(soft), nb * dl)[:, :n].copy()
    for a in (soft, dec, f):
        a.setflags(write=False)
    return soft, dec, f.reshape(len(soft), nb)


# ---------------------------------------------------------------------------------------------------- crafted frames
# Noise-free frames, PSK4, CRC-32, 64-byte payload, fec1 = Reed-Solomon, fec0 none or V27, in which 24 bytes of the Reed-Solomon block
# carry one bit on the wrong side each, sent at a small amplitude.  PSK4 under ref_decode.demap_soft: with r = x + j y the label's MSB
# has the soft value 127 - 153.6 (x + y), its LSB 127 - 153.6 (x - y); so u = x + y and w = x - y set the two bits separately.  A
# crafted symbol has the wrong bit at |u| = 0.15 on the wrong side (margin about 46) and its other bit, right, at |w| = 0.6 (margin
# about 184, wherever that bit's byte lies): amplitude 0.44 against 1.  The 24 wrong bytes are then the 24 least reliable of the block:
# the hard decoder (radius 16) gives up, E_24 erases exactly them.  fec0 = V27: the wrong bits are chosen so that behind the
# de-interleaver they are 24 of about 30 consecutive coded bits of fec0's word, which no Viterbi decoder repairs.
FRAME_N, FRAME_WRONG, FRAME_LEAD = 64, 24, 333
U_WRONG, U_RIGHT = 0.15, 0.6


@functools.lru_cache(None)
def frame_case(fec0):
    """dict: payload, sent (fec1's codeword), word (the crafted fec1 input: the codeword with 24 wrong bits), wrong (their byte positions), x (the frame's
    samples, complex128, as ref_framegen.frame builds them at dt = 0), dims (k, l0, l1)"""
    import ref_framegen as G
    rng = np.random.RandomState(6400 + fec0)
    msg = rng.randint(0, 256, FRAME_N).astype(np.uint8)
    k, l0, l1 = rd.packet_dims(FRAME_N, rd.CRC_32, fec0, rd.FEC_RS)
    trace = {}
    chan = rd.packet_encode(msg, rd.CRC_32, fec0, rd.FEC_RS, trace)
    cw1 = trace["cw1"]
    assert rd.rs_dims(l0) == (1, l0) and len(cw1) == l1 == l0 + 32
    to_chan = np.empty(8 * l1, np.int64)
    to_chan[rd._ilv_perm(l1, False)] = np.arange(8 * l1)            # codeword bit q -> its channel bit
    if fec0 == rd.FEC_NONE:
        order = rng.permutation(8 * l1)                             # any bits
    else:
        order = rd._ilv_perm(l0, True)[8 * l0 // 3:]                # the codeword bits behind consecutive bits of fec0's word
    bits, used_bytes, used_syms = [], set(), set()
    for q in order:
        q = int(q)
        if q // 8 in used_bytes or int(to_chan[q]) // 2 in used_syms:
            continue
        bits.append(q); used_bytes.add(q // 8); used_syms.add(int(to_chan[q]) // 2)
        if len(bits) == FRAME_WRONG:
            break
    word_bits = rd.bits_of(cw1).copy()
    word_bits[bits] ^= 1
    labels = G.payload_words(chan, 2)
    pts = G._points_of_labels(rd.PSK4, labels).astype(np.complex128)
    for q in bits:
        p = int(to_chan[q])
        lab = int(labels[p // 2])
        ut, wt = (1.0 if not lab & 2 else -1.0), (1.0 if not lab & 1 else -1.0)     # the signs of u and w that say the label's bits
        u, w = (-U_WRONG * ut, U_RIGHT * wt) if p % 2 == 0 else (U_RIGHT * ut, -U_WRONG * wt)
        pts[p // 2] = 0.5 * (u + w) + 0.5j * (u - w)
    sym = G.frame_symbols(msg, rd.PSK4, fec0, rd.FEC_RS, rd.CRC_32, points=pts)
    up = np.zeros(G.K * len(sym), np.complex128)
    up[::G.K] = sym
    x = np.convolve(up, G.tx_taps(0.0))[:G.K * len(sym)]
    x.setflags(write=False)
    return dict(payload=msg.tobytes(), word=rd.bytes_of(word_bits, l1), sent=cw1.copy(), wrong=sorted(used_bytes), x=x, dims=(k, l0, l1), fec0=fec0)


def frame_stream(fec0):
    """the frame in a capture of its own: zeros, the frame, zeros (complex64)"""
    x = frame_case(fec0)["x"]
    return np.concatenate([np.zeros(FRAME_LEAD, np.complex64), x.astype(np.complex64), np.zeros(700, np.complex64)])
