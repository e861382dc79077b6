"""The frames of tests/test_ref_framegen.py (reference against oracle, CPU) and tests/test_gpu_ref_framegen.py (reference against
fx_txenc_kernel / fx_txgen_kernel, GPU): one list of small frames chosen at the generator's edges (payloads of at most 300
bytes, except the four Reed-Solomon block-split cases, whose k = 446 and 447 need 442 .. 447).

  codes     every modulation x every code as fec0 (fec1 none), at two payload lengths; V27 and V27P34 as fec0 x every block
            code and Reed-Solomon as fec1; Reed-Solomon as fec0 under V27 / V27P34 as fec1; all six checks at n = 0, 1, 2
  tails     Golay / Hamming(12,8): k = n + crc = 0, 1, 2 mod 3; the SECDED codes: k = 16 .. 23 (0, 1 mod 2, 4, 8);
            Reed-Solomon: k = 222, 223, 224, 446, 447 (block split, unequal fill), with and without a check
  carry     each DPSK order at npay = 63, 64, 65, 128, 129 payload symbols where a frame with that count exists (DPSK2 has
            npay = 8 l1 and DPSK4 npay = 4 l1: only 64 and 128 occur; there the nearest counts on both sides are taken too)
  tiles     nsym = 64 + 231 + npay + 14 = 511, 512, 513, 768, 769 (fx_txgen_kernel's 256-symbol tile and 14-symbol halo);
            the shortest frame (npay = 0)
  widths    8 l1 not a multiple of bps for bps = 3, 5, 6
  offsets   gaps 0, 1, 2, 0, 3, 1, ... between frames: odd and even offsets (frame lengths are even)
  delays    dt cycles through ref_framegen.DTS; the user header is absent / random bytes in turns of two frames

Reference frames are computed once per process (reference_frames) and must not be modified."""
import functools

import numpy as np

import ref_decode as R
import ref_framegen as G

MODS = R.PAYLOAD_MODS
CODES = R.ALL_FEC
CHECKS = (R.CRC_NONE, R.CRC_CHECKSUM, R.CRC_8, R.CRC_16, R.CRC_24, R.CRC_32)
GAPS = (0, 1, 2, 0, 3, 1, 5)
LEAD = 3                                  # the first frame's offset (odd)
DPSK_COUNTS = (63, 64, 65, 128, 129)
TILE_NSYM = (511, 512, 513, 768, 769)
HEAD = G.PN_LEN + G.HDR_SYM + G.FLUSH     # 309 symbols around the payload


SEARCH_CODES = (R.FEC_NONE, R.FEC_V27, R.FEC_V27P34, R.FEC_H74, R.FEC_H128, R.FEC_SD22, R.FEC_V27P78, R.FEC_GOLAY)


@functools.lru_cache(None)
def _by_count(mod):
    """npay -> (n, check, fec0) of the first frame of `mod` (fec1 none, n <= 300) with that many payload symbols."""
    found = {}
    for fec0 in SEARCH_CODES:
        for check in CHECKS:
            for n in range(301):
                found.setdefault(G.num_payload_symbols(n, mod, fec0, R.FEC_NONE, check), (n, check, fec0))
    return found


def find_length(mod, npay):
    return _by_count(mod).get(npay)


def reachable(mod, npay):
    return npay in _by_count(mod)


def _build():
    rng = np.random.default_rng(20260)
    cases = []

    def add(tag, n, mod, fec0, fec1, check):
        i = len(cases)
        cases.append(dict(tag=tag, payload=rng.integers(0, 256, n, dtype=np.uint8), mod=mod, fec0=fec0, fec1=fec1, check=check,
                          header=rng.integers(0, 256, 14, dtype=np.uint8) if (i // 2) % 2 else None, dt=G.DTS[i % len(G.DTS)],
                          gap=GAPS[i % len(GAPS)]))

    short = (0, 1, 2, 3, 5, 8, 13, 21, 34, 55)
    long_ = (89, 100, 127, 128, 144, 200, 233, 255, 256, 300)
    j = 0
    for mod in MODS:                                              # codes: every modulation x every fec0, two lengths
        for fec0 in CODES:
            add("codes", short[j % len(short)], mod, fec0, R.FEC_NONE, CHECKS[j % 6])
            add("codes", long_[(j // 3) % len(long_)], mod, fec0, R.FEC_NONE, CHECKS[(j + 3) % 6])
            j += 1
    for fec0 in (R.FEC_V27, R.FEC_V27P34):                        # two stages
        for fec1 in R.BLOCK + (R.FEC_RS,):
            for n in (1, 47, 230):
                add("two-stage", n, MODS[j % len(MODS)], fec0, fec1, CHECKS[2 + j % 4])
                j += 1
    for fec1 in (R.FEC_V27, R.FEC_V27P34):
        for n in (0, 100, 222, 300):
            add("rs-under-conv", n, MODS[j % len(MODS)], R.FEC_RS, fec1, CHECKS[j % 6])
            j += 1
    for check in CHECKS:                                          # checks at the shortest payloads
        for n in (0, 1, 2):
            add("checks", n, MODS[j % len(MODS)], (R.FEC_NONE, R.FEC_V27, R.FEC_H84)[n], R.FEC_NONE, check)
            j += 1
    for fec0 in (R.FEC_GOLAY, R.FEC_H128):                        # tails
        for check, n in ((R.CRC_NONE, 0), (R.CRC_NONE, 9), (R.CRC_NONE, 10), (R.CRC_NONE, 11), (R.CRC_8, 8), (R.CRC_8, 9), (R.CRC_8, 10),
                         (R.CRC_16, 298), (R.CRC_16, 299), (R.CRC_16, 300)):
            add("tails-3", n, MODS[j % len(MODS)], fec0, R.FEC_NONE, check)
            j += 1
    for fec0 in (R.FEC_SD22, R.FEC_SD39, R.FEC_SD72):
        for k in range(16, 24):
            check = (R.CRC_NONE, R.CRC_8, R.CRC_32)[k % 3]
            add("tails-secded", k - R.crc_len(check), MODS[j % len(MODS)], fec0, R.FEC_NONE, check)
            j += 1
    for k in (222, 223, 224, 446, 447):
        for check in (R.CRC_NONE, R.CRC_32):
            add("tails-rs", k - R.crc_len(check), MODS[j % len(MODS)], R.FEC_RS, R.FEC_NONE, check)
            j += 1
    for mod in R.DPSK:                                            # the DPSK carry
        want = set()
        for c in DPSK_COUNTS:
            if reachable(mod, c):
                want.add(c)
            else:                                                 # the nearest counts that do occur, below and above
                want.add(max(x for x in range(c) if reachable(mod, x)))
                want.add(min(x for x in range(c + 1, c + 64) if reachable(mod, x)))
        for c in sorted(want):
            n, check, fec0 = find_length(mod, c)
            add("dpsk-carry-%d" % c, n, mod, fec0, R.FEC_NONE, check)
    for nsym in TILE_NSYM:                                        # the generator kernel's tiles
        hits = 0
        for mod in MODS:
            f = find_length(mod, nsym - HEAD)
            if f is not None and hits < 3:
                add("tiles-%d" % nsym, f[0], mod, f[2], R.FEC_NONE, f[1])
                hits += 1
        assert hits, nsym
    add("shortest", 0, R.PSK4, R.FEC_NONE, R.FEC_NONE, R.CRC_NONE)
    add("shortest", 0, R.QAM64, R.FEC_NONE, R.FEC_NONE, R.CRC_NONE)
    for mod in (R.PSK8, R.DPSK8, R.QAM32, R.QAM64):               # padded last symbol
        for n in (1, 2, 4, 5, 7):
            add("widths", n, mod, R.FEC_NONE, R.FEC_NONE, R.CRC_NONE)
    return cases


@functools.lru_cache(None)
def cases():
    return _build()


def layout(frame_len_of):
    """[(offset, case)] back to back with each case's gap behind it, and the total length.  frame_len_of(case) -> samples."""
    out, off = [], LEAD
    for c in cases():
        out.append((off, c))
        off += frame_len_of(c) + c["gap"]
    return out, off + 16


def ref_len(c):
    return G.frame_len(len(c["payload"]), c["mod"], c["fec0"], c["fec1"], c["check"])


def ref_frame(c, **controls):
    return G.frame(c["payload"], c["mod"], c["fec0"], c["fec1"], c["check"], header=c["header"], dt=c["dt"], **controls)


@functools.lru_cache(None)
def reference_frames():
    """The reference's frame of every case, in order (read-only arrays)."""
    out = []
    for c in cases():
        f = ref_frame(c)
        f.setflags(write=False)
        out.append(f)
    return out


def tx_desc(c, offset=0):
    """The case as a TxContext frame description."""
    return dict(payload=c["payload"], mod=c["mod"], fec0=c["fec0"], fec1=c["fec1"], check=c["check"], header=c["header"], dt=c["dt"],
                offset=offset)


def subset(n=60):
    """Indices of n cases that hold every modulation, every delay and every code (as fec0 or fec1)."""
    cs = cases()
    need = [("mod", m) for m in MODS] + [("dt", d) for d in G.DTS] + [("fec0", f) for f in CODES] + [("fec1", f) for f in CODES]
    need += [("check", k) for k in CHECKS] + [("hdr", False), ("hdr", True)]

    def has(c, what):
        k, v = what
        return (c["header"] is not None) == v if k == "hdr" else c[k] == v
    need = [w for w in need if any(has(c, w) for c in cs)]
    picked = []
    for w in need:
        if not any(has(cs[i], w) for i in picked):
            picked.append(next(i for i, c in enumerate(cs) if has(c, w) and i not in picked))
    step = max(1, len(cs) // n)
    for i in list(range(7, len(cs), step)) + list(range(len(cs))):
        if len(picked) >= n:
            break
        if i not in picked:
            picked.append(i)
    return sorted(picked[:n])
