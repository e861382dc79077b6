"""The payload PLL's fetch-ahead ring at its edges (fx_paypll_kernel, `pll_frame`: DESIGN.md section 6, "PLL fetch-ahead log").

A lane keeps the raw symbols of PLL_AHEAD + 1 = R blocks of eight in a register ring and walks the ring in whole turns, then a
partial one that ends in the frame's TAIL block.  What can go wrong is which slot a block is read from and which loads the guard
on `nsym` lets out, so the cases are frames whose payload symbol count nsym = 8 nfull + rem has
nfull in {0, 1, R - 1, R, R + 1, 2 R + 1}, each with and without a remainder.  R is read from the kernel source (no PLL_AHEAD
there: one block ahead, R = 2), so the file pins the same behaviour on either side of the ring.

Which remainders exist: nsym = ceil(8 e / bps) for e coded bytes (fx_fecdims.h, `header_parse`), so with two bits per symbol
nsym = 4 e and rem is 0 or 4; with four, rem is even.  Over all eleven schemes (1 to 6 bits per symbol) rem = 1 never occurs and
rem = 7 only with five or six bits per symbol; `_reachable` below works that out and the cases assert it.  So PSK4 runs every
nfull with rem 0 and 4 (rate 1/2 where the code allows it: its nsym is always a multiple of eight, so the rem = 4 frames are
uncoded), QAM16 runs the smallest remainder there is (2), QAM64 the largest (7), DPSK4 a differential demodulator.  nfull = 0
with rem = 0 is a frame without payload symbols, which the PLL never sees.

Every case frame is the last of its block and the only one of its modulation class (two frames of another class lie in front of
it): its PLL wave has 63 padding lanes and its last granule is the last of the symbol arena in use.  Each block runs alone
(depth 1) and with four blocks in flight under FXRX_TAIL_GANG=2, where PLL launches carry two blocks.  Against the CPU oracle:
everything `compare_frames` checks, and carrier-recovered symbols and evm_sum bit for bit."""
import os
import re

import numpy as np
import pytest

from parity_util import oracle_frames, compare_frames

pytestmark = pytest.mark.gpu

PSK4, DPSK4, QAM16, QAM64 = 2, 10, 27, 29
BPS = {1: 1, 2: 2, 3: 3, 4: 4, 9: 1, 10: 2, 11: 3, 18: 2, 27: 4, 28: 5, 29: 6}
FEC_NONE, FEC_V27 = 1, 11
CRC_NONE, CRC_24 = 1, 5
CRC_LEN = {CRC_NONE: 0, CRC_24: 3}


def _ring():
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gr-liquiddsp_amd", "csrc", "fx_kernels.hip")
    m = re.search(r"^#define\s+PLL_AHEAD\s+(\d+)", open(src).read(), re.M)
    return (int(m.group(1)) if m else 1) + 1


def _enc_len(fec, n):
    """fec_enc_len of fx_fecdims.h for the two schemes used here: rate 1/2, K = 7 sends 2 (8 n + 6) bits"""
    return (2 * (8 * n + 6) + 7) // 8 if fec == FEC_V27 else n


def _nsym(mod, fec0, check, pay_len):
    return -(-8 * _enc_len(fec0, pay_len + CRC_LEN[check]) // BPS[mod])


def _reachable(bps):
    return {(-(-8 * e // bps)) % 8 for e in range(48)}


def _props(mod, nfull, rem):
    """(fec0, check, payload length) of a frame with 8 nfull + rem payload symbols, the rate-1/2 code and the CRC where they fit"""
    for fec0, check in ((FEC_V27, CRC_24), (FEC_V27, CRC_NONE), (FEC_NONE, CRC_24), (FEC_NONE, CRC_NONE)):
        for n in range(0, 400):
            if _nsym(mod, fec0, check, n) == 8 * nfull + rem:
                return fec0, check, n
    raise AssertionError("no frame of scheme %d has %d full blocks and %d symbols beyond them" % (mod, nfull, rem))


def _cases():
    R = _ring()
    nfulls = sorted({0, 1, R - 1, R, R + 1, 2 * R + 1})
    cases = [(PSK4, nf, rem) for nf in nfulls for rem in (0, 4) if (nf, rem) != (0, 0)]
    cases += [(QAM16, R, 2), (QAM64, R - 1, 7), (QAM64, 2 * R + 1, 7), (DPSK4, R + 1, 4), (DPSK4, R, 0)]
    return cases


CASES = _cases()


def _chan(x, rng):
    n = np.arange(len(x))
    y = x * np.exp(1j * (0.011 * n + 0.3))
    s = np.sqrt(0.5 * 10 ** (-30.0 / 10))
    return (y + s * (rng.standard_normal(len(x)) + 1j * rng.standard_normal(len(x)))).astype(np.complex64)


@pytest.fixture(scope="module")
def blocks(fx, oracle):
    """One block per case with its oracle frames (computed once, never changed)."""
    assert all(1 not in _reachable(b) for b in set(BPS.values())) and _reachable(2) == {0, 4} and min(_reachable(4) - {0}) == 2
    assert 7 in _reachable(6) and 7 not in _reachable(4) | _reachable(3) | _reachable(2) | _reachable(1)
    out = []
    for i, (mod, nfull, rem) in enumerate(CASES):
        rng = np.random.default_rng(7000 + i)
        fec0, check, n = _props(mod, nfull, rem)
        other = fx.FrameGen(QAM16 if mod != QAM16 else PSK4, FEC_V27, 1, CRC_24)
        g = fx.FrameGen(mod, fec0, 1, check)
        z = lambda k: np.zeros(k, np.complex64)
        x = _chan(np.concatenate([z(300), other.frame(rng.integers(0, 256, 40, dtype=np.uint8)), z(280),
                                  other.frame(rng.integers(0, 256, 64, dtype=np.uint8)), z(300),
                                  g.frame(rng.integers(0, 256, n, dtype=np.uint8)), z(1200)]), rng)
        other.close(); g.close()
        of = oracle_frames(oracle, x)
        assert len(of) == 3 and all(f.header_valid for f in of), (mod, nfull, rem)
        last = of[-1]
        assert last.mod_scheme == mod and [f.mod_scheme for f in of[:2]] == [QAM16 if mod != QAM16 else PSK4] * 2
        ns = len(last.framesyms)
        assert (ns // 8, ns % 8) == (nfull, rem), "the case frame has %d payload symbols, not %d full blocks + %d" % (ns, nfull, rem)
        out.append((x, of))
    return out


def _check(of, gf, case):
    dev = compare_frames(of, gf)
    print("case", case, "deviations", dev)
    assert dev["bitexact_syms"], case
    for a, b in zip(of, gf):
        assert np.float32(a.info["evm_sum"]).view(np.uint32) == np.float32(b["evm_sum"]).view(np.uint32), (case, a.info["evm_sum"], b["evm_sum"])
        assert b["framesyms"] is not None and np.array_equal(a.framesyms.view(np.uint32), b["framesyms"].view(np.uint32)), case
    mod, nfull, rem = case
    assert (gf[-1]["mod_scheme"], gf[-1]["num_framesyms"]) == (mod, 8 * nfull + rem)


@pytest.mark.parametrize("k", range(len(CASES)), ids=["mod%d-nfull%d-rem%d" % c for c in CASES])
def test_ring_edges_one_block_at_a_time(fx, blocks, k):
    x, of = blocks[k]
    ctx = fx.RxContext(1, want_framesyms=True)
    gf = ctx.process([x])
    ctx.close()
    _check(of, gf, CASES[k])


def test_ring_edges_four_blocks_in_flight_ganged(fx, blocks, monkeypatch):
    """Every case block, then the first six again, through a pipeline of depth 4; with the gang setting 2 tails go out in pairs."""
    monkeypatch.setenv("FXRX_TAIL_GANG", "2")
    order = list(range(len(CASES))) + list(range(6))
    ctx = fx.RxContext(1, want_framesyms=True)
    ctx.set_depth(4)
    res, inflight = [], 0
    for k in order:
        if inflight == 4:
            res.append(ctx.results(ctx.collect_raw())); inflight -= 1
        ctx.reset()
        ctx.submit_raw([blocks[k][0].ctypes.data], [len(blocks[k][0])], False); inflight += 1
    while inflight:
        res.append(ctx.results(ctx.collect_raw())); inflight -= 1
    launches, members = ctx.gang_stats()
    ctx.close()
    print("ganged PLL launches %d carrying %d blocks" % (launches, members))
    assert launches >= 1 and members >= 2 * launches, "no PLL launch carried two blocks: the ganged path was not exercised"
    assert len(res) == len(order)
    for k, gf in zip(order, res):
        _check(blocks[k][1], gf, CASES[k])
