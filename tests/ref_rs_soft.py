"""Soft-decision Reed-Solomon decoding (fxrx_config.soft_rs), the reference in numpy: generalized-minimum-distance decoding of
RS(255,223) blocks by 17 errors-and-erasures trials.  The rule, for one block of N = dl + 32 bytes with soft
values s[8 j + b] (codeword order, b = 0 the MSB):

  hard byte h_j (bit set iff s > 127), bit margin m = |2 s - 255|, byte reliability rho_j = min_b m[8 j + b];
  erasure order: positions ascending by (rho_j, j), E_f its first f;
  candidate c_f, f = 0, 2, ..., 32: the codeword of the shortened code that differs from h in at most (32 - f) / 2 positions
    outside E_f (unique if it exists);
  cost D(c) = sum of m over the bits where c and h differ; the winner is the least D, ties to the smallest f; no candidate at
    all: h as received.

The errors-and-erasures decoder here is linear algebra only, as ref_decode.rs_decode_block is: Forney syndromes, the rank of their
Hankel matrix for the number of errors, Peterson-Gorenstein-Zierler for the locator, an exhaustive root search, one Vandermonde
solve for all values, and the result is accepted only if it is a codeword within the radius.  It shares no step with the kernel's
Berlekamp-Massey / Forney.  Everything is batched over blocks of one length (the Gauss-Jordan runs on a stack of matrices), so
that a few thousand random blocks take seconds."""
import numpy as np

import ref_decode as rd

F_LIST = tuple(range(0, 33, 2))
NO_F = 255


# ---------------------------------------------------------------------------------------------------- soft values -> bytes
def hard_bytes(soft):
    """(..., 8 N) soft values -> (..., N) hard bytes"""
    s = np.asarray(soft, np.uint8)
    return np.packbits((s > 127).astype(np.uint8), axis=-1)


def bit_margins(soft):
    return np.abs(2 * np.asarray(soft, np.int64) - 255)


def byte_reliability(soft):
    """(..., 8 N) soft values -> (..., N) rho_j = min_b |2 s - 255|"""
    m = bit_margins(soft)
    return m.reshape(m.shape[:-1] + (m.shape[-1] // 8, 8)).min(axis=-1)


def erasure_order(soft):
    """positions ascending by (rho_j, j): (..., N)"""
    rho = byte_reliability(soft)
    return np.argsort(rho * 256 + np.arange(rho.shape[-1]), axis=-1, kind="stable")


def cost(soft, c, h):
    """D(c): the sum of the bit margins where c and h differ, per block"""
    diff = np.unpackbits(np.asarray(c, np.uint8) ^ np.asarray(h, np.uint8), axis=-1)
    return (bit_margins(soft) * diff).sum(axis=-1)


# ---------------------------------------------------------------------------------------------------- GF(2^8) on stacks
def _ginv_np(a):
    return rd.EXP_NP[(255 - rd.LOG_NP[a]) % 255]


def _gf_eliminate_batch(M):
    """Gauss-Jordan over GF(2^8) on all but the last column of the stack M (B, r, c + 1), in place; returns the ranks.  Where a
    matrix has full column rank c = r its last column ends as the solution."""
    B, r, c1 = M.shape
    row = np.zeros(B, np.int64)
    ar = np.arange(B)
    for c in range(c1 - 1):
        cand = (M[:, :, c] != 0) & (np.arange(r)[None, :] >= row[:, None])
        has = cand.any(axis=1)
        if not has.any():
            continue
        b = ar[has]
        p, q = cand[has].argmax(axis=1), row[has]
        tmp = M[b, p].copy()
        M[b, p] = M[b, q]
        tmp = rd.gmul_np(tmp, _ginv_np(tmp[:, c])[:, None])
        M[b, q] = tmp
        fac = M[b][:, :, c].copy()
        fac[np.arange(len(b)), q] = 0
        M[b] = M[b] ^ rd.gmul_np(fac[:, :, None], tmp[:, None, :])
        row[has] += 1
    return row


def _solve_batch(A, y):
    """A (B, n, n), y (B, n) -> x (B, n), ok (B,)"""
    M = np.concatenate([A, y[:, :, None]], axis=2).astype(np.int64)
    rank = _gf_eliminate_batch(M)
    return M[:, :, -1], rank == A.shape[1]


def _pow_np(xlog, i):
    """alpha^(xlog i)"""
    return rd.EXP_NP[(np.asarray(xlog, np.int64) * i) % 255]


# ---------------------------------------------------------------------------------------------------- errors and erasures
def rs_decode_erasures_batch(h, erased):
    """h (B, N) hard blocks, erased (B, f) erased positions (distinct within a block).  Returns (c (B, N), ok (B,)): the codeword of
    the shortened code that differs from h in at most (32 - f) / 2 positions outside `erased`, where there is one."""
    h = np.asarray(h, np.uint8)
    B, N = h.shape
    erased = np.asarray(erased, np.int64).reshape(B, -1)
    f = erased.shape[1]
    t = (32 - f) // 2
    S = rd.rs_syndromes(h).astype(np.int64)                         # (B, 32): S_1 .. S_32
    xe = (N - 1 - erased) % 255                                     # logs of the erasure locators
    # erasure locator Gamma(x) = prod (1 + X x), coefficients by power
    G = np.zeros((B, f + 1), np.int64)
    G[:, 0] = 1
    for k in range(f):
        G[:, 1:] ^= rd.gmul_np(G[:, :-1], rd.EXP_NP[xe[:, k]][:, None])
    # Forney syndromes T_k = sum_i Gamma_i S_(k - i), k = f + 1 .. 32 (1-based): free of the erasures' contributions
    T = np.zeros((B, 32 - f), np.int64)
    for k in range(f, 32):
        for i in range(f + 1):
            T[:, k - f] ^= rd.gmul_np(G[:, i], S[:, k - i])
    c = h.copy()
    ok = np.zeros(B, bool)
    if t:
        H = np.stack([np.stack([T[:, i + j] for j in range(t)], axis=1) for i in range(t)], axis=1)       # (B, t, t) Hankel
        nu = _gf_eliminate_batch(np.concatenate([H, np.zeros((B, t, 1), np.int64)], axis=2))
    else:
        nu = np.zeros(B, np.int64)
    pos_log = (N - 1 - np.arange(N)) % 255
    inv_log = (255 - pos_log) % 255
    for n in np.unique(nu):
        n = int(n)
        b = np.nonzero(nu == n)[0]
        good = np.ones(len(b), bool)
        if n:
            A = np.stack([np.stack([T[b, i + j] for j in range(n)], axis=1) for i in range(n)], axis=1)
            lam, good = _solve_batch(A, np.stack([T[b, i + n] for i in range(n)], axis=1))
            lam = np.concatenate([np.ones((len(b), 1), np.int64), lam[:, ::-1]], axis=1)                   # sigma_0 .. sigma_n
            val = np.zeros((len(b), N), np.int64)
            for i in range(n + 1):
                val ^= rd.gmul_np(lam[:, i][:, None], _pow_np(inv_log, i)[None, :])
            root = val == 0
            in_erased = np.zeros((len(b), N), bool)
            if f:
                in_erased[np.arange(len(b))[:, None], erased[b]] = True
            good &= (root.sum(axis=1) == n) & ~(root & in_erased).any(axis=1)
            b, root = b[good], root[good]
            if not len(b):
                continue
            epos = np.argsort(~root, axis=1, kind="stable")[:, :n]                                        # the n root positions
            allpos = np.concatenate([erased[b], epos], axis=1)
        else:
            allpos = erased[b]
        v = f + n
        if v == 0:
            ok[b] = ~S[b].any(axis=1)
            continue
        xl = (N - 1 - allpos) % 255                                                                       # (b, v)
        V = np.stack([_pow_np(xl, i) for i in range(1, v + 1)], axis=1)                                   # V[., i - 1, k] = X_k^i
        Y, solved = _solve_batch(V, S[b, :v])
        cb = h[b].copy()
        cb[np.arange(len(b))[:, None], allpos] ^= Y.astype(np.uint8)
        outside = cb != h[b]
        if f:
            outside[np.arange(len(b))[:, None], erased[b]] = False
        acc = solved & ~rd.rs_syndromes(cb).any(axis=1) & (outside.sum(axis=1) <= t)
        c[b[acc]] = cb[acc]
        ok[b[acc]] = True
    return c, ok


def rs_decode_erasures(h, erased):
    """one block: (codeword, True) or (h, False)"""
    c, ok = rs_decode_erasures_batch(np.asarray(h, np.uint8)[None], np.asarray(erased, np.int64)[None])
    return c[0], bool(ok[0])


# ---------------------------------------------------------------------------------------------------- the soft rule
def rs_decode_soft_blocks(soft, trace=None):
    """soft (B, 8 N) -> (blocks (B, N) after decoding, chosen f (B,), 255 for none).  trace (a dict) gets 'cand' (17, B, N), 'ok'
    (17, B) and 'cost' (17, B)."""
    soft = np.asarray(soft, np.uint8)
    h = hard_bytes(soft)
    order = erasure_order(soft)
    B = h.shape[0]
    best = h.copy()
    best_cost = np.full(B, np.iinfo(np.int64).max)
    chosen = np.full(B, NO_F, np.int64)
    cands, oks, costs = [], [], []
    for f in F_LIST:
        c, ok = rs_decode_erasures_batch(h, order[:, :f])
        d = cost(soft, c, h)
        better = ok & (d < best_cost)
        best[better], best_cost[better], chosen[better] = c[better], d[better], f
        cands.append(c), oks.append(ok), costs.append(d)
    if trace is not None:
        trace.update(cand=np.stack(cands), ok=np.stack(oks), cost=np.stack(costs), hard=h, order=order)
    return best, chosen.astype(np.uint8)


def rs_decode_soft(soft, n, chosen=None):
    """one packet: 8 fec_enc_len(RS, n) soft values (codeword order) -> n message bytes; chosen (a list) gets f per block"""
    nb, dl = rd.rs_dims(n)
    blocks, f = rs_decode_soft_blocks(np.asarray(soft, np.uint8)[:8 * nb * (dl + 32)].reshape(nb, 8 * (dl + 32)))
    if chosen is not None:
        chosen.extend(int(x) for x in f)
    return blocks[:, :dl].ravel()[:n].copy()


def packet_decode_soft_rs(soft, n, check, fec0, fec1, soft_rs=True):
    """ref_decode.packet_decode_soft with fxrx_config.soft_rs: the Reed-Solomon stage that decodes from soft values (fec1, or fec0
    when fec1 is none) uses the rule above; its output is hard bytes.  Everything else, and soft_rs off, is packet_decode_soft."""
    k, l0, l1 = rd.packet_dims(n, check, fec0, fec1)
    rs_stage = fec1 == rd.FEC_RS or (fec1 == rd.FEC_NONE and fec0 == rd.FEC_RS)
    if not soft_rs or not rs_stage:
        return rd.packet_decode_soft(soft, n, check, fec0, fec1)
    v = rd.interleave_soft(np.asarray(soft, np.uint8)[:8 * l1], l1, decode=True)
    if fec1 == rd.FEC_NONE:
        b0 = rs_decode_soft(rd.interleave_soft(v, l0, decode=True), k)
    else:
        b0 = rd.fec_decode(fec0, rd.interleave(rs_decode_soft(v, l0), decode=True), k)
    return rd._finish(b0, n, check)
