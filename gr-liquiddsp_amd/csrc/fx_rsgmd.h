// fx_rsgmd.h -- one trial of the soft-decision Reed-Solomon decoder (fxrx_config.soft_rs): errors-and-erasures
// decoding of one RS(255,223) block of N = dl + 32 bytes with its f least reliable positions erased.  rs_decode_soft_wave
// (fx_kernels.hip) runs 17 of these side by side, one per lane; the host-side test driver (tests/cpp/rsgmd_check.cpp) runs them
// one after the other.
//
// Conventions are rs_decode_block's: byte j of the block is the coefficient of x^(N - 1 - j), its locator X_j = alpha^(N - 1 - j);
// the generator's roots are alpha^1 .. alpha^32, S[i] = r(alpha^(i + 1)); ex / lg are the GF(2^8) / 0x11d tables (ex doubled).
//
// The trial: erasure locator Gamma(x) = prod (1 + X_j x) over the f erased positions; Forney syndromes U_k = sum_i Gamma_i
// S[k + f - i], k = 0 .. 31 - f, which the erased positions' values do not reach; Berlekamp-Massey on them for the error locator
// sigma of length L; errata locator Psi = Gamma sigma of degree v = f + L, evaluator Omega = S Psi mod x^32; Chien search over the
// N positions; Forney values Omega(1 / X) / Psi'(1 / X).  The result is accepted iff L <= (32 - f) / 2 and Psi has v roots among
// the N positions, each simple.  That makes it exactly the candidate of the rule: S then obeys Psi's recurrence from index v on,
// Psi has v distinct roots, so S is the power sums of values at those v positions and the corrected word is a codeword; it
// differs from the hard word in at most L positions outside the erased ones; and such a codeword is unique (distance 33).
// Conversely, where the candidate exists, the U_k are the power sums of its at most (32 - f) / 2 errors and Berlekamp-Massey
// finds their locator.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FX_RSG_HD __host__ __device__
#else
#define FX_RSG_HD
#endif

#define RSG_TRIALS 17u              // f = 0, 2, ..., 32
#define RSG_NO_COST 0xFFFFFFFFu     // no candidate

struct RsgTrial {
    uint32_t cost;                  // D: the sum of the bit margins |2 s - 255| over the bits the candidate changes
    uint32_t np;                    // changed positions (v: a value may be zero)
    uint8_t pos[32], val[32];
};

FX_RSG_HD inline uint8_t rsg_mul(const uint8_t *ex, const uint8_t *lg, uint8_t a, uint8_t b) { return (a && b) ? ex[lg[a] + lg[b]] : (uint8_t)0; }
// a alpha^l, l < 256
FX_RSG_HD inline uint8_t rsg_mul_log(const uint8_t *ex, const uint8_t *lg, uint8_t a, unsigned l) { return a ? ex[lg[a] + l] : (uint8_t)0; }

// S: the 32 syndromes of the hard word; era: the erasure order's first 32 positions; soft: the block's 8 N soft values
FX_RSG_HD inline void rsg_trial(unsigned f, unsigned N, const uint8_t *S, const uint8_t *era, const uint8_t *soft, const uint8_t *ex, const uint8_t *lg,
                                RsgTrial &out)
{
    out.cost = RSG_NO_COST; out.np = 0;
    uint8_t G[33], Lm[33], B[33], Tm[33], P[33], U[32], Om[32];
    for (int i = 0; i < 33; i++) { G[i] = 0; Lm[i] = 0; B[i] = 0; P[i] = 0; }
    G[0] = 1;
    for (unsigned k = 0; k < f; k++) {
        const uint8_t X = ex[N - 1u - era[k]];
        for (unsigned i = k + 1; i >= 1; i--) G[i] ^= rsg_mul(ex, lg, G[i - 1], X);
    }
    const unsigned nu = 32u - f;
    for (unsigned k = 0; k < nu; k++) {
        uint8_t u = 0;
        for (unsigned i = 0; i <= f; i++) u ^= rsg_mul(ex, lg, G[i], S[k + f - i]);
        U[k] = u;
    }
    Lm[0] = B[0] = 1;
    unsigned L = 0, m = 1; uint8_t b = 1;
    for (unsigned k = 0; k < nu; k++) {
        uint8_t d = U[k];
        for (unsigned i = 1; i <= L; i++) d ^= rsg_mul(ex, lg, Lm[i], U[k - i]);
        if (d == 0) { m++; continue; }
        for (int i = 0; i < 33; i++) Tm[i] = Lm[i];
        const uint8_t coef = ex[lg[d] + 255 - lg[b]];
        for (unsigned i = 0; i + m <= 32; i++) Lm[i + m] ^= rsg_mul(ex, lg, coef, B[i]);
        if (2 * L <= k) { L = k + 1 - L; for (int i = 0; i < 33; i++) B[i] = Tm[i]; b = d; m = 1; } else m++;
    }
    if (2 * L > nu) return;
    const unsigned v = f + L;
    for (unsigned i = 0; i <= f; i++)
        for (unsigned j = 0; j <= L; j++) P[i + j] ^= rsg_mul(ex, lg, G[i], Lm[j]);
    for (unsigned i = 0; i < 32; i++) {
        uint8_t o = 0;
        for (unsigned j = 0; j <= i && j <= v; j++) o ^= rsg_mul(ex, lg, P[j], S[i - j]);
        Om[i] = o;
    }
    unsigned np = 0;
    for (unsigned j = 0; j < N; j++) {
        const unsigned inv = (255u - (N - 1u - j)) % 255u;                  // log of 1 / X_j
        uint8_t p = P[v];
        for (unsigned i = v; i-- > 0;) p = (uint8_t)(rsg_mul_log(ex, lg, p, inv) ^ P[i]);
        if (p) continue;
        if (np == 32) return;
        uint8_t num = Om[31], den = 0;
        for (unsigned i = 31; i-- > 0;) num = (uint8_t)(rsg_mul_log(ex, lg, num, inv) ^ Om[i]);
        for (unsigned i = 1; i <= v; i += 2) den ^= rsg_mul_log(ex, lg, P[i], (inv * (i - 1u)) % 255u);
        if (den == 0) return;
        out.pos[np] = (uint8_t)j; out.val[np] = num ? ex[lg[num] + 255 - lg[den]] : (uint8_t)0; np++;
    }
    if (np != v) return;
    uint32_t cost = 0;
    for (unsigned i = 0; i < np; i++) {
        const uint8_t *s = soft + 8u * out.pos[i];
        for (unsigned bit = 0; bit < 8; bit++)
            if (out.val[i] & (0x80u >> bit)) cost += s[bit] > 127u ? 2u * s[bit] - 255u : 255u - 2u * s[bit];
    }
    out.cost = cost; out.np = np;
}

// The winner, give-up and output rule around the trials (fxrx_config.soft_rs_fmax, soft_rs_chain), written once for the kernel and
// the host-side test driver (tests/cpp/rschain_check.cpp):
//   trial f runs iff f <= fmax (fmax even, 0 .. 32; 32: every trial, the unbounded rule);
//   trial t = f / 2 with cost D enters the minimum as (D << 8) | t (D < 2^16), so the least D wins, ties to the smallest f; a trial
//   without a candidate, or one that did not run, as RSG_NO_COST; a minimum of RSG_NO_COST: no candidate, the block is given up on --
//   passed on as received, chosen f 255.
FX_RSG_HD inline bool rsg_trial_runs(unsigned f, unsigned fmax) { return f <= fmax; }
FX_RSG_HD inline uint32_t rsg_key(uint32_t cost, unsigned t) { return cost == RSG_NO_COST ? RSG_NO_COST : (cost << 8) | t; }
FX_RSG_HD inline unsigned rsg_chosen(uint32_t best) { return best == RSG_NO_COST ? 255u : 2u * (best & 255u); }
// soft hand-over of one data byte, its eight values as they lie in memory (value b, the byte's bit 7 - b, in bits 8 b .. 8 b + 7 of
// the word): a block with a winner emits 0 / 255 for the winner's byte c, a block given up on its own soft values w unchanged
FX_RSG_HD inline unsigned long long rsg_soft_out(bool accepted, uint8_t c, unsigned long long w)
{
    if (!accepted) return w;
    unsigned long long o = 0;
    for (unsigned b = 0; b < 8; b++) if (c & (0x80u >> b)) o |= 0xFFull << (8 * b);
    return o;
}

// hard byte and reliability rho = min over the bits of |2 s - 255| from a byte's eight soft values (MSB first)
FX_RSG_HD inline void rsg_byte(const uint8_t *s, uint8_t &h, uint8_t &rho)
{
    unsigned v = 0, r = 255;
    for (unsigned bit = 0; bit < 8; bit++) {
        const unsigned x = s[bit], mg = x > 127u ? 2u * x - 255u : 255u - 2u * x;
        v = (v << 1) | (x > 127u ? 1u : 0u); r = mg < r ? mg : r;
    }
    h = (uint8_t)v; rho = (uint8_t)r;
}
