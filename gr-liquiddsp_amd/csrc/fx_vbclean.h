// fx_vbclean.h -- the rate-1/2 K = 7 code inverted word by word: is a frame's coded bit stream, as received, exactly the
// encoding of a message with a zero tail?  If it is, that message is what the Viterbi decoder outputs
// and no trellis has to run.  Shared by fx_vbpre_kernel and the host-side test driver (tests/cpp/vbclean_check.cpp).
//
// Conventions are those of fx_codec.hpp:fec_encode and vb_costs: step t of the trellis is coded bits 2t (poly A = 0x6d) and
// 2t + 1 (poly B = 0x4f), MSB first in bytes; the register holds the last 7 message bits, the newest in bit 0, so
// A = (1 + D^2 + D^3 + D^5 + D^6) u and B = (1 + D + D^2 + D^3 + D^6) u.  The delay-free inverse
//     (D^2 + D^4) A + (1 + D + D^2 + D^3 + D^4) B = u       over GF(2)
// recovers u from the received bits with no recurrence (u_t for t < 0 and received bits before step 0 are zero).
//
// Words: word w is coded bits 64 w .. 64 w + 63 (steps 32 w .. 32 w + 31), read as a big-endian 64-bit value; split into its
// A and B halves, step 32 w + i sits at bit 31 - i.  A delay by d steps is then a right shift by d with the previous word's
// low bits shifted in.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FX_VBC_HD __host__ __device__
#else
#define FX_VBC_HD
#endif

// bits 2i of x -> bit i
FX_VBC_HD inline uint32_t vbc_even_bits(uint64_t x)
{
    x &= 0x5555555555555555ull;
    x = (x | (x >> 1)) & 0x3333333333333333ull;
    x = (x | (x >> 2)) & 0x0F0F0F0F0F0F0F0Full;
    x = (x | (x >> 4)) & 0x00FF00FF00FF00FFull;
    x = (x | (x >> 8)) & 0x0000FFFF0000FFFFull;
    x = (x | (x >> 16)) & 0x00000000FFFFFFFFull;
    return (uint32_t)x;
}
// the word's A bits (coded bits 2t) and B bits (2t + 1)
FX_VBC_HD inline void vbc_split(uint64_t x, uint32_t &a, uint32_t &b) { a = vbc_even_bits(x >> 1); b = vbc_even_bits(x); }
// delay by D steps (1 <= D <= 31): the value each step of cur held D steps earlier, prev the word before
template <int D>
FX_VBC_HD inline uint32_t vbc_delay(uint32_t cur, uint32_t prev) { return (cur >> D) | (prev << (32 - D)); }
// the message bits of a word from its received A / B bits and those of the word before
FX_VBC_HD inline uint32_t vbc_invert(uint32_t a, uint32_t b, uint32_t pa, uint32_t pb)
{
    return vbc_delay<2>(a, pa) ^ vbc_delay<4>(a, pa) ^ b ^ vbc_delay<1>(b, pb) ^ vbc_delay<2>(b, pb) ^ vbc_delay<3>(b, pb) ^ vbc_delay<4>(b, pb);
}
// bits 31 - i of a word for i in [i0, i1), 0 <= i0 <= i1 <= 32
FX_VBC_HD inline uint32_t vbc_span(uint32_t i0, uint32_t i1)
{
    const uint32_t from = i0 >= 32u ? 0u : 0xFFFFFFFFu >> i0, below = i1 >= 32u ? 0u : 0xFFFFFFFFu >> i1;
    return from & ~below;
}

// Word w of a frame of Tn = 8 k + 6 trellis steps (w < (Tn + 31) / 32): x0 is the word, x1 and x2 the two before it (zero
// where w < 1 / w < 2).  Returns the mismatches -- received bits that differ from the re-encoded message, and tail steps
// Tn - 6 .. Tn - 1 whose message bit is not zero -- over the steps below Tn only (bits behind the 2 Tn coded bits, the
// padding of the last byte, are the channel's and are ignored).  u: the word's message bits, step 32 w + i at bit 31 - i.
FX_VBC_HD inline uint32_t vbc_check_word(uint64_t x2, uint64_t x1, uint64_t x0, uint32_t w, uint32_t Tn, uint32_t &u)
{
    uint32_t a2, b2, a1, b1, a0, b0;
    vbc_split(x2, a2, b2); vbc_split(x1, a1, b1); vbc_split(x0, a0, b0);
    const uint32_t u1 = vbc_invert(a1, b1, a2, b2), u0 = vbc_invert(a0, b0, a1, b1);
    const uint32_t d1 = vbc_delay<1>(u0, u1), d2 = vbc_delay<2>(u0, u1), d3 = vbc_delay<3>(u0, u1), d5 = vbc_delay<5>(u0, u1), d6 = vbc_delay<6>(u0, u1);
    const uint32_t ea = u0 ^ d2 ^ d3 ^ d5 ^ d6, eb = u0 ^ d1 ^ d2 ^ d3 ^ d6;
    const uint32_t s0 = 32u * w, n = Tn - s0;                             // steps of this word below Tn (>= 1)
    const uint32_t live = vbc_span(0u, n), t0 = Tn - 6u;
    const uint32_t tail = vbc_span(t0 > s0 ? t0 - s0 : 0u, n < 32u ? n : 32u);
    u = u0;
    return (((ea ^ a0) | (eb ^ b0)) & live) | (u0 & tail);
}

// the bytes of word w of a byte buffer of nbytes (zero past its end), big-endian
FX_VBC_HD inline uint64_t vbc_load_word(const uint8_t *enc, uint32_t nbytes, uint32_t w)
{
    uint64_t x = 0;
    for (uint32_t i = 0; i < 8u; i++) { const uint32_t j = 8u * w + i; x = (x << 8) | (j < nbytes ? enc[j] : 0u); }
    return x;
}

// A whole frame, one word after the other (the kernel spreads the words over a wave's lanes instead): enc holds the
// ceil(2 Tn / 8) coded bytes of a k-byte message.  True if they are a terminated codeword; dec then holds its k bytes.
FX_VBC_HD inline bool vbc_check_frame(const uint8_t *enc, uint32_t k, uint8_t *dec)
{
    const uint32_t Tn = 8u * k + 6u, nbytes = (2u * Tn + 7u) / 8u, nw = (Tn + 31u) / 32u;
    bool ok = true;
    uint64_t x2 = 0, x1 = 0;
    for (uint32_t w = 0; w < nw; w++) {
        const uint64_t x0 = vbc_load_word(enc, nbytes, w);
        uint32_t u;
        ok = ok && vbc_check_word(x2, x1, x0, w, Tn, u) == 0u;
        for (uint32_t q = 0; q < 4u; q++) if (4u * w + q < k) dec[4u * w + q] = (uint8_t)(u >> (24u - 8u * q));
        x2 = x1; x1 = x0;
    }
    return ok;
}
