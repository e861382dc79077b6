// fx_fecdims.h -- the frame format's code rules: how long a check and each code stage make a packet, which schemes are
// decoded, and how the K = 7 convolutional codes are punctured.  One text for the kernels (fx_device.h), the host's encoder
// and runtime (fx_codec.hpp) and the host-side test driver (tests/cpp/fecdims_check.cpp); tests/ref_decode.py,
// tests/ref_framegen.py and oracle/ keep tables of their own, which these rules are tested against.
//
// Conventions: a message of n bytes runs the K = 7 encoder for T = 8 n + 6 trellis steps (six zero tail bits); step t emits
// generator A (0x6d), then B (0x4f), each only where its puncturing row has a one in column t mod p.
#pragma once
#include <stdint.h>
#include "fx_common.h"          // FX_FEC_* / FX_CRC_*

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FX_FD_HD __host__ __device__
#else
#define FX_FD_HD
#endif

// bytes the check appends to the payload
FX_FD_HD inline unsigned crc_len(unsigned check)
{
    switch (check) {
    case FX_CRC_CHECKSUM: case FX_CRC_8: return 1;
    case FX_CRC_16: return 2;
    case FX_CRC_24: return 3;
    case FX_CRC_32: return 4;
    default: return 0;
    }
}
// puncturing period; 0 = not a K = 7 convolutional scheme
FX_FD_HD inline int conv_p(unsigned fs)
{
    switch (fs) {
    case FX_FEC_CONV_V27: return 1;
    case FX_FEC_CONV_V27P23: return 2;
    case FX_FEC_CONV_V27P34: return 3;
    case FX_FEC_CONV_V27P45: return 4;
    case FX_FEC_CONV_V27P56: return 5;
    case FX_FEC_CONV_V27P67: return 6;
    case FX_FEC_CONV_V27P78: return 7;
    default: return 0;
    }
}
// puncturing rows (A, B) of the code with period p as bit masks over the column: bit c set = the bit is sent at steps t = c mod p
FX_FD_HD inline void conv_punct(int p, unsigned &pa, unsigned &pb)
{
    switch (p) {
    case 2: pa = 0x3; pb = 0x1; break;                 // 11 / 10
    case 3: pa = 0x3; pb = 0x5; break;                 // 110 / 101
    case 4: pa = 0xf; pb = 0x1; break;                 // 1111 / 1000
    case 5: pa = 0xb; pb = 0x15; break;                // 11010 / 10101
    case 6: pa = 0x17; pb = 0x29; break;               // 111010 / 100101
    case 7: pa = 0x2f; pb = 0x51; break;               // 1111010 / 1000101
    default: pa = 0x1; pb = 0x1; break;                // rate 1/2: both, every step
    }
}
// coded bits in front of trellis step t (p >= 2: every step sends one bit, column 0 both)
FX_FD_HD inline uint32_t conv_bits_before(uint32_t t, unsigned p) { return p == 1u ? 2u * t : t + (t + p - 1u) / p; }
// bit-packed block codes: k-bit blocks -> n-bit code words
FX_FD_HD inline bool blk_spec(unsigned fs, unsigned &k, unsigned &n)
{
    switch (fs) {
    case FX_FEC_HAMMING74: k = 4; n = 7; return true;
    case FX_FEC_HAMMING128: k = 8; n = 12; return true;
    case FX_FEC_GOLAY2412: k = 12; n = 24; return true;
    default: k = n = 0; return false;
    }
}
// Reed-Solomon: n message bytes in nb blocks of at most 223, dl message bytes each (the last may hold fewer), 32 parity bytes behind each
FX_FD_HD inline void rs_dims(unsigned n, unsigned &nb, unsigned &dl) { nb = (n + 222) / 223; if (nb == 0) nb = 1; dl = (n + nb - 1) / nb; }
FX_FD_HD inline bool fec_supported(unsigned fs)
{
    unsigned k, n;
    return fs == FX_FEC_NONE || fs == FX_FEC_HAMMING84 || fs == FX_FEC_SECDED7264 || fs == FX_FEC_SECDED2216 ||
           fs == FX_FEC_SECDED3932 || fs == FX_FEC_RS_M8 || blk_spec(fs, k, n) || conv_p(fs) != 0;
}
// bytes one code stage makes of n
FX_FD_HD inline unsigned fec_enc_len(unsigned fs, unsigned n)
{
    const int p = conv_p(fs);
    if (p) return (conv_bits_before(8 * n + 6, (unsigned)p) + 7) / 8;
    unsigned bk, bn;
    if (blk_spec(fs, bk, bn)) { unsigned nb = (8 * n + bk - 1) / bk; return (nb * bn + 7) / 8; }
    if (fs == FX_FEC_RS_M8) { unsigned nb, dl; rs_dims(n, nb, dl); return nb * (dl + 32); }
    if (fs == FX_FEC_SECDED2216) return 3 * (n / 2) + ((n % 2) ? (n % 2) + 1 : 0);
    if (fs == FX_FEC_SECDED3932) return 5 * (n / 4) + ((n % 4) ? (n % 4) + 1 : 0);
    if (fs == FX_FEC_HAMMING84) return 2 * n;
    if (fs == FX_FEC_SECDED7264) return 9 * (n / 8) + ((n % 8) ? (n % 8) + 1 : 0);
    return n;
}
