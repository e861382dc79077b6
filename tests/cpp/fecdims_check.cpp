// fecdims_check.cpp -- prints what the frame format's code rules (gr-liquiddsp_amd/csrc/fx_fecdims.h, the one text the
// kernels and the host share) give, compiled host-only with g++: tests/test_fecdims.py compares every line with
// tests/ref_decode.py's own rules and with a count over the reference's puncturing matrices.
//   L <scheme> <n> <fec_enc_len>                        every scheme, n = 0 .. 700 and 65535 + 4
//   B <scheme> <t> <conv_bits_before(t, p)>             the seven convolutional schemes, t = 0 .. 40
//   E <scheme> <n> <conv_bits_before(8 n + 6, p)>       the same schemes, the n of the L lines
//   M <scheme> <p> <pa> <pb>                            their puncturing rows
#include <cstdio>
#include <cstdint>
#include "../../gr-liquiddsp_amd/csrc/fx_fecdims.h"

static const unsigned kSchemes[] = { FX_FEC_NONE, FX_FEC_HAMMING74, FX_FEC_HAMMING84, FX_FEC_HAMMING128, FX_FEC_GOLAY2412, FX_FEC_SECDED2216,
                                     FX_FEC_SECDED3932, FX_FEC_SECDED7264, FX_FEC_CONV_V27, FX_FEC_CONV_V27P23, FX_FEC_CONV_V27P34,
                                     FX_FEC_CONV_V27P45, FX_FEC_CONV_V27P56, FX_FEC_CONV_V27P67, FX_FEC_CONV_V27P78, FX_FEC_RS_M8 };

static void one_n(unsigned fs, unsigned n)
{
    std::printf("L %u %u %u\n", fs, n, fec_enc_len(fs, n));
    const int p = conv_p(fs);
    if (p) std::printf("E %u %u %u\n", fs, n, (unsigned)conv_bits_before(8u * n + 6u, (unsigned)p));
}

int main()
{
    for (unsigned fs : kSchemes) {
        if (!fec_supported(fs)) { std::printf("FAIL scheme %u not supported\n", fs); return 1; }
        for (unsigned n = 0; n <= 700; n++) one_n(fs, n);
        one_n(fs, 65535u + 4u);
        const int p = conv_p(fs);
        if (!p) continue;
        unsigned pa, pb; conv_punct(p, pa, pb);
        std::printf("M %u %d %u %u\n", fs, p, pa, pb);
        for (unsigned t = 0; t <= 40; t++) std::printf("B %u %u %u\n", fs, t, (unsigned)conv_bits_before(t, (unsigned)p));
    }
    return 0;
}
