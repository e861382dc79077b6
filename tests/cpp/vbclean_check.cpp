// vbclean_check.cpp -- the word-parallel codeword check of the batch Viterbi path (gr-liquiddsp_amd/csrc/fx_vbclean.h)
// against the encoder (fx_codec.hpp:fec_encode, rate 1/2, K = 7), compiled host-only with g++: tests/test_vbclean.py.
// Every clean encoding is accepted with its message recovered; every single-bit error in the 2 Tn coded bits, random
// 2- and 3-bit errors and nonzero tails are rejected; the padding bits behind the coded bits do not matter.
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../gr-liquiddsp_amd/csrc/fx_codec.hpp"
#include "../../gr-liquiddsp_amd/csrc/fx_vbclean.h"

static unsigned long long g_s = 0x243F6A8885A308D3ull;
static unsigned rnd() { g_s ^= g_s << 13; g_s ^= g_s >> 7; g_s ^= g_s << 17; return (unsigned)(g_s >> 32); }
static int g_fail = 0;
#define CHECK(c, ...) do { if (!(c)) { std::printf("FAIL " __VA_ARGS__); std::printf("\n"); if (++g_fail > 20) return; } } while (0)

static void flip(std::vector<uint8_t> &e, unsigned bit) { e[bit >> 3] ^= (uint8_t)(0x80u >> (bit & 7u)); }

// the encoding of k message bytes followed by six tail bits `tail` (0: the encoder's own flush), as fec_encode lays it out
static std::vector<uint8_t> encode_with_tail(const std::vector<uint8_t> &msg, unsigned k, unsigned tail)
{
    const unsigned T = 8 * k + 6, nbytes = (2 * T + 7) / 8;
    std::vector<uint8_t> e(nbytes + 16, 0);
    unsigned sr = 0;
    for (unsigned t = 0; t < T; t++) {
        const unsigned bit = t < 8 * k ? (msg[t >> 3] >> (7 - (t & 7))) & 1u : (tail >> (5 - (t - 8 * k))) & 1u;
        sr = ((sr << 1) | bit) & 0x7f;
        if (__builtin_popcount(sr & 0x6d) & 1) e[(2 * t) >> 3] |= (uint8_t)(0x80u >> ((2 * t) & 7));
        if (__builtin_popcount(sr & 0x4f) & 1) e[(2 * t + 1) >> 3] |= (uint8_t)(0x80u >> ((2 * t + 1) & 7));
    }
    return e;
}

static void one_length(unsigned k, bool all_single)
{
    const unsigned T = 8 * k + 6, nbits = 2 * T, nbytes = (nbits + 7) / 8;
    CHECK(nbytes == fx::fec_enc_len(FX_FEC_CONV_V27, k), "k %u: coded length %u vs %u", k, nbytes, fx::fec_enc_len(FX_FEC_CONV_V27, k));
    std::vector<uint8_t> msg(k), dec(k + 8);
    for (auto &b : msg) b = (uint8_t)rnd();
    std::vector<uint8_t> enc(nbytes + 16, 0);
    fx::fec_encode(FX_FEC_CONV_V27, k, msg.data(), enc.data());
    CHECK(encode_with_tail(msg, k, 0) == enc, "k %u: reference encoder differs from fec_encode", k);
    // clean: accepted, message recovered
    std::memset(dec.data(), 0xA5, dec.size());
    CHECK(vbc_check_frame(enc.data(), k, dec.data()), "k %u: clean encoding rejected", k);
    CHECK(std::memcmp(dec.data(), msg.data(), k) == 0, "k %u: wrong message recovered", k);
    // padding bits behind the coded bits: the channel's, ignored
    if (nbits % 8) {
        std::vector<uint8_t> e = enc;
        e[nbytes - 1] ^= (uint8_t)((1u << (8 - nbits % 8)) - 1u);
        CHECK(vbc_check_frame(e.data(), k, dec.data()) && std::memcmp(dec.data(), msg.data(), k) == 0, "k %u: padding bits flipped -> rejected", k);
    }
    // single-bit errors: all of them, or a sample (and always the first and last few) for long frames
    const unsigned nsingle = all_single ? nbits : 64;
    for (unsigned i = 0; i < nsingle; i++) {
        const unsigned bit = all_single ? i : (i < 16 ? i : (i < 32 ? nbits - 1 - (i - 16) : rnd() % nbits));
        std::vector<uint8_t> e = enc; flip(e, bit);
        CHECK(!vbc_check_frame(e.data(), k, dec.data()), "k %u: single-bit error at %u accepted", k, bit);
    }
    // 2- and 3-bit errors
    for (int r = 0; r < 64; r++) {
        std::vector<uint8_t> e = enc;
        const unsigned nerr = 2 + (r & 1);
        unsigned at[3];
        for (unsigned j = 0; j < nerr; j++) {
            bool dup;
            do { at[j] = rnd() % nbits; dup = false; for (unsigned q = 0; q < j; q++) dup = dup || at[q] == at[j]; } while (dup);
            flip(e, at[j]);
        }
        CHECK(!vbc_check_frame(e.data(), k, dec.data()), "k %u: %u-bit error accepted", k, nerr);
    }
    // a nonzero tail: the received bits are a codeword, but not a terminated one
    for (unsigned tail = 1; tail < 64; tail += (k < 64 ? 1 : 13)) {
        const std::vector<uint8_t> e = encode_with_tail(msg, k, tail);
        CHECK(!vbc_check_frame(e.data(), k, dec.data()), "k %u: tail %02x accepted", k, tail);
    }
}

int main()
{
    unsigned runs = 0;
    for (unsigned k = 1; k <= 2048; k++) {
        one_length(k, k <= 96 || k == 1027);
        runs++;
        if (g_fail) break;
    }
    std::printf("%u lengths, %d failures\n", runs, g_fail);
    return g_fail ? 1 : 0;
}
