// rsgmd_check.cpp -- the soft-decision Reed-Solomon trial of the decode kernel (gr-liquiddsp_amd/csrc/fx_rsgmd.h) run serially on
// the host, compiled with g++: tests/test_rs_soft.py compares it with the numpy reference (tests/ref_rs_soft.py).
//   rsgmd_check IN OUT: IN holds uint32 N, uint32 count, then count blocks of 8 N soft values; OUT gets, per block, the N decoded
//   bytes and the chosen f (255: none).
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../../gr-liquiddsp_amd/csrc/fx_rsgmd.h"

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    uint8_t ex[512], lg[256];
    unsigned x = 1;
    for (unsigned i = 0; i < 255; i++) { ex[i] = (uint8_t)x; lg[x] = (uint8_t)i; x <<= 1; if (x & 0x100) x ^= 0x11d; }
    for (unsigned i = 255; i < 512; i++) ex[i] = ex[i - 255];
    lg[0] = 0;
    FILE *fi = std::fopen(argv[1], "rb"); if (!fi) return 2;
    uint32_t hdr[2];
    if (std::fread(hdr, 4, 2, fi) != 2) return 2;
    const unsigned N = hdr[0], count = hdr[1];
    if (N < 33 || N > 255) return 2;
    std::vector<uint8_t> soft((size_t)count * 8 * N), out((size_t)count * (N + 1));
    if (std::fread(soft.data(), 1, soft.size(), fi) != soft.size()) return 2;
    std::fclose(fi);
    for (unsigned blk = 0; blk < count; blk++) {
        const uint8_t *s = soft.data() + (size_t)blk * 8 * N;
        uint8_t h[255], rho[255], era[32], S[32];
        for (unsigned j = 0; j < N; j++) rsg_byte(s + 8 * j, h[j], rho[j]);
        for (unsigned j = 0; j < N; j++) {                                     // rank counting on the keys (rho, j)
            unsigned rank = 0;
            for (unsigned i = 0; i < N; i++) rank += ((unsigned)rho[i] << 8 | i) < ((unsigned)rho[j] << 8 | j);
            if (rank < 32) era[rank] = (uint8_t)j;
        }
        for (unsigned i = 0; i < 32; i++) {
            uint8_t sy = 0;
            for (unsigned j = 0; j < N; j++) sy = (uint8_t)(rsg_mul_log(ex, lg, sy, i + 1) ^ h[j]);
            S[i] = sy;
        }
        RsgTrial best; best.cost = RSG_NO_COST; best.np = 0; unsigned chosen = 255;
        for (unsigned t = 0; t < RSG_TRIALS; t++) {
            RsgTrial tr; rsg_trial(2 * t, N, S, era, s, ex, lg, tr);
            if (tr.cost != RSG_NO_COST && (chosen == 255 || tr.cost < best.cost)) { best = tr; chosen = 2 * t; }
        }
        for (unsigned i = 0; i < best.np && chosen != 255; i++) h[best.pos[i]] ^= best.val[i];
        uint8_t *o = out.data() + (size_t)blk * (N + 1);
        for (unsigned j = 0; j < N; j++) o[j] = h[j];
        o[N] = (uint8_t)chosen;
    }
    FILE *fo = std::fopen(argv[2], "wb"); if (!fo) return 2;
    if (std::fwrite(out.data(), 1, out.size(), fo) != out.size()) return 2;
    std::fclose(fo);
    return 0;
}
