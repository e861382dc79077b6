// rschain_check.cpp -- the bounded soft-decision Reed-Solomon rule and its soft hand-over as the decode kernel states them
// (gr-liquiddsp_amd/csrc/fx_rsgmd.h: rsg_trial, rsg_trial_runs, rsg_key, rsg_chosen, rsg_soft_out), run serially on the host, compiled
// with g++: tests/test_rs_chain.py compares it with the numpy reference (tests/ref_rs_chain.py).
//   rschain_check IN OUT: IN holds uint32 n, uint32 count, uint32 fmax, uint32 chain, then count packets of 8 fec_enc_len(RS, n) soft
//   values; OUT gets, per packet, the output (chain = 0: n bytes; chain = 1: 8 n soft values) and then one chosen f per block (255: none).
//   As in the kernel's frame path the soft form is written in place, into the packet's own input.
#include <cstdint>
#include <cstdio>
#include <cstring>
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
    uint32_t hdr[4];
    if (std::fread(hdr, 4, 4, fi) != 4) return 2;
    const unsigned n = hdr[0], count = hdr[1], fmax = hdr[2], chain = hdr[3];
    if (n == 0 || n > (1u << 18) || fmax > 32 || (fmax & 1)) return 2;
    const unsigned nb = n <= 223 ? 1u : (n + 222u) / 223u, dl = (n + nb - 1) / nb, N = dl + 32;
    const size_t in_len = (size_t)8 * nb * N, out_len = chain ? (size_t)8 * n : n;
    std::vector<uint8_t> soft(count * in_len), out(count * (out_len + nb));
    if (std::fread(soft.data(), 1, soft.size(), fi) != soft.size()) return 2;
    std::fclose(fi);
    for (unsigned p = 0; p < count; p++) {
        uint8_t *S = soft.data() + p * in_len, *o = out.data() + p * (out_len + nb);
        for (unsigned blk = 0; blk < nb; blk++) {
            const uint8_t *s = S + (size_t)8 * blk * N;
            uint8_t h[255], rho[255], era[32], Sy[32];
            for (unsigned j = 0; j < N; j++) rsg_byte(s + 8 * j, h[j], rho[j]);
            for (unsigned j = 0; j < N; j++) {                                 // rank counting on the keys (rho, j)
                unsigned rank = 0;
                for (unsigned i = 0; i < N; i++) rank += ((unsigned)rho[i] << 8 | i) < ((unsigned)rho[j] << 8 | j);
                if (rank < 32) era[rank] = (uint8_t)j;
            }
            bool dirty = false;
            for (unsigned i = 0; i < 32; i++) {
                uint8_t sy = 0;
                for (unsigned j = 0; j < N; j++) sy = (uint8_t)(rsg_mul_log(ex, lg, sy, i + 1) ^ h[j]);
                Sy[i] = sy; dirty = dirty || sy;
            }
            unsigned chosen = 0;
            if (dirty) {                                                       // (a codeword is its own f = 0 candidate at cost 0)
                RsgTrial win; win.cost = RSG_NO_COST; win.np = 0;
                uint32_t best = RSG_NO_COST;
                for (unsigned t = 0; t < RSG_TRIALS; t++) {
                    if (!rsg_trial_runs(2 * t, fmax)) continue;
                    RsgTrial tr; rsg_trial(2 * t, N, Sy, era, s, ex, lg, tr);
                    const uint32_t key = rsg_key(tr.cost, t);
                    if (key < best) { best = key; win = tr; }
                }
                chosen = rsg_chosen(best);
                for (unsigned i = 0; i < win.np && chosen != 255; i++) h[win.pos[i]] ^= win.val[i];
            }
            const unsigned off = blk * dl, len = off < n ? (n - off < dl ? n - off : dl) : 0;
            if (chain) {
                // in place: block blk's 8 len values go to S + 8 blk dl, at or below its own input and below the next block's
                for (unsigned j = 0; j < len; j++) {
                    unsigned long long w; std::memcpy(&w, s + 8 * (size_t)j, 8);
                    w = rsg_soft_out(chosen != 255, h[j], w);
                    std::memcpy(S + 8 * ((size_t)off + j), &w, 8);
                }
            } else {
                for (unsigned j = 0; j < len; j++) o[off + j] = h[j];
            }
            o[out_len + blk] = (uint8_t)chosen;
        }
        if (chain) std::memcpy(o, S, out_len);
    }
    FILE *fo = std::fopen(argv[2], "wb"); if (!fo) return 2;
    if (std::fwrite(out.data(), 1, out.size(), fo) != out.size()) return 2;
    std::fclose(fo);
    return 0;
}
