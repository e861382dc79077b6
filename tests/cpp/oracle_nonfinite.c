/* The oracle's synchroniser and detector over the streams of tests/nonfinite_cases.py (NaN, +-Inf, overflowing and subnormal
 * IQ samples), read from tests/golden/nonfinite_cases.bin.  Built by tests/test_ref_nonfinite.py with
 * -fsanitize=address,undefined,float-cast-overflow: every float -> integer conversion of a poisoned value that does not go through
 * fxr_f2i_sat / fxr_f2ll_sat stops the run.  Prints one line per case: frames delivered (valid headers), detections. */
#include "../../oracle/fxref.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static unsigned g_frames, g_valid;
static int on_frame(unsigned char *header, int header_valid, unsigned char *payload, unsigned payload_len, int payload_valid, fxr_stats st, void *ud)
{
    (void)header; (void)payload; (void)payload_len; (void)payload_valid; (void)st; (void)ud;
    g_frames++; g_valid += header_valid ? 1u : 0u;
    return 0;
}

static uint32_t rd32(FILE *f) { uint32_t v = 0; if (fread(&v, 4, 1, f) != 1) { fprintf(stderr, "short fixture\n"); exit(2); } return v; }

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s nonfinite_cases.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    char magic[4];
    if (!f || fread(magic, 1, 4, f) != 4 || memcmp(magic, "FXNF", 4)) { fprintf(stderr, "bad fixture\n"); return 2; }
    uint32_t nl = rd32(f);
    if (nl > 16) return 2;
    fxr_c32 *base[16]; uint32_t len[16], longest = 0;
    for (uint32_t l = 0; l < nl; l++) {
        len[l] = rd32(f);
        if (len[l] > (1u << 20)) return 2;
        base[l] = (fxr_c32 *)malloc(len[l] * sizeof(fxr_c32));
        if (fread(base[l], sizeof(fxr_c32), len[l], f) != len[l]) return 2;
        if (len[l] > longest) longest = len[l];
    }
    fxr_c32 *x = (fxr_c32 *)malloc(longest * sizeof(fxr_c32));
    fxr_detection *det = (fxr_detection *)malloc(256 * sizeof(fxr_detection));
    uint32_t nc = rd32(f);
    for (uint32_t c = 0; c < nc; c++) {
        uint32_t l = rd32(f), pos = rd32(f), run = rd32(f), which = rd32(f), eq = rd32(f);
        float value, scale;
        if (fread(&value, 4, 1, f) != 1 || fread(&scale, 4, 1, f) != 1 || l >= nl || pos + run > len[l]) return 2;
        for (uint32_t i = 0; i < len[l]; i++) { x[i].re = base[l][i].re * scale; x[i].im = base[l][i].im * scale; }
        for (uint32_t i = pos; i < pos + run; i++) { if (which & 1u) x[i].re = value; if (which & 2u) x[i].im = value; }
        g_frames = g_valid = 0;
        for (int soft = 0; soft < 2; soft++) {
            fxr_sync *q = fxr_sync_create(on_frame, NULL);
            fxr_sync_set_equalizer(q, (int)eq);
            fxr_sync_set_soft(q, soft);
            fxr_sync_execute_chunked(q, x, len[l], 256);
            fxr_sync_destroy(q);
        }
        fxr_qdet *d = fxr_qdet_create_flexframe();
        unsigned nd = fxr_qdet_run(d, x, len[l], 0, det, 256);
        fxr_qdet_destroy(d);
        printf("case %u: %u frames (%u valid headers), %u detections\n", c, g_frames, g_valid, nd);
    }
    for (uint32_t l = 0; l < nl; l++) free(base[l]);
    free(x); free(det); fclose(f);
    printf("%u cases done\n", nc);
    return 0;
}
