// fx_launch.h -- the host-callable launchers of the kernels, one prototype each: included by the translation units that
// define them (fx_kernels.hip, fx_ingest.hip, fx_detwin.hip) and by those that call them (fx_host.cpp, fx_tx.cpp), so that a
// definition that disagrees with what the callers see does not compile.  Declarations only.
#pragma once
#include <hip/hip_runtime.h>
#include "fx_common.h"

struct FxTables;   // fx_device.h

// ---- receive path (fx_host.cpp)
extern "C" hipError_t fx_launch_walk(unsigned mode, int eq, int sh, unsigned njobs, hipStream_t st, const FxWalkJob *jobs, const uint32_t *job_list, FxWalkResult *results,
                                     FxFrame *frames, FxVerifyRun *runs, uint32_t run_cap, FxBlockHdr *hdr, const FxTables *T, int ext, uint32_t n_jobs_total,
                                     const uint32_t *n_list, uint32_t list_cap);
// (the pre-lock scan of the n_spec speculative jobs listed in spec_list: words_per_job chunks each, a workgroup per chunk)
extern "C" hipError_t fx_launch_prescan(hipStream_t st, unsigned n_spec, unsigned words_per_job, const FxWalkJob *jobs, const uint32_t *spec_list, const FxTables *T);
extern "C" hipError_t fx_launch_seekverify(unsigned grid, hipStream_t st, const FxVerifyRun *runs, uint32_t run_cap, const FxWalkJob *jobs, FxWalkResult *results,
                                           FxFrame *frames, FxBlockHdr *hdr, const FxTables *T, uint32_t phase);
extern "C" hipError_t fx_launch_chain(unsigned mode, int eq, int sh, unsigned nstreams, hipStream_t st, const FxStreamDesc *streams, const FxWalkJob *jobs, uint32_t n_jobs_total,
                                      FxWalkResult *results, FxFrame *frames, FxFrame *chain, uint32_t *chain_count, FxVerifyRun *runs, uint32_t run_cap,
                                      FxBlockHdr *hdr, uint32_t force_slow, const FxTables *T);
extern "C" hipError_t fx_launch_hdrdec(int soft, unsigned n, hipStream_t st, const uint8_t *in, uint8_t *out, int32_t *valid, const FxTables *T);
extern "C" hipError_t fx_launch_blkdec(int soft, unsigned fs, unsigned n, unsigned count, hipStream_t st, const uint8_t *in, uint8_t *out, const FxTables *T);
extern "C" hipError_t fx_launch_blksiso(unsigned fs, unsigned n, unsigned count, hipStream_t st, const uint8_t *in, uint8_t *out, const FxTables *T);
extern "C" hipError_t fx_launch_rssoft(unsigned n, unsigned count, hipStream_t st, const uint8_t *in, uint8_t *out, uint8_t *chosen_f, const FxTables *T);
extern "C" hipError_t fx_launch_rschain(unsigned n, unsigned count, unsigned fmax, int chain, hipStream_t st, const uint8_t *in, uint8_t *out, uint8_t *chosen_f, const FxTables *T);
extern "C" hipError_t fx_launch_chainfast(unsigned nstreams, hipStream_t st, const FxStreamDesc *streams, const FxWalkJob *jobs, const FxWalkResult *results,
                                          const FxFrame *frames, FxFrame *chain, uint32_t *chain_count, FxBlockHdr *hdr, uint32_t force_repair,
                                          FxWalkJob *jobs_rw, uint32_t *req_list, uint32_t *stat, uint32_t pass);
// (grid workgroups, clamped; fused: a grid of one takes the one-workgroup kernel, of `threads` threads: 256 or 512)
extern "C" hipError_t fx_launch_plan(hipStream_t st, unsigned grid, int fused, unsigned threads, const FxPlanArgs &a);
extern "C" unsigned fx_plan_ws_words(void);
// (gang launches, fx_common.h: one launch for up to FX_GANG_MAX blocks; members without waves are left out)
extern "C" hipError_t fx_launch_vbpre(const FxVbpreGang *gang, hipStream_t st, const FxTables *T, int clean_on, int early_tail);
extern "C" hipError_t fx_launch_vbitems(unsigned first_item, unsigned n_items, hipStream_t st, const FxPayJob *jobs, const uint32_t *vb_items, uint32_t item_cap,
                                        const FxBlockHdr *hdr, uint8_t *bufA, const uint8_t *bufB, unsigned long long *dwv, uint8_t *vec_arena, uint32_t *vb_st, uint32_t dbg, int packed,
                                        int with_fix);
extern "C" hipError_t fx_launch_vbfinish(unsigned first_wave, unsigned n_waves, hipStream_t st, const FxPayJob *jobs, const uint32_t *job_idx, FxBlockHdr *hdr,
                                         uint8_t *bufA, uint8_t *bufB, unsigned long long *dwv, const uint8_t *vec_arena, const uint32_t *vb_st, uint32_t *fb_list, uint32_t list_cap,
                                         uint8_t *out, FxOutRec *recs, FxBlockHdr *hdr_host, int early_tail);
extern "C" hipError_t fx_launch_paymf(unsigned grid, int eq, hipStream_t st, const FxPayJob *jobs, const uint32_t *blk_job, const uint32_t *blk_c0, const FxBlockHdr *hdr,
                                      const FxFrame *chain, float2 *sym_raw, const FxTables *T);
extern "C" hipError_t fx_launch_paypll(const FxPllGang *gang, const unsigned *grid_waves, unsigned waves_per_wg, hipStream_t st, const FxTables *T);
// (rs_chain: the soft hand-over of soft Reed-Solomon decoding, fxrx_config.soft_rs_chain; its bound on f, soft_rs_fmax, travels in T->rs_fmax)
extern "C" hipError_t fx_launch_paydec(int with_rs, int soft, int soft_rs, int rs_chain, unsigned first_wave, unsigned grid_waves, unsigned waves_per_wg, hipStream_t st, const FxPayJob *jobs,
                                       const uint32_t *job_idx, const FxBlockHdr *hdr, const uint8_t *hard, uint8_t *bufA, uint8_t *bufB, uint8_t *soft_arena,
                                       unsigned long long *dw_arena, uint8_t *out, FxOutRec *recs, FxPayResult *res, const FxTables *T, FxBlockHdr *fallback_host);
extern "C" hipError_t fx_launch_symcopy(unsigned grid, hipStream_t st, const FxBlockHdr *hdr, const float2 *sym, float2 *host);
extern "C" hipError_t fx_launch_upload(hipStream_t st, const void *src, void *dst, size_t bytes, unsigned n_cus);
extern "C" hipError_t fx_launch_ingest(hipStream_t st, int fmt, const void *src, float2 *dst, size_t n, float scale, unsigned n_cus);   // fx_ingest.hip
extern "C" hipError_t fx_launch_detwin(hipStream_t st, unsigned grid, const FxStreamDesc *streams, uint32_t nstreams, const uint32_t *stream_base, const FxPayJob *pjobs,
                                       const FxBlockHdr *hdr, uint32_t first, uint32_t reserved, float2 *out, float2 *out_tail, uint32_t *flag_host, int with_tails,
                                       int skip_tail);   // fx_detwin.hip
extern "C" hipError_t fx_launch_copy_u32(hipStream_t st, const uint32_t *src, uint32_t *dst);
extern "C" hipError_t fx_launch_softdemod(unsigned grid, hipStream_t st, const FxPayJob *jobs, const uint32_t *blk_job, const uint32_t *blk_c0, const FxBlockHdr *hdr,
                                          const float2 *framesyms, const uint8_t *hard, uint8_t *soft_arena, const FxTables *T);

// ---- frame generator, channel and quantiser (fx_tx.cpp)
extern "C" hipError_t fx_launch_txgen(unsigned ntiles, hipStream_t st, const FxTxJob *jobs, const uint32_t *tile_job, const uint32_t *tile_n0,
                                      const uint8_t *head_idx, const uint8_t *pay_idx, const FxTxTables *T, float2 *out);
extern "C" hipError_t fx_launch_txenc(unsigned njobs, hipStream_t st, const FxTxEncJob *jobs, const uint8_t *pay, const uint32_t *perm_arena,
                                      uint8_t *bufA, uint8_t *bufB, uint8_t *pay_idx, const FxTxTables *T);
extern "C" hipError_t fx_launch_channel(hipStream_t st, float2 *x, unsigned n_streams, unsigned long long n_per_stream, const FxChannel *chs, const FxTxTables *T);
extern "C" hipError_t fx_launch_quantize(hipStream_t st, int fmt, const float2 *in, void *out, size_t n, float inv_scale, unsigned long long *saturated,
                                         unsigned n_cus);          // fx_ingest.hip
