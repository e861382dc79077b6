// fx_host.cpp -- host runtime of libfxrx.so: device tables, block descriptors, the stream-ordered kernel chain of a
// block, result marshalling and the C ABI declared in include/fxrx.h.
//
// A block (one fxrx_submit: new samples of every stream) is submitted in three steps (submit_block).  Stage: the block's snapshot of every
// stream, its plan (fx_frontplan.h), a route for every stream's input (fx_ingestplan.h), its descriptors -- on the host, into the block's
// slot.  Reserve: every buffer; a submit that fails fails up to here, the context untouched and nothing enqueued.  Enqueue: ONE chain of
// kernels on the block's own HIP stream, and only then does the context move on; the host never waits between the kernels:
//
//   input (host IQ, integer IQ)         -- a copy and / or fx_upload_kernel / fx_ingest_kernel per stream, into the slot's staging buffers
//   pre-lock scan (flex_rx)             -- fx_prescan_kernel: the first hops of every speculative segment, all at once
//   walkers (speculative segments)      -- fx_walk_kernel, launched at once
//   seek verification, phase 0          -- fx_seekverify_kernel over the runs those walkers emitted (continuing streams only)
//   [wait: chain kernel of the previous block]   -- an event, on the device; from here to the chain kernel a block of
//                                          continuing streams is on the context's high-priority stream
//   true walkers of continuing streams  -- fx_walk_kernel; their start state is read from device memory
//   seek verification (phase 1)         -- the remaining runs
//   chain                               -- fx_chainfast_kernel: stitch / resume state / carried tail, per stream
//   plan                                -- fx_planfused_kernel (or fx_plan_kernel + fx_planlists_kernel): payload jobs, work lists, host result records
//   payload MF -> PLL -> packet decode  -- results land in pinned host memory
//   (detector mode with want_framesyms: fx_detwin_kernel instead -- the detections' aligned windows into pinned host memory)
//
// Slow paths, all at fxrx_collect (repair_and_replay, finish_decode, finish_windows): repair rounds (segments walked again in parallel:
// hand-off misses, fired skipped hops), the full-size fx_chain_kernel, a whole-block walk without hop skipping, carry
// buffers that have to grow, decode launches that the hint-sized grids did not cover, windows beyond the reserved slots.
//
// Why segments: liquid's synchroniser is one sequential state machine per stream (where the detector restarts after a
// frame depends on that frame's header).  Each stream is cut into segments that are walked concurrently from a
// freshly-reset detector; a segment's walker, once past its end, keeps seeking until its next detection (a, cfo_bin) --
// the hand-off target.  If the next segment's speculative list contains that same (a, cfo_bin), everything after it is
// provably what the sequential machine would have produced, so the lists are spliced; otherwise that segment is walked
// again from the true state.  The result is identical to a single sequential walk, for any segment size.
//
// What carries a stream from block to block lives on the device: FxStreamState (resume hop, zero-floor, freshness) in a
// ring indexed by block number, and the unconsumed tail, right-aligned in one of three carry buffers per stream (block b
// reads buffer b mod 3 and writes (b+1) mod 3).  The host learns both at fxrx_collect.  The one thing the device cannot
// do is grow a carry buffer: a tail longer than the buffer marks the state invalid, every block behind it exits at once,
// and fxrx_collect of the overflowing block enlarges the buffers, copies the tail itself and enqueues the blocks behind
// it again ("replay"; their inputs are still there: input buffers stay valid until their block is collected).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>
#include "../../include/fxrx.h"
#include "fx_device.h"
#include "fx_codec.hpp"
#include "fx_launch.h"
#include "fx_traffic.h"
#include "fx_frontplan.h"
#include "fx_ingestplan.h"

namespace {

thread_local std::string g_err;
void set_err(const std::string &s) { g_err = s; }

#define HIP_OK(expr)                                                                          \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess) {                                                               \
            set_err(std::string(#expr) + ": " + hipGetErrorString(e_));                       \
            return FXRX_ERR_HIP;                                                              \
        }                                                                                     \
    } while (0)

// growable device / pinned-host buffers (contents are NOT preserved across a growth)
template <class T> struct DevBuf {
    T *p = nullptr; size_t cap = 0;
    int reserve(size_t n)
    {
        if (n <= cap) return 0;
        size_t nc = std::max(n, cap + cap / 2);
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
        if (hipMalloc((void **)&p, nc * sizeof(T)) != hipSuccess) { set_err("hipMalloc failed"); return FXRX_ERR_HIP; }
        cap = nc; return 0;
    }
    ~DevBuf() { if (p) (void)hipFree(p); }
};
template <class T> struct PinBuf {
    T *p = nullptr; size_t cap = 0;
    int reserve(size_t n)
    {
        if (n <= cap) return 0;
        size_t nc = std::max(n, cap + cap / 2);
        if (p) (void)hipHostFree(p);
        p = nullptr; cap = 0;
        if (hipHostMalloc((void **)&p, nc * sizeof(T), hipHostMallocDefault) != hipSuccess) { set_err("hipHostMalloc failed"); return FXRX_ERR_HIP; }
        cap = nc; return 0;
    }
    // grow to n elements and keep the first `keep` of what is there
    int grow_keep(size_t n, size_t keep)
    {
        if (n <= cap) return 0;
        T *np = nullptr;
        if (hipHostMalloc((void **)&np, n * sizeof(T), hipHostMallocDefault) != hipSuccess) { set_err("hipHostMalloc failed"); return FXRX_ERR_HIP; }
        if (p) { std::memcpy(np, p, std::min(keep, cap) * sizeof(T)); (void)hipHostFree(p); }
        p = np; cap = n; return 0;
    }
    ~PinBuf() { if (p) (void)hipHostFree(p); }
};

// is p page-locked host memory the device can read, and at which address?
static bool pinned_device_ptr(const void *p, const void **dev)
{
    if (!p) return false;
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }     // (pageable memory: not an error here)
    if (a.type != hipMemoryTypeHost || !a.devicePointer) return false;
    *dev = a.devicePointer;
    return true;
}
constexpr unsigned kMaxDepth = 32;
constexpr unsigned kStateRing = kMaxDepth + 3;      // FxStreamState records per stream: one per block in flight and then some

struct StreamState {
    float2 *carry[3] = { nullptr, nullptr, nullptr };   // tails, right-aligned: block b reads carry[b % 3], writes carry[(b + 1) % 3]
    int64_t carry_cap = 0;                  // samples per buffer
    int64_t total = 0;                      // absolute index of the next new sample (since the last reset)
    bool fresh_start = true;                // the next block starts from a freshly reset synchroniser (no state to read)
    int64_t carry_bound = 0;                // upper bound of the tail the next block will find (sizes its arenas)
    unsigned noskip_left = 0;               // blocks this stream is still walked with the exact detector on every hop (a skipped hop fired recently; survives a reset)
};

// new samples of one stream on their way into the slot's float staging buffer, in front of the block's chain (fx_ingestplan.h).
// src: where the route's first step reads -- the caller's pointer, or its device-visible address where a kernel reads host memory
struct IngestJob { unsigned stream = 0; IngestRoute route = kRouteNone; const void *src = nullptr; uint64_t n = 0; };

// what a block needs to know about a stream at submit time (kept for a replay)
struct StreamSnap { int64_t tot0 = 0; bool fresh_start = true; int64_t carry_bound = 0; bool noskip = false; };

}  // namespace

struct Out { fxrx_frame f; };

// Slot::ev, the stage events of a block.  Start (in front of the walkers), Walk, Verify, Plan and Dec are recorded at timing level 2 only, Pll from level 1 on
// (fxrx_set_timing: the stage times are their differences); the others always.  Chain, behind the chain kernel: the next block's chain kernel waits for it
// (prev_chain).  Mf, behind the payload matched filter (detector mode: the window kernel), the last reader of the carried tail: the chain kernel of the next block
// but one waits for it (carry_reader), and so does the gang that holds the block's tail.  Done: the block's last event, which fxrx_collect waits for (not recorded
// while the tail is deferred).  Handover, behind the speculative walkers of a block with continuing streams: the context's high-priority chain stream waits for it.
enum StageEv { kEvStart = 0, kEvWalk, kEvVerify, kEvChain, kEvPlan, kEvMf, kEvPll, kEvDec, kEvDone, kEvHandover, kEvCount };
enum DecList { kDecPlain = 0, kDecRs, kDecBatch, kDecFallback, kDecLists };     // the four quarters of Slot::d_dec_list, list_cap() entries each

// One block in flight: descriptors, device tables, arenas, result buffers and its own HIP stream.
struct Slot {
    hipStream_t st = nullptr;
    hipEvent_t ev[kEvCount] = {};            // indexed by StageEv
    unsigned index = 0;
    bool busy = false;
    uint64_t seq = 0;                        // block number since context creation
    // the input, as submitted (kept for a replay)
    std::vector<const float2 *> x; std::vector<uint64_t> n; std::vector<StreamSnap> snap;
    std::vector<DevBuf<float2>> d_in;        // staging of host inputs (and of integer inputs, host or device, after their conversion)
    std::vector<DevBuf<uint8_t>> d_raw;      // integer IQ that reaches the device through the copy engines (pageable memory, very large blocks)
    std::vector<IngestJob> ingest; int ingest_fmt = FXRX_IQ_FC32; float ingest_scale = 0.0f;   // uploads and conversions enqueue_front still has to launch
    // descriptor arena, one upload: [FxWalkJob x NJ | job lists | FxStreamDesc x NS]
    PinBuf<uint8_t> hp_desc; DevBuf<uint8_t> d_desc;
    size_t NJ = 0, n_early = 0, n_late = 0, o_list = 0, o_streams = 0;
    // device tables
    DevBuf<FxWalkResult> d_wres; DevBuf<FxFrame> d_frames, d_chain; DevBuf<FxVerifyRun> d_runs;
    DevBuf<FxBlockHdr> d_hdr;                // [0] walk-phase counters (zero between blocks), [1] what the payload kernels read
    DevBuf<uint32_t> d_chain_count, d_stream_base, d_mf_job, d_mf_c0, d_pll_list, d_dec_list, d_vb_items;
    DevBuf<uint32_t> d_plan_ws;              // plan kernels: look-back state, list counts and cursors (zero between blocks)
    DevBuf<uint32_t> d_req;                  // repair rounds: segments to be walked again from their true start state
    DevBuf<uint32_t> d_prescan;              // pre-lock scan: chunk words of the speculative jobs (ps_words each), written by fx_prescan_kernel in front of the walkers
    uint32_t ps_jobs = 0, ps_words = 0, ps_hops = 0, ps_taken = 0, ps_fallback = 0;   // jobs scanned / chunks and hops per job; fxrx_debug_prescan_stats
    DevBuf<uint32_t> d_cstat;                // in-chain repair round: per stream 1 stitched | 2 pending (segments queued) | 3 left to fxrx_collect
    DevBuf<uint8_t> d_vb_vec;                // batch Viterbi: metric differences at the start and end of every trellis block
    DevBuf<unsigned long long> d_vb_dw;      // its decision words, step-major within the 64 work items of a wave
    DevBuf<uint32_t> d_vb_st;                // traceback states and flags per work item
    uint32_t vb_cap = 0, vb_blk = 0;
    uint64_t vb_dw_words = 0, vb_slots_alloc = 128;
    DevBuf<FxPayJob> d_pjobs; DevBuf<FxPayResult> d_pres;
    uint32_t run_cap = 0, chain_cap = 0, mf_cap = 0, frame_slots = 0;
    uint64_t sym_cap = 0, byte_cap = 0, dw_cap = 0, out_cap = 0;
    // payload arenas
    DevBuf<float2> d_symraw;                 // matched-filter output; the PLL overwrites it in place with the carrier-recovered symbols
    DevBuf<uint8_t> d_hard, d_bufA, d_bufB, d_soft; DevBuf<unsigned long long> d_dw;
    // results (pinned host memory the kernels write into)
    PinBuf<FxBlockHdr> h_hdr; PinBuf<FxOutRec> h_recs; PinBuf<uint8_t> h_out, h_soft; PinBuf<float2> h_framesyms;
    // detector mode with want_framesyms: the detections' aligned windows, 512 samples (4096 bytes) a slot.  h_win: slot i = record i, for the
    // win_reserved records the block was sized for (and, once finish_windows has grown it, for all of them); h_wintail: slot 2 s + k = record k
    // of stream s where that record lies beyond the reservation and starts in the carried tail; h_winflag: a third such record turned up
    PinBuf<float2> h_win, h_wintail; PinBuf<uint32_t> h_winflag; uint32_t win_reserved = 0;
    std::vector<Out> out;
    uint64_t n_syms = 0;
    fxrx_timing timing{};
    double host_submit_ms = 0.0;
    bool any_late = false;
    double dbg_submit_ms = 0.0, dbg_collect_ms = 0.0, dbg_gpu_start_ms = 0.0, dbg_gpu_done_ms = 0.0;   // fxrx_debug_block_times
    bool force_noskip = false;               // walk this block with the exact detector on every hop (nothing to verify)
    int timing_level = 0;                    // which stage events this block recorded (fxrx_set_timing)
    bool inchain = false;                    // the repair round within the chain was enqueued with it
    uint32_t kept_hops = 0, kept_cheap = 0, kept_vhops = 0, kept_vfail = 0, kept_repairs = 0;   // walk-phase counters of a block whose back part was run again
    // the block's tail -- everything behind the payload matched filter: PLL, decode launches, symbol copy, ev[kEvPll .. kEvDone] --, whose grids are
    // fixed when the block is submitted; the launches themselves may wait in the context's open gang (launch_tails)
    TailPlan tail;
    bool tail_launched = true;               // false: deferred -- ev[kEvDone] has not been recorded for this block, nobody may wait for it
    hipStream_t tail_st = nullptr;           // the stream the tail went to (a gang's: its last member's)
    // views of the arenas: nothing is allocated or kept (jobs_rw: the chain kernel rewrites the jobs of the segments it queues for repair)
    uint32_t list_cap() const { return chain_cap + 64 * FX_PLL_CLASSES; }      // entries of d_pll_list and of each quarter of d_dec_list
    uint32_t *dec_list(DecList which) const { return d_dec_list.p + (size_t)which * list_cap(); }
    FxBlockHdr *hdr_walk() const { return d_hdr.p; } FxBlockHdr *hdr_pay() const { return d_hdr.p + 1; }
    const FxWalkJob *jobs() const { return reinterpret_cast<const FxWalkJob *>(d_desc.p); } FxWalkJob *jobs_rw() const { return reinterpret_cast<FxWalkJob *>(d_desc.p); }
    const uint32_t *job_list() const { return reinterpret_cast<const uint32_t *>(d_desc.p + o_list); } const FxStreamDesc *streams() const { return reinterpret_cast<const FxStreamDesc *>(d_desc.p + o_streams); }
#ifdef FX_STAMPS
    FxPayResult *pres() const { return d_pres.p; }      // decode-phase clocks per frame: diagnostic builds only
#else
    FxPayResult *pres() const { return nullptr; }
#endif
};

struct fxrx_ctx_s {
    fxrx_config cfg{};
    FxTables *d_tables = nullptr;
    std::vector<StreamState> st;
    FxStreamState *d_state = nullptr; FxStreamState *h_state = nullptr;   // [kStateRing][n_streams], device / pinned mirror
    float taper = -1.0f;                 // FXRX_TAPER: segment lengths of a stream fall from (1 + t) to (1 - t) times the mean (-1: chosen per block)
    bool skip_seek = true;               // FXRX_SKIP_SEEK=0: walkers run the full detector on every hop (nothing to verify)
    bool chain_slow = false;             // FXRX_CHAIN_SLOW=1: every block goes through the full-size chain kernel's general (sequential) path
    unsigned pll_waves = 1, dec_waves = 1;   // waves per workgroup of the PLL / decode grids (placement only)
    int n_cus = 256;
    uint64_t seq = 0;                    // blocks submitted so far
    hipEvent_t prev_chain = nullptr;     // chain kernel of the newest submitted block (borrowed from its slot)
    hipEvent_t carry_reader[3] = { nullptr, nullptr, nullptr };   // payload MF of the newest block that reads carry[i]
    Traffic traffic;                     // what the last collected block held: sizes the next blocks' grids and arenas (fx_traffic.h)
    bool batch_viterbi = true;           // FXRX_BATCH_VITERBI=0: every frame through the wave-per-frame decoder
    bool vb_clean = true;                // FXRX_VB_CLEAN=0: no codeword check in fx_vbpre_kernel, every batch-path frame runs the trellis
    // The repair round within the chain costs two launches per block -- and launches are what the pipeline is short of (DESIGN.md
    // section 6) --, so it is only enqueued while blocks keep needing it: for the next 16 blocks after one that did.
    // FXRX_INCHAIN_REPAIR=0: never, 1: while needed (default), 2: always.
    int inchain_repair = 1; unsigned inchain_left = 0;
    bool plan_fused = true;              // FXRX_PLAN_FUSED=0: the plan stage is two launches even when one workgroup plans the block
    unsigned plan_threads = 512;         // FXRX_PLAN_THREADS: width of the one-workgroup plan kernel, 256 / 512 (anything else: this default)
    // FXRX_VB_EARLY_TAIL=0: the tail of clean frames runs in fx_vbfinish_kernel and the trellis kernels are launched with every block.
    // Otherwise fx_vbpre_kernel finishes clean frames, and the trellis kernels join the chain only while frames that need them keep turning
    // up (Traffic::trellis_left).  A block that meets one without them is completed when it is collected.
    bool vb_early_tail = true;
    int timing_level = -1;               // stage events per block: -1 auto (all stages one block at a time, none with blocks in flight) | 0 none | 1 the PLL only | 2 all stages
    hipEvent_t ref_event = nullptr; double ref_host_ms = 0.0;   // fxrx_debug_block_times: a common origin of GPU and host clocks
    int debug_walk_twice = 0;            // FXRX_DEBUG_WALK_TWICE: the speculative walkers are launched twice, the stage time is the second launch's (cold-start experiment)
    int debug_stop_after = 0;            // FXRX_DEBUG_STOP_AFTER (tools/dev/dev_stage_cost.py): 4 plan | 5 matched filter | 6 PLL -- the chain ends there, no results
    uint32_t walk_per_cu = 2;            // walker workgroups resident per CU (FXRX_WALK_PER_CU; follows the kernel's register budget)
    hipStream_t st_chain = nullptr;      // highest priority: the state-dependent stretch of continuing blocks (true walkers, their verification, chain kernel)
    uint32_t verify_per_cu = 4;          // FXRX_VERIFY_PER_CU: workgroups of the seek verifier per CU (they stride over the runs)
    uint32_t mf_per_cu = 0;              // FXRX_MF_PER_CU: workgroups of the payload matched filter per CU (0: one per item of the last block)
    uint32_t plan_grid = 0;              // FXRX_PLAN_GRID: workgroups of the plan kernels (tests; default: from the last block's frame count)
    uint32_t vb_debug = 0, vb_blk_force = 0;   // tests: FXRX_VB_DEBUG (see fx_vbfix_kernel / fx_vbtrace_kernel), FXRX_VB_BLK (trellis steps per block)
    // pipeline: a ring of depth + 1 slots, so that the block whose results are exposed is never the one being refilled
    std::vector<std::unique_ptr<Slot>> slots; unsigned depth = 1, head = 0, tail = 0, inflight = 0;
    Slot *last = nullptr;                // slot whose results are currently exposed through fxrx_result
    uint64_t replays = 0, repairs_host = 0, late_decodes = 0;
    uint64_t late_reason[6] = {};        // fxrx_debug_late_stats: collected blocks finish_decode acted on, per reason (a block may count under several)
    uint64_t late_windows = 0;           // blocks whose aligned windows had to be completed at collect (more detections than slots were reserved)
    uint32_t detwin_reserve = 0;         // FXRX_DETWIN_RESERVE (tests): window slots reserved per block instead of the last block's count plus a margin
    unsigned noskip_left = 0;            // blocks still to be walked with the exact detector on every hop (after a verification failure)
    unsigned debug_fail_submit = 0, debug_fail_collect = 0;   // tests (fxrx_debug_fail): the next n submits / collects report a failure
    uint64_t discarded = 0;              // blocks dropped by a failing fxrx_collect (see discard_inflight)
    IngestLimits ingest_limits;          // sizes up to which a kernel reads page-locked host IQ itself (FXRX_INGEST_KERNEL_MAX: the integer formats')
    float iq_scale[3] = { 1.0f, 1.0f / 32768.0f, 1.0f / 128.0f };   // fxrx_set_iq_scale, indexed by FXRX_IQ_*
    // FXRX_TAIL_GANG: tails per gang launch (1: off; at most FX_GANG_MAX).  The PLL and fx_vbpre_kernel hold a hardware queue for as
    // long with one block's frames as with four blocks', and queue time is what bounds the pipeline.
    unsigned tail_gang = 4;
    // FXRX_PRESCAN=1: the first hops of every speculative segment are scanned by fx_prescan_kernel ahead of the walkers (default 0: the
    // walkers scan for their first preamble themselves -- measured faster on config 2, the extra launch costs more than the walkers
    // save).  FXRX_PRESCAN_HOPS: hops scanned per speculative job instead of the traffic's figure (0: none).
    bool prescan = false; int prescan_hops = -1;
    std::vector<Slot *> gang;            // the open gang: blocks in flight whose tails are deferred, oldest first
    uint64_t gang_launches = 0, gang_members = 0;   // fxrx_debug_gang_stats: tail launches that carried more than one block / the blocks they carried
};

namespace {

std::unique_ptr<FxTables> make_tables()
{
    const fx::HostTables &H = fx::host_tables();
    const fx::BlockCodes &B = fx::block_codes();
    std::unique_ptr<FxTables> t(new FxTables);
    std::memset(t.get(), 0, sizeof(FxTables));
    for (int i = 0; i < 512; i++) { t->tw[i] = make_float2(H.tw[i].re, H.tw[i].im); t->S[i] = make_float2(H.S[i].re, H.S[i].im); }
    for (int i = 0; i < 1024; i++) t->sc[i] = make_float2(H.sc[i].re, H.sc[i].im);
    for (int i = 0; i < FX_S_LEN; i++) t->s[i] = make_float2(H.s[i].re, H.s[i].im);
    for (int i = 0; i < FX_HDR_PILOTS; i++) t->pilots[i] = make_float2(H.pilots[i].re, H.pilots[i].im);
    for (int i = 0; i < FX_PN_LEN; i++) t->pn[i] = make_float2(H.pn[i].re, H.pn[i].im);
    fx::design_eq_init(t->eq0);
    std::memcpy(t->proto, H.proto, sizeof H.proto);
    t->s2sum = H.s2sum;
    {   // differential template for the speculative walkers' coarse scan
        fx::cf td[512]; std::memset(td, 0, sizeof td);
        float e = 0.0f, mr = 0.0f, mi = 0.0f;
        const int nd = FX_S_LEN - 1;
        for (int k = 0; k < nd; k++) {
            td[k].re = H.s[k + 1].re * H.s[k].re + H.s[k + 1].im * H.s[k].im;
            td[k].im = H.s[k + 1].im * H.s[k].re - H.s[k + 1].re * H.s[k].im;
            mr += td[k].re; mi += td[k].im;
        }
        mr /= (float)nd; mi /= (float)nd;                       // zero-mean over its support (see the kernel)
        for (int k = 0; k < nd; k++) { td[k].re -= mr; td[k].im -= mi; e += td[k].re * td[k].re + td[k].im * td[k].im; }
        fx::cf TD[512]; fx::hfft::fft512(td, TD, H.tw);
        for (int i = 0; i < 512; i++) t->TD[i] = make_float2(TD[i].re, TD[i].im);
        t->td2sum = e;
    }
    for (size_t i = 0; i < H.perm54.size(); i++) t->perm54[i] = (uint16_t)H.perm54[i];
    for (size_t i = 0; i < H.perm27.size(); i++) t->perm27[i] = (uint16_t)H.perm27[i];
    std::memcpy(t->h84dec, B.h84_dec, 256); std::memcpy(t->h84enc, B.h84_enc, 16); std::memcpy(t->sdcol, B.sd_col, 64);
    std::memcpy(t->sd22col, B.sd22_col, 16); std::memcpy(t->sd39col, B.sd39_col, 32);
    std::memcpy(t->h74dec, B.h74_dec, 128); std::memcpy(t->h128dec, B.h128_dec, 4096);
    std::memcpy(t->golenc, B.gol_enc, sizeof B.gol_enc); std::memcpy(t->golerr, B.gol_err, sizeof B.gol_err);
    std::memcpy(t->rsexp, B.rs_exp, 512); std::memcpy(t->rslog, B.rs_log, 256);
    for (int d = 0; d < 16; d++) t->h74enc[d] = B.h74_enc[d];
    for (int d = 0; d < 256; d++) t->h128enc[d] = B.h128_enc[d];
    {   // SECDED: syndrome -> data column + 1 (the columns are distinct and of weight 3 or 5)
        const uint8_t *cols[3] = { B.sd22_col, B.sd39_col, B.sd_col };
        const unsigned ncol[3] = { 16, 32, 64 };
        for (int c = 0; c < 3; c++) for (unsigned j = 0; j < ncol[c]; j++) t->sdinv[c][cols[c][j]] = (uint8_t)(j + 1);
    }
    return t;
}

int upload_tables(fxrx_ctx_s *c)
{
    std::unique_ptr<FxTables> t = make_tables();
    t->rs_fmax = c->cfg.soft_rs_fmax ? (uint32_t)c->cfg.soft_rs_fmax - 1u : 32u;      // (fxrx_create has checked the value)
    HIP_OK(hipMalloc((void **)&c->d_tables, sizeof(FxTables)));
    HIP_OK(hipMemcpy(c->d_tables, t.get(), sizeof(FxTables), hipMemcpyHostToDevice));
    return 0;
}

int alloc_carry(StreamState &S, int64_t cap)
{
    for (auto &p : S.carry) {
        if (p) (void)hipFree(p);
        p = nullptr;
        if (hipMalloc((void **)&p, (size_t)cap * sizeof(float2)) != hipSuccess) { set_err("hipMalloc (carry buffer) failed"); return FXRX_ERR_HIP; }
    }
    S.carry_cap = cap;
    return 0;
}

// the codes the decode kernel's block decoders take (fxrx_debug_block_decode, fxrx_debug_block_siso)
bool is_block_fec(unsigned fec)
{
    return fec == FX_FEC_HAMMING74 || fec == FX_FEC_HAMMING84 || fec == FX_FEC_HAMMING128 || fec == FX_FEC_GOLAY2412 ||
           fec == FX_FEC_SECDED2216 || fec == FX_FEC_SECDED3932 || fec == FX_FEC_SECDED7264;
}

// the longest packet the fxrx_debug_* decoders take: a stage's message is up to fec0's output for a 65535-byte payload and its CRC,
// 131 080 bytes behind a rate-1/2 code; the kernels index in 32 bits up to 2^29 bytes
constexpr unsigned kDebugMaxN = 1u << 18;

// What the fxrx_debug_* decoders share: tables and input up, launch(d_in, d_out, d_out2, d_tables) on the null stream, outputs
// back, everything freed on every path.  who: the entry point, for the error message; in_pad: spare bytes behind the input;
// out2: a second output, or null.
template <class Launch>
int debug_decode(const char *who, const uint8_t *in, size_t in_bytes, size_t in_pad, void *out, size_t out_bytes, void *out2, size_t out2_bytes,
                        Launch launch)
{
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || nd <= 0) { set_err(std::string(who) + ": no usable HIP device"); return FXRX_ERR_NODEVICE; }
    std::unique_ptr<FxTables> t = make_tables();
    FxTables *d_t = nullptr; uint8_t *d_in = nullptr, *d_out = nullptr, *d_out2 = nullptr;
    auto run = [&]() -> int {
        HIP_OK(hipMalloc((void **)&d_t, sizeof(FxTables)));
        HIP_OK(hipMalloc((void **)&d_in, in_bytes + in_pad));
        HIP_OK(hipMalloc((void **)&d_out, out_bytes));
        if (out2) HIP_OK(hipMalloc((void **)&d_out2, out2_bytes));
        HIP_OK(hipMemcpy(d_t, t.get(), sizeof(FxTables), hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(d_in, in, in_bytes, hipMemcpyHostToDevice));
        HIP_OK(launch(d_in, d_out, d_out2, d_t));
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipMemcpy(out, d_out, out_bytes, hipMemcpyDeviceToHost));
        if (out2) HIP_OK(hipMemcpy(out2, d_out2, out2_bytes, hipMemcpyDeviceToHost));
        return 0;
    };
    const int rc = run();
    for (void *p : { (void *)d_t, (void *)d_in, (void *)d_out, (void *)d_out2 }) if (p) (void)hipFree(p);
    return rc;
}

}  // namespace

// HIP multiplexes streams onto GPU_MAX_HW_QUEUES hardware queues (4 unless told otherwise) and streams sharing a queue
// serialise; the pipeline wants one queue per block in flight.  The runtime reads the variable when it initialises, so
// this only helps when the library is loaded before the first HIP call.  An existing value is never overridden.
__attribute__((constructor)) static void fxrx_default_hw_queues() { setenv("GPU_MAX_HW_QUEUES", "16", 0); }

// ============================================================================ batched API
extern "C" {

const char *fxrx_last_error(void) { return g_err.c_str(); }
void fxrx_set_error(const char *msg) { set_err(msg ? msg : ""); }      // for the library's other translation units
const char *fxrx_version(void) { return "fxrx 0.2 (gfx950)"; }
int fxrx_device_count(void) { int n = 0; if (hipGetDeviceCount(&n) != hipSuccess) return 0; return n; }
// page-locked host memory: uploads from it are asynchronous (fxrx_submit returns while the copy is still under way)
void *fxrx_pinned_alloc(size_t bytes)
{
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) { set_err("fxrx_pinned_alloc: hipHostMalloc failed"); return nullptr; }
    return p;
}
void fxrx_pinned_free(void *p) { if (p) (void)hipHostFree(p); }

static int make_slot(fxrx_ctx_s *c)
{
    std::unique_ptr<Slot> s(new Slot);
    HIP_OK(hipStreamCreateWithFlags(&s->st, hipStreamNonBlocking));
    for (auto &e : s->ev) HIP_OK(hipEventCreate(&e));
    s->index = (unsigned)c->slots.size();
    if (s->h_hdr.reserve(1) || s->d_hdr.reserve(2) || s->d_plan_ws.reserve(fx_plan_ws_words())) return FXRX_ERR_HIP;
    std::memset(s->h_hdr.p, 0, sizeof(FxBlockHdr));
    HIP_OK(hipMemset(s->d_hdr.p, 0, 2 * sizeof(FxBlockHdr)));     // (fx_plan_kernel zeroes the counters again after every block)
    HIP_OK(hipMemset(s->d_plan_ws.p, 0, fx_plan_ws_words() * sizeof(uint32_t)));     // (the plan kernels leave their workspace zero)
    c->slots.push_back(std::move(s));
    return 0;
}

static int close_gang(fxrx_ctx_s *c);
static void sync_all(fxrx_ctx_s *c) { if (c->st_chain) (void)hipStreamSynchronize(c->st_chain); for (auto &s : c->slots) if (s->st) (void)hipStreamSynchronize(s->st); }

// FXRX_DEBUG_SUBMIT_PROFILE: where the host time of fxrx_submit goes (printed when a context is destroyed)
static double g_prof[8]; static unsigned long g_prof_n;
static const bool g_prof_on = std::getenv("FXRX_DEBUG_SUBMIT_PROFILE") != nullptr;
static inline double prof_now() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
void fxrx_destroy(fxrx_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->cfg.device);
    (void)close_gang(c);
    sync_all(c);
    if (g_prof_on && g_prof_n) {
        std::fprintf(stderr, "[fxrx] submit profile over %lu blocks (ms per block): input routes + bookkeeping %.4f, segments %.4f, memory + descriptors %.4f, front launches %.4f, back launches %.4f\n",
                     g_prof_n, g_prof[0] / g_prof_n, g_prof[1] / g_prof_n, g_prof[2] / g_prof_n, g_prof[3] / g_prof_n, g_prof[4] / g_prof_n);
        for (auto &v : g_prof) v = 0.0; g_prof_n = 0;
    }
    for (auto &s : c->slots) {
        for (auto e : s->ev) if (e) (void)hipEventDestroy(e);
        if (s->st) (void)hipStreamDestroy(s->st);
    }
    if (c->st_chain) { (void)hipStreamSynchronize(c->st_chain); (void)hipStreamDestroy(c->st_chain); }
    if (c->ref_event) (void)hipEventDestroy(c->ref_event);
    for (auto &S : c->st) for (auto &p : S.carry) if (p) (void)hipFree(p);
    if (c->d_tables) (void)hipFree(c->d_tables);
    if (c->d_state) (void)hipFree(c->d_state);
    if (c->h_state) (void)hipHostFree(c->h_state);
    delete c;
}

fxrx_ctx *fxrx_create(const fxrx_config *cfg)
{
    if (!cfg || cfg->n_streams == 0) { set_err("fxrx_create: bad config"); return nullptr; }
    if (cfg->threshold != cfg->threshold) { set_err("fxrx_create: threshold is NaN (FXRX_ERR_ARG)"); return nullptr; }
    if (cfg->mode == FXRX_MODE_DETECTOR && cfg->soft_header) { set_err("fxrx_create: soft_header needs flex_rx mode (FXRX_ERR_ARG)"); return nullptr; }
    if (cfg->soft_block && (cfg->mode == FXRX_MODE_DETECTOR || !cfg->soft_decision)) {
        set_err("fxrx_create: soft_block needs soft_decision and flex_rx mode (FXRX_ERR_ARG)"); return nullptr;
    }
    if (cfg->soft_chain && (cfg->mode == FXRX_MODE_DETECTOR || !cfg->soft_decision || !cfg->soft_block)) {
        set_err("fxrx_create: soft_chain needs soft_block, soft_decision and flex_rx mode (FXRX_ERR_ARG)"); return nullptr;
    }
    if (cfg->soft_rs && (cfg->mode == FXRX_MODE_DETECTOR || !cfg->soft_decision)) {
        set_err("fxrx_create: soft_rs needs soft_decision and flex_rx mode (FXRX_ERR_ARG)"); return nullptr;
    }
    if (cfg->soft_rs_fmax && (cfg->soft_rs_fmax < 0 || cfg->soft_rs_fmax > 33 || (cfg->soft_rs_fmax & 1) == 0)) {
        set_err("fxrx_create: soft_rs_fmax is 0 or an even bound 0 .. 32 plus one (FXRX_ERR_ARG)"); return nullptr;
    }
    if (cfg->soft_rs_fmax && !cfg->soft_rs) { set_err("fxrx_create: soft_rs_fmax needs soft_rs (FXRX_ERR_ARG)"); return nullptr; }
    if (cfg->soft_rs_chain && !cfg->soft_rs) { set_err("fxrx_create: soft_rs_chain needs soft_rs (FXRX_ERR_ARG)"); return nullptr; }
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || nd <= 0 || cfg->device >= nd) {
        set_err("fxrx_create: no usable HIP device (this library has no CPU path)"); return nullptr;
    }
    if (hipSetDevice(cfg->device) != hipSuccess) { set_err("hipSetDevice failed"); return nullptr; }
    fxrx_ctx_s *c = new fxrx_ctx_s;
    auto fail = [&]() -> fxrx_ctx * { const std::string keep = g_err; fxrx_destroy(c); set_err(keep); return nullptr; };   // frees whatever was created
    c->cfg = *cfg;
    if (c->cfg.threshold <= 0.0f) c->cfg.threshold = cfg->mode == FXRX_MODE_DETECTOR ? 0.45f : 0.5f;
    if (const char *e = std::getenv("FXRX_PLL_WAVES")) c->pll_waves = (unsigned)std::min(4, std::max(1, std::atoi(e)));
    if (const char *e = std::getenv("FXRX_DEC_WAVES")) c->dec_waves = (unsigned)std::min(8, std::max(1, std::atoi(e)));
    if (const char *e = std::getenv("FXRX_SKIP_SEEK")) c->skip_seek = std::atoi(e) != 0;
    if (const char *e = std::getenv("FXRX_TAPER")) c->taper = std::min(0.95f, (float)std::atof(e));
    if (const char *e = std::getenv("FXRX_CHAIN_SLOW")) c->chain_slow = std::atoi(e) != 0;
    if (const char *e = std::getenv("FXRX_BATCH_VITERBI")) c->batch_viterbi = std::atoi(e) != 0;
    if (const char *e = std::getenv("FXRX_VB_CLEAN")) c->vb_clean = std::atoi(e) != 0;
    if (const char *e = std::getenv("FXRX_INCHAIN_REPAIR")) c->inchain_repair = std::min(2, std::max(0, std::atoi(e)));
    if (const char *e = std::getenv("FXRX_PLAN_FUSED")) c->plan_fused = std::atoi(e) != 0;
    if (const char *e = std::getenv("FXRX_PLAN_THREADS")) { const int v = std::atoi(e); if (v == 256 || v == 512) c->plan_threads = (unsigned)v; }
    if (const char *e = std::getenv("FXRX_VB_EARLY_TAIL")) c->vb_early_tail = std::atoi(e) != 0;
    if (const char *e = std::getenv("FXRX_DEBUG_STOP_AFTER")) c->debug_stop_after = std::atoi(e);
    if (const char *e = std::getenv("FXRX_DEBUG_WALK_TWICE")) c->debug_walk_twice = std::atoi(e);
    if (const char *e = std::getenv("FXRX_TIMING")) c->timing_level = std::min(2, std::max(0, std::atoi(e)));
    if (const char *e = std::getenv("FXRX_WALK_PER_CU")) c->walk_per_cu = (uint32_t)std::min(8, std::max(1, std::atoi(e)));
    if (const char *e = std::getenv("FXRX_VERIFY_PER_CU")) c->verify_per_cu = (uint32_t)std::min(64, std::max(1, std::atoi(e)));
    if (const char *e = std::getenv("FXRX_MF_PER_CU")) c->mf_per_cu = (uint32_t)std::min(64, std::max(0, std::atoi(e)));
    if (const char *e = std::getenv("FXRX_INGEST_KERNEL_MAX")) c->ingest_limits.ingest_kernel_max = (size_t)std::max<long long>(0, std::atoll(e));
    if (const char *e = std::getenv("FXRX_PLAN_GRID")) c->plan_grid = (uint32_t)std::min(256, std::max(0, std::atoi(e)));
    if (const char *e = std::getenv("FXRX_DETWIN_RESERVE")) c->detwin_reserve = (uint32_t)std::max(0, std::atoi(e));
    if (const char *e = std::getenv("FXRX_VB_DEBUG")) c->vb_debug = (uint32_t)std::atoi(e);
    if (const char *e = std::getenv("FXRX_PRESCAN")) c->prescan = std::atoi(e) != 0;
    if (const char *e = std::getenv("FXRX_PRESCAN_HOPS")) c->prescan_hops = std::min<int>(FX_PRESCAN_MAX_HOPS, std::max(0, std::atoi(e)));
    if (const char *e = std::getenv("FXRX_TAIL_GANG")) c->tail_gang = (unsigned)std::min(FX_GANG_MAX, std::max(1, std::atoi(e)));
    // (a block is at least as long as the warm-up of the next one: 128 steps)
    if (const char *e = std::getenv("FXRX_VB_BLK")) if (std::atoi(e) > 0) c->vb_blk_force = (uint32_t)std::min(4096, std::max(128, (std::atoi(e) + 63) / 64 * 64));
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, cfg->device) == hipSuccess) c->n_cus = prop.multiProcessorCount;
    // FXRX_DEBUG_CUS (tests): plan every launch as for a chip, or a partition, of that many CUs -- never more than there are
    if (const char *e = std::getenv("FXRX_DEBUG_CUS")) c->n_cus = std::min(c->n_cus, std::max(1, std::atoi(e)));
    if (upload_tables(c) != 0) return fail();
    const unsigned NS = cfg->n_streams;
    c->st.resize(NS);
    // carry buffers: the unconsumed tail is an incomplete frame (plus a detector window); 2 MB covers everything up to
    // 260 k samples per stream, longer tails grow the buffers through the replay path
    int64_t cap0 = std::max<int64_t>(1 << 15, std::min<int64_t>(1 << 18, (int64_t)(1 << 24) / (int64_t)NS));
    if (const char *e = std::getenv("FXRX_CARRY_SAMPLES")) cap0 = std::max<int64_t>(1024, std::atoll(e));
    for (auto &S : c->st) if (alloc_carry(S, cap0) != 0) return fail();
    if (hipMalloc((void **)&c->d_state, sizeof(FxStreamState) * kStateRing * NS) != hipSuccess ||
        hipHostMalloc((void **)&c->h_state, sizeof(FxStreamState) * kStateRing * NS, hipHostMallocDefault) != hipSuccess) { set_err("fxrx_create: state ring allocation failed"); return fail(); }
    if (hipMemset(c->d_state, 0, sizeof(FxStreamState) * kStateRing * NS) != hipSuccess) { set_err("hipMemset failed"); return fail(); }
    std::memset(c->h_state, 0, sizeof(FxStreamState) * kStateRing * NS);
    for (unsigned i = 0; i < 2; i++) if (make_slot(c) != 0) return fail();
    return c;
}

// forget all per-stream state (position, carried tail).  Blocks in flight are unaffected: what they leave behind on the
// device is simply never read.
void fxrx_reset(fxrx_ctx *c)
{
    if (!c) return;
    for (auto &S : c->st) { S.total = 0; S.fresh_start = true; S.carry_bound = 0; }
}

int fxrx_set_depth(fxrx_ctx *c, unsigned int depth)
{
    if (!c || depth == 0 || depth > kMaxDepth) return FXRX_ERR_ARG;
    HIP_OK(hipSetDevice(c->cfg.device));
    { const int r = close_gang(c); if (r) return r; }
    if (c->inflight) { set_err("fxrx_set_depth: blocks in flight"); return FXRX_ERR_STATE; }
    while (c->slots.size() < depth + 1) if (make_slot(c) != 0) return FXRX_ERR_HIP;
    c->depth = depth; c->head = c->tail = 0; c->last = nullptr;
    return 0;
}

// diagnostics (timing level 2 set before the first submit): of the last collected block, in ms since a common origin --
// host time when fxrx_submit was entered, GPU time of its first stage event, GPU time of its last event, host time when
// fxrx_collect had it
int fxrx_debug_block_times(const fxrx_ctx *c, double out[4])
{
    if (!c || !c->last || !out) return FXRX_ERR_ARG;
    out[0] = c->last->dbg_submit_ms; out[1] = c->last->dbg_gpu_start_ms; out[2] = c->last->dbg_gpu_done_ms; out[3] = c->last->dbg_collect_ms;
    return 0;
}

int fxrx_set_timing(fxrx_ctx *c, int level)
{
    if (!c || level < -1 || level > 2) return FXRX_ERR_ARG;
    c->timing_level = level;
    if (!c->gang.empty()) { HIP_OK(hipSetDevice(c->cfg.device)); return close_gang(c); }
    return 0;
}

void *fxrx_stream(const fxrx_ctx *c) { return (c && !c->slots.empty()) ? (void *)c->slots[0]->st : nullptr; }

int fxrx_last_timing(const fxrx_ctx *c, fxrx_timing *t) { if (!c || !t || !c->last) return FXRX_ERR_ARG; *t = c->last->timing; return 0; }

const void *fxrx_device_framesyms(const fxrx_ctx *c, uint64_t *n)
{
    if (!c || !c->last) return nullptr;
    if (n) *n = c->last->n_syms;
    return c->last->n_syms ? c->last->d_symraw.p : nullptr;
}

// ---- launch helpers: a kernel launched from more than one place has its arguments named here, once; a helper takes what differs between its call sites
// walker.  kWalkList: the njobs entries of `list`; kWalkRequests: `list` holds njobs repair requests (repair_rounds); kWalkRequestsInChain:
// repair requests whose number is read on the device, njobs workgroups stride over them (the repair round within the chain)
enum WalkForm { kWalkList, kWalkRequests, kWalkRequestsInChain };
static inline hipError_t launch_walk(const fxrx_ctx_s *c, const Slot &sl, hipStream_t st, const uint32_t *list, unsigned njobs, WalkForm form = kWalkList)
{
    return fx_launch_walk(c->cfg.mode == FXRX_MODE_DETECTOR ? FX_MODE_DETECT : FX_MODE_FLEXRX, c->cfg.equalizer ? 1 : 0, c->cfg.soft_header ? 1 : 0, njobs, st, sl.jobs(), list, sl.d_wres.p, sl.d_frames.p, sl.d_runs.p,
                          sl.run_cap, sl.hdr_walk(), c->d_tables, form == kWalkList ? 0 : 1, (uint32_t)sl.NJ, form == kWalkRequestsInChain ? &sl.hdr_walk()->n_repair_req : nullptr, form == kWalkRequestsInChain ? (uint32_t)(2 * sl.NJ + 16) : 0u);
}
static inline hipError_t launch_seekverify(const fxrx_ctx_s *c, const Slot &sl, hipStream_t st, unsigned grid, uint32_t phase)
{
    return fx_launch_seekverify(grid, st, sl.d_runs.p, sl.run_cap, sl.jobs(), sl.d_wres.p, sl.d_frames.p, sl.hdr_walk(), c->d_tables, phase);
}
// lean chain kernel.  kStitch: stitch, nothing else (FXRX_CHAIN_SLOW: flag everything for repair); kStitchQueue: and rewrite and list in d_req the segments to walk again
// (repair_rounds); kStitchPass1 / 2: the repair round within the chain -- pass 1 queues likewise and notes every stream's state in d_cstat, pass 2, behind the walk, stitches again
enum ChainForm { kStitch, kStitchQueue, kStitchPass1, kStitchPass2 };
static inline hipError_t launch_chainfast(const fxrx_ctx_s *c, const Slot &sl, hipStream_t st, ChainForm form)
{
    const bool queue = form == kStitchQueue || form == kStitchPass1;
    return fx_launch_chainfast(c->cfg.n_streams, st, sl.streams(), sl.jobs(), sl.d_wres.p, sl.d_frames.p, sl.d_chain.p, sl.d_chain_count.p, sl.hdr_walk(), form == kStitch && c->chain_slow ? 1u : 0u,
                               queue ? sl.jobs_rw() : nullptr, queue ? sl.d_req.p : nullptr, form >= kStitchPass1 ? sl.d_cstat.p : nullptr, form == kStitchPass1 ? 1u : form == kStitchPass2 ? 2u : 0u);
}
// wave-per-frame decoder over the frames [first_wave, first_wave + n_waves) of one list (no waves: no launch).  The Reed-Solomon list takes the
// Reed-Solomon instance; the fallback list holds frames of the batch path -- hard decisions -- and its launch reports to the host's header
static inline int soft_level(const fxrx_config &cfg) { return cfg.soft_decision ? (cfg.soft_block ? (cfg.soft_chain ? 3 : 2) : 1) : 0; }
static inline hipError_t launch_paydec(const fxrx_ctx_s *c, const Slot &sl, hipStream_t st, DecList which, unsigned first_wave, unsigned n_waves, unsigned waves_per_wg)
{
    return fx_launch_paydec(which == kDecRs ? 1 : 0, which == kDecFallback ? 0 : soft_level(c->cfg), c->cfg.soft_rs ? 1 : 0, c->cfg.soft_rs_chain ? 1 : 0, first_wave, n_waves, waves_per_wg, st, sl.d_pjobs.p, sl.dec_list(which), sl.hdr_pay(), sl.d_hard.p, sl.d_bufA.p, sl.d_bufB.p,
                            sl.d_soft.p, sl.d_dw.p, sl.h_out.p, sl.h_recs.p, sl.pres(), c->d_tables, which == kDecFallback ? sl.h_hdr.p : nullptr);
}
// decode, one wave per frame: the lean instance, then the Reed-Solomon instance (which strides)
static inline hipError_t launch_decoders(const fxrx_ctx_s *c, const Slot &sl, hipStream_t st, unsigned first_plain, unsigned n_plain, unsigned n_rs)
{
    const hipError_t e = launch_paydec(c, sl, st, kDecPlain, first_plain, n_plain, c->dec_waves);
    return e != hipSuccess ? e : launch_paydec(c, sl, st, kDecRs, 0u, n_rs, 1u);
}
// batch Viterbi path: the trellis kernels over the first n_items work items, the back part for the first n_fin frames, fb_waves of the fallback decoder for what it hands back
static inline hipError_t launch_trellis(const fxrx_ctx_s *c, const Slot &sl, hipStream_t st, unsigned n_items, int packed, int with_fix, unsigned n_fin, unsigned fb_waves)
{
    hipError_t e = fx_launch_vbitems(0, n_items, st, sl.d_pjobs.p, sl.d_vb_items.p, sl.vb_cap, sl.hdr_pay(), sl.d_bufA.p, sl.d_bufB.p, sl.d_vb_dw.p, sl.d_vb_vec.p, sl.d_vb_st.p, c->vb_debug, packed, with_fix);
    if (e == hipSuccess) e = fx_launch_vbfinish(0, n_fin, st, sl.d_pjobs.p, sl.dec_list(kDecBatch), sl.hdr_pay(), sl.d_bufA.p, sl.d_bufB.p, sl.d_vb_dw.p, sl.d_vb_vec.p, sl.d_vb_st.p, sl.dec_list(kDecFallback),
                                                sl.list_cap(), sl.h_out.p, sl.h_recs.p, sl.h_hdr.p, sl.tail.vb_early ? 1 : 0);
    return e != hipSuccess ? e : launch_paydec(c, sl, st, kDecFallback, 0u, fb_waves, 1u);
}
// detector windows of the records [first, last), on the block's stream; late: at collect (windows that start in the carried tail are not written again)
static inline hipError_t launch_detwin(const fxrx_ctx_s *c, const Slot &sl, uint32_t first, uint32_t last, bool late)
{
    return fx_launch_detwin(sl.st, std::min<unsigned>(std::max<unsigned>(last - first, 1u), 4u * (unsigned)c->n_cus), sl.streams(), c->cfg.n_streams, sl.d_stream_base.p, sl.d_pjobs.p, sl.hdr_pay(), first, last,
                            sl.h_win.p, sl.h_wintail.p, sl.h_winflag.p, late ? 0 : 1, late ? 1 : 0);
}
// streams in which a skipped hop fired (req: the block's repair requests, copied from d_req): their next blocks are walked with the exact detector on every hop
static void mark_noskip(fxrx_ctx_s *c, const Slot &sl, const std::vector<uint32_t> &req)
{
    const FxWalkJob *hj = reinterpret_cast<const FxWalkJob *>(sl.hp_desc.p);
    for (uint32_t r : req) if ((r & 0x80000000u) && (r & 0x7fffffffu) < sl.NJ) c->st[hj[r & 0x7fffffffu].stream].noskip_left = 32;
}

enum { kChainFast = 0, kChainFull = 1, kChainDone = 2 };
static int enqueue_back(fxrx_ctx_s *c, Slot &sl, int chain_mode, hipStream_t chain_st = nullptr, bool may_defer = false);

// ---- enqueue the whole kernel chain of the block in `sl` (descriptors are rebuilt: a replay calls this again), as five steps ----
// what the steps hand on: the block's plan and the host copies of the descriptors it becomes
struct FrontBuild {
    FrontPlan plan;
    std::vector<FxWalkJob> jobs; std::vector<FxStreamDesc> sds;
    // job lists: speculative walkers in launch order | true walkers of continuing streams | speculative jobs the pre-lock scan takes
    std::vector<uint32_t> early, late, spec;
    size_t desc_bytes = 0;
};

// 1. the plan (fx_frontplan.h), from what the context and the block's snapshot say; its capacities go to the slot
static int plan_front(const fxrx_ctx_s *c, Slot &sl, FrontPlan &plan)
{
    const unsigned NS = c->cfg.n_streams;
    FrontKnobs k;
    k.detect = c->cfg.mode == FXRX_MODE_DETECTOR; k.depth = c->depth; k.n_cus = c->n_cus; k.walk_per_cu = c->walk_per_cu;
    k.segment_len = c->cfg.segment_len; k.taper = c->taper; k.prescan = c->prescan; k.prescan_hops = c->prescan_hops;
    k.batch_viterbi = c->batch_viterbi; k.soft_decision = c->cfg.soft_decision != 0; k.vb_blk_force = c->vb_blk_force;
    std::vector<StreamIn> in(NS);
    for (unsigned s = 0; s < NS; s++) in[s] = StreamIn{ sl.n[s], !sl.snap[s].fresh_start, sl.snap[s].carry_bound };
    plan = front_plan(in, c->traffic, k);
    const FrontCaps &cap = plan.caps;
    sl.NJ = plan.cuts.size();
    sl.frame_slots = cap.frame_slots; sl.chain_cap = cap.chain_slots; sl.run_cap = cap.run_cap; sl.mf_cap = cap.mf_cap;
    sl.sym_cap = cap.sym_cap; sl.byte_cap = cap.byte_cap; sl.dw_cap = cap.dw_cap; sl.out_cap = cap.out_cap;
    sl.vb_blk = cap.vb_blk; sl.vb_cap = cap.vb.vb_cap; sl.vb_dw_words = cap.vb.vb_dw_words; sl.vb_slots_alloc = cap.vb.vb_slots_alloc;
    sl.ps_hops = plan.ps_hops; sl.ps_words = prescan_words(plan.ps_hops); sl.ps_taken = sl.ps_fallback = 0;
    if (cap.too_large) { set_err("fxrx_submit: batch too large for 32-bit arena offsets"); return FXRX_ERR_ARG; }
    return 0;
}

// 2. the cuts as FxWalkJob and FxStreamDesc records -- everything that points into the context's or the block's memory --, the job lists,
// and the layout of the descriptor arena
static void build_descriptors(const fxrx_ctx_s *c, Slot &sl, FrontBuild &fb)
{
    const unsigned NS = c->cfg.n_streams;
    const bool detect = c->cfg.mode == FXRX_MODE_DETECTOR;
    const uint64_t b = sl.seq;
    const FrontPlan &plan = fb.plan;
    fb.jobs.reserve(plan.cuts.size()); fb.sds.resize(NS);
    for (unsigned s = 0; s < NS; s++) {
        const StreamState &S = c->st[s]; const StreamSnap &sn = sl.snap[s]; const StreamCaps &sc = plan.caps.streams[s];
        const int64_t ns = (int64_t)sl.n[s];
        const bool cont = !sn.fresh_start;
        FxStreamDesc &sd = fb.sds[s];
        sd.x = sl.x[s]; sd.xa_end = cont ? S.carry[b % 3] + S.carry_cap : nullptr; sd.n = ns;
        sd.first_job = plan.first_cut[s]; sd.n_jobs = plan.first_cut[s + 1] - plan.first_cut[s];
        sd.state_in = cont ? c->d_state + ((b + kStateRing - 1) % kStateRing) * NS + s : nullptr;
        sd.state_out = c->d_state + (b % kStateRing) * NS + s;
        sd.state_out_host = c->h_state + (b % kStateRing) * NS + s;
        sd.carry_out_end = S.carry[(b + 1) % 3] + S.carry_cap; sd.carry_cap = S.carry_cap;
        sd.abs_base = sn.tot0;
        sd.chain_base = sc.chain_base; sd.chain_cap = sc.chain_cap; sd.repair_base = sc.repair_base; sd.repair_cap = kRepairCap;
        for (uint32_t ji = plan.first_cut[s]; ji < plan.first_cut[s + 1]; ji++) {
            const Cut &cut = plan.cuts[ji];
            const bool true_walker = cut.first && cont;       // starts from the state the previous block leaves, behind that block's chain kernel
            FxWalkJob j{};
            j.x = sd.x; j.xa_end = sd.xa_end; j.n = ns; j.start = cut.start; j.stop = cut.stop;
            j.fresh = 1u; j.floor = cut.start;
            j.mode = detect ? FX_MODE_DETECT : FX_MODE_FLEXRX;
            j.handoff = j.stop < ns ? 1u : 0u;
            j.prelock = cut.first ? 0u : 1u;
            j.frame_base = plan.caps.frame_base[ji]; j.max_frames = cut.max_frames;
            j.threshold = c->cfg.threshold;
            j.no_skip = (detect || !c->skip_seek || sl.force_noskip || sn.noskip) ? 1u : 0u;
            j.state_in = true_walker ? sd.state_in : nullptr;
            j.stream = s; j.verify_per = c->traffic.verify_per; j.eq = (!detect && c->cfg.equalizer) ? 1u : 0u;
            (true_walker ? fb.late : fb.early).push_back(ji);
            fb.jobs.push_back(j);
        }
    }
    if (plan.taper > 0.0f) longest_first(fb.early, plan.cuts);
    if (plan.ps_hops) for (uint32_t ji : fb.early) if (fb.jobs[ji].prelock && fb.jobs[ji].mode == FX_MODE_FLEXRX) {
        FxWalkJob &j = fb.jobs[ji];
        j.prescan_words = sl.ps_words; j.prescan_hops = fx_prescan_valid_hops(j.start, j.stop, j.n, plan.ps_hops);     // (j.prescan: pack_descriptors, once its table is reserved)
        fb.spec.push_back(ji);
    }
    sl.n_early = fb.early.size(); sl.n_late = fb.late.size(); sl.any_late = !fb.late.empty(); sl.ps_jobs = (uint32_t)fb.spec.size();
    // (the job lists: early | late, NJ entries together, and behind them the speculative jobs the pre-lock scan takes)
    auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
    sl.o_list = up16(sl.NJ * sizeof(FxWalkJob)); sl.o_streams = sl.o_list + up16(2 * sl.NJ * sizeof(uint32_t));
    fb.desc_bytes = sl.o_streams + up16(NS * sizeof(FxStreamDesc));
}

// 3. every buffer of the block at the capacity the plan gives it (buffers only ever grow)
static int reserve_block(fxrx_ctx_s *c, Slot &sl, const FrontBuild &fb)
{
    const unsigned NS = c->cfg.n_streams;
    const size_t NJ = sl.NJ;
    const uint32_t chain_slots = sl.chain_cap;
    const bool detect = c->cfg.mode == FXRX_MODE_DETECTOR, flex = !detect, syms = c->cfg.want_framesyms != 0, soft = flex && c->cfg.soft_decision;
    // pre-lock scan table; descriptors, walk and chain tables, payload jobs and lists
    if (!fb.spec.empty() && sl.d_prescan.reserve(fb.spec.size() * sl.ps_words)) return FXRX_ERR_HIP;
    if (sl.hp_desc.reserve(fb.desc_bytes) || sl.d_desc.reserve(fb.desc_bytes) || sl.d_wres.reserve(NJ + NS) || sl.d_frames.reserve(sl.frame_slots) ||
        sl.d_runs.reserve(sl.run_cap) || sl.d_req.reserve(2 * NJ + 16) || sl.d_cstat.reserve(NS) || sl.d_chain.reserve(chain_slots) || sl.d_chain_count.reserve(NS) || sl.d_stream_base.reserve(NS + 1) ||
        sl.d_pjobs.reserve(chain_slots) || sl.h_recs.reserve(chain_slots) || sl.d_mf_job.reserve(sl.mf_cap) || sl.d_mf_c0.reserve(sl.mf_cap) ||
        sl.d_pll_list.reserve(sl.list_cap()) || sl.d_dec_list.reserve(kDecLists * (size_t)sl.list_cap())) return FXRX_ERR_HIP;
    // flex_rx only: the payload arenas
    if (flex && (sl.d_symraw.reserve(sl.sym_cap) || sl.d_hard.reserve(sl.sym_cap + 64) ||
                 sl.d_bufA.reserve(sl.byte_cap + 256) || sl.d_bufB.reserve(sl.byte_cap + 256) || sl.d_dw.reserve(sl.dw_cap) || sl.h_out.reserve(sl.out_cap))) return FXRX_ERR_HIP;
    // frame symbols for the host
    if (flex && syms && sl.h_framesyms.reserve(sl.sym_cap)) return FXRX_ERR_HIP;
    // detector windows (a block that holds more than were reserved is completed when it is collected: finish_windows)
    if (detect && syms) {
        sl.win_reserved = window_slots(c->traffic, chain_slots, c->detwin_reserve);
        if (sl.h_win.reserve((size_t)sl.win_reserved * FX_NFFT) || sl.h_wintail.reserve(2 * (size_t)NS * FX_NFFT) || sl.h_winflag.reserve(1)) return FXRX_ERR_HIP;
        *sl.h_winflag.p = 0u;
    }
    // batch Viterbi (the item list also without the path)
    if (sl.d_vb_items.reserve(2 * (size_t)sl.vb_slots_alloc) ||
        (sl.vb_blk && (sl.d_vb_vec.reserve(128 * (size_t)sl.vb_slots_alloc) || sl.d_vb_dw.reserve((size_t)sl.vb_dw_words) || sl.d_vb_st.reserve(sl.vb_slots_alloc)))) return FXRX_ERR_HIP;
    // soft values
    if (soft && (sl.d_soft.reserve(8 * sl.byte_cap) || (syms && sl.h_soft.reserve(8 * sl.byte_cap)))) return FXRX_ERR_HIP;
#ifdef FX_STAMPS
    if (flex && sl.d_pres.reserve(chain_slots)) return FXRX_ERR_HIP;
#endif
    return 0;
}

// 4. the descriptor arena in page-locked memory: [FxWalkJob x NJ | job lists | FxStreamDesc x NS]
static void pack_descriptors(Slot &sl, FrontBuild &fb)
{
    const size_t NJ = sl.NJ;
    for (size_t i = 0; i < fb.spec.size(); i++) fb.jobs[fb.spec[i]].prescan = sl.d_prescan.p + i * sl.ps_words;
    std::memcpy(sl.hp_desc.p, fb.jobs.data(), NJ * sizeof(FxWalkJob));
    uint32_t *hl = reinterpret_cast<uint32_t *>(sl.hp_desc.p + sl.o_list);
    if (!fb.early.empty()) std::memcpy(hl, fb.early.data(), fb.early.size() * sizeof(uint32_t));
    if (!fb.late.empty()) std::memcpy(hl + fb.early.size(), fb.late.data(), fb.late.size() * sizeof(uint32_t));
    if (!fb.spec.empty()) std::memcpy(hl + NJ, fb.spec.data(), fb.spec.size() * sizeof(uint32_t));
    std::memcpy(sl.hp_desc.p + sl.o_streams, fb.sds.data(), fb.sds.size() * sizeof(FxStreamDesc));
}

// 5. the chain, front part: walkers and seek verification.  *chain_st: the stream the chain kernel goes to
static int enqueue_front(fxrx_ctx_s *c, Slot &sl, const FrontBuild &fb, hipStream_t *chain_st)
{
    const bool detect = c->cfg.mode == FXRX_MODE_DETECTOR;
    const uint64_t b = sl.seq;
    const size_t NJ = sl.NJ;
    const unsigned n_early = (unsigned)fb.early.size(), n_late = (unsigned)fb.late.size(), n_spec = (unsigned)fb.spec.size();
    hipStream_t st = sl.st;
    const uint32_t *d_list = sl.job_list();
    // (the block's input first, every format: a copy where the route has one -- float IQ into the staging buffer the descriptors point at, integer IQ into
    // the raw one --, then fx_upload_kernel or fx_ingest_kernel where it has one.  Behind every check and reservation of the block; a replay finds the list empty.)
    if (!sl.ingest.empty()) {
        std::vector<IngestJob> todo; todo.swap(sl.ingest);
        const size_t bytes = iq_sample_bytes(sl.ingest_fmt);
        for (const IngestJob &j : todo) {
            float2 *x = sl.d_in[j.stream].p;
            const void *src = j.src;
            if (route_copies(j.route)) {
                void *to = route_converts(j.route) ? (void *)sl.d_raw[j.stream].p : (void *)x;
                HIP_OK(hipMemcpyAsync(to, src, j.n * bytes, hipMemcpyHostToDevice, st)); src = to;
            }
            if (j.route == kRouteUploadKernel) HIP_OK(fx_launch_upload(st, src, x, j.n * bytes, (unsigned)c->n_cus));
            if (route_converts(j.route)) HIP_OK(fx_launch_ingest(st, sl.ingest_fmt, src, x, (size_t)j.n, sl.ingest_scale, (unsigned)c->n_cus));
        }
    }
    HIP_OK(fx_launch_upload(st, sl.hp_desc.p, sl.d_desc.p, fb.desc_bytes, (unsigned)c->n_cus));     // (descriptors: our own page-locked buffer)
    const int tl = c->timing_level >= 0 ? c->timing_level : (c->depth > 1 ? 0 : 2);      // stage events: see fxrx_set_timing
    sl.timing_level = tl;
    // (the speculative jobs' pre-lock scan: part of the walk stage, in front of every walker launch that reads its table)
    if (c->debug_walk_twice > 0) HIP_OK(fx_launch_prescan(st, n_spec, sl.ps_words, sl.jobs(), d_list + NJ, c->d_tables));
    for (int rep = 0; rep < c->debug_walk_twice; rep++) HIP_OK(launch_walk(c, sl, st, d_list, n_early));
    if (tl >= 2) HIP_OK(hipEventRecord(sl.ev[kEvStart], st));
    if (c->debug_walk_twice <= 0) HIP_OK(fx_launch_prescan(st, n_spec, sl.ps_words, sl.jobs(), d_list + NJ, c->d_tables));
    HIP_OK(launch_walk(c, sl, st, d_list, n_early));
    // the true walkers of continuing streams read the state the previous block's chain kernel leaves.  What the speculative
    // walkers skipped is verified before that wait -- it does not depend on the state --, so that the chain of dependencies
    // from one block's chain kernel to the next one's is just: true walkers, their few verification runs, chain kernel
    const bool verify = !detect && c->skip_seek && !sl.force_noskip;
    hipStream_t cst = st;                                     // the stream the rest of the front part and the chain kernel go to
    if (n_late) {
        if (verify) {
            HIP_OK(fx_launch_copy_u32(st, &sl.hdr_walk()->n_runs, &sl.hdr_walk()->runs_done));
            HIP_OK(launch_seekverify(c, sl, st, c->verify_per_cu * (unsigned)c->n_cus, 0u));
        }
        // (from here to the chain kernel the block is on the chain of dependencies that runs through all blocks of a continuing
        // stream: a single workgroup or two that must not queue behind the chip-filling kernels of the other blocks in flight
        // -- so this stretch goes to the context's high-priority stream, which also keeps the chain kernels in block order)
        if (!c->st_chain) {
            int lo = 0, hi = 0;
            HIP_OK(hipDeviceGetStreamPriorityRange(&lo, &hi));
            HIP_OK(hipStreamCreateWithPriority(&c->st_chain, hipStreamNonBlocking, hi));
        }
        HIP_OK(hipEventRecord(sl.ev[kEvHandover], st));
        cst = c->st_chain;
        HIP_OK(hipStreamWaitEvent(cst, sl.ev[kEvHandover], 0));
        if (c->prev_chain) HIP_OK(hipStreamWaitEvent(cst, c->prev_chain, 0));
        HIP_OK(launch_walk(c, sl, cst, d_list + n_early, n_late));
    }
    if (tl >= 2) HIP_OK(hipEventRecord(sl.ev[kEvWalk], cst));
    if (verify)
        HIP_OK(launch_seekverify(c, sl, cst, !n_late ? c->verify_per_cu * (unsigned)c->n_cus : (unsigned)std::min<size_t>((size_t)c->verify_per_cu * (size_t)c->n_cus, std::max<size_t>(64, 16 * (size_t)n_late)), 1u));
    if (tl >= 2) HIP_OK(hipEventRecord(sl.ev[kEvVerify], cst));
    // chain kernels run in block order in any case (they write the carry buffers in rotation); this one writes
    // carry[(b + 1) % 3], which the payload MF of block b - 2 may still be reading
    if (!n_late && c->prev_chain) HIP_OK(hipStreamWaitEvent(cst, c->prev_chain, 0));
    if (c->carry_reader[(b + 1) % 3]) HIP_OK(hipStreamWaitEvent(cst, c->carry_reader[(b + 1) % 3], 0));
    *chain_st = cst;
    return 0;
}

// FXRX_DEBUG_SUBMIT_PROFILE: the host time since *t goes to part `part` of the profile, and *t moves on
static inline void prof_lap(int part, double *t) { if (g_prof_on) { const double now = prof_now(); g_prof[part] += now - *t; *t = now; } }

// steps 4 and 5 and the back part: only a HIP launch error can follow from here on
static int launch_block(fxrx_ctx_s *c, Slot &sl, FrontBuild &fb, bool may_defer, double *t)
{
    pack_descriptors(sl, fb); prof_lap(2, t);
    hipStream_t cst = nullptr;
    { const int r = enqueue_front(c, sl, fb, &cst); if (r) return r; }
    prof_lap(3, t);
    const int rb = enqueue_back(c, sl, kChainFast, cst, may_defer);
    prof_lap(4, t); if (g_prof_on) g_prof_n++;
    return rb;
}
// a block whose snapshot the slot holds (a replay): plan, build, reserve, pack, enqueue
static int enqueue_block(fxrx_ctx_s *c, Slot &sl)
{
    double t = g_prof_on ? prof_now() : 0.0;
    FrontBuild fb;
    { const int r = plan_front(c, sl, fb.plan); if (r) return r; }
    build_descriptors(c, sl, fb); prof_lap(1, &t);
    { const int r = reserve_block(c, sl, fb); if (r) return r; }
    return launch_block(c, sl, fb, /* may_defer */ false, &t);
}

static FxVbpreMember vbpre_member(Slot &sl, uint32_t first_wave, uint32_t n_waves)
{
    return FxVbpreMember{ sl.d_pjobs.p, sl.dec_list(kDecBatch), sl.hdr_pay(), sl.d_hard.p, sl.d_bufA.p, sl.d_bufB.p, sl.h_out.p, sl.h_recs.p, sl.h_hdr.p, sl.d_vb_items.p, sl.vb_cap, first_wave, n_waves };
}
// ---- the tails of n blocks (n <= FX_GANG_MAX; n = 1: a block's own tail, on its own stream), on the last one's stream: one PLL
// launch for all, each block's own decode launches where it has any, one fx_vbpre_kernel launch for all, each block's trellis
// kernels / fallback decoder / symbol copy, and every block's ev[kEvDone] ----
static int launch_tails(fxrx_ctx_s *c, Slot *const *m, unsigned n)
{
    hipStream_t st = m[n - 1]->st;
    for (unsigned i = 0; i + 1 < n; i++) HIP_OK(hipStreamWaitEvent(st, m[i]->ev[kEvMf], 0));      // (the other members' matched filters)
    auto done = [&]() -> int {
        for (unsigned i = 0; i < n; i++) { HIP_OK(hipEventRecord(m[i]->ev[kEvDone], st)); m[i]->tail_launched = true; m[i]->tail_st = st; }
        if (n > 1) { c->gang_launches++; c->gang_members += n; }
        return 0;
    };
    {
        FxPllGang g; unsigned waves[FX_GANG_MAX]; g.n = n;
        for (unsigned i = 0; i < n; i++) { const Slot &sl = *m[i]; g.m[i] = FxPllMember{ sl.d_pjobs.p, sl.d_pll_list.p, sl.hdr_pay(), sl.d_symraw.p, sl.d_symraw.p, sl.d_hard.p, sl.h_recs.p }; waves[i] = sl.tail.pll_waves; }
        HIP_OK(fx_launch_paypll(&g, waves, c->pll_waves, st, c->d_tables));
    }
    for (unsigned i = 0; i < n; i++) if (m[i]->timing_level >= 1) HIP_OK(hipEventRecord(m[i]->ev[kEvPll], st));
    if (c->debug_stop_after == 6) return done();
    for (unsigned i = 0; i < n; i++) {
        Slot &sl = *m[i];
        if (c->cfg.soft_decision) {
            // per-bit soft values from the carrier-recovered symbols (data parallel, off the PLL's recurrence); the decoder
            // de-interleaves them in place, so a caller that wants to see them gets a copy first
            HIP_OK(fx_launch_softdemod(sl.tail.mf_grid, st, sl.d_pjobs.p, sl.d_mf_job.p, sl.d_mf_c0.p, sl.hdr_pay(), sl.d_symraw.p, sl.d_hard.p, sl.d_soft.p, c->d_tables));
            if (c->cfg.want_framesyms) HIP_OK(hipMemcpyAsync(sl.h_soft.p, sl.d_soft.p, 8 * sl.byte_cap, hipMemcpyDeviceToHost, st));
        }
        HIP_OK(launch_decoders(c, sl, st, 0u, sl.tail.plain, sl.tail.rs));
    }
    {
        FxVbpreGang g; g.n = n;
        for (unsigned i = 0; i < n; i++) g.m[i] = vbpre_member(*m[i], 0u, m[i]->vb_blk ? m[i]->tail.vb_pre : 0u);
        HIP_OK(fx_launch_vbpre(&g, st, c->d_tables, c->vb_clean ? 1 : 0, c->vb_early_tail && c->vb_clean ? 1 : 0));
    }
    for (unsigned i = 0; i < n; i++) {
        Slot &sl = *m[i];
        if (sl.vb_blk) HIP_OK(launch_trellis(c, sl, st, sl.tail.vb_items, sl.tail.vb_packed, sl.tail.with_fix, sl.tail.vb_fin, sl.tail.fb));
        if (sl.timing_level >= 2) HIP_OK(hipEventRecord(sl.ev[kEvDec], st));
        // (a copy kernel: it knows how many symbols the block really holds)
        if (c->cfg.want_framesyms) HIP_OK(fx_launch_symcopy(2u * (unsigned)c->n_cus, st, sl.hdr_pay(), sl.d_symraw.p, sl.h_framesyms.p));
    }
    return done();
}

// launch what the open gang holds (nothing: no-op).  Called when the gang is full, and before anything that waits for a member's
// ev[kEvDone], moves what the members read, or changes what a submit means.
// If a launch fails part-way the gang is empty all the same and its members stay without a tail (tail_launched false: nobody
// waits on their ev[kEvDone]).  The HIP error goes up to the caller; fxrx_collect, when it reaches such a member, reports a block
// without a tail and drops everything in flight (discard_inflight).  Not mended further: a HIP error at launch is fatal to
// the context, every later call fails the same way.
static int close_gang(fxrx_ctx_s *c)
{
    if (c->gang.empty()) return 0;
    if (c->gang.size() > FX_GANG_MAX) { set_err("open gang larger than FX_GANG_MAX (internal error)"); return FXRX_ERR_STATE; }   // (the deferral rule closes it at tail_gang <= FX_GANG_MAX)
    Slot *m[FX_GANG_MAX]; unsigned n = 0;
    for (Slot *s : c->gang) m[n++] = s;
    c->gang.clear();
    return launch_tails(c, m, n);
}

// ---- back part of the chain: chain kernel, plan, payload stage.  `full`: the full-size chain kernel, which can walk
// (fxrx_collect runs it for a block whose lean chain kernel reported FX_BLK_NEEDS_REPAIR) ----
static int enqueue_back(fxrx_ctx_s *c, Slot &sl, int chain_mode, hipStream_t chain_st, bool may_defer)
{
    const unsigned NS = c->cfg.n_streams; const bool detect = c->cfg.mode == FXRX_MODE_DETECTOR;
    const uint64_t b = sl.seq; const uint32_t chain_slots = sl.chain_cap; hipStream_t st = sl.st;
    sl.tail_launched = true; sl.tail_st = st;
    if (chain_mode == kChainFull)
        HIP_OK(fx_launch_chain(detect ? FX_MODE_DETECT : FX_MODE_FLEXRX, c->cfg.equalizer ? 1 : 0, c->cfg.soft_header ? 1 : 0, NS, st, sl.streams(), sl.jobs(), (uint32_t)sl.NJ, sl.d_wres.p, sl.d_frames.p, sl.d_chain.p,
                               sl.d_chain_count.p, sl.d_runs.p, sl.run_cap, sl.hdr_walk(), c->chain_slow ? 1u : 0u, c->d_tables));
    else if (chain_mode == kChainFast) {
        // stitch; one repair round within the chain for what only takes a walk from a hand-off state (a hand-off target missing
        // from the next list, a skipped hop on which the exact detector fires): its walkers read the number of queued segments
        // on the device -- normally none: two launches that leave at once --; stitch the streams concerned again.  Whatever
        // is still open after that is flagged and mended when the block is collected (repair_and_replay).
        hipStream_t cs = chain_st ? chain_st : st;
        sl.inchain = !c->chain_slow && (c->inchain_repair == 2 || (c->inchain_repair == 1 && c->inchain_left > 0));
        if (c->inchain_left) c->inchain_left--;
        if (!sl.inchain) HIP_OK(launch_chainfast(c, sl, cs, kStitch));
        else {
            HIP_OK(launch_chainfast(c, sl, cs, kStitchPass1));
            HIP_OK(launch_walk(c, sl, cs, sl.d_req.p, (unsigned)std::min<size_t>(2 * sl.NJ, 64), kWalkRequestsInChain));
            HIP_OK(launch_chainfast(c, sl, cs, kStitchPass2));
        }
    }
    // (kChainDone: the repair rounds have stitched the block already)
    HIP_OK(hipEventRecord(sl.ev[kEvChain], chain_mode == kChainFast && chain_st ? chain_st : st));
    if (chain_mode == kChainFast && chain_st && chain_st != st) HIP_OK(hipStreamWaitEvent(st, sl.ev[kEvChain], 0));   // back onto the block's own stream
    c->prev_chain = sl.ev[kEvChain];
    // (the plan kernels' workgroups take contiguous ranges of the chain's frames: about 2048 each, from the last block's count)
    {
        FxPlanArgs a;
        a.streams = sl.streams(); a.nstreams = NS; a.detect = detect ? 1u : 0u; a.eq = c->cfg.equalizer ? 1u : 0u; a.vb_blk = sl.vb_blk;
        a.chain = sl.d_chain.p; a.chain_count = sl.d_chain_count.p; a.stream_base = sl.d_stream_base.p;
        a.pjobs = sl.d_pjobs.p; a.recs = sl.h_recs.p;
        a.mf_job = sl.d_mf_job.p; a.mf_c0 = sl.d_mf_c0.p; a.mf_cap = sl.mf_cap;
        a.pll_list = sl.d_pll_list.p; a.dec_list = sl.dec_list(kDecPlain); a.list_cap = sl.list_cap();
        a.vb_items = sl.d_vb_items.p; a.vb_cap = sl.vb_cap;
        a.hdr = sl.hdr_walk(); a.hdr_pay = sl.hdr_pay(); a.hdr_host = sl.h_hdr.p; a.ws = sl.d_plan_ws.p;
        HIP_OK(fx_launch_plan(st, c->plan_grid ? c->plan_grid : (unsigned)std::min<uint64_t>(64, c->traffic.frames / 2048 + 1), c->plan_fused ? 1 : 0, c->plan_threads, a));
    }
    const int tl = sl.timing_level;
    if (tl >= 2) HIP_OK(hipEventRecord(sl.ev[kEvPlan], st));
    if (c->debug_stop_after == 4) { c->carry_reader[b % 3] = nullptr; HIP_OK(hipEventRecord(sl.ev[kEvDone], st)); return 0; }
    if (!detect) {
        // grids stride over lists whose lengths only the device knows; size them from what the last collected block held, as it stands now
        // (a replay plans again).  What a launch did not cover is decoded when the block is collected (finish_decode).
        const TailPlan plan = plan_tail(c->traffic, TailCaps{ chain_slots, sl.mf_cap, sl.vb_cap, sl.vb_blk }, TailKnobs{ c->depth, c->n_cus, c->mf_per_cu, c->vb_debug, c->vb_early_tail, c->vb_clean });
        HIP_OK(fx_launch_paymf(plan.mf_grid, c->cfg.equalizer ? 1 : 0, st, sl.d_pjobs.p, sl.d_mf_job.p, sl.d_mf_c0.p, sl.hdr_pay(), sl.d_chain.p, sl.d_symraw.p, c->d_tables));
        HIP_OK(hipEventRecord(sl.ev[kEvMf], st));
        c->carry_reader[b % 3] = sl.ev[kEvMf];
        if (c->debug_stop_after == 5) { HIP_OK(hipEventRecord(sl.ev[kEvDone], st)); return 0; }
        // ---- the block's tail: its grids now, its launches now or with the gang (launch_tails) ----
        sl.tail = plan;
        if (sl.vb_blk && c->traffic.trellis_left) c->traffic.trellis_left--;
        sl.timing.trellis_launched = plan.vb_fin ? 1 : 0;
        // Deferred into the open gang when there is enough ahead of this block to keep the queues busy meanwhile: a deep pipeline
        // (depth >= 4), the traffic known (not the first block), no more events than the PLL's pair, and at least a gang's worth of
        // blocks in flight in front of it whose tails are out.  Anything else goes at once, alone, behind whatever the gang holds.
        unsigned ahead = 0;
        for (unsigned k = 0; k < c->inflight; k++) ahead += c->slots[(c->tail + k) % (c->depth + 1)]->tail_launched ? 1u : 0u;
        const unsigned G = c->tail_gang;
        if (G >= 2 && may_defer && c->depth >= 4 && c->traffic.seen && !c->debug_stop_after && tl <= 1 && ahead >= G) {
            sl.tail_launched = false; sl.tail_st = nullptr;
            c->gang.push_back(&sl);
            return c->gang.size() >= G ? close_gang(c) : 0;
        }
        { const int r = close_gang(c); if (r) return r; }
        Slot *one = &sl;
        return launch_tails(c, &one, 1u);
    } else {
        // (in front of the event the next-but-one block's chain kernel waits for before it writes over the carried tail this one reads)
        if (c->cfg.want_framesyms) HIP_OK(launch_detwin(c, sl, 0u, sl.win_reserved, false));
        HIP_OK(hipEventRecord(sl.ev[kEvMf], st));
        if (tl >= 1) HIP_OK(hipEventRecord(sl.ev[kEvPll], st));
        if (tl >= 2) HIP_OK(hipEventRecord(sl.ev[kEvDec], st));
        c->carry_reader[b % 3] = sl.ev[kEvMf];
    }
    HIP_OK(hipEventRecord(sl.ev[kEvDone], st));
    return 0;
}

// The input of a block, every format: the argument checks, a route per stream with new samples (fx_ingestplan.h), and whatever the
// routes write to, reserved for ALL streams.  Nothing is enqueued: the block's sample pointers (sl.x) and the list of uploads and
// conversions stay in the slot for enqueue_front.
static int prepare_ingest(fxrx_ctx_s *c, Slot &sl, const void *const *iq, const uint64_t *n_samples, int on_device, int fmt)
{
    const unsigned NS = c->cfg.n_streams;
    const bool flt = fmt == FXRX_IQ_FC32; const size_t bytes = iq_sample_bytes(fmt);
    sl.ingest.clear(); sl.x.assign(NS, nullptr);
    for (unsigned s = 0; s < NS && !flt; s++)
        if (n_samples[s] && (!iq[s] || (reinterpret_cast<uintptr_t>(iq[s]) & (bytes - 1)))) {
            set_err("fxrx_submit_fmt: integer IQ must be aligned to its sample size (sc16: 4 bytes, sc8: 2 bytes)"); return FXRX_ERR_ARG;
        }
    if (sl.d_in.size() < NS) { sl.d_in.resize(NS); sl.d_raw.resize(NS); }
    std::vector<IngestJob> jobs;
    for (unsigned s = 0; s < NS; s++) {
        if (flt && on_device) { sl.x[s] = static_cast<const float2 *>(iq[s]); continue; }     // kRouteInPlace: nothing to launch
        const uint64_t nn = n_samples[s]; const uintptr_t addr = reinterpret_cast<uintptr_t>(iq[s]);
        if (sl.d_in[s].reserve(nn + 1)) return FXRX_ERR_HIP;
        sl.x[s] = sl.d_in[s].p;
        IngestJob j{ s, kRouteNone, iq[s], nn };
        // (whether the memory is page-locked takes a call into the runtime: asked only where the answer changes the route)
        const bool locked = nn && !on_device && kernel_may_read_host(fmt, addr, nn, c->ingest_limits) && pinned_device_ptr(iq[s], &j.src);
        j.route = ingest_route(fmt, on_device != 0, locked, addr, nn, c->ingest_limits);
        if (j.route == kRouteConvertCopy && sl.d_raw[s].reserve(nn * bytes + 16)) return FXRX_ERR_HIP;
        if (j.route != kRouteNone) jobs.push_back(j);
    }
    sl.ingest.swap(jobs); sl.ingest_fmt = fmt; sl.ingest_scale = c->iq_scale[fmt];
    return 0;
}

// fxrx_debug_block_times: a common origin of the GPU's and the host's clocks, taken once per context
static void clock_origin(fxrx_ctx_s *c, hipStream_t st)
{
    if (c->timing_level < 2 || c->ref_event || hipEventCreate(&c->ref_event) != hipSuccess) return;
    (void)hipEventRecord(c->ref_event, st); (void)hipEventSynchronize(c->ref_event);
    c->ref_host_ms = prof_now();
}
// fxrx_submit in three steps.  A submit that fails for a reason the caller can mend fails in the first two, which write to the block's
// slot and to nothing else: the context is as it was, nothing is enqueued that reads the caller's buffers, and the next block -- the
// same samples again, or others -- continues from the state before the call.
static int submit_block(fxrx_ctx *c, const void *const *iq, const uint64_t *n_samples, int on_device, int fmt)
{
    if (!c || !iq || !n_samples) { set_err("fxrx_submit: null argument"); return FXRX_ERR_ARG; }
    if (iq_sample_bytes(fmt) == 0) { set_err("fxrx_submit_fmt: unknown IQ format"); return FXRX_ERR_ARG; }
    if (c->inflight >= c->depth) { set_err("fxrx_submit: pipeline full, call fxrx_collect first"); return FXRX_ERR_STATE; }
    HIP_OK(hipSetDevice(c->cfg.device));
    const double t_enter = prof_now(); double t = t_enter;
    const unsigned NS = c->cfg.n_streams;
    Slot &sl = *c->slots[c->head];
    // ---- stage: the block's snapshot of every stream, its plan, its input routes, its descriptors.  No call on a HIP stream; the
    // streams' successor state is worked out in `next`, not in the context ----
    sl.out.clear(); sl.timing = fxrx_timing{}; sl.kept_hops = sl.kept_cheap = sl.kept_vhops = sl.kept_vfail = sl.kept_repairs = 0;
    sl.seq = c->seq; sl.force_noskip = c->noskip_left > 0;
    sl.n.assign(n_samples, n_samples + NS); sl.snap.assign(NS, StreamSnap{});
    std::vector<StreamState> next = c->st;
    for (unsigned s = 0; s < NS; s++) {
        const StreamState &S = c->st[s]; StreamState &N = next[s]; StreamSnap &sn = sl.snap[s];
        const uint64_t nn = n_samples[s];
        sl.timing.samples += nn; if (N.noskip_left) N.noskip_left--;
        sn.tot0 = S.total; sn.fresh_start = S.fresh_start; sn.carry_bound = S.fresh_start ? 0 : S.carry_bound; sn.noskip = S.noskip_left > 0;
        N.total += (int64_t)nn; N.fresh_start = false; N.carry_bound = std::min<int64_t>(S.carry_cap, sn.carry_bound + (int64_t)nn);
    }
    FrontBuild fb;
    prof_lap(0, &t);
    { const int r = plan_front(c, sl, fb.plan); if (r) return r; }           // (first: a batch too large fails before any staging buffer is sized for it)
    prof_lap(1, &t);
    { const int r = prepare_ingest(c, sl, iq, n_samples, on_device, fmt); if (r) return r; }
    prof_lap(0, &t);
    build_descriptors(c, sl, fb); prof_lap(1, &t);
    // ---- reserve: every buffer of the block.  The last point at which a submit fails and the caller can mend it ----
    { const int r = reserve_block(c, sl, fb); if (r) return r; }
    if (c->debug_fail_submit) { c->debug_fail_submit--; set_err("fxrx_submit: injected failure (fxrx_debug_fail)"); return FXRX_ERR_STATE; }
    // ---- enqueue: the input's uploads and conversions, then the chain; then the context moves on.  enqueue_back changes the context
    // once launches have begun (inchain_left, traffic.trellis_left, prev_chain, carry_reader, the open gang): only a HIP launch error
    // can follow those, and that is fatal to the context -- every later call fails the same way ----
    clock_origin(c, sl.st); sl.dbg_submit_ms = t_enter - c->ref_host_ms;
    { const int r = launch_block(c, sl, fb, /* may_defer */ true, &t); if (r) return r; }
    c->st.swap(next); if (c->noskip_left) c->noskip_left--;
    c->seq++; sl.busy = true; c->head = (c->head + 1) % (c->depth + 1); c->inflight++;
    sl.host_submit_ms = prof_now() - t_enter;
    return 0;
}

int fxrx_submit(fxrx_ctx *c, const void *const *iq, const uint64_t *n_samples, int on_device) { return submit_block(c, iq, n_samples, on_device, FXRX_IQ_FC32); }
int fxrx_submit_fmt(fxrx_ctx *c, const void *const *iq, const uint64_t *n_samples, int on_device, int fmt) { return submit_block(c, iq, n_samples, on_device, fmt); }

unsigned int fxrx_iq_sample_bytes(int fmt) { return iq_sample_bytes(fmt); }

int fxrx_set_iq_scale(fxrx_ctx *c, int fmt, float scale)
{
    if (!c || (fmt != FXRX_IQ_SC16 && fmt != FXRX_IQ_SC8) || !std::isfinite(scale) || !(scale > 0.0f)) { set_err("fxrx_set_iq_scale: bad argument"); return FXRX_ERR_ARG; }
    c->iq_scale[fmt] = scale;
    return 0;
}

// the definition of an integer sample: one exact conversion, one binary32 multiply (this file is compiled with -ffp-contract=off)
int fxrx_iq_convert_host(int fmt, float scale, const void *in, uint64_t n_samples, float *out_re_im)
{
    if (iq_sample_bytes(fmt) == 0 || (n_samples && (!in || !out_re_im))) { set_err("fxrx_iq_convert_host: bad argument"); return FXRX_ERR_ARG; }
    const uint64_t nc = 2 * n_samples;
    if (fmt == FXRX_IQ_FC32) { if (nc) std::memcpy(out_re_im, in, nc * sizeof(float)); }
    else if (fmt == FXRX_IQ_SC16) { const int16_t *q = static_cast<const int16_t *>(in); for (uint64_t i = 0; i < nc; i++) out_re_im[i] = (float)q[i] * scale; }
    else { const int8_t *q = static_cast<const int8_t *>(in); for (uint64_t i = 0; i < nc; i++) out_re_im[i] = (float)q[i] * scale; }
    return 0;
}

// Two things the device cannot finish by itself, both rare, both handled here when the block concerned is collected:
//  * FX_BLK_NEEDS_REPAIR: the lean chain kernel met a stretch that has to be walked again (a hand-off target missing from
//    the next list, a skipped hop on which the exact detector fires, a full frame table).  The full-size chain kernel does
//    that; the block's back part (chain, plan, payload) is enqueued again with it.
//  * FX_BLK_CARRY_OVERFLOW: a tail did not fit its carry buffer.  The block's own results are good; the buffers are grown
//    and the tail is copied by hand.
// Either way the state the block left was marked invalid, so every block behind it did nothing: they are enqueued again,
// in order, once the state is there.
// Repair rounds.  The lean chain kernel, asked to, rewrites the job of every segment whose predecessor's hand-off target it
// cannot find -- start / floor / fresh := the predecessor's hand-off hop state, exact detector on every hop -- and lists
// those segments; they are walked again, all at once, and the chain kernel runs again: a re-walked segment is entered plainly
// when its predecessor still hands over that state (it does unless the predecessor was itself re-walked and ended
// differently: then the next round mends it).  Low SNR is where this matters: marginal detections depend on where the
// detector's hops happen to fall, so speculative lists and true chain disagree dozens of times per block, and the
// full-size chain kernel would walk those stretches one after the other.  Returns 0: stitched, 1: leave it to that kernel.
static int repair_rounds(fxrx_ctx_s *c, Slot &sl)
{
    if (c->chain_slow) return 1;
    hipStream_t st = sl.st; FxBlockHdr *hdr = sl.hdr_walk();
    for (int round = 0; round < 64; round++) {
        HIP_OK(hipMemsetAsync(hdr, 0, sizeof(FxBlockHdr), st));
        HIP_OK(launch_chainfast(c, sl, st, kStitchQueue));
        FxBlockHdr hh;
        HIP_OK(hipMemcpyAsync(&hh, hdr, sizeof hh, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        if (std::getenv("FXRX_DEBUG_ROUNDS")) std::fprintf(stderr, "[fxrx] repair round %d: flags %x requests %u\n", round, hh.flags, hh.n_repair_req);
        if (!(hh.flags & FX_BLK_NEEDS_REPAIR)) return 0;          // (hdr keeps what the chain kernel left there -- flags, stamps -- for the plan kernel)
        if ((hh.flags & FX_BLK_NEEDS_SLOW) || hh.n_repair_req == 0 || hh.n_repair_req > 2 * sl.NJ) break;   // (a segment is queued at most twice: as a miss target and for a fired hop)
        {   // streams in which a skipped hop fired: their next blocks are walked with the exact detector on every hop from the start
            std::vector<uint32_t> req(hh.n_repair_req);
            HIP_OK(hipMemcpyAsync(req.data(), sl.d_req.p, req.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            HIP_OK(hipStreamSynchronize(st));
            mark_noskip(c, sl, req);
        }
        HIP_OK(hipMemsetAsync(hdr, 0, sizeof(FxBlockHdr), st));
        HIP_OK(launch_walk(c, sl, st, sl.d_req.p, hh.n_repair_req, kWalkRequests));
        HIP_OK(hipMemcpyAsync(&hh, hdr, sizeof hh, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        sl.kept_hops += hh.hops; sl.kept_cheap += hh.hops_cheap; sl.kept_repairs += hh.walk_jobs_run ? hh.walk_jobs_run : 0;
    }
    HIP_OK(hipMemsetAsync(hdr, 0, sizeof(FxBlockHdr), st));
    return 1;
}

static int repair_and_replay(fxrx_ctx_s *c, Slot &sl)
{
    const unsigned NS = c->cfg.n_streams;
    const unsigned nslots = c->depth + 1;
    // Blocks behind this one that continue its streams started from the state it failed to leave: they are enqueued again
    // afterwards (and are drained first: a true walker must not read a state entry while it is being rewritten).  Blocks whose
    // streams all start afresh (separate captures) never looked at it; they, and whatever continues *them*, run on untouched.
    unsigned n_dep = 0;
    for (unsigned k = 1; k < c->inflight; k++) {
        const Slot &nx = *c->slots[(c->tail + k) % nslots];
        bool dep = false;
        for (unsigned s = 0; s < NS; s++) dep = dep || !nx.snap[s].fresh_start;
        if (!dep) break;
        n_dep++;
    }
    const hipEvent_t newest_chain = c->prev_chain;
    bool carry_moved = false;
    // (blocks behind this one may sit in the open gang: their tails go out now, so that every block in flight is on streams that
    // can be drained; the tails enqueued from here are replays and go alone)
    { const int r = close_gang(c); if (r) return r; }
    for (int round = 0; round < 6; round++) {
        HIP_OK(hipStreamSynchronize(sl.st));
        for (unsigned k = 1; k <= n_dep; k++) {
            const Slot &nx = *c->slots[(c->tail + k) % nslots];
            HIP_OK(hipStreamSynchronize(nx.st));
            if (nx.tail_st && nx.tail_st != nx.st) HIP_OK(hipStreamSynchronize(nx.tail_st));      // (its tail ran with a gang, on another block's stream)
        }
        const uint32_t flags = sl.h_hdr.p->flags;
        if (std::getenv("FXRX_DEBUG_ROUNDS")) std::fprintf(stderr, "[fxrx] block %llu at collect: flags %x verify_failures %u (pass %d)\n", (unsigned long long)sl.seq, flags, sl.h_hdr.p->verify_failures, round);
        if (flags & FX_BLK_NEEDS_REPAIR) {
            c->repairs_host++; c->inchain_left = 16;
            const FxBlockHdr &h0 = *sl.h_hdr.p;         // the walk-phase counters are zeroed with the first plan kernel: keep them
            sl.kept_hops += h0.hops; sl.kept_cheap += h0.hops_cheap; sl.kept_vhops += h0.verify_hops; sl.kept_vfail += h0.verify_failures;
            sl.ps_taken += h0.ps_taken; sl.ps_fallback += h0.ps_fallback;
            if (!sl.force_noskip && c->cfg.mode != FXRX_MODE_DETECTOR && c->skip_seek && h0.verify_failures > std::max<uint32_t>(16u, (uint32_t)sl.NJ / 8u)) {
                // Skipped hops on which the exact detector fires, all over the block (weak preambles, false alarms: low SNR; a
                // few of them are mended segment by segment in the repair rounds below).  Walk the block
                // again, all segments in parallel, with the exact detector on every hop -- exact by itself, nothing to
                // verify -- and stay in that mode for the next blocks: the channel will not have improved meanwhile.
                sl.force_noskip = true; c->noskip_left = 32;
                if (enqueue_block(c, sl)) return FXRX_ERR_HIP;
            } else {
                // What is left: hand-off targets that the next segment's list does not hold.  Repair rounds mend those in parallel;
                // anything else (or a block that does not settle) goes through the full-size chain kernel, one workgroup per stream.
                const int rr = repair_rounds(c, sl);
                if (rr < 0 || enqueue_back(c, sl, rr == 0 ? kChainDone : kChainFull)) return FXRX_ERR_HIP;
            }
            continue;                                   // (its tail may in turn overflow the carry buffer)
        }
        if (!(flags & FX_BLK_CARRY_OVERFLOW)) break;
        const uint64_t b = sl.seq;
        FxStreamState *hs = c->h_state + (b % kStateRing) * NS, *ds = c->d_state + (b % kStateRing) * NS;
        for (auto &o : c->slots) if (o->busy) HIP_OK(hipStreamSynchronize(o->st));      // (carry buffers are about to move under every block in flight)
        carry_moved = true;
        for (unsigned s = 0; s < NS; s++) {
            if (!hs[s].overflow) continue;
            StreamState &S = c->st[s];
            const int64_t keep = hs[s].carry_len, old_cap = S.carry_cap;
            float2 *old[3] = { S.carry[0], S.carry[1], S.carry[2] };
            S.carry[0] = S.carry[1] = S.carry[2] = nullptr;
            int64_t cap = std::max<int64_t>(2 * old_cap, 2 * keep); cap = (cap + 4095) & ~(int64_t)4095;
            if (alloc_carry(S, cap)) return FXRX_ERR_HIP;
            // tail = logical samples [n - keep, n) of block b: a piece of its own carried tail (old buffer b % 3), then its new samples
            const int64_t nb = (int64_t)sl.n[s], from = nb - keep;
            float2 *dst = S.carry[(b + 1) % 3] + cap - keep;
            if (from < 0) HIP_OK(hipMemcpy(dst, old[b % 3] + old_cap + from, (size_t)(-from) * sizeof(float2), hipMemcpyDeviceToDevice));
            const int64_t n_new = std::min<int64_t>(keep, nb);
            if (n_new > 0) HIP_OK(hipMemcpy(dst + (keep - n_new), sl.x[s] + (nb - n_new), (size_t)n_new * sizeof(float2), hipMemcpyDeviceToDevice));
            for (auto p : old) if (p) (void)hipFree(p);
            hs[s].overflow = 0; hs[s].invalid = 0;
            HIP_OK(hipMemcpy(ds + s, hs + s, sizeof(FxStreamState), hipMemcpyHostToDevice));
        }
        sl.h_hdr.p->flags &= ~(uint32_t)FX_BLK_CARRY_OVERFLOW;
        c->replays++;
        break;
    }
    if (sl.h_hdr.p->flags & (FX_BLK_NEEDS_REPAIR | FX_BLK_CARRY_OVERFLOW)) { set_err("fxrx_collect: block could not be repaired"); return FXRX_ERR_STATE; }
    if (sl.h_hdr.p->flags & FX_BLK_CHAIN_FULL) { set_err("fxrx_collect: chain table overflow (internal sizing error)"); return FXRX_ERR_STATE; }
    // the blocks behind it, oldest first (descriptors are rebuilt: carry buffers may have moved)
    c->prev_chain = sl.ev[kEvChain];
    const unsigned n_replay = carry_moved ? c->inflight - 1 : n_dep;
    for (unsigned k = 1; k <= n_replay; k++) {
        Slot &nx = *c->slots[(c->tail + k) % nslots];
        for (unsigned s = 0; s < NS; s++) if (!nx.snap[s].fresh_start) nx.snap[s].carry_bound = c->st[s].carry_cap;
        int r = enqueue_block(c, nx);
        if (r) return r;
    }
    if (n_replay + 1 < c->inflight) c->prev_chain = newest_chain;      // (the newest block in flight was not touched: the next block waits for its chain)
    for (auto &S : c->st) S.carry_bound = S.carry_cap;
    return 0;
}

// frames the decode launches of the chain did not cover (more frames than the grid sized from the previous block, or
// Reed-Solomon frames turning up unannounced): decode them now, on the block's stream, and wait
static int finish_decode(fxrx_ctx_s *c, Slot &sl)
{
    FxBlockHdr *hdr_pay = sl.hdr_pay();
    // frames the batch path handed back: how many (the block is done: a plain copy)
    auto fetch_fb = [&]() -> int { uint32_t nfb = 0; HIP_OK(hipMemcpy(&nfb, &hdr_pay->n_vb_fallback, sizeof nfb, hipMemcpyDeviceToHost)); sl.h_hdr.p->n_vb_fallback = nfb; sl.h_hdr.p->vb_ticket = 0; return 0; };
    if (sl.vb_blk && sl.h_hdr.p->vb_ticket && fetch_fb()) return FXRX_ERR_HIP;
    FxBlockHdr h = *sl.h_hdr.p; h.vb_dirty = *(volatile const uint32_t *)&sl.h_hdr.p->vb_dirty;
    TailPlan &p = sl.tail;
    const LateWork w = late_work(p, h, sl.vb_blk);
    if (!w.any()) return 0;
    HIP_OK(launch_decoders(c, sl, sl.st, p.plain, w.more_plain ? h.n_dec_plain - p.plain : 0u, w.more_rs ? h.n_dec_rs : 0u));
    // late_trellis: fx_vbpre_kernel met a frame that is not clean and the trellis kernels were not launched: they run now, over all items (clean
    // frames' items are off, their waves of the back part leave at once); fx_vbpre_kernel itself is done and is not needed again
    if (w.more_batch() || w.late_trellis) {       // (all parts again, for all of the path's frames: they are idempotent -- but for the fallback list, which starts over)
        HIP_OK(hipMemsetAsync(&hdr_pay->n_vb_fallback, 0, sizeof(uint32_t), sl.st));
        if (w.more_batch()) {
            FxVbpreGang g; g.n = 1; g.m[0] = vbpre_member(sl, 0u, h.n_dec_batch);
            HIP_OK(fx_launch_vbpre(&g, sl.st, c->d_tables, c->vb_clean ? 1 : 0, p.vb_early ? 1 : 0));
        }
        HIP_OK(launch_trellis(c, sl, sl.st, h.n_vb_items, 1, 1, h.n_dec_batch, kFallbackWaves));
        p.vb_pre = p.vb_fin = h.n_dec_batch; p.vb_items = h.n_vb_items; p.fb = kFallbackWaves;
        HIP_OK(hipStreamSynchronize(sl.st));
        if (fetch_fb()) return FXRX_ERR_HIP;
    }
    const uint32_t n_fb = *(volatile const uint32_t *)&sl.h_hdr.p->n_vb_fallback;
    if (sl.vb_blk && n_fb > p.fb) {
        HIP_OK(launch_paydec(c, sl, sl.st, kDecFallback, p.fb, n_fb - p.fb, c->dec_waves));
        p.fb = n_fb;
    }
    HIP_OK(hipStreamSynchronize(sl.st));
    p.plain = std::max(p.plain, h.n_dec_plain); if (w.more_rs) p.rs = h.n_dec_rs;
    c->late_decodes++;
    w.count(c->late_reason);
    return 0;
}

// Detector mode with want_framesyms: a block with more detections than window slots were reserved for it.  The slots are grown to the
// count -- what is there is kept -- and fx_detwin_kernel runs for the rest, from the block's input (valid until now: the API asks for
// that).  Windows that start in the carried tail, which is not, were written with the chain (fx_detwin.hip).
static int finish_windows(fxrx_ctx_s *c, Slot &sl)
{
    if (*(volatile const uint32_t *)sl.h_winflag.p) { set_err("fxrx_collect: more than two detections of a stream start in its carried tail (internal sizing error)"); return FXRX_ERR_STATE; }
    const uint32_t n = sl.h_hdr.p->n_frames;
    if (n <= sl.win_reserved) return 0;
    { const int r = sl.h_win.grow_keep((size_t)n * FX_NFFT, (size_t)sl.win_reserved * FX_NFFT); if (r) return r; }     // (n > win_reserved: every reserved slot was written)
    HIP_OK(launch_detwin(c, sl, sl.win_reserved, n, true));
    HIP_OK(hipStreamSynchronize(sl.st));
    c->late_windows++;
    return 0;
}

// A block that cannot be completed takes the blocks in flight behind it along (they continue its streams, or at least share its
// arenas' fate): everything in flight is dropped, the slots' device-side counters are cleared, and every stream restarts from a
// freshly reset synchroniser with its next block -- sample positions keep counting, the dropped samples are simply never
// searched.  The context stays usable (unless the HIP runtime itself is gone: then every later call fails the same way).
static void discard_inflight(fxrx_ctx_s *c)
{
    const std::string keep = g_err;
    (void)close_gang(c);
    sync_all(c);
    const unsigned nslots = c->depth + 1;
    while (c->inflight) {
        Slot &s = *c->slots[c->tail];
        s.busy = false; s.out.clear();
        c->tail = (c->tail + 1) % nslots; c->inflight--; c->discarded++;
    }
    for (auto &s : c->slots) {
        if (s->d_hdr.p) (void)hipMemset(s->d_hdr.p, 0, 2 * sizeof(FxBlockHdr));
        if (s->d_plan_ws.p) (void)hipMemset(s->d_plan_ws.p, 0, fx_plan_ws_words() * sizeof(uint32_t));
        if (s->h_hdr.p) std::memset(s->h_hdr.p, 0, sizeof(FxBlockHdr));
    }
    for (auto &S : c->st) { S.fresh_start = true; S.carry_bound = 0; }
    c->last = nullptr; c->prev_chain = nullptr;
    for (auto &e : c->carry_reader) e = nullptr;
    set_err(keep);
}

static int collect_block(fxrx_ctx_s *c);

int fxrx_collect(fxrx_ctx *c)
{
    if (!c) return FXRX_ERR_ARG;
    if (!c->inflight) { set_err("fxrx_collect: nothing in flight"); return FXRX_ERR_STATE; }
    const int r = collect_block(c);
    if (r < 0) discard_inflight(c);
    return r;
}

int fxrx_ready(fxrx_ctx *c)
{
    if (!c) return FXRX_ERR_ARG;
    if (!c->inflight) return 0;
    if (!c->slots[c->tail]->tail_launched) {                   // still in the open gang: out with it, or a caller that polls would wait for ever
        if (hipSetDevice(c->cfg.device) != hipSuccess || close_gang(c)) return FXRX_ERR_HIP;
    }
    const hipError_t e = hipEventQuery(c->slots[c->tail]->ev[kEvDone]);
    return e == hipSuccess ? 1 : (e == hipErrorNotReady ? 0 : FXRX_ERR_HIP);
}

unsigned int fxrx_inflight(const fxrx_ctx *c) { return c ? c->inflight : 0; }

// of the last collected block: speculative jobs whose first hops fx_prescan_kernel scanned | those that took their first
// candidate from its table | those whose table held none (their own scan carried on behind the scanned hops)
int fxrx_debug_prescan_stats(const fxrx_ctx *c, uint64_t out[3])
{
    if (!c || !c->last || !out) return FXRX_ERR_ARG;
    out[0] = c->last->ps_jobs; out[1] = c->last->ps_taken; out[2] = c->last->ps_fallback;
    return 0;
}

// tests, no device: what a speculative walker makes of `words` (fx_common.h: fx_prescan_valid_hops, fx_prescan_entry).  Returns 1
// when a chunk word holds a hit; out[0] = where the walk goes on, out[1] = hops added to the cheap-hop counter, out[2] = hops scanned
int fxrx_debug_prescan_words(const uint32_t *words, uint32_t n_words, uint32_t K, int64_t start, int64_t stop, int64_t n, int64_t out[3])
{
    if (!out || (n_words && !words)) return FXRX_ERR_ARG;
    const uint32_t hops = fx_prescan_valid_hops(start, stop, n, K);
    int64_t p = 0; uint32_t scanned = 0;
    const bool took = fx_prescan_entry(words, n_words, hops, start, &p, &scanned);
    out[0] = p; out[1] = scanned; out[2] = hops;
    return took ? 1 : 0;
}

int fxrx_debug_gang_stats(const fxrx_ctx *c, uint64_t out[2])
{
    if (!c || !out) return FXRX_ERR_ARG;
    out[0] = c->gang_launches; out[1] = c->gang_members;
    return 0;
}

// out[0..5]: collected blocks so far that finish_decode completed because of -- plain frames beyond the launch | Reed-Solomon frames without
// a launch | batch-path frames beyond the launch | trellis work items beyond the launch | handed-back frames beyond the fallback launch |
// frames that were not clean in a chain without the trellis kernels; out[6..9]: n_dec_plain, n_dec_batch, n_dec_rs, n_vb_items of the last collected block
int fxrx_debug_late_stats(const fxrx_ctx *c, uint64_t out[10])
{
    if (!c || !out) return FXRX_ERR_ARG;
    for (int i = 0; i < 6; i++) out[i] = c->late_reason[i];
    const FxBlockHdr *h = c->last ? c->last->h_hdr.p : nullptr;
    out[6] = h ? h->n_dec_plain : 0; out[7] = h ? h->n_dec_batch : 0; out[8] = h ? h->n_dec_rs : 0; out[9] = h ? h->n_vb_items : 0;
    return 0;
}

int fxrx_debug_gang_open(const fxrx_ctx *c) { return c ? (int)c->gang.size() : FXRX_ERR_ARG; }

int fxrx_debug_fail(fxrx_ctx *c, unsigned int submits, unsigned int collects)
{
    if (!c) return FXRX_ERR_ARG;
    c->debug_fail_submit = submits; c->debug_fail_collect = collects;
    return 0;
}

int fxrx_debug_header_decode(int soft, const uint8_t *in, unsigned int n, uint8_t *out20, int *valid)
{
    static_assert(sizeof(int) == sizeof(int32_t), "the kernel writes int32_t flags");
    if (!in || !out20 || !valid) return FXRX_ERR_ARG;
    if (n == 0) return 0;
    return debug_decode("fxrx_debug_header_decode", in, (size_t)n * (soft ? 8 * FX_HDR_ENC : FX_HDR_ENC), 0, out20, (size_t)n * FX_HDR_DEC, valid, (size_t)n * sizeof(int32_t),
                        [&](const uint8_t *d_in, uint8_t *d_out, uint8_t *d_valid, const FxTables *d_t) {
                            return fx_launch_hdrdec(soft ? 1 : 0, n, nullptr, d_in, d_out, reinterpret_cast<int32_t *>(d_valid), d_t);
                        });
}

int fxrx_debug_block_decode(unsigned int fec, int soft, unsigned int n, unsigned int count, const uint8_t *in, uint8_t *out)
{
    if (!is_block_fec(fec) || !in || !out || n == 0 || n > kDebugMaxN) { set_err("fxrx_debug_block_decode: bad argument"); return FXRX_ERR_ARG; }
    if (count == 0) return 0;
    return debug_decode("fxrx_debug_block_decode", in, (size_t)count * fx::fec_enc_len(fec, n) * (soft ? 8 : 1), 0, out, (size_t)count * n, nullptr, 0,
                        [&](const uint8_t *d_in, uint8_t *d_out, uint8_t *, const FxTables *d_t) { return fx_launch_blkdec(soft ? 1 : 0, fec, n, count, nullptr, d_in, d_out, d_t); });
}

int fxrx_debug_block_siso(unsigned int fec, unsigned int n, unsigned int count, const uint8_t *in, uint8_t *out_soft)
{
    if (!is_block_fec(fec) || !in || !out_soft || n == 0 || n > kDebugMaxN) { set_err("fxrx_debug_block_siso: bad argument"); return FXRX_ERR_ARG; }
    if (count == 0) return 0;
    // (16 spare input bytes: the decoders load whole words)
    return debug_decode("fxrx_debug_block_siso", in, (size_t)count * fx::fec_enc_len(fec, n) * 8, 16, out_soft, (size_t)count * n * 8, nullptr, 0,
                        [&](const uint8_t *d_in, uint8_t *d_out, uint8_t *, const FxTables *d_t) { return fx_launch_blksiso(fec, n, count, nullptr, d_in, d_out, d_t); });
}

int fxrx_debug_rs_soft(unsigned int n, unsigned int count, const uint8_t *in_soft, uint8_t *out, uint8_t *chosen_f)
{
    if (!in_soft || !out || !chosen_f || n == 0 || n > kDebugMaxN) { set_err("fxrx_debug_rs_soft: bad argument"); return FXRX_ERR_ARG; }
    if (count == 0) return 0;
    unsigned nb, dl; fx::rs_dims(n, nb, dl);
    return debug_decode("fxrx_debug_rs_soft", in_soft, (size_t)count * fx::fec_enc_len(FX_FEC_RS_M8, n) * 8, 0, out, (size_t)count * n, chosen_f, (size_t)count * nb,
                        [&](const uint8_t *d_in, uint8_t *d_out, uint8_t *d_f, const FxTables *d_t) { return fx_launch_rssoft(n, count, nullptr, d_in, d_out, d_f, d_t); });
}

int fxrx_debug_rs_chain(unsigned int n, unsigned int count, int fmax, int chain, const uint8_t *in_soft, uint8_t *out, uint8_t *chosen_f)
{
    if (!in_soft || !out || !chosen_f || n == 0 || n > kDebugMaxN || fmax < 0 || fmax > 32 || (fmax & 1)) { set_err("fxrx_debug_rs_chain: bad argument"); return FXRX_ERR_ARG; }
    if (count == 0) return 0;
    unsigned nb, dl; fx::rs_dims(n, nb, dl);
    return debug_decode("fxrx_debug_rs_chain", in_soft, (size_t)count * fx::fec_enc_len(FX_FEC_RS_M8, n) * 8, 0, out, (size_t)count * n * (chain ? 8 : 1), chosen_f, (size_t)count * nb,
                        [&](const uint8_t *d_in, uint8_t *d_out, uint8_t *d_f, const FxTables *d_t) { return fx_launch_rschain(n, count, (unsigned)fmax, chain ? 1 : 0, nullptr, d_in, d_out, d_f, d_t); });
}

static int collect_block(fxrx_ctx_s *c)
{
    HIP_OK(hipSetDevice(c->cfg.device));
    const unsigned NS = c->cfg.n_streams;
    const unsigned nslots = c->depth + 1;
    Slot &sl = *c->slots[c->tail];
    const auto tw = std::chrono::steady_clock::now();
    // (a block whose tail is still deferred has no ev[kEvDone] to wait for: waiting on the event as an earlier use left it would return at once)
    if (!sl.tail_launched) { const int r = close_gang(c); if (r) return r; }
    if (!sl.tail_launched) { set_err("fxrx_collect: block without a tail (internal error)"); return FXRX_ERR_STATE; }
    HIP_OK(hipEventSynchronize(sl.ev[kEvDone]));
    // what collect still enqueues for this block goes to its own stream: behind the tail, wherever that ran
    if (sl.tail_st != sl.st) { HIP_OK(hipStreamWaitEvent(sl.st, sl.ev[kEvDone], 0)); sl.tail_st = sl.st; }
    if (c->debug_fail_collect) { c->debug_fail_collect--; set_err("fxrx_collect: injected failure (fxrx_debug_fail)"); return FXRX_ERR_STATE; }
    {
        const uint32_t flags = sl.h_hdr.p->flags;
        if (flags & FX_BLK_CHAIN_FULL) { set_err("fxrx_collect: chain table overflow (internal sizing error)"); return FXRX_ERR_STATE; }
        // (an invalid block sits behind an overflowing one, whose collect replays it before it is collected itself)
        if (flags & FX_BLK_INVALID) { set_err("fxrx_collect: block has no valid start state"); return FXRX_ERR_STATE; }
        if (flags & (FX_BLK_CARRY_OVERFLOW | FX_BLK_NEEDS_REPAIR)) { int r = repair_and_replay(c, sl); if (r) return r; }
    }
    sl.dbg_collect_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count() - c->ref_host_ms;
    if (sl.timing_level >= 2 && c->ref_event) { float m = 0; (void)hipEventElapsedTime(&m, c->ref_event, sl.ev[kEvStart]); sl.dbg_gpu_start_ms = m; (void)hipEventElapsedTime(&m, c->ref_event, sl.ev[kEvDone]); sl.dbg_gpu_done_ms = m; }
    if (c->debug_stop_after) { sl.out.clear(); sl.busy = false; c->last = &sl; c->tail = (c->tail + 1) % nslots; c->inflight--; return 0; }
    if (c->cfg.mode != FXRX_MODE_DETECTOR) { int r = finish_decode(c, sl); if (r) return r; }
    else if (c->cfg.want_framesyms) { int r = finish_windows(c, sl); if (r) return r; }
    if (sl.h_hdr.p->n_repair_req) c->inchain_left = 16;
    if (sl.h_hdr.p->n_repair_req && sl.h_hdr.p->verify_failures) {
        // the chain mended something by itself; the list says in which streams a skipped hop fired (a rare, small copy)
        std::vector<uint32_t> req(std::min<size_t>(sl.h_hdr.p->n_repair_req, 2 * sl.NJ + 16));
        HIP_OK(hipMemcpy(req.data(), sl.d_req.p, req.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        mark_noskip(c, sl, req);
    }
    sl.timing.host_collectwait_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tw).count();
    const FxBlockHdr &h = *sl.h_hdr.p;
    const bool detect = c->cfg.mode == FXRX_MODE_DETECTOR;
    sl.out.resize(h.n_frames);
    uint64_t vb_rep = 0;                       // trellis blocks the batch Viterbi path had to run again (hand-over check failed)
    uint64_t vb_clean = 0;                     // frames it decoded by the codeword check alone
    uint32_t s_cur = 0xFFFFFFFFu, s_first = 0; // detector windows: the stream of the last record and that stream's first record
    for (uint32_t i = 0; i < h.n_frames; i++) {
        const FxOutRec &r = sl.h_recs.p[i];
        fxrx_frame &f = sl.out[i].f; std::memset(&f, 0, sizeof f);
        f.stream = r.stream; f.start = r.start; f.cfo_bin = r.offset;
        f.rxy = r.rxy; f.tau = r.tau; f.gamma = r.gamma; f.dphi = r.dphi; f.phi = r.phi; f.pfb_index = r.pfb;
        f.pilot_dphi = r.pilot_dphi; f.pilot_phi = r.pilot_phi; f.pilot_gain = r.pilot_gain;
        f.header_valid = (r.flags & FX_FLAG_HEADER_VALID) ? 1 : 0;
        std::memcpy(f.header, r.header, FX_HDR_DEC);
        f.rssi_db = 20.0f * log10f(r.gamma); f.cfo = r.dphi;
        if (detect && c->cfg.want_framesyms && r.stream < NS) {
            if (r.stream != s_cur) { s_cur = r.stream; s_first = i; }
            // (beyond the reservation a window that starts in the carried tail has its own slot: see fx_detwin.hip)
            const bool tail = i >= sl.win_reserved && r.start < sl.snap[r.stream].tot0;
            f.framesyms = (const fx_complex *)(tail ? sl.h_wintail.p + (2 * (size_t)r.stream + (i - s_first)) * FX_NFFT : sl.h_win.p + (size_t)i * FX_NFFT);
            f.num_framesyms = FX_NFFT;
        }
        if (!detect && f.header_valid) {
            f.mod_scheme = r.ms; f.mod_bps = r.bps; f.check = r.check; f.fec0 = r.fec0; f.fec1 = r.fec1;
            f.payload_len = r.pay_len; f.num_framesyms = r.nsym;
            f.payload = sl.h_out.p + r.out_off; f.payload_valid = (int)r.payload_valid;
            vb_rep += r.status >> 8; vb_clean += r.status & FX_REC_VB_CLEAN;
            f.evm_sum = r.evm_sum; f.evm_db = 10.0f * log10f(r.evm_sum / (float)(r.nsym ? r.nsym : 1));
            f.framesyms = c->cfg.want_framesyms ? (const fx_complex *)(sl.h_framesyms.p + r.sym_off) : nullptr;
            if (c->cfg.soft_decision && c->cfg.want_framesyms) {
                f.soft_bits = sl.h_soft.p + 8 * (size_t)r.byte_off;
                f.num_soft_bits = 8u * fx::packet_plan(r.pay_len, r.check, r.fec0, r.fec1).l1;
            }
        }
    }
    sl.n_syms = h.sym_total;
    // what the streams carry now (bounds the next blocks' arenas), and the traffic hints for the next launches
    const FxStreamState *hs = c->h_state + (sl.seq % kStateRing) * NS;
    for (unsigned s = 0; s < NS; s++) {
        StreamState &S = c->st[s];
        const int64_t end_total = sl.snap[s].tot0 + (int64_t)sl.n[s];
        if (!S.fresh_start && S.total >= end_total)
            S.carry_bound = std::min<int64_t>(S.carry_bound, std::min<int64_t>(S.carry_cap, hs[s].carry_len + (S.total - end_total)));
    }
    sl.ps_taken += h.ps_taken; sl.ps_fallback += h.ps_fallback;
    { uint64_t tot = 0; for (unsigned s = 0; s < NS; s++) tot += sl.n[s]; c->traffic.observe(h, vb_rep, vb_clean, sl.tail.vb_early, tot, c->n_cus); }
    fxrx_timing &t = sl.timing;
    float ms = 0;
    if (sl.timing_level >= 2) {
        (void)hipEventElapsedTime(&ms, sl.ev[kEvStart], sl.ev[kEvWalk]); t.walk_ms = ms;
        (void)hipEventElapsedTime(&ms, sl.ev[kEvWalk], sl.ev[kEvVerify]); t.seekverify_ms = ms;
        (void)hipEventElapsedTime(&ms, sl.ev[kEvVerify], sl.ev[kEvPlan]); t.chain_ms = ms;
        if (!detect) {
            (void)hipEventElapsedTime(&ms, sl.ev[kEvPlan], sl.ev[kEvMf]); t.paymf_ms = ms;
            (void)hipEventElapsedTime(&ms, sl.ev[kEvPll], sl.ev[kEvDec]); t.paydec_ms = ms;
        }
    }
    if (sl.timing_level >= 1 && !detect) { (void)hipEventElapsedTime(&ms, sl.ev[kEvMf], sl.ev[kEvPll]); t.paypll_ms = ms; }
    t.total_ms = t.walk_ms + t.seekverify_ms + t.chain_ms + t.paymf_ms + t.paypll_ms + t.paydec_ms;
    t.hops = h.hops + sl.kept_hops; t.hops_cheap = h.hops_cheap + sl.kept_cheap; t.walk_jobs = sl.NJ; t.repairs = h.repairs + sl.kept_repairs + h.n_repair_req; t.frames = h.n_frames;
    t.payload_symbols = h.sym_total; t.verify_hops = h.verify_hops + sl.kept_vhops; t.verify_failures = h.verify_failures + sl.kept_vfail;
    t.host_submit_ms = sl.host_submit_ms; t.host_walkwait_ms = 0.0; t.walk_mode = sl.any_late ? 1 : 0; t.replays = c->replays + c->repairs_host;
    t.vb_blocks = h.n_vb_items; t.vb_repairs = vb_rep; t.late_decodes = c->late_decodes; t.vb_fallbacks = h.n_vb_fallback;
    t.vb_clean = vb_clean; t.late_windows = c->late_windows;
    sl.busy = false; c->last = &sl;
    c->tail = (c->tail + 1) % nslots; c->inflight--;
    return (int)sl.out.size();
}

int fxrx_process_fmt(fxrx_ctx *c, const void *const *iq, const uint64_t *n_samples, int on_device, int fmt)
{
    if (!c) return FXRX_ERR_ARG;
    while (c->inflight) { int r = fxrx_collect(c); if (r < 0) return r; }      // drain anything a caller left in flight
    int r = submit_block(c, iq, n_samples, on_device, fmt);
    if (r < 0) return r;
    return fxrx_collect(c);
}
int fxrx_process(fxrx_ctx *c, const void *const *iq, const uint64_t *n_samples, int on_device) { return fxrx_process_fmt(c, iq, n_samples, on_device, FXRX_IQ_FC32); }

// diagnostic builds (-DFX_STAMPS): walker phase clocks of the last collected block, summed over its walk jobs / of the slowest job
static int walk_stamps(const fxrx_ctx *c, uint64_t sum[4], uint64_t maxjob[8])
{
    for (int i = 0; i < 4; i++) sum[i] = 0;
    for (int i = 0; i < 8; i++) maxjob[i] = 0;
#ifdef FX_STAMPS
    if (!c->last || !c->last->NJ) return 0;
    std::vector<FxWalkResult> r(c->last->NJ);
    if (hipMemcpy(r.data(), c->last->d_wres.p, r.size() * sizeof(FxWalkResult), hipMemcpyDeviceToHost) != hipSuccess) return FXRX_ERR_HIP;
    for (const auto &w : r) {
        uint64_t tot = 0;
        for (int i = 0; i < 4; i++) { sum[i] += w.stamp[i]; tot += w.stamp[i]; }
        if (tot > maxjob[7]) { for (int i = 0; i < 4; i++) maxjob[i] = w.stamp[i]; maxjob[4] = w.hops; maxjob[5] = w.hops_cheap; maxjob[6] = w.n_frames; maxjob[7] = tot; }
    }
#endif
    return 0;
}
// diagnostic builds: per walk job of the last collected block 6 words -- stamp[0..3], hops, frames (detector-only mode: start / end on the
// 100 MHz wall clock, CU id, 0); returns the number of jobs
int fxrx_debug_walk_jobs(const fxrx_ctx *c, uint32_t *out, unsigned int cap_jobs)
{
    if (!c || !out || !c->last) return FXRX_ERR_ARG;
    const size_t nj = std::min<size_t>(c->last->NJ, cap_jobs);
    std::vector<FxWalkResult> r(nj);
    if (nj && hipMemcpy(r.data(), c->last->d_wres.p, nj * sizeof(FxWalkResult), hipMemcpyDeviceToHost) != hipSuccess) return FXRX_ERR_HIP;
    for (size_t i = 0; i < nj; i++) { for (int k = 0; k < 4; k++) out[6 * i + k] = r[i].stamp[k]; out[6 * i + 4] = r[i].hops; out[6 * i + 5] = r[i].n_frames; }
    return (int)nj;
}
// shader clocks of the chain kernel's phases (stream 0) of the last collected block: whole fast path, -, pointer chase, kernel total
int fxrx_debug_chain_stamps(const fxrx_ctx *c, uint32_t out[8]) { if (!c || !c->last) return FXRX_ERR_ARG; std::memcpy(out, c->last->h_hdr.p->stamp, 8 * sizeof(uint32_t)); return 0; }
int fxrx_debug_walk_stamps(const fxrx_ctx *c, uint64_t out[4]) { if (!c) return FXRX_ERR_ARG; uint64_t mj[8]; return walk_stamps(c, out, mj); }
int fxrx_debug_walk_maxjob(const fxrx_ctx *c, uint64_t out[8]) { if (!c) return FXRX_ERR_ARG; uint64_t sm[4]; return walk_stamps(c, sm, out); }

// diagnostic: decode-phase shader-clock deltas of frame i of the last collected block (zeros unless built with -DFX_STAMPS)
int fxrx_debug_stamps(const fxrx_ctx *c, unsigned int i, uint32_t out[8])
{
    if (!c || !c->last || i >= c->last->out.size()) return FXRX_ERR_ARG;
    std::memset(out, 0, 8 * sizeof(uint32_t));
#ifdef FX_STAMPS
    if (c->last->d_pres.p && hipMemcpy(out, c->last->d_pres.p[i].stamp, 8 * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) return FXRX_ERR_HIP;
#endif
    return 0;
}

int fxrx_result(const fxrx_ctx *c, unsigned int i, fxrx_frame *out)
{
    if (!c || !out || !c->last || i >= c->last->out.size()) return FXRX_ERR_ARG;
    *out = c->last->out[i].f; return 0;
}

unsigned int fxrx_gen_frame_len(unsigned int ms, unsigned int check, unsigned int fec0, unsigned int fec1, unsigned int n)
{
    fx::FrameGen g; g.ms = ms; g.check = check; g.fec0 = fec0; g.fec1 = fec1;
    return g.frame_len(n);
}

// ---- block-API index maps (reference: lib/flex_tx_impl.cc:75-181, lib/flex_rx_impl.cc:74-179) ----
static const int kMod[11] = { FX_MODEM_PSK2, FX_MODEM_PSK4, FX_MODEM_PSK8, FX_MODEM_PSK16, FX_MODEM_DPSK2, FX_MODEM_DPSK4,
                              FX_MODEM_DPSK8, FX_MODEM_ASK4, FX_MODEM_QAM16, FX_MODEM_QAM32, FX_MODEM_QAM64 };
static const int kInner[7] = { FX_FEC_NONE, FX_FEC_CONV_V27, FX_FEC_CONV_V27P23, FX_FEC_CONV_V27P45, FX_FEC_CONV_V27P56,
                               FX_FEC_CONV_V27P67, FX_FEC_CONV_V27P78 };
static const int kOuter[8] = { FX_FEC_NONE, FX_FEC_GOLAY2412, FX_FEC_RS_M8, FX_FEC_HAMMING74, FX_FEC_HAMMING128,
                               FX_FEC_SECDED2216, FX_FEC_SECDED3932, FX_FEC_SECDED7264 };
int fxrx_mod_from_index(int i) { return (i >= 0 && i < 11) ? kMod[i] : -1; }
int fxrx_inner_from_index(int i) { return (i >= 0 && i < 7) ? kInner[i] : -1; }
int fxrx_outer_from_index(int i) { return (i >= 0 && i < 8) ? kOuter[i] : -1; }
int fxrx_mod_to_index(unsigned v) { for (int i = 0; i < 11; i++) if ((unsigned)kMod[i] == v) return i; return -1; }
int fxrx_inner_to_index(unsigned v) { for (int i = 0; i < 7; i++) if ((unsigned)kInner[i] == v) return i; return -1; }
int fxrx_outer_to_index(unsigned v) { for (int i = 0; i < 8; i++) if ((unsigned)kOuter[i] == v) return i; return -1; }

}  // extern "C"
