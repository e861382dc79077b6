// fx_traffic.h -- what the host runtime knows about a block before the block exists.  A block's kernel chain is enqueued before
// the host knows what the block holds, so the grids of its tail, and whether the plain, Reed-Solomon, trellis and fallback launches
// exist at all, follow the last collected block:
//   Traffic   what that block held                                  (written by fxrx_collect: observe)
//   TailPlan  the grids and optional launches of a block's tail     (plan_tail, every time fx_host.cpp:enqueue_back runs)
//   LateWork  what such a plan left undone for the block it met     (late_work, asked once by fx_host.cpp:finish_decode)
// The front of a block reads the same Traffic (fx_frontplan.h, every time fx_host.cpp:plan_front runs: a submit, a replay): frames and samples for
// the depth of the pre-lock scan (and frames for the detector's window slots), vb_steps for the trellis block length and the batch
// Viterbi arenas, verify_per for every walk job.
// Host only and pure -- no HIP call, no allocation --, so that tests/cpp/traffic_check.cpp checks it with g++ alone.
#pragma once
#include <algorithm>
#include <stdint.h>
#include "fx_common.h"

constexpr unsigned kTrellisHold = 8;                // blocks that keep the trellis kernels in their chain after a collected block with frames that were not clean
constexpr uint32_t kFallbackWaves = 32;             // in-chain launch for frames the batch Viterbi path hands back (normally none)

// The last collected block.  (A context's blocks share one record: consecutive blocks of different stream groups overwrite each other's.)
struct Traffic {
    bool seen = false;                   // false: nothing observed yet -- every launch covers its list's capacity
    uint64_t samples = 0, frames = 0;    // new samples of all streams / frames (together: the mean frame spacing)
    uint64_t plain = 0, rs = 0;          // frames of the wave-per-frame decoder's lean / Reed-Solomon instance; rs fades out over blocks without any
    uint64_t batch = 0, vb_items = 0;    // frames of the batch Viterbi path / their trellis blocks (work items of the forward pass)
    uint64_t vb_steps = 0;               // trellis steps the block's traffic asked for, whether or not the arena held them
    uint64_t vb_fix = 0;                 // trellis blocks that ran again + frames handed back: nonzero launches the hand-over check
    uint64_t fb = 0;                     // frames the batch path handed back to the wave-per-frame decoder
    uint64_t mf_items = 0;               // items of 1024 symbols of the payload matched filter
    uint32_t verify_per = 4;             // hops per verification run: some four runs per CU
    // Blocks that still get the trellis kernels (forward pass, hand-over check, traceback, back part, fallback decoder: up to five launches) although
    // fx_vbpre_kernel finishes clean frames by itself: reloaded by a block with frames that were not clean, counted down by enqueue_back
    unsigned trellis_left = 0;

    // vb_rep / vb_clean: trellis blocks run again / frames decoded by the codeword check alone, summed over the block's records; vb_early: the block's own plan
    void observe(const FxBlockHdr &h, uint64_t vb_rep, uint64_t vb_clean, bool vb_early, uint64_t n_samples, int n_cus)
    {
        samples = n_samples; frames = h.n_frames; plain = h.n_dec_plain; batch = h.n_dec_batch; vb_items = h.n_vb_items; mf_items = h.n_mfblk;
        vb_steps = (uint64_t)h.vb_want * (h.vb_blk ? h.vb_blk : 1u);
        fb = h.n_vb_fallback; vb_fix = h.n_vb_fallback + vb_rep;
        if (vb_early && h.n_dec_batch > vb_clean) trellis_left = kTrellisHold;
        rs = h.n_dec_rs ? h.n_dec_rs : rs - std::min<uint64_t>(rs, std::max<uint64_t>(1, rs / 8));      // (to zero, over a few dozen blocks)
        if (h.verify_hops) verify_per = (uint32_t)std::min<uint64_t>(16, std::max<uint64_t>(1, ((uint64_t)h.verify_hops + 4ull * n_cus - 1) / (4ull * n_cus)));
        seen = true;
    }
};

// The margin rule: a grid that strides over a list only the device can count covers what the last block held plus half plus `extra`,
// at least `floor`, at most the list's capacity
inline uint32_t with_margin(uint64_t count, uint64_t cap, uint64_t extra = 64, uint64_t floor = 0) { return (uint32_t)std::min(cap, std::max(floor, count + count / 2 + extra)); }

// A block's tail -- everything behind the payload matched filter -- as launched with its chain; finish_decode raises the counts to what it completed.
struct TailPlan {
    uint32_t pll_waves = 0, mf_grid = 0; // PLL waves; workgroups of the matched filter in front of it (and of the soft demapper)
    uint32_t plain = 0, rs = 0;          // decode waves of the lean / Reed-Solomon instance (the latter strides: any launch covers all)
    // batch Viterbi path: waves of fx_vbpre_kernel, work items of the trellis kernels, waves of fx_vbfinish_kernel and of the fallback decoder
    uint32_t vb_pre = 0, vb_items = 0, vb_fin = 0, fb = 0;      // vb_fin 0: the trellis kernels were left out
    int vb_packed = 0, with_fix = 0;     // two work items per lane / the hand-over check is launched
    bool vb_early = false;               // clean frames finish in fx_vbpre_kernel
};
struct TailCaps { uint32_t chain_slots, mf_cap, vb_cap, vb_blk; };      // capacities of the block's lists; vb_blk 0: no batch Viterbi path
struct TailKnobs { unsigned depth; int n_cus; uint32_t mf_per_cu, vb_debug; bool vb_early_tail, vb_clean; };

inline TailPlan plan_tail(const Traffic &t, const TailCaps &cap, const TailKnobs &k)
{
    const uint64_t slots = cap.chain_slots, cus = (uint64_t)k.n_cus;
    TailPlan p;
    p.pll_waves = (t.frames ? with_margin(t.frames, slots) : cap.chain_slots) / 64 + FX_PLL_CLASSES;
    // (one workgroup per item of 1024 symbols when the previous block's count is anything to go by -- measured better than
    // fewer workgroups striding over the items: 8 per CU 34.3, 18: 35.1, one per item (36 per CU on config 2): 35.3 Gsamples/s)
    p.mf_grid = (uint32_t)std::min<uint64_t>(cap.mf_cap, k.mf_per_cu ? k.mf_per_cu * cus : std::max<uint64_t>(8 * cus, t.mf_items + t.mf_items / 8 + 64));
    p.vb_early = cap.vb_blk && k.vb_early_tail && k.vb_clean;
    // the trellis kernels: always without the early tail; with it, while the traffic has frames for them
    const bool trellis = cap.vb_blk && (!p.vb_early || !t.seen || k.vb_debug || t.trellis_left > 0);
    if (!t.seen) {
        // every launch at its capacity; the Reed-Solomon instance strides, a margin's worth of waves covers whatever the block holds
        p.plain = cap.chain_slots; p.rs = std::min<uint32_t>(cap.chain_slots, 64u);
        if (cap.vb_blk) { p.vb_pre = p.fb = cap.chain_slots; p.vb_items = cap.vb_cap; }
    } else {
        // Decode, one wave per frame.  The lean instance has no loop (it would double its registers) and an empty workgroup still has to be given
        // its registers before it can leave: so the grid follows the traffic, not the list's capacity, and an instance is only launched while
        // its frames keep turning up -- plain frames (with the batch path on, a block normally has none), Reed-Solomon frames (256 registers a
        // wave), and frames whose hand-overs could not be verified, which take the trellis kernels to be found at all
        p.plain = t.plain || !cap.vb_blk ? with_margin(t.plain, slots) : 0u;
        p.rs = t.rs ? with_margin(t.rs, slots) : 0u;
        if (cap.vb_blk) {
            p.vb_pre = with_margin(t.batch, slots);
            p.vb_items = trellis ? with_margin(t.vb_items, cap.vb_cap, 1024) : 0u;
            p.fb = trellis && (t.fb || k.vb_debug) ? with_margin(t.fb, slots, 16, kFallbackWaves) : 0u;
        }
    }
    p.vb_fin = trellis ? p.vb_pre : 0u;
    if (cap.vb_blk) {
        // (two work items per lane once the items fill the chip or other blocks do; one per lane for a lone small block)
        p.vb_packed = (k.depth > 1 || t.vb_items > 64ull * 4ull * cus * 3ull / 2ull) ? 1 : 0;
        p.with_fix = (!t.seen || t.vb_fix || k.vb_debug) ? 1 : 0;
    }
    return p;
}

// What a block's chain left for fxrx_collect to complete, in the order of fxrx_debug_late_stats (RxContext.LATE_REASONS)
struct LateWork {
    bool more_plain = false;             // plain frames beyond the launch
    bool more_rs = false;                // Reed-Solomon frames without a launch
    bool more_batch_frames = false;      // batch-path frames beyond fx_vbpre_kernel's launch
    bool more_batch_items = false;       // trellis work items beyond the launch
    bool more_fb = false;                // handed-back frames beyond the fallback launch
    bool late_trellis = false;           // a frame that was not clean in a chain without the trellis kernels
    bool more_batch() const { return more_batch_frames || more_batch_items; }
    bool any() const { return more_plain || more_rs || more_batch() || more_fb || late_trellis; }
    void count(uint64_t n[6]) const { n[0] += more_plain; n[1] += more_rs; n[2] += more_batch_frames; n[3] += more_batch_items; n[4] += more_fb; n[5] += late_trellis; }
};

// h: the block's header as the host has it -- n_vb_fallback fetched where the kernels raised vb_ticket, vb_dirty read now
inline LateWork late_work(const TailPlan &p, const FxBlockHdr &h, uint32_t vb_blk)
{
    LateWork w;
    const bool no_trellis = vb_blk && p.vb_fin == 0;
    w.more_plain = h.n_dec_plain > p.plain; w.more_rs = h.n_dec_rs > 0 && p.rs == 0;
    w.more_batch_frames = h.n_dec_batch > p.vb_pre; w.more_batch_items = !no_trellis && h.n_vb_items > p.vb_items;
    w.more_fb = vb_blk && h.n_vb_fallback > p.fb;
    // (with more_batch every part of the path runs again anyway)
    w.late_trellis = no_trellis && !w.more_batch() && h.vb_dirty != 0u;
    return w;
}
