// fx_frontplan.h -- every sizing decision of a block's front, made before the block exists: how long its walk segments are, where each
// stream is cut into walker jobs, how far the pre-lock scan looks, and what the frame table, the chain table, the payload arenas and the
// batch Viterbi arenas have to hold.  fx_host.cpp:plan_front fills a FrontKnobs from the context and calls front_plan; build_descriptors
// turns the cuts into FxWalkJob / FxStreamDesc records and reserve_block reserves what FrontCaps says.  Of the last collected block
// (fx_traffic.h: Traffic) the plan reads frames and samples (pre-lock scan depth), vb_steps (trellis block length and arenas) and
// verify_per (copied into every job).  The same inputs give the same plan: a replay of a block rebuilds its descriptors from the same
// snapshot and traffic (a replay with the exact detector on every hop differs in FxWalkJob::no_skip alone, which is no part of the plan).
// Host only and pure -- no HIP call, no getenv, nothing allocated but the std::vector results --, so that tests/cpp/frontplan_check.cpp
// prints every value with g++ alone and tests/test_frontplan.py compares them with its own statement of the rules.
#pragma once
#include <algorithm>
#include <stdint.h>
#include <vector>
#include "fx_common.h"
#include "fx_traffic.h"

constexpr uint32_t kRepairCap = 256;                // frame-table slots per stream for walks done by the chain kernel

// what the plan reads from the context and its configuration
struct FrontKnobs {
    bool detect = false;                 // detector-only mode
    unsigned depth = 1;                  // blocks in flight
    int n_cus = 256;
    uint32_t walk_per_cu = 2;            // walker workgroups resident per CU
    uint64_t segment_len = 0;            // fxrx_config.segment_len (0: chosen per block)
    float taper = -1.0f;                 // segment lengths of a stream fall from (1 + t) to (1 - t) times the mean (negative: chosen per block)
    bool prescan = false; int prescan_hops = -1;    // pre-lock scan on / hops per speculative job as given (negative: from the traffic)
    bool batch_viterbi = true, soft_decision = false;
    uint32_t vb_blk_force = 0;           // tests: trellis steps per block (0: from the traffic)
};
// what the plan reads from a stream: new samples, whether it continues (not freshly reset), upper bound of the carried tail it will find
struct StreamIn { uint64_t n = 0; bool cont = false; int64_t carry_bound = 0; };

inline uint64_t block_total(const std::vector<StreamIn> &streams) { uint64_t tot = 0; for (const StreamIn &s : streams) tot += s.n; return tot; }

// Densest possible traffic: a flexframe is at least ~630 samples long (preamble, header, tail), so flex_rx finds at most one frame
// per 600 samples; the bare detector (frame_detector_cc) can fire again on the very next hop, 256 samples on.  Plus 8.
inline uint64_t frames_cap(uint64_t samples, bool detect) { return samples / (detect ? 256u : 600u) + 8u; }
// frame-table slots per walk job: the densest legal traffic is a header-only frame (618 samples) after the other.  (Should a
// table fill up all the same -- FX_EXIT_TABLE_FULL -- the full-size chain kernel continues the segment.)
inline uint32_t seg_frames_cap(uint64_t seg, bool detect) { return (uint32_t)std::min<uint64_t>(frames_cap(seg, detect), 4000); }

// samples per walk segment, for a block of `tot` new samples in all
inline uint64_t segment_len(uint64_t tot, const FrontKnobs &k)
{
    uint64_t seg = k.segment_len;
    if (seg == 0) {
        // Walker workgroups resident at once: two per CU for the flex_rx instance (4 waves x 256 VGPRs each), two for the
        // leaner detector-only instance.  One block at a time (latency): little work -> a single round of workgroups with a
        // small margin (the kernel then lasts as long as its slowest segment); lots of work -> ~4 rounds so that uneven
        // segments even out.  Several blocks in flight (throughput): every segment start costs a speculative walker a
        // pre-lock scan of half a frame on average -- about as much as two frames' worth of real work -- and the chip is
        // kept busy by the other blocks anyway, so fewer, longer segments: down to one workgroup per two CUs.
        const uint64_t slots = (uint64_t)k.n_cus * k.walk_per_cu;
        // (about three blocks' walkers overlap at any time: keep that many workgroups' worth of segments between them)
        // (Measured again with the tails ganged, DESIGN.md section 6, pre-scan log: twice as many segments, down to one workgroup per
        // CU -- 6 x slots / depth, 256 at depth 12 -- give the higher rates on config 2.  Why they do is not established.)
        if (k.depth > 1 && !k.detect) seg = tot / std::max<uint64_t>(std::max<uint64_t>(1, k.n_cus), std::min<uint64_t>(slots, 6 * slots / k.depth));
        else if (tot / slots < 131072) seg = tot / (slots - slots / 16);
        else seg = std::max<uint64_t>(tot / (4 * slots), 65536);
        seg = std::max<uint64_t>(seg, 32768); seg = std::min<uint64_t>(seg, 1u << 20);
    }
    return std::max<uint64_t>(seg, 4096);
}

// (detector-only mode with more jobs than fit on the chip at once: config 3 alone 28.7 -> 24.7 ms; the flex_rx walker, whose launches
// overlap the rest of the chain, gains nothing from it: configs 4, 5 and 2 measured equal or worse)
inline float choose_taper(uint64_t tot, uint64_t seg, const FrontKnobs &k)
{
    if (k.taper >= 0.0f) return k.taper;
    return (k.detect && tot / seg > 4ull * (uint64_t)k.n_cus) ? 0.75f : 0.0f;
}

// hops of every speculative job that fx_prescan_kernel scans ahead of the walkers (0: no such launch): a mean frame spacing
// of the last collected block plus two hops -- a segment start falls anywhere in a frame --, whole chunks
inline uint32_t prescan_hops(const Traffic &t, const FrontKnobs &k)
{
    if (!k.prescan || k.detect) return 0;
    if (k.prescan_hops >= 0) return (uint32_t)k.prescan_hops;              // (as given: the last chunk may be a short one)
    const uint32_t K = t.frames ? (uint32_t)std::min<uint64_t>(128, std::max<uint64_t>(16, t.samples / t.frames / FX_HOP + 2)) : 64u;
    return (K + FX_PRESCAN_CHUNK - 1) / FX_PRESCAN_CHUNK * FX_PRESCAN_CHUNK;
}
inline uint32_t prescan_words(uint32_t K) { return (K + FX_PRESCAN_CHUNK - 1) / FX_PRESCAN_CHUNK; }       // chunk words per speculative job

// one walk job of a stream: samples [start, stop), its frame-table slots, and whether it is the stream's first (a continuing
// stream's true walker; every other job starts speculatively)
struct Cut { int64_t start = 0, stop = 0; uint32_t max_frames = 0; bool first = false; };

// the segments of one stream of n new samples, appended to `cuts` in order: they tile [0, n), and a stream without samples still gets one job
inline void cut_stream(std::vector<Cut> &cuts, uint64_t n, bool cont, int64_t carry_bound, uint64_t seg_len, float taper, bool detect)
{
    const int64_t ns = (int64_t)n, seg = (int64_t)seg_len;
    // a continuing stream's true walker only has to reach its first hand-off, so its own segment is short: it starts
    // late (after the previous block's chain kernel) while the speculative walkers of the other segments are long under way
    int64_t p = 0; bool first = true;
    const int64_t seg0 = cont ? std::min<int64_t>(seg, 8192) : seg;
    // Tapered segments: what is launched last is short.  A walker workgroup alone on its CU runs at well under half the rate four
    // of them reach together (tools/dev/dev_walk_timeline.py), so the last jobs of a launch set the length of its drain.
    const int64_t p_t = cont ? std::min<int64_t>(ns, seg0) : 0;                       // the taper covers [p_t, ns)
    const int64_t k_t = taper > 0.0f ? std::max<int64_t>(1, ((ns - p_t) + seg / 2) / seg) : 0;
    int64_t i_t = 0;
    while (first || p < ns) {
        Cut j;
        j.start = p; j.first = first;
        j.stop = std::min<int64_t>(ns, p + (first ? seg0 : seg));
        if (ns - j.stop < seg / 2) j.stop = ns;          // fold a short last segment in
        if (k_t > 1 && p >= p_t) {
            // piece i of k: boundary at the integral of the falling line (1 + t) -> (1 - t)
            const double u = (double)(i_t + 1) / (double)k_t;
            const int64_t e = p_t + (int64_t)((double)(ns - p_t) * (u * (1.0 + taper) - taper * u * u));
            j.stop = (i_t + 1 >= k_t) ? ns : std::min<int64_t>(ns, std::max<int64_t>(p + 4096, e & ~(int64_t)255));
            i_t++;
        }
        j.max_frames = seg_frames_cap((uint64_t)(j.stop - j.start) + (first && cont ? (uint64_t)carry_bound : 0u), detect);
        cuts.push_back(j);
        p = j.stop; first = false;
        if (p >= ns) break;
    }
}

// the launch order of the speculative jobs (indices into the cut list) under a taper: longest job first, equal lengths in stream order
inline void longest_first(std::vector<uint32_t> &order, const std::vector<Cut> &cuts)
{
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return cuts[a].stop - cuts[a].start > cuts[b].stop - cuts[b].start; });
}

// Batch Viterbi: trellis steps per block from the traffic of the last block (0: no batch Viterbi path).  The forward pass is arithmetic
// bound, three waves to a SIMD: some six waves per SIMD spread evenly over the chip, fewer and the slowest SIMD sets the time; blocks
// shorter than a couple of warm-ups waste their work.  (Longer blocks with several blocks in flight -- less warm-up, the
// chip is full anyway -- measured worse: 192 steps 30.0, 256: 29.8, 384: 28.8, 512: 27.6, 1024: 24.6 Gsamples/s on config 2.)
constexpr uint64_t kVbBlkMin = 192, kVbBlkMax = 4096;      // the block lengths the rule chooses between
inline uint32_t trellis_block(const Traffic &t, const FrontKnobs &k)
{
    if (k.detect || k.soft_decision || !k.batch_viterbi) return 0u;
    if (k.vb_blk_force) return k.vb_blk_force;
    const uint64_t want_items = 64ull * 4ull * (uint64_t)k.n_cus * 6ull;
    return (uint32_t)std::min<uint64_t>(kVbBlkMax, std::max<uint64_t>(kVbBlkMin, ((t.vb_steps / want_items + 63) / 64) * 64));
}

// The batch Viterbi arenas of a block whose frames can occupy `span` samples.  Work items: 1.5 trellis steps per sample of span -- QPSK
// r1/2 has 0.47, QAM16 r2/3 1.17 -- or what the last block's traffic asked for plus a quarter, in work items of vb_blk steps, plus
// kVbSpare, rounded up to 128; frames whose work items do not fit are decoded by the wave-per-frame kernel, and the next block's arena is
// larger.  The allocations are sized in steps, not items, so that a change of block length does not reallocate gigabytes: the decision
// words price the spare items (and the round-up) at the longest block, the per-item arenas price the steps at the shortest -- the same
// figures for every vb_blk from kVbBlkMin to kVbBlkMax.
constexpr uint64_t kVbSpare = 2048, kVbSparePriced = kVbSpare + 128;
struct TrellisCaps { uint32_t vb_cap = 128; uint64_t vb_dw_words = 0, vb_slots_alloc = 128; };     // work items / decision words / per-item records allocated
inline TrellisCaps size_trellis(uint64_t span, uint64_t vb_steps, uint32_t vb_blk)
{
    TrellisCaps c;
    if (!vb_blk) return c;
    const uint64_t steps_cap = std::min<uint64_t>(std::max<uint64_t>(span + span / 2, vb_steps + vb_steps / 4), 4 * span);
    c.vb_cap = (uint32_t)((steps_cap / vb_blk + kVbSpare + 127) & ~127ull);
    c.vb_dw_words = std::max<uint64_t>((uint64_t)c.vb_cap * vb_blk, steps_cap + kVbSparePriced * kVbBlkMax);
    c.vb_slots_alloc = std::max<uint64_t>(c.vb_cap, steps_cap / kVbBlkMin + kVbSparePriced);
    return c;
}

// detector mode with want_framesyms: 4 KB window slots of a block -- the last collected block's count plus a margin, as for the other
// lists only the device can count (one slot per possible detection would be twice the input, in pinned memory); a block that holds more
// is completed when it is collected.  forced: FXRX_DETWIN_RESERVE (tests), 0: none
inline uint32_t window_slots(const Traffic &t, uint32_t chain_slots, uint32_t forced) { return forced ? std::min(chain_slots, forced) : with_margin(t.frames, chain_slots); }

// a stream's regions of the chain table and of the frame table (the latter for walks the chain kernel does itself: kRepairCap slots)
struct StreamCaps { uint32_t chain_base = 0, chain_cap = 0, repair_base = 0; };
struct FrontCaps {
    std::vector<uint32_t> frame_base;    // per cut: first slot of the job in the frame table
    std::vector<StreamCaps> streams;
    uint32_t frame_slots = 0, chain_slots = 0;       // frame table (jobs, then every stream's repair slots) / chain table
    uint32_t run_cap = 0, mf_cap = 0;    // verification runs / items of the payload matched filter
    uint64_t sym_cap = 0, byte_cap = 0, dw_cap = 0, out_cap = 0;      // payload arenas
    uint32_t vb_blk = 0; TrellisCaps vb;
    bool too_large = false;              // the arenas outgrow their 32-bit offsets: the block is refused
};

// cuts: the cut lists of all streams, one behind the other
inline FrontCaps size_front(const std::vector<StreamIn> &streams, const std::vector<Cut> &cuts, const Traffic &t, const FrontKnobs &k)
{
    FrontCaps c;
    c.frame_base.reserve(cuts.size()); c.streams.resize(streams.size());
    for (const Cut &j : cuts) { c.frame_base.push_back(c.frame_slots); c.frame_slots += j.max_frames; }
    uint64_t carry_total = 0;
    for (size_t s = 0; s < streams.size(); s++) {
        const uint64_t carry = streams[s].cont ? (uint64_t)streams[s].carry_bound : 0u;
        c.streams[s].chain_base = c.chain_slots; c.streams[s].chain_cap = (uint32_t)frames_cap(streams[s].n + carry, k.detect);
        c.chain_slots += c.streams[s].chain_cap;
        carry_total += carry;
    }
    for (StreamCaps &s : c.streams) { s.repair_base = c.frame_slots; c.frame_slots += kRepairCap; }
    const uint64_t span = block_total(streams) + carry_total;        // samples the block's frames can occupy
    const uint64_t slots = c.chain_slots;
    c.run_cap = (uint32_t)std::min<uint64_t>(span / FX_HOP + 2 * (uint64_t)cuts.size() + 1024, 0x7fffffffu);
    c.sym_cap = span / 2 + 8 * slots + 64;
    c.byte_cap = (span / 2) * 3 / 4 + 48 * slots + 64;
    c.dw_cap = k.detect ? 0 : (span / 2) * 6 + 200 * slots + 64;
    c.out_cap = (span / 2) * 3 / 4 + 16 * slots + 64;
    c.mf_cap = (uint32_t)std::min<uint64_t>(span / 2 / 1024 + slots + 16, 0x7fffffffu);
    c.vb_blk = trellis_block(t, k); c.vb = size_trellis(span, t.vb_steps, c.vb_blk);
    c.too_large = c.sym_cap >= (1ull << 32) || c.dw_cap >= (1ull << 32);
    return c;
}

// A block's front plan, whole: one segment length and one taper for the block, every stream cut with them
struct FrontPlan {
    uint64_t seg = 0; float taper = 0.0f; uint32_t ps_hops = 0;
    std::vector<Cut> cuts; std::vector<uint32_t> first_cut;      // stream s owns cuts [first_cut[s], first_cut[s + 1])
    FrontCaps caps;
};
inline FrontPlan front_plan(const std::vector<StreamIn> &streams, const Traffic &t, const FrontKnobs &k)
{
    FrontPlan p;
    const uint64_t tot = block_total(streams);
    p.seg = segment_len(tot, k); p.taper = choose_taper(tot, p.seg, k); p.ps_hops = prescan_hops(t, k);
    p.first_cut.reserve(streams.size() + 1);
    for (const StreamIn &s : streams) { p.first_cut.push_back((uint32_t)p.cuts.size()); cut_stream(p.cuts, s.n, s.cont, s.carry_bound, p.seg, p.taper, k.detect); }
    p.first_cut.push_back((uint32_t)p.cuts.size());
    p.caps = size_front(streams, p.cuts, t, k);
    return p;
}
