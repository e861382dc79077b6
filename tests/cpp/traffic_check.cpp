// traffic_check.cpp -- properties of the host runtime's launch planning (gr-liquiddsp_amd/csrc/fx_traffic.h: Traffic, plan_tail,
// late_work), compiled host-only with g++: tests/test_traffic_plan.py.  Not a copy of the formulas: a first block covers
// every list, a block like the last one leaves nothing for fxrx_collect, one quantity beyond the plan gives exactly its
// reason, and the Reed-Solomon launch and the trellis kernels fade out as documented.
#include <cstdio>
#include <cstdint>
#include <initializer_list>
#include "../../gr-liquiddsp_amd/csrc/fx_traffic.h"

static int g_fail = 0, g_checks = 0;
#define CHECK(c, ...) do { g_checks++; if (!(c)) { if (++g_fail <= 20) { std::printf("FAIL %s: ", #c); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static const uint32_t kBlk = 192;        // trellis steps per work item; 0 in a TailCaps: no batch Viterbi path
struct Setup { int n_cus; uint32_t chain_slots, vb_cap; bool early; };
static TailCaps caps(const Setup &s, bool batch = true) { return TailCaps{ s.chain_slots, s.chain_slots + 16, s.vb_cap, batch ? kBlk : 0u }; }
static TailKnobs knobs(const Setup &s) { return TailKnobs{ 1u, s.n_cus, 0u, 0u, s.early, true }; }

static FxBlockHdr header(uint32_t plain, uint32_t rs, uint32_t batch, uint32_t items, uint32_t fb)
{
    FxBlockHdr h{};
    h.n_dec_plain = plain; h.n_dec_rs = rs; h.n_dec_batch = batch; h.n_frames = plain + rs + batch;
    h.n_vb_items = h.vb_want = items; h.vb_blk = kBlk; h.n_vb_fallback = fb; h.n_mfblk = 3 * h.n_frames; h.verify_hops = 40 * h.n_frames;
    return h;
}
// the next block's plan, as enqueue_back makes it: the hold is counted down by the caller
static TailPlan next_plan(Traffic &t, const Setup &s, bool batch = true)
{
    const TailPlan p = plan_tail(t, caps(s, batch), knobs(s));
    if (batch && t.trellis_left) t.trellis_left--;
    return p;
}
static int reasons(const LateWork &w) { uint64_t n[6] = {}; w.count(n); int m = 0; for (int i = 0; i < 6; i++) m |= (int)n[i] << i; return m; }

static void nothing_observed(const Setup &s)
{
    Traffic t;
    const TailPlan p = next_plan(t, s);
    CHECK(p.plain == s.chain_slots && p.vb_pre == s.chain_slots && p.fb == s.chain_slots, "first block: plain %u batch front %u fallback %u of %u", p.plain, p.vb_pre, p.fb, s.chain_slots);
    CHECK(p.rs == (s.chain_slots < 64 ? s.chain_slots : 64u), "first block: Reed-Solomon grid %u of %u", p.rs, s.chain_slots);
    CHECK(p.vb_items == s.vb_cap, "first block: work items %u of %u", p.vb_items, s.vb_cap);
    CHECK(p.vb_fin == p.vb_pre && p.with_fix == 1, "first block: back part %u front %u hand-over check %d", p.vb_fin, p.vb_pre, p.with_fix);
    CHECK(p.pll_waves * 64u >= s.chain_slots && p.mf_grid >= 1, "first block: PLL waves %u matched-filter grid %u", p.pll_waves, p.mf_grid);
    // whatever a first block holds within its lists, nothing is left to collect
    FxBlockHdr h = header(s.chain_slots, s.chain_slots, s.chain_slots, s.vb_cap, s.chain_slots); h.vb_dirty = 1;
    CHECK(!late_work(p, h, kBlk).any(), "first block at capacity: reasons %02x", reasons(late_work(p, h, kBlk)));
    const TailPlan q = next_plan(t, s, false);       // no batch path: an all-zero batch part
    CHECK(q.plain == s.chain_slots && !q.vb_pre && !q.vb_items && !q.vb_fin && !q.fb && !q.vb_early && !q.vb_packed && !q.with_fix, "first block without a batch path");
}

static void steady_state(const Setup &s)
{
    const uint32_t cap = s.chain_slots;
    for (uint32_t plain : { 0u, 1u, 63u, 64u, 65u, cap }) for (uint32_t rs0 : { 0u, 1u, 200u }) for (uint32_t batch : { 0u, 1u, cap })
        for (uint32_t items0 : { 0u, 1u, 5000u }) for (uint32_t fb : { 0u, 1u, 33u, 500u }) for (int clean = 0; clean < 2; clean++) {
            // consistent headers only: no list holds more than its capacity, the lists share the chain's slots, work items and handed-back frames
            // belong to batch frames, a clean block hands none back
            const uint32_t rs = rs0 < cap ? rs0 : cap, items = items0 < s.vb_cap ? items0 : s.vb_cap;
            if ((uint64_t)plain + rs + batch > cap || (batch == 0) != (items == 0) || fb > batch || (clean && fb)) continue;
            const FxBlockHdr h = header(plain, rs, batch, items, fb);
            Traffic t;
            t.observe(header(5, 0, 5, 50, 0), 0, 5, s.early, 100000, s.n_cus);
            t.observe(h, fb ? 2 : 0, clean ? batch : batch - fb - (batch > fb ? 1u : 0u), s.early, 1000000, s.n_cus);
            const TailPlan p = next_plan(t, s);
            FxBlockHdr again = h; again.vb_dirty = !clean && batch ? 1u : 0u;
            CHECK(!late_work(p, again, kBlk).any(), "plain %u rs %u batch %u items %u fb %u clean %d: reasons %02x", plain, rs, batch, items, fb, clean, reasons(late_work(p, again, kBlk)));
            CHECK(!(s.early && clean && batch) || p.vb_fin == 0, "a clean block announces no trellis kernels (batch %u: back part %u)", batch, p.vb_fin);
            CHECK(t.verify_per >= 1 && t.verify_per <= 16, "verify_per %u", t.verify_per);
        }
}

static void each_reason_alone(const Setup &s)
{
    // steady state: 10 plain and 20 batch frames of 300 work items, none handed back, no Reed-Solomon frames; dirty: one frame was not clean
    for (int dirty = 0; dirty < 2; dirty++) {
        if (dirty && !s.early) continue;
        const FxBlockHdr h0 = header(10, 0, 20, 300, 0);
        Traffic t;
        t.observe(h0, 0, dirty ? 19 : 20, s.early, 1000000, s.n_cus);
        const TailPlan p = next_plan(t, s);
        const bool trellis = p.vb_fin != 0;
        CHECK(trellis == (dirty || !s.early), "trellis kernels %d (dirty %d, early tail %d)", (int)trellis, dirty, (int)s.early);
        FxBlockHdr h = h0; h.vb_dirty = (uint32_t)dirty;
        CHECK(reasons(late_work(p, h, kBlk)) == 0, "steady state: %02x", reasons(late_work(p, h, kBlk)));
        h = h0; h.n_dec_plain = p.plain + 1;
        if (p.plain < s.chain_slots) CHECK(reasons(late_work(p, h, kBlk)) == 0x01, "one plain frame beyond the launch: %02x", reasons(late_work(p, h, kBlk)));
        h = h0; h.n_dec_rs = 1;
        CHECK(reasons(late_work(p, h, kBlk)) == 0x02, "one Reed-Solomon frame after none: %02x", reasons(late_work(p, h, kBlk)));
        h = h0; h.n_dec_batch = p.vb_pre + 1;
        if (p.vb_pre < s.chain_slots) CHECK(reasons(late_work(p, h, kBlk)) == 0x04, "one batch frame beyond the launch: %02x", reasons(late_work(p, h, kBlk)));
        h = h0; h.n_vb_items = p.vb_items + 1;
        if (trellis) CHECK(reasons(late_work(p, h, kBlk)) == 0x08, "one work item beyond the launch: %02x", reasons(late_work(p, h, kBlk)));
        else CHECK(reasons(late_work(p, h, kBlk)) == 0, "work items count for nothing without the trellis kernels: %02x", reasons(late_work(p, h, kBlk)));
        h = h0; h.n_vb_fallback = p.fb + 1;
        CHECK(reasons(late_work(p, h, kBlk)) == 0x10, "one handed-back frame beyond the launch: %02x", reasons(late_work(p, h, kBlk)));
        h = h0; h.vb_dirty = 1;
        CHECK(reasons(late_work(p, h, kBlk)) == (trellis ? 0 : 0x20), "a frame that is not clean, trellis kernels %d: %02x", (int)trellis, reasons(late_work(p, h, kBlk)));
    }
}

static void fade(const Setup &s)
{
    Traffic t;
    t.observe(header(0, s.chain_slots < 200 ? s.chain_slots : 200u, 0, 0, 0), 0, 0, s.early, 1000000, s.n_cus);
    uint32_t last = next_plan(t, s).rs; int blocks = 0;
    CHECK(last > 0, "Reed-Solomon frames announce a launch");
    while (last && blocks < 200) {
        t.observe(header(3, 0, 0, 0, 0), 0, 0, s.early, 1000000, s.n_cus);
        const uint32_t now = next_plan(t, s).rs; blocks++;
        CHECK(now < last || (now == last && now == s.chain_slots), "block %d without Reed-Solomon frames: grid %u after %u", blocks, now, last);
        last = now;
    }
    CHECK(last == 0 && blocks < 100, "Reed-Solomon grid %u after %d blocks", last, blocks);
    if (!s.early) return;
    // one block with a frame that was not clean, then clean ones: the trellis kernels stay for exactly kTrellisHold plans
    Traffic u;
    u.observe(header(0, 0, 20, 300, 0), 0, 19, true, 1000000, s.n_cus);
    for (unsigned i = 0; i <= kTrellisHold + 2; i++) {
        const TailPlan p = next_plan(u, s);
        CHECK((p.vb_fin != 0) == (i < kTrellisHold) && (p.vb_items != 0) == (i < kTrellisHold), "plan %u after a block that was not clean: back part %u, items %u", i, p.vb_fin, p.vb_items);
        if (i % 2) u.observe(header(0, 0, 20, 300, 0), 0, 20, p.vb_early, 1000000, s.n_cus);
    }
}

int main()
{
    for (int n_cus : { 256, 8 }) for (uint32_t slots : { 1000u, 40u }) for (bool early : { true, false }) {
        const Setup s{ n_cus, slots, slots == 40u ? 4096u : 100000u, early };
        nothing_observed(s); steady_state(s); each_reason_alone(s); fade(s);
    }
    std::printf("%d checks, %d failures\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
