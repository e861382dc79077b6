// frontplan_check.cpp -- every value of every function of the host runtime's front plan (gr-liquiddsp_amd/csrc/fx_frontplan.h), compiled
// host-only with g++: tests/test_frontplan.py writes the cases, one a line, and compares what this prints, line by line, with its own
// statement of the rules.  A case is a word and its arguments; the answer is the same word and the values.
//   cap  samples detect                                         -> frames_cap seg_frames_cap
//   seg  <knobs> total                                          -> segment_len
//   tap  <knobs> total seg                                      -> choose_taper
//   ps   <knobs> frames samples                                 -> prescan_hops prescan_words
//   cut  n cont carry_bound seg taper detect                    -> count, then start:stop:max_frames:first of every cut, then the tapered launch order
//   vb   <knobs> vb_steps span                                  -> trellis_block, size_trellis at that length, at kVbBlkMin and at kVbBlkMax
//   win  frames chain_slots forced                              -> window_slots
//   plan <knobs> frames samples vb_steps NS (n cont carry) x NS -> front_plan, whole, and whether a second call gave the same
// <knobs>: detect depth n_cus walk_per_cu segment_len taper prescan prescan_hops batch_viterbi soft_decision vb_blk_force
#include <cinttypes>
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include "../../gr-liquiddsp_amd/csrc/fx_frontplan.h"

static FrontKnobs read_knobs(std::istream &in)
{
    FrontKnobs k; int detect, prescan, batch, soft;
    in >> detect >> k.depth >> k.n_cus >> k.walk_per_cu >> k.segment_len >> k.taper >> prescan >> k.prescan_hops >> batch >> soft >> k.vb_blk_force;
    k.detect = detect != 0; k.prescan = prescan != 0; k.batch_viterbi = batch != 0; k.soft_decision = soft != 0;
    return k;
}
static void print_cuts(const std::vector<Cut> &cuts, size_t first, size_t last)
{
    for (size_t i = first; i < last; i++) std::printf(" %" PRId64 ":%" PRId64 ":%u:%d", cuts[i].start, cuts[i].stop, cuts[i].max_frames, (int)cuts[i].first);
}
static void print_trellis(const TrellisCaps &c) { std::printf(" %u %" PRIu64 " %" PRIu64, c.vb_cap, c.vb_dw_words, c.vb_slots_alloc); }
static bool same(const Cut &a, const Cut &b) { return a.start == b.start && a.stop == b.stop && a.max_frames == b.max_frames && a.first == b.first; }
static bool same(const FrontPlan &a, const FrontPlan &b)
{
    const FrontCaps &p = a.caps, &q = b.caps;
    bool eq = a.seg == b.seg && a.taper == b.taper && a.ps_hops == b.ps_hops && a.first_cut == b.first_cut && a.cuts.size() == b.cuts.size() &&
              p.frame_base == q.frame_base && p.streams.size() == q.streams.size() && p.frame_slots == q.frame_slots && p.chain_slots == q.chain_slots &&
              p.run_cap == q.run_cap && p.mf_cap == q.mf_cap && p.sym_cap == q.sym_cap && p.byte_cap == q.byte_cap && p.dw_cap == q.dw_cap && p.out_cap == q.out_cap &&
              p.vb_blk == q.vb_blk && p.vb.vb_cap == q.vb.vb_cap && p.vb.vb_dw_words == q.vb.vb_dw_words && p.vb.vb_slots_alloc == q.vb.vb_slots_alloc && p.too_large == q.too_large;
    for (size_t i = 0; eq && i < a.cuts.size(); i++) eq = same(a.cuts[i], b.cuts[i]);
    for (size_t s = 0; eq && s < p.streams.size(); s++)
        eq = p.streams[s].chain_base == q.streams[s].chain_base && p.streams[s].chain_cap == q.streams[s].chain_cap && p.streams[s].repair_base == q.streams[s].repair_base;
    return eq;
}

int main(int argc, char **argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: frontplan_check <cases>\n"); return 2; }
    std::ifstream file(argv[1]);
    std::string line, word;
    unsigned long n_cases = 0;
    while (std::getline(file, line)) {
        std::istringstream in(line);
        if (!(in >> word)) continue;
        n_cases++;
        std::printf("%s", word.c_str());
        if (word == "cap") {
            uint64_t samples; int detect; in >> samples >> detect;
            std::printf(" %" PRIu64 " %u", frames_cap(samples, detect != 0), seg_frames_cap(samples, detect != 0));
        } else if (word == "seg") {
            const FrontKnobs k = read_knobs(in); uint64_t tot; in >> tot;
            std::printf(" %" PRIu64, segment_len(tot, k));
        } else if (word == "tap") {
            const FrontKnobs k = read_knobs(in); uint64_t tot, seg; in >> tot >> seg;
            std::printf(" %.9g", (double)choose_taper(tot, seg, k));
        } else if (word == "ps") {
            const FrontKnobs k = read_knobs(in); Traffic t; in >> t.frames >> t.samples;
            const uint32_t K = prescan_hops(t, k);
            std::printf(" %u %u", K, prescan_words(K));
        } else if (word == "cut") {
            uint64_t n, seg; int cont, detect; int64_t carry; float taper; in >> n >> cont >> carry >> seg >> taper >> detect;
            std::vector<Cut> cuts;
            cut_stream(cuts, n, cont != 0, carry, seg, taper, detect != 0);
            std::printf(" %zu", cuts.size()); print_cuts(cuts, 0, cuts.size());
            std::vector<uint32_t> order;
            for (uint32_t i = 0; i < cuts.size(); i++) if (!(cuts[i].first && cont)) order.push_back(i);
            longest_first(order, cuts);
            std::printf(" order"); for (uint32_t i : order) std::printf(" %u", i);
        } else if (word == "vb") {
            const FrontKnobs k = read_knobs(in); Traffic t; uint64_t span; in >> t.vb_steps >> span;
            const uint32_t blk = trellis_block(t, k);
            std::printf(" %u", blk); print_trellis(size_trellis(span, t.vb_steps, blk));
            print_trellis(size_trellis(span, t.vb_steps, (uint32_t)kVbBlkMin)); print_trellis(size_trellis(span, t.vb_steps, (uint32_t)kVbBlkMax));
        } else if (word == "win") {
            Traffic t; uint32_t slots, forced; in >> t.frames >> slots >> forced;
            std::printf(" %u", window_slots(t, slots, forced));
        } else if (word == "plan") {
            const FrontKnobs k = read_knobs(in); Traffic t; size_t NS; in >> t.frames >> t.samples >> t.vb_steps >> NS;
            std::vector<StreamIn> streams(NS);
            for (StreamIn &s : streams) { int cont; in >> s.n >> cont >> s.carry_bound; s.cont = cont != 0; }
            const FrontPlan p = front_plan(streams, t, k);
            const FrontCaps &c = p.caps;
            std::printf(" seg %" PRIu64 " taper %.9g ps %u jobs %zu repair_cap %u", p.seg, (double)p.taper, p.ps_hops, p.cuts.size(), kRepairCap);
            std::printf(" caps %u %u %u %u %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %u", c.frame_slots, c.chain_slots, c.run_cap, c.mf_cap, c.sym_cap, c.byte_cap, c.dw_cap, c.out_cap, c.vb_blk);
            print_trellis(c.vb);
            std::printf(" too_large %d same %d", (int)c.too_large, (int)same(p, front_plan(streams, t, k)));
            for (size_t s = 0; s < NS; s++) {
                std::printf("\nstream %u %u %u %u %u cuts", p.first_cut[s], p.first_cut[s + 1] - p.first_cut[s], c.streams[s].chain_base, c.streams[s].chain_cap, c.streams[s].repair_base);
                print_cuts(p.cuts, p.first_cut[s], p.first_cut[s + 1]);
                std::printf(" frame_base"); for (uint32_t i = p.first_cut[s]; i < p.first_cut[s + 1]; i++) std::printf(" %u", c.frame_base[i]);
            }
        } else { std::fprintf(stderr, "unknown case %s\n", word.c_str()); return 2; }
        if (!in) { std::fprintf(stderr, "short case: %s\n", line.c_str()); return 2; }
        std::printf("\n");
    }
    std::printf("%lu cases\n", n_cases);
    return 0;
}
