// blockfeed_check.cpp -- the drop-in's block feeder (gr-liquiddsp_amd/csrc/fx_blockfeed.h) against fakes of the eleven fxrx_*
// functions it uses, compiled host-only with g++: tests/test_blockfeed.py.  Every sample carries its own index; the fake context
// records each submitted block (pointer, length, checksum), refuses more than `depth` in flight, checks at collect that the block's
// buffer still holds what was submitted, and fails the k-th submit, collect or page-locked allocation on request.
#include <algorithm>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <set>
#include <string>
#include <vector>
#include <unistd.h>
#include "../../gr-liquiddsp_amd/csrc/fx_blockfeed.h"

static int g_fail = 0, g_checks = 0;
#define CHECK(c, ...) do { g_checks++; if (!(c)) { if (++g_fail <= 20) { std::printf("FAIL %s: ", #c); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

// ------------------------------------------------------------------------------------------ the fakes
static fx_complex sample(uint64_t i) { return fx_complex{ (float)(i & 0xFFFFu), (float)(i >> 16) }; }        // (exact below 2^40)
static uint64_t index_of(fx_complex s) { return ((uint64_t)s.im << 16) | (uint64_t)s.re; }
static uint64_t checksum(const fx_complex *p, uint64_t n)
{
    uint64_t h = 14695981039346656037ull;
    const unsigned char *b = (const unsigned char *)p;
    for (uint64_t i = 0; i < n * sizeof(fx_complex); i++) { h ^= b[i]; h *= 1099511628211ull; }
    return h;
}
struct Blk { const fx_complex *p; uint64_t n, sum; };
struct fxrx_ctx_s { unsigned depth = 1; std::deque<Blk> inflight; fxrx_config cfg; };

struct World {
    std::set<unsigned> fail_submits, fail_collects, fail_allocs;       // 1-based call numbers since the last clear()
    bool fail_create = false, fail_depth = false;
    unsigned submits = 0, collects = 0, allocs = 0, frees = 0, creates = 0, destroys = 0, resets = 0;
    std::vector<uint64_t> delivered, lost;                              // sample indices of blocks collected / dropped, in order of the event
    std::string events;                                                 // S s: submit good / failed, C c: collect, R: reset
    std::vector<fxrx_ctx *> destroyed;
    std::set<void *> live;                                              // page-locked allocations
    void clear() { *this = World(); }
} W;
static void log_block(std::vector<uint64_t> &to, const fx_complex *p, uint64_t n) { for (uint64_t i = 0; i < n; i++) to.push_back(index_of(p[i])); }

extern "C" {
const char *fxrx_last_error(void) { return "fake error"; }
void *fxrx_pinned_alloc(size_t bytes)
{
    if (W.fail_allocs.count(++W.allocs)) return nullptr;
    void *p = std::malloc(bytes ? bytes : 1); W.live.insert(p); return p;
}
void fxrx_pinned_free(void *p) { CHECK(W.live.erase(p) == 1, "free of a pointer that is not a live allocation"); W.frees++; std::free(p); }
fxrx_ctx *fxrx_create(const fxrx_config *cfg) { if (W.fail_create) return nullptr; W.creates++; fxrx_ctx *c = new fxrx_ctx_s; c->cfg = *cfg; return c; }
void fxrx_destroy(fxrx_ctx *c) { W.destroys++; W.destroyed.push_back(c); delete c; }
int fxrx_set_depth(fxrx_ctx *c, unsigned int depth) { if (W.fail_depth) return FXRX_ERR_ARG; c->depth = depth; return 0; }
void fxrx_reset(fxrx_ctx *c) { CHECK(c->inflight.empty(), "reset with %zu blocks in flight", c->inflight.size()); W.resets++; W.events += 'R'; }
unsigned int fxrx_inflight(const fxrx_ctx *c) { return (unsigned)c->inflight.size(); }
int fxrx_ready(fxrx_ctx *c) { return c->inflight.empty() ? 0 : 1; }
int fxrx_submit(fxrx_ctx *c, const void *const *iq, const uint64_t *n, int on_device)
{
    const fx_complex *p = (const fx_complex *)iq[0];
    CHECK(!on_device && n[0] > 0 && W.live.count((void *)p), "a submit of %llu samples from a buffer outside the ring", (unsigned long long)n[0]);
    for (const Blk &b : c->inflight) CHECK(b.p != p, "a buffer submitted again while in flight");
    if (W.fail_submits.count(++W.submits)) { W.events += 's'; log_block(W.lost, p, n[0]); return FXRX_ERR_STATE; }      // (the context is as it was)
    CHECK(c->inflight.size() < c->depth, "%zu in flight at depth %u", c->inflight.size() + 1, c->depth);
    c->inflight.push_back(Blk{ p, n[0], checksum(p, n[0]) });
    W.events += 'S';
    return 0;
}
int fxrx_collect(fxrx_ctx *c)
{
    if (c->inflight.empty()) { CHECK(false, "collect with nothing in flight"); return FXRX_ERR_STATE; }
    for (const Blk &b : c->inflight) CHECK(checksum(b.p, b.n) == b.sum, "a buffer was refilled while in flight");
    if (W.fail_collects.count(++W.collects)) {                          // every block in flight goes with it
        for (const Blk &b : c->inflight) log_block(W.lost, b.p, b.n);
        c->inflight.clear(); W.events += 'c';
        return FXRX_ERR_STATE;
    }
    log_block(W.delivered, c->inflight.front().p, c->inflight.front().n);
    c->inflight.pop_front(); W.events += 'C';
    return 0;
}
}

// ------------------------------------------------------------------------------------------ a feeder's owner
struct Feed : BlockFeed<Feed> {
    static constexpr const char *entry = "blockfeed_check";
    unsigned n_before = 0, n_submitted = 0, n_dropped = 0, n_taken = 0;
    uint64_t next = 0;                  // index of the next sample handed in
    Feed(unsigned block, unsigned depth) : BlockFeed(block, depth) {}
    void before_collect() { n_before++; }
    void submitted() { n_submitted++; }
    void dropped() { n_dropped++; }
    void take(int) { n_taken++; }
    bool start() { fxrx_config cfg{}; return replace_ctx(cfg) && set_ring(block); }
    // hand in n samples, `piece` at a time, the way both execute entries do
    void feed(uint64_t n, unsigned piece)
    {
        while (n) {
            uint64_t k = std::min<uint64_t>(n, piece); n -= k;
            while (k) {
                const uint64_t m = std::min<uint64_t>(k, block - fill);
                for (uint64_t i = 0; i < m; i++) bufs[cur][fill + i] = sample(next + i);
                fill += m; next += m; k -= m;
                if (fill == block) submit_current();
            }
        }
    }
};

// what the feeder wrote to stderr while f ran
template <class F> static std::string stderr_of(F f)
{
    std::fflush(stderr);
    FILE *t = std::tmpfile(); const int saved = dup(2);
    dup2(fileno(t), 2);
    f();
    std::fflush(stderr); dup2(saved, 2); close(saved);
    std::string s; char buf[4096]; size_t n;
    std::rewind(t);
    while ((n = std::fread(buf, 1, sizeof buf, t)) > 0) s.append(buf, n);
    std::fclose(t);
    return s;
}
static unsigned count_of(const std::string &s, const std::string &what)
{
    unsigned n = 0;
    for (size_t p = s.find(what); p != std::string::npos; p = s.find(what, p + 1)) n++;
    return n;
}

// every sample handed in was submitted exactly once and in order, or lies in a dropped block; `lost` is [lo, hi) exactly
static void check_account(uint64_t total, uint64_t lo, uint64_t hi, const char *tag)
{
    std::vector<uint64_t> expect_lost; for (uint64_t i = lo; i < hi; i++) expect_lost.push_back(i);
    std::vector<uint64_t> lost = W.lost; std::sort(lost.begin(), lost.end());
    CHECK(lost == expect_lost, "%s: %zu samples dropped, expected [%llu, %llu)", tag, lost.size(), (unsigned long long)lo, (unsigned long long)hi);
    bool ordered = true; for (size_t i = 1; i < W.delivered.size(); i++) ordered = ordered && W.delivered[i - 1] < W.delivered[i];
    CHECK(ordered, "%s: delivered samples out of order or twice", tag);
    std::vector<uint64_t> all = W.delivered; all.insert(all.end(), lost.begin(), lost.end()); std::sort(all.begin(), all.end());
    bool whole = all.size() == total; for (size_t i = 0; whole && i < all.size(); i++) whole = all[i] == i;
    CHECK(whole, "%s: %zu of %llu samples accounted for, or one twice", tag, all.size(), (unsigned long long)total);
}
// a failed submit is followed by collects of everything in flight (the fake's reset checks that) and then exactly one reset
static void check_resets(const char *tag)
{
    unsigned failed = 0; bool ok = true;
    for (size_t i = 0; i < W.events.size(); i++) {
        if (W.events[i] != 's') continue;
        failed++;
        size_t j = i + 1; while (j < W.events.size() && (W.events[j] == 'C' || W.events[j] == 'c')) j++;
        ok = ok && j < W.events.size() && W.events[j] == 'R' && (j + 1 == W.events.size() || W.events[j + 1] != 'R');
    }
    CHECK(ok && W.resets == failed, "%s: %u resets for %u failed submits (%s)", tag, W.resets, failed, W.events.size() < 200 ? W.events.c_str() : "...");
}

// fail_submit / fail_collect: the 1-based call to fail, 0 for none
static void stream_case(unsigned depth, unsigned block, unsigned piece, unsigned fail_submit, unsigned fail_collect)
{
    char tag[96]; std::snprintf(tag, sizeof tag, "depth %u block %u piece %u submit %u collect %u", depth, block, piece, fail_submit, fail_collect);
    W.clear();
    const uint64_t total = (uint64_t)block * (2 * (depth + 1) + 3) + block / 2;
    {
        Feed f(block, depth);
        CHECK(f.start(), "%s: start", tag);
        if (fail_submit) W.fail_submits.insert(fail_submit);
        if (fail_collect) W.fail_collects.insert(fail_collect);
        (void)stderr_of([&] { f.feed(total, piece); f.flush(); });
        CHECK(f.fill == 0 && fxrx_inflight(f.ctx) == 0, "%s: something left behind after flush", tag);
        // the k-th submit carries block k - 1; while samples stream in a collect happens only at `depth` in flight, k - 1 blocks after the first
        uint64_t lo = 0, hi = 0;
        if (fail_submit) { lo = (uint64_t)(fail_submit - 1) * block; hi = lo + block; }
        if (fail_collect) { lo = (uint64_t)(fail_collect - 1) * block; hi = lo + (uint64_t)depth * block; }
        check_account(total, lo, hi, tag);
        check_resets(tag);
        const unsigned failures = (fail_submit ? 1 : 0) + (fail_collect ? 1 : 0);
        CHECK(f.errors == failures, "%s: errors %u", tag, f.errors);
        CHECK(f.n_dropped == (fail_collect ? 1u : 0u) && f.n_submitted == W.submits - (fail_submit ? 1 : 0) && f.n_before == W.collects && f.n_taken == W.collects - f.n_dropped, "%s: hooks", tag);
    }
    CHECK(W.allocs == depth + 1 && W.frees == W.allocs && W.live.empty() && W.creates == 1 && W.destroys == 1, "%s: %u allocs %u frees, %u contexts %u destroyed", tag, W.allocs, W.frees, W.creates, W.destroys);
}

// a collect that fails inside the drain behind a failed submit: submit depth + 2 (block depth + 1) fails with two blocks collected and
// blocks 2 .. depth in flight; the drain's first collect, the third in all, fails and takes those with it; then the one reset
static void drain_drops_case(unsigned depth, unsigned block)
{
    char tag[64]; std::snprintf(tag, sizeof tag, "failed drain, depth %u block %u", depth, block);
    W.clear();
    const uint64_t total = (uint64_t)block * (2 * (depth + 1) + 3) + block / 2;
    Feed f(block, depth);
    CHECK(f.start(), "%s: start", tag);
    W.fail_submits.insert(depth + 2); W.fail_collects.insert(3);
    (void)stderr_of([&] { f.feed(total, 97); f.flush(); });
    check_account(total, 2 * (uint64_t)block, (uint64_t)(depth + 2) * block, tag);
    check_resets(tag);
    CHECK(W.events.find("scR") != std::string::npos && W.resets == 1, "%s: the reset does not follow the failed collect of the drain", tag);
    CHECK(f.errors == 2 && f.n_dropped == 1 && f.fill == 0 && fxrx_inflight(f.ctx) == 0, "%s: errors %u, dropped %u", tag, f.errors, f.n_dropped);
}

// 20 scripted failures: errors counts each once, stderr speaks at failures 1, 2, 4, 8 and 16 only
static void report_rule(bool at_submit)
{
    W.clear();
    Feed f(7, 2);
    CHECK(f.start(), "report rule: start");
    for (unsigned k = 1; k <= 20; k++) (at_submit ? W.fail_submits : W.fail_collects).insert(3 * k);
    const std::string err = stderr_of([&] { f.feed(7 * 200, 256); f.flush(); });
    CHECK(f.errors == 20, "report rule: errors %u after 20 failures", f.errors);
    CHECK(count_of(err, "\n") == 5 && count_of(err, "failures so far]\n") == 5, "report rule: %u lines", count_of(err, "\n"));
    for (unsigned n : { 1u, 2u, 4u, 8u, 16u }) {
        char line[160]; std::snprintf(line, sizeof line, "libfxrx: blockfeed_check: %s failed (%d): fake error [%u failures so far]\n", at_submit ? "submit" : "block", FXRX_ERR_STATE, n);
        CHECK(count_of(err, line) == 1, "report rule: no line for failure %u in:\n%s", n, err.c_str());
    }
    check_resets("report rule");
    std::vector<uint64_t> all = W.delivered; all.insert(all.end(), W.lost.begin(), W.lost.end()); std::sort(all.begin(), all.end());
    bool whole = all.size() == 7 * 200; for (size_t i = 0; whole && i < all.size(); i++) whole = all[i] == i;
    CHECK(whole && !W.lost.empty(), "report rule: samples fed twice or left behind");
}

// resizing fails at each of its depth + 1 allocations in turn: nothing of the old ring moves
static void resize_case(unsigned depth, unsigned block)
{
    W.clear();
    {
        Feed f(block, depth);
        CHECK(f.start(), "resize: start");
        (void)stderr_of([&] { f.feed((uint64_t)block + block / 2, 256); });            // one block in flight, half of the next in the buffer
        const std::vector<fx_complex *> ring = f.bufs; const unsigned cur = f.cur; const size_t fill = f.fill;
        CHECK(cur == 1 && fill == block / 2, "resize: cur %u fill %zu", cur, fill);
        const std::vector<fx_complex> held(f.bufs[cur], f.bufs[cur] + fill);
        for (unsigned i = 1; i <= depth + 1; i++) {
            const unsigned errors = f.errors, allocs = W.allocs, frees = W.frees;
            W.fail_allocs = { W.allocs + i };
            bool ok = true;
            const std::string err = stderr_of([&] { ok = f.resize(2 * block + 3, "the_caller"); });
            CHECK(!ok && f.errors == errors + 1, "resize: allocation %u of %u fails, errors %u -> %u", i, depth + 1, errors, f.errors);
            CHECK(err == "libfxrx: the_caller: fake error (block length unchanged)\n", "resize: stderr '%s'", err.c_str());
            CHECK(f.bufs == ring && f.block == block && f.cur == cur && f.fill == fill && std::equal(held.begin(), held.end(), f.bufs[cur], [](fx_complex a, fx_complex b) { return a.re == b.re && a.im == b.im; }), "resize: the old ring moved at failing allocation %u", i);
            CHECK(W.allocs == allocs + i && W.frees == frees + (i - 1), "resize: %u allocations, %u freed at failing allocation %u", W.allocs - allocs, W.frees - frees, i);
        }
        f.flush();
        check_account((uint64_t)block + block / 2, 0, 0, "resize: the old ring after the failures");
        CHECK(f.resize(2 * block + 3, "the_caller") && f.block == 2 * block + 3 && f.cur == 0 && f.fill == 0 && f.bufs.size() == depth + 1, "resize: the new ring");
        for (fx_complex *p : ring) CHECK(!W.live.count(p), "resize: a buffer of the old ring is still allocated");
        W.delivered.clear(); f.next = 0;
        f.feed(3 * (uint64_t)f.block, 97); f.flush();
        check_account(3 * (uint64_t)f.block, 0, 0, "resize: the new ring");
    }
    CHECK(W.frees + (depth + 1) == W.allocs && W.live.empty(), "resize: %u allocation calls (%u refused), %u frees", W.allocs, depth + 1, W.frees);
}

static void context_case()
{
    W.clear();
    {
        Feed f(7, 3);
        fxrx_config cfg{}; cfg.threshold = 0.25f;
        setenv("FXRX_DEVICE", "3", 1);
        CHECK(f.replace_ctx(cfg) && f.ctx && f.ctx->depth == 3 && f.ctx->cfg.device == 3 && f.ctx->cfg.threshold == 0.25f, "context: made with depth and FXRX_DEVICE");
        unsetenv("FXRX_DEVICE");
        fxrx_ctx *old = f.ctx;
        W.fail_create = true;
        CHECK(!f.replace_ctx(cfg) && f.ctx == old && W.destroys == 0, "context: a failed creation keeps the old one");
        W.fail_create = false; W.fail_depth = true;
        CHECK(!f.replace_ctx(cfg) && f.ctx == old && W.creates == 2 && W.destroys == 1 && W.destroyed[0] != old, "context: a failed set_depth destroys the new one, keeps the old");
        W.fail_depth = false;
        CHECK(f.replace_ctx(cfg) && f.ctx != old && f.ctx->cfg.device == 0 && W.destroys == 2 && W.destroyed[1] == old, "context: a good replacement destroys the old one once");
        CHECK(f.errors == 0, "context: errors are the caller's to count");
    }
    CHECK(W.creates == 3 && W.destroys == 3 && std::count(W.destroyed.begin(), W.destroyed.end(), W.destroyed[1]) == 1, "context: %u made, %u destroyed", W.creates, W.destroys);
}

static void empty_cases()
{
    W.clear();
    {
        Feed f(7, 2);
        CHECK(f.start(), "empty: start");
        f.flush(); f.drain(); f.submit_current();
        CHECK(W.submits == 0 && W.collects == 0 && W.resets == 0 && f.cur == 0, "empty: flush on an empty feeder submitted or collected");
    }
    {   // a handle without a context: nothing is called, and report says so
        Feed f(7, 2);
        const std::string err = stderr_of([&] { f.flush(); f.drain(); f.submit_current(); f.report("block", -4); });
        CHECK(W.submits == 0 && W.collects == 0 && f.errors == 1, "no context: calls were made");
        CHECK(err == "libfxrx: blockfeed_check: block failed (-4): no context [1 failures so far]\n", "no context: stderr '%s'", err.c_str());
        CHECK(!f.set_ring(7) || f.bufs.size() == 3, "no context: a ring");
    }
    CHECK(W.frees == W.allocs && W.live.empty() && W.creates == W.destroys, "empty: leaks");
}

int main()
{
    for (unsigned depth : { 1u, 2u, 3u, 15u }) for (unsigned block : { 1u, 7u, 4096u }) {
        for (unsigned piece : { 1u, 256u, 97u }) {
            stream_case(depth, block, piece, 0, 0);
            for (unsigned k : { 1u, 2u, depth + 2 }) { stream_case(depth, block, piece, k, 0); stream_case(depth, block, piece, 0, k); }
        }
        if (depth > 1) drain_drops_case(depth, block);         // (at depth 1 nothing is in flight when a submit fails)
        resize_case(depth, block);
    }
    report_rule(true); report_rule(false);
    context_case();
    empty_cases();
    std::printf("%d checks, %d failures\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
