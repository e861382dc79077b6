// fx_blockfeed.h -- the block feeder under flexframesync_execute and qdetector_cccf_execute (fx_dropin.cpp), host only: a ring of
// depth + 1 page-locked buffers of `block` samples on one batched context (include/fxrx.h, layer 2; nothing else is used here, so
// tests/cpp/blockfeed_check.cpp links it against fakes of those eleven functions).  The caller fills bufs[cur] up to `fill`; a
// buffer handed over (submit_current) is the next block of one continuing stream, and the next buffer of the ring fills while up to
// `depth` blocks are in flight: a buffer comes round again only after depth collects.  The rule the public header promises: no
// sample is fed twice and no block is left behind.  A block that fails, at its submit or at its collect, is dropped with its
// samples (a failed collect takes every block in flight with it), the stream restarts freshly reset behind the gap, `errors` goes
// up and one line goes to stderr at failures 1, 2, 4, 8, ...
// Owner (CRTP, bound statically: nothing here is a virtual call) supplies `entry`, the name its stderr lines begin with, and
// take(nr), which reads the nr results of the block just collected (fxrx_result); it may shadow the three empty hooks below.
#ifndef FX_BLOCKFEED_H
#define FX_BLOCKFEED_H
#include <vector>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <xmmintrin.h>
#include "../../include/fxrx.h"

template <class Owner> struct BlockFeed {
    fxrx_ctx *ctx = nullptr;
    unsigned block, depth;              // samples per buffer; blocks in flight at most
    std::vector<fx_complex *> bufs; unsigned cur = 0; size_t fill = 0;
    unsigned errors = 0;

    BlockFeed(unsigned block_, unsigned depth_) : block(block_), depth(depth_) {}
    BlockFeed(const BlockFeed &) = delete;
    BlockFeed &operator=(const BlockFeed &) = delete;
    ~BlockFeed() { if (ctx) fxrx_destroy(ctx); free_ring(); }       // (the context first: its blocks in flight read the ring)

    void before_collect() {}            // the context's results are about to be replaced
    void submitted() {}                 // the buffer just handed over is in flight
    void dropped() {}                   // a collect failed: every block in flight went with it

    // ---- the ring: all or nothing
    void free_ring() { for (auto p : bufs) fxrx_pinned_free(p); bufs.clear(); cur = 0; fill = 0; }
    // a new ring of depth + 1 buffers of `samples`; the old one (with block, cur, fill and what it holds) is given up only once the
    // new one stands.  Call it with nothing queued or in flight (after flush)
    bool set_ring(unsigned samples)
    {
        std::vector<fx_complex *> ring;
        for (unsigned i = 0; i < depth + 1; i++) {
            fx_complex *p = (fx_complex *)fxrx_pinned_alloc((size_t)samples * sizeof(fx_complex));
            if (!p) { for (auto o : ring) fxrx_pinned_free(o); return false; }
            ring.push_back(p);
        }
        free_ring();
        bufs.swap(ring); block = samples;
        return true;
    }
    bool resize(unsigned samples, const char *what)
    {
        if (set_ring(samples)) return true;
        errors++; std::fprintf(stderr, "libfxrx: %s: %s (block length unchanged)\n", what, fxrx_last_error());
        return false;
    }

    // ---- the context: FXRX_DEVICE overrides the device; `depth` blocks in flight or no context at all
    static fxrx_ctx *make_ctx(fxrx_config cfg, unsigned depth)
    {
        if (const char *d = std::getenv("FXRX_DEVICE")) cfg.device = std::atoi(d);
        fxrx_ctx *nc = fxrx_create(&cfg);
        if (nc && fxrx_set_depth(nc, depth) != 0) { fxrx_destroy(nc); nc = nullptr; }
        return nc;
    }
    // the old context is given up only once the new one stands (call it with nothing in flight that is still wanted)
    bool replace_ctx(const fxrx_config &cfg)
    {
        fxrx_ctx *nc = make_ctx(cfg, depth);
        if (!nc) return false;
        if (ctx) fxrx_destroy(ctx);
        ctx = nc;
        return true;
    }

    // ---- feeding
    void report(const char *what, int rc)
    {
        if (errors++ == 0 || (errors & (errors - 1)) == 0)
            std::fprintf(stderr, "libfxrx: %s: %s failed (%d): %s [%u failures so far]\n", Owner::entry, what, rc, ctx ? fxrx_last_error() : "no context", errors);
    }
    // the oldest block in flight: wait for it, let the owner take its results
    void collect_one()
    {
        self().before_collect();
        const int nr = fxrx_collect(ctx);
        if (nr < 0) { report("block", nr); self().dropped(); return; }      // (the streams restart fresh with the next block)
        self().take(nr);
    }
    void drain() { while (ctx && fxrx_inflight(ctx)) collect_one(); }
    // hand the buffer being filled to the GPU as the stream's next block
    void submit_current()
    {
        if (!fill || !ctx) return;
        if (fxrx_inflight(ctx) >= depth) collect_one();
        _mm_sfence();                   // (samples written with non-temporal stores are in memory before the upload is enqueued; once a block)
        const void *p = bufs[cur]; uint64_t n = fill;
        const int r = fxrx_submit(ctx, &p, &n, 0);
        if (r < 0) {                    // the context is as it was before the call; these samples are lost to it, never fed again
            report("submit", r);
            drain();
            fxrx_reset(ctx);
        } else self().submitted();
        cur = (cur + 1) % (unsigned)bufs.size(); fill = 0;
    }
    void flush() { submit_current(); drain(); }

private:
    Owner &self() { return *static_cast<Owner *>(this); }
};
#endif
