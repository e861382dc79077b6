// dropin_feed.cpp -- bench / test driver for the boundary the reference really has: a host IQ buffer goes through the C++
// flex_rx block shell (gr-liquiddsp_amd/csrc/blocks/fx_blocks.hpp) the way GNU Radio's scheduler would feed it -- work() calls
// of `items_per_work` items from pageable memory, inside each the reference's own loop of flexframesync_execute(q, in, 256)
// calls (/root/reference/lib/flex_rx_impl.cc:212-215), one frame drained and published as three messages after each
// (:216-250).  Messages are counted and the payload bytes hashed so that the caller can check every frame.
// Built by csrc/Makefile into csrc/libdropin_feed.so; links against libfxrx.so only.
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>
#include "fx_blocks.hpp"

extern "C" {

struct dropin_stats {
    double   seconds;               // wall time of the work() loop including the final flush
    uint64_t frames, header_valid, payload_valid, payload_bytes, constellation_syms, packet_infos;
    uint64_t payload_hash;          // FNV-1a over all payload_data bytes in order of arrival
    uint64_t errors;                // fxrx_sync_errors() at the end
    double   first_frame_seconds;   // wall time from the first work() call to the first published frame
};

// returns 0, or -1 when the block could not be made (no GPU: the text is in fxrx_last_error())
int dropin_feed(const float *iq, unsigned long long n_samples, unsigned items_per_work, unsigned repeats, dropin_stats *out)
{
    using namespace gr::liquiddsp;
    using clk = std::chrono::steady_clock;
    dropin_stats st{}; st.payload_hash = 14695981039346656037ull;
    flex_rx::sptr rx;
    try { rx = flex_rx::make(); } catch (const std::exception &e) { std::fprintf(stderr, "dropin_feed: %s\n", e.what()); return -1; }
    clk::time_point t0; bool first = true;
    rx->set_msg_sink([&](const std::string &port, const msg_t &m) {
        if (port == "constellation") {
            st.frames++; st.constellation_syms += m.c32.size();
            if (first) { first = false; st.first_frame_seconds = std::chrono::duration<double>(clk::now() - t0).count(); }
        }
        else if (port == "payload_data") {
            st.header_valid++; st.payload_bytes += m.u8.size();
            uint64_t h = st.payload_hash;
            for (uint8_t b : m.u8) { h ^= b; h *= 1099511628211ull; }
            st.payload_hash = h;
        } else if (port == "packet_info") { st.packet_infos++; st.payload_valid += (uint64_t)m.dict.at("payload_valid"); }
    });
    if (items_per_work < 256) items_per_work = 256;
    items_per_work -= items_per_work % 256;
    gr_vector_const_void_star in(1); gr_vector_void_star outv;
    t0 = clk::now();
    for (unsigned r = 0; r < (repeats ? repeats : 1u); r++) {
        if (r) flexframesync_reset(rx->handle());      // every repeat is an independent capture
        unsigned long long p = 0;
        while (p + 256 <= n_samples) {
            const unsigned long long left = n_samples - p;
            int n = (int)(left < items_per_work ? left - left % 256 : items_per_work);
            in[0] = iq + 2 * p;
            rx->work(n, in, outv);
            p += (unsigned long long)n;
        }
        rx->flush();
    }
    st.seconds = std::chrono::duration<double>(clk::now() - t0).count();
    st.errors = fxrx_sync_errors(rx->handle());
    *out = st;
    return 0;
}

// The bare C boundary without the block shell's messages: flexframesync_execute(q, x, 256) over the buffer, a callback that
// counts frames and hashes payload bytes where they lie (no copies) -- what the library itself costs behind the reference's
// calling convention, apart from what the caller does with a frame.
static int raw_cb(unsigned char *, int hv, unsigned char *p, unsigned int n, int pv, framesyncstats_s st, void *ud)
{
    dropin_stats *s = (dropin_stats *)ud;
    s->frames++; s->constellation_syms += st.num_framesyms;
    if (hv) {
        s->header_valid++; s->payload_bytes += n; s->payload_valid += (uint64_t)(pv != 0); s->packet_infos++;
        uint64_t h = s->payload_hash;
        for (unsigned i = 0; i < n; i++) { h ^= p[i]; h *= 1099511628211ull; }
        s->payload_hash = h;
    }
    return 0;
}
int dropin_feed_raw(const float *iq, unsigned long long n_samples, unsigned repeats, dropin_stats *out)
{
    using clk = std::chrono::steady_clock;
    dropin_stats st{}; st.payload_hash = 14695981039346656037ull;
    flexframesync q = flexframesync_create(raw_cb, &st);
    if (!q) return -1;
    const auto t0 = clk::now();
    for (unsigned r = 0; r < (repeats ? repeats : 1u); r++) {
        if (r) flexframesync_reset(q);
        for (unsigned long long p = 0; p + 256 <= n_samples; p += 256) flexframesync_execute(q, (fx_complex *)(iq + 2 * p), 256);
        fxrx_sync_flush(q);
        while (fxrx_sync_pending(q)) flexframesync_execute(q, nullptr, 0);
    }
    st.seconds = std::chrono::duration<double>(clk::now() - t0).count();
    st.errors = fxrx_sync_errors(q);
    flexframesync_destroy(q);
    *out = st;
    return 0;
}

#ifndef DROPIN_NO_CEILING      /* (built without it against round 2's library, which has no fxrx_pinned_alloc) */
// What the calling convention alone costs: the same stream in the same 256-sample pieces, each piece only copied into a page-locked
// buffer of `block` samples (what any GPU implementation behind flexframesync_execute has to do with pageable caller memory
// before it can upload).  Returns samples per second of that loop -- the ceiling of the drop-in boundary on this host.
double dropin_copy_ceiling(const float *iq, unsigned long long n_samples, unsigned block, unsigned repeats)
{
    using clk = std::chrono::steady_clock;
    fx_complex *buf[4];                                         // a ring like the library's: the destination is never cache-resident
    for (auto &b : buf) { b = (fx_complex *)fxrx_pinned_alloc((size_t)block * sizeof(fx_complex)); if (!b) return 0.0; }
    volatile size_t sink = 0;
    const auto t0 = clk::now();
    for (unsigned r = 0; r < (repeats ? repeats : 1u); r++) {
        size_t fill = 0; unsigned cur = 0;
        for (unsigned long long p = 0; p + 256 <= n_samples; p += 256) {
            std::memcpy(buf[cur] + fill, iq + 2 * p, 256 * sizeof(fx_complex));
            fill += 256; if (fill + 256 > block) { sink = sink + fill; fill = 0; cur = (cur + 1) & 3u; }
        }
    }
    const double dt = std::chrono::duration<double>(clk::now() - t0).count();
    for (auto b : buf) fxrx_pinned_free(b);
    return (double)(repeats ? repeats : 1u) * (double)(n_samples - n_samples % 256) / dt;
}
#endif

// frame_detector_cc's boundary: the reference's per-sample loop (/root/reference/lib/frame_detector_cc_impl.cc:76-82) over a host buffer --
// qdetector_cccf_execute(q, in[i]) for every sample, a non-NULL return is a detection.  Afterwards what is queued is flushed and the
// pending detections are drawn with calls that hand in zeros.  Every detection's estimates and window are hashed in order of arrival
// (FNV-1a over the four floats and the 512 samples), and copied to est (4 floats each) / wins (1024 floats each) for the first `cap`.
// block: fxrx_qdet_set_block (0: default); fail_collect_at: sample index in front of which the next collect is made to fail (~0: never).
struct dropin_det_stats { double seconds; uint64_t detections, hash, errors, samples_fed; };
int dropin_feed_detector(const float *iq, unsigned long long n_samples, unsigned block, unsigned long long fail_collect_at, float threshold,
                         float *est, float *wins, unsigned cap, dropin_det_stats *out)
{
    using clk = std::chrono::steady_clock;
    dropin_det_stats st{}; st.hash = 14695981039346656037ull;
    fx_complex pn[64];
    msequence ms = msequence_create(7, 0x0089, 1);                          // :47-52
    if (!ms) return -1;
    for (int i = 0; i < 64; i++) {
        pn[i].re = msequence_advance(ms) ? (float)M_SQRT1_2 : -(float)M_SQRT1_2;
        pn[i].im = msequence_advance(ms) ? (float)M_SQRT1_2 : -(float)M_SQRT1_2;
    }
    msequence_destroy(ms);
    qdetector_cccf q = qdetector_cccf_create_linear(pn, 64, LIQUID_FIRFILT_ARKAISER, 2, 7, 0.3f);   // :54
    if (!q) return -1;
    qdetector_cccf_set_threshold(q, threshold);                             // :55
    if (block) fxrx_qdet_set_block(q, block);
    auto take = [&](void *v) {
        const float e[4] = { qdetector_cccf_get_tau(q), qdetector_cccf_get_gamma(q), qdetector_cccf_get_dphi(q), qdetector_cccf_get_phi(q) };
        uint64_t h = st.hash;
        const unsigned char *b = (const unsigned char *)e;
        for (unsigned i = 0; i < sizeof e; i++) { h ^= b[i]; h *= 1099511628211ull; }
        b = (const unsigned char *)v;
        for (unsigned i = 0; i < 512 * sizeof(fx_complex); i++) { h ^= b[i]; h *= 1099511628211ull; }
        st.hash = h;
        if (st.detections < cap) {
            if (est) std::memcpy(est + 4 * st.detections, e, sizeof e);
            if (wins) std::memcpy(wins + 1024 * st.detections, v, 512 * sizeof(fx_complex));
        }
        st.detections++;
    };
    const fx_complex *in = (const fx_complex *)iq;
    const auto t0 = clk::now();
    for (unsigned long long i = 0; i < n_samples; i++) {
        if (i == fail_collect_at) fxrx_debug_fail(fxrx_qdet_context(q), 0, 1);
        void *v = qdetector_cccf_execute(q, in[i]);                         // :77
        if (v) take(v);                                                     // :78-81
    }
    st.samples_fed = n_samples;
    fxrx_qdet_flush(q);
    const fx_complex zero{ 0.0f, 0.0f };
    while (fxrx_qdet_pending(q)) { void *v = qdetector_cccf_execute(q, zero); if (v) take(v); }
    st.seconds = std::chrono::duration<double>(clk::now() - t0).count();
    st.errors = fxrx_qdet_errors(q);
    qdetector_cccf_destroy(q);
    *out = st;
    return 0;
}

// A paced source: the buffer in 256-sample flexframesync_execute calls, call k not before t0 + 256 k / rate (busy-waiting on the wall
// clock: an SDR's sample clock), streaming delivery with `streaming_floor` (0: off).  frame_end[j] is the index of the last sample of
// injected frame j; frames arrive in order, so callback j belongs to it, and latency[j] (seconds) is the time from the entry of the call
// that handed in that sample to the callback (never negative: a callback inside that very call counts from its entry).  No call is
// made after the input ends: *undelivered = frames that had not arrived by then; a flush fetches them afterwards, they get no
// latency.  The pairing is checked: -2 unless exactly n_frames callbacks came in all, every one with a valid header and payload.
// Before the clock starts the first 2^18 samples run through the handle unpaced and unmeasured (first launches, first-size
// allocations of the block's arenas), and the handle is reset.  Returns the number of callbacks with a latency, -1 or -2.
struct pace_state { std::vector<double> *t_cb; std::chrono::steady_clock::time_point t0; unsigned invalid; };
static int pace_cb(unsigned char *, int hv, unsigned char *, unsigned int, int pv, framesyncstats_s, void *ud)
{
    pace_state *s = (pace_state *)ud;
    s->t_cb->push_back(std::chrono::duration<double>(std::chrono::steady_clock::now() - s->t0).count());
    if (!hv || !pv) s->invalid++;
    return 0;
}
int dropin_feed_paced(const float *iq, unsigned long long n_samples, double rate, unsigned streaming_floor, const unsigned long long *frame_end,
                      unsigned n_frames, double *latency, unsigned *undelivered, double *achieved_rate)
{
    using clk = std::chrono::steady_clock;
    std::vector<double> t_cb; pace_state ps; ps.t_cb = &t_cb; ps.invalid = 0; ps.t0 = clk::now();
    flexframesync q = flexframesync_create(pace_cb, &ps);
    if (!q) return -1;
    fxrx_sync_set_streaming(q, streaming_floor);
    const unsigned long long n_calls = n_samples / 256;
    std::vector<double> t_in(n_calls);
    {   // warm-up: a real block's worth, the way the measurement feeds
        const unsigned long long w = std::min<unsigned long long>(n_calls, 1024);
        for (unsigned long long k = 0; k < w; k++) flexframesync_execute(q, (fx_complex *)(iq + 512 * k), 256);
        fxrx_sync_flush(q);
        while (fxrx_sync_pending(q)) flexframesync_execute(q, nullptr, 0);
        flexframesync_reset(q); t_cb.clear(); ps.invalid = 0;
    }
    ps.t0 = clk::now();
    double t_last = 0.0;
    for (unsigned long long k = 0; k < n_calls; k++) {
        const double due = (double)(256 * k) / rate;
        double now;
        while ((now = std::chrono::duration<double>(clk::now() - ps.t0).count()) < due) { }
        t_in[k] = now;
        flexframesync_execute(q, (fx_complex *)(iq + 512 * k), 256);
    }
    t_last = std::chrono::duration<double>(clk::now() - ps.t0).count();
    if (achieved_rate) *achieved_rate = n_calls ? (double)(256 * n_calls) / t_last : 0.0;
    const unsigned got = (unsigned)std::min<size_t>(t_cb.size(), n_frames);
    const size_t seen = t_cb.size();
    for (unsigned j = 0; j < got; j++) {
        const unsigned long long k = std::min<unsigned long long>(frame_end[j] / 256, n_calls ? n_calls - 1 : 0);
        latency[j] = std::max(0.0, t_cb[j] - t_in[k]);
    }
    if (undelivered) *undelivered = n_frames - got;
    fxrx_sync_flush(q);
    while (fxrx_sync_pending(q)) flexframesync_execute(q, nullptr, 0);
    const bool paired = seen <= n_frames && t_cb.size() == n_frames && ps.invalid == 0 && fxrx_sync_errors(q) == 0;
    flexframesync_destroy(q);
    return paired ? (int)got : -2;
}

// the same from `n_threads` threads at once, each with its own block instance (GNU Radio: one thread per block) and its own
// buffer; stats[t] per thread.  Returns the number of threads that failed to make their block.
int dropin_feed_threads(const float *const *iq, const unsigned long long *n_samples, unsigned n_threads, unsigned items_per_work, dropin_stats *stats)
{
    std::vector<std::thread> th; std::vector<int> rc(n_threads, 0);
    for (unsigned t = 0; t < n_threads; t++)
        th.emplace_back([&, t]() { rc[t] = dropin_feed(iq[t], n_samples[t], items_per_work, 1, stats + t); });
    for (auto &x : th) x.join();
    int bad = 0; for (int r : rc) bad += r != 0;
    return bad;
}

}  // extern "C"
