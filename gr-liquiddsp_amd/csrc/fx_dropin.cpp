// fx_dropin.cpp -- the liquid-dsp entry points that gr::liquiddsp's blocks call, re-hosted on the
// batched GPU context (include/fxrx.h, layer 1).  Each function cites the reference call site it serves.
#include <algorithm>
#include <deque>
#include <memory>
#include <vector>
#include <cstring>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <emmintrin.h>
#include "../../include/fxrx.h"
#include "fx_blockfeed.h"
#include "fx_codec.hpp"

namespace {

// Samples go from the caller's (hot, pageable) buffer into a page-locked ring that the CPU never reads again: stream them past
// the cache with non-temporal stores (no read-for-ownership of the destination lines: half the DRAM traffic of a plain memcpy,
// which a single core's copy of tens of MB per second-fraction is bound by).  Falls back to memcpy for unaligned pieces.
inline void stream_copy(fx_complex *dst, const fx_complex *src, size_t n)
{
    if ((reinterpret_cast<uintptr_t>(dst) & 15u) || n < 8) { std::memcpy(dst, src, n * sizeof(fx_complex)); return; }
    const size_t n16 = n / 2;                                  // 16-byte pieces (two samples)
    __m128i *d = reinterpret_cast<__m128i *>(dst); const __m128i *s = reinterpret_cast<const __m128i *>(src);
    size_t i = 0;
    for (; i + 4 <= n16; i += 4) {
        const __m128i a = _mm_loadu_si128(s + i), b = _mm_loadu_si128(s + i + 1), c = _mm_loadu_si128(s + i + 2), e = _mm_loadu_si128(s + i + 3);
        _mm_stream_si128(d + i, a); _mm_stream_si128(d + i + 1, b); _mm_stream_si128(d + i + 2, c); _mm_stream_si128(d + i + 3, e);
    }
    for (; i < n16; i++) _mm_stream_si128(d + i, _mm_loadu_si128(s + i));
    if (n & 1) dst[n - 1] = src[n - 1];
}

// A completed frame waiting for its callback.  Buffers are BORROWED from the context's result arenas (pinned host memory the
// kernels wrote into; valid until the next fxrx_collect on the context) unless `own` holds copies.
struct HeldFrame {
    unsigned char header[20]; int header_valid = 0, payload_valid = 0;
    const unsigned char *payload = nullptr; unsigned payload_len = 0;
    const fx_complex *syms = nullptr; unsigned nsyms = 0;
    bool owned = false; std::vector<unsigned char> own_payload; std::vector<fx_complex> own_syms;
    framesyncstats_s stats{};
    void materialise()                      // take copies: the arenas are about to be reused
    {
        if (owned) return;
        if (payload && payload_len) { own_payload.assign(payload, payload + payload_len); payload = own_payload.data(); }
        if (syms && nsyms) { own_syms.assign(syms, syms + nsyms); syms = own_syms.data(); }
        owned = true;
    }
};

constexpr unsigned kSyncBlockDefault = 1u << 20;    // samples per GPU block (fxrx_sync_set_block / FXRX_SYNC_BLOCK); see DESIGN.md section 7
constexpr unsigned kSyncDepthDefault = 3;           // blocks in flight (FXRX_SYNC_DEPTH)
constexpr unsigned kSyncPollEvery = 1u << 15;       // samples between two looks at whether the oldest block has finished (an event query costs about as much as copying 4000 samples)
constexpr unsigned kQdetBlockDefault = 1u << 16;    // qdetector_cccf_execute: samples per GPU block (fxrx_qdet_set_block / FXRX_QDET_BLOCK)
constexpr unsigned kQdetDepthDefault = 1;           // ... blocks in flight (FXRX_QDET_DEPTH)
constexpr unsigned kQdetPollEvery = 1u << 10;       // ... calls between two looks at the oldest block in flight

}  // namespace

// ------------------------------------------------------------------------------------------ flexframesync
// The reference feeds 256 samples per call from pageable memory (/root/reference/lib/flex_rx_impl.cc:212-215).  Here a call
// copies them into the pinned buffer being filled; a full buffer is submitted as one block of the continuing stream
// (fxrx_submit: upload and the whole kernel chain are enqueued, nothing is waited for) and the next buffer of the ring is
// filled while up to `depth` blocks are in flight (fx_blockfeed.h).  Finished blocks are collected when a slot is needed or when a
// poll (every few thousand samples) finds the oldest one done; their frames wait in `pending` and leave one per call.
struct fxrx_sync_s : BlockFeed<fxrx_sync_s> {
    static constexpr const char *entry = "flexframesync_execute";
    framesync_callback cb = nullptr; void *ud = nullptr;
    float threshold = 0.0f; int equalizer = 0, soft = 0, soft_header = 0, soft_block = 0, soft_chain = 0, soft_rs = 0, soft_rs_fmax = 0, soft_rs_chain = 0;
    std::deque<HeldFrame> pending; HeldFrame current;
    unsigned since_poll = 0;
    unsigned stream_floor = 0;          // streaming delivery (fxrx_sync_set_streaming / FXRX_SYNC_STREAMING): 0 off, else the fewest samples worth a block

    fxrx_sync_s() : BlockFeed(kSyncBlockDefault, kSyncDepthDefault) {}
    // what an option needs to be in force, as fxrx_create demands it: read by config() and by the setters that refuse without
    bool soft_on() const { return soft != 0; }
    bool soft_block_on() const { return soft && soft_block; }
    bool soft_rs_on() const { return soft && soft_rs; }
    fxrx_config config() const
    {
        fxrx_config cfg{}; cfg.device = 0; cfg.mode = FXRX_MODE_FLEX_RX; cfg.n_streams = 1; cfg.want_framesyms = 1;
        cfg.threshold = threshold; cfg.equalizer = equalizer; cfg.soft_decision = soft; cfg.soft_header = soft_header;
        cfg.soft_block = soft_block_on(); cfg.soft_chain = soft_block_on() && soft_chain; cfg.soft_rs = soft_rs_on();
        cfg.soft_rs_fmax = soft_rs_on() ? soft_rs_fmax : 0; cfg.soft_rs_chain = soft_rs_on() && soft_rs_chain;
        return cfg;
    }
    void materialise_all() { for (auto &h : pending) h.materialise(); current.materialise(); }
    void before_collect() { materialise_all(); }           // (rare: frames are normally delivered long before the next block is due)
    // queue the frames of the block just collected
    void take(int nr)
    {
        for (int i = 0; i < nr; i++) {
            fxrx_frame f; if (fxrx_result(ctx, (unsigned)i, &f) != 0) continue;
            pending.emplace_back();
            HeldFrame &h = pending.back();
            std::memcpy(h.header, f.header, 20); h.header_valid = f.header_valid; h.payload_valid = f.payload_valid;
            h.payload = f.payload_len ? f.payload : nullptr; h.payload_len = f.payload ? f.payload_len : 0;
            h.syms = f.num_framesyms ? f.framesyms : nullptr; h.nsyms = f.framesyms ? f.num_framesyms : 0;
            h.stats.evm = f.header_valid ? f.evm_db : 0.0f; h.stats.rssi = f.rssi_db; h.stats.cfo = f.cfo;
            h.stats.mod_scheme = f.mod_scheme; h.stats.mod_bps = f.mod_bps; h.stats.check = f.check; h.stats.fec0 = f.fec0; h.stats.fec1 = f.fec1;
        }
    }
    void deliver_one()
    {
        if (pending.empty()) return;
        current = std::move(pending.front()); pending.pop_front();
        if (current.owned) { current.payload = current.own_payload.empty() ? nullptr : current.own_payload.data(); current.syms = current.own_syms.empty() ? nullptr : current.own_syms.data(); }
        current.stats.framesyms = const_cast<fx_complex *>(current.syms);
        current.stats.num_framesyms = current.nsyms;
        if (cb)
            cb(current.header, current.header_valid, const_cast<unsigned char *>(current.payload), current.payload_len, current.payload_valid, current.stats, ud);
    }
};

extern "C" {

// /root/reference/lib/flex_rx_impl.cc:49
flexframesync flexframesync_create(framesync_callback callback, void *userdata)
{
    std::unique_ptr<fxrx_sync_s> q(new fxrx_sync_s); q->cb = callback; q->ud = userdata;
    if (const char *e = std::getenv("FXRX_SYNC_BLOCK")) q->block = (unsigned)std::max(256, std::atoi(e));
    if (const char *e = std::getenv("FXRX_SYNC_DEPTH")) q->depth = (unsigned)std::min(15, std::max(1, std::atoi(e)));
    if (!q->replace_ctx(q->config())) return nullptr;
    if (const char *e = std::getenv("FXRX_SYNC_STREAMING")) q->stream_floor = (unsigned)std::max(0, std::atoi(e));
    if (!q->set_ring(q->block)) return nullptr;
    return q.release();
}
// /root/reference/lib/flex_rx_impl.cc:71
void flexframesync_destroy(flexframesync q) { delete q; }
void flexframesync_reset(flexframesync q)
{
    if (!q || !q->ctx) return;
    q->drain(); q->pending.clear(); q->fill = 0;
    fxrx_reset(q->ctx);
}
// /root/reference/lib/flex_rx_impl.cc:213
void flexframesync_execute(flexframesync q, fx_complex *x, unsigned int n)
{
    if (!q || !q->ctx) return;
    if (q->bufs.empty()) { q->errors++; return; }           // (cannot happen: a ring is only ever swapped for a complete one)
    q->since_poll += n;
    while (n) {
        const size_t take = std::min<size_t>(n, (size_t)q->block - q->fill);
        stream_copy(q->bufs[q->cur] + q->fill, x, take);
        q->fill += take; x += take; n -= (unsigned)take;
        if (q->fill == q->block) q->submit_current();
    }
    if (q->since_poll >= (q->stream_floor ? std::min(kSyncPollEvery, q->stream_floor) : kSyncPollEvery)) {
        q->since_poll = 0;
        if (q->pending.empty() && fxrx_ready(q->ctx) == 1) q->collect_one();
    }
    // streaming delivery: the GPU is idle and enough has gathered -- run it now, as the next (shorter) block of the continuing stream.
    // While that block is under way the next one gathers, so block length follows the offered rate by itself.
    if (q->stream_floor && q->fill >= q->stream_floor && fxrx_inflight(q->ctx) == 0) q->submit_current();
    q->deliver_one();
}
void fxrx_sync_flush(flexframesync q) { if (q) q->flush(); }
void fxrx_sync_set_block(flexframesync q, unsigned int samples)
{
    if (!q || !q->ctx) return;
    const unsigned nb = samples < 256 ? 256u : samples;
    if (nb == q->block) return;
    q->flush();                              // what is queued runs at the old size (buffers move)
    q->materialise_all();
    (void)q->resize(nb, "fxrx_sync_set_block");
}
void fxrx_sync_set_streaming(flexframesync q, unsigned int floor_samples) { if (q) q->stream_floor = floor_samples; }
unsigned int fxrx_sync_pending(flexframesync q) { return q ? (unsigned)q->pending.size() : 0; }
unsigned int fxrx_sync_errors(flexframesync q) { return q ? q->errors : 0; }
fxrx_ctx *fxrx_sync_context(flexframesync q) { return q ? q->ctx : nullptr; }
// A setting lives in the context configuration: what is queued runs under the old value (pending frames are kept, as copies), the new
// value is tried on a new context and kept only if that context could be made (state is reset, as liquid's setters do not promise
// otherwise); else the old context and value stay and the error is reported
extern "C++" template <class T> static int sync_set_value(flexframesync q, T fxrx_sync_s::*field, T value, const char *what)
{
    if (!q) return -1;
    q->flush();
    q->materialise_all();
    const T old = q->*field;
    q->*field = value;
    if (q->replace_ctx(q->config())) return 0;
    q->*field = old; q->errors++;
    std::fprintf(stderr, "libfxrx: %s: %s (setting unchanged)\n", what, fxrx_last_error());
    return -1;
}
// an option.  `needs` (with its text): what must be on for a value other than 0 -- turning the option on without is refused, as
// fxrx_create would; `bad_value`: the text of a value fxrx_create would not take, or null
static int sync_set(flexframesync q, int fxrx_sync_s::*field, int value, const char *what, bool (fxrx_sync_s::*needs)() const = nullptr,
                    const char *needs_text = nullptr, const char *bad_value = nullptr)
{
    if (q && value && needs && !(q->*needs)()) { std::fprintf(stderr, "libfxrx: %s: needs %s (setting unchanged)\n", what, needs_text); return -1; }
    if (q && bad_value) { std::fprintf(stderr, "libfxrx: %s: %s (setting unchanged)\n", what, bad_value); return -1; }
    return sync_set_value(q, field, value, what);
}
// (a NaN is no threshold -- fxrx_create refuses it --: the value stays, nothing is flushed, re-created or counted)
void fxrx_sync_set_threshold(flexframesync q, float t) { if (t != t) return; (void)sync_set_value(q, &fxrx_sync_s::threshold, t, "fxrx_sync_set_threshold"); }
void fxrx_sync_set_equalizer(flexframesync q, int on) { (void)sync_set(q, &fxrx_sync_s::equalizer, on != 0, "fxrx_sync_set_equalizer"); }
void fxrx_sync_set_soft(flexframesync q, int on) { (void)sync_set(q, &fxrx_sync_s::soft, on != 0, "fxrx_sync_set_soft"); }
int fxrx_sync_set_soft_block(flexframesync q, int on) { return sync_set(q, &fxrx_sync_s::soft_block, on != 0, "fxrx_sync_set_soft_block"); }
int fxrx_sync_set_soft_chain(flexframesync q, int on) { return sync_set(q, &fxrx_sync_s::soft_chain, on != 0, "fxrx_sync_set_soft_chain", &fxrx_sync_s::soft_block_on, "soft payload decoding and soft_block"); }
int fxrx_sync_set_soft_rs(flexframesync q, int on) { return sync_set(q, &fxrx_sync_s::soft_rs, on != 0, "fxrx_sync_set_soft_rs", &fxrx_sync_s::soft_on, "soft payload decoding"); }
int fxrx_sync_set_soft_rs_fmax(flexframesync q, int fmax_plus_1)
{
    const bool takes = fmax_plus_1 == 0 || (fmax_plus_1 > 0 && fmax_plus_1 <= 33 && (fmax_plus_1 & 1));
    return sync_set(q, &fxrx_sync_s::soft_rs_fmax, fmax_plus_1, "fxrx_sync_set_soft_rs_fmax", &fxrx_sync_s::soft_rs_on, "soft payload decoding and soft_rs",
                    takes ? nullptr : "0, or an even bound 0 .. 32 plus one");
}
int fxrx_sync_set_soft_rs_chain(flexframesync q, int on) { return sync_set(q, &fxrx_sync_s::soft_rs_chain, on != 0, "fxrx_sync_set_soft_rs_chain", &fxrx_sync_s::soft_rs_on, "soft payload decoding and soft_rs"); }
// [RECALLED liquid 1.3.x] flexframesync_decode_header_soft / flexframesync_decode_payload_soft (include/liquid/liquid.h)
int flexframesync_decode_header_soft(flexframesync q, int soft) { return sync_set(q, &fxrx_sync_s::soft_header, soft != 0, "flexframesync_decode_header_soft"); }
int flexframesync_decode_payload_soft(flexframesync q, int soft) { return sync_set(q, &fxrx_sync_s::soft, soft != 0, "flexframesync_decode_payload_soft"); }

}  // extern "C"

// ------------------------------------------------------------------------------------------ msequence
struct fxrx_mseq_s { fx::MSeq ms; fxrx_mseq_s(unsigned m, unsigned g, unsigned a) : ms(m, g, a) {} };
extern "C" {
// /root/reference/lib/frame_detector_cc_impl.cc:47
msequence msequence_create(unsigned int m, unsigned int g, unsigned int a) { if (m < 2 || m > 15) return nullptr; return new fxrx_mseq_s(m, g, a); }
// /root/reference/lib/frame_detector_cc_impl.cc:49-50
unsigned int msequence_advance(msequence ms) { return ms ? ms->ms.advance() : 0; }
// /root/reference/lib/frame_detector_cc_impl.cc:52
void msequence_destroy(msequence ms) { delete ms; }
}

// ------------------------------------------------------------------------------------------ qdetector_cccf
// The reference hands over one sample per call (/root/reference/lib/frame_detector_cc_impl.cc:76-82).  The same feeder
// (fx_blockfeed.h) under a call that is one store into the buffer being filled plus a counter, on a detector context that returns the
// aligned windows (want_framesyms: fx_detwin_kernel).  What differs from fxrx_sync_s: a block in flight is collected when its slot is
// needed, when a poll finds it done, or -- so that delivery never depends on how fast the GPU happens to be -- once an eighth of a
// block length (plus depth - 1 block lengths) has been handed in since it was submitted (`submitted_at`): a detection leaves at most
// that long after its block filled, whatever the timing.  That bound is kept by a forced wait: the call that reaches the age limit
// blocks in fxrx_collect, on the caller's thread, until the GPU has finished the block (a block takes far less than an eighth of its
// length to fill only above some hundred Msamples/s).  Detections wait in `pending` with their windows (copies: the context's are
// valid until its next collect) and leave one per call.  There is no host-side history of the samples.
struct fxrx_qdet_s : BlockFeed<fxrx_qdet_s> {
    static constexpr const char *entry = "qdetector_cccf_execute";
    struct Det { float tau, gamma, dphi, phi; fx_complex win[FX_NFFT]; };
    float threshold = 0.5f;
    std::deque<uint64_t> submitted_at;  // per block in flight: `count` when it was submitted
    uint64_t count = 0;                 // samples handed in so far
    std::deque<Det> pending;
    fx_complex window[FX_NFFT];         // what the last non-NULL call returned (valid until the next call)
    float tau = 0, gamma = 0, dphi = 0, phi = 0;
    unsigned since_poll = 0;

    fxrx_qdet_s() : BlockFeed(kQdetBlockDefault, kQdetDepthDefault) {}
    bool make_ctx()                     // the detector starts over; a failed re-creation keeps the old context and what it holds
    {
        fxrx_config cfg{}; cfg.device = 0; cfg.mode = FXRX_MODE_DETECTOR; cfg.n_streams = 1; cfg.threshold = threshold; cfg.want_framesyms = 1;
        if (!replace_ctx(cfg)) { errors++; std::fprintf(stderr, "libfxrx: qdetector_cccf: %s\n", fxrx_last_error()); return false; }
        submitted_at.clear(); pending.clear(); fill = 0;
        return true;
    }
    void submitted() { submitted_at.push_back(count); }
    void dropped() { submitted_at.clear(); }
    // queue the detections of the block just collected
    void take(int nr)
    {
        if (!submitted_at.empty()) submitted_at.pop_front();
        for (int i = 0; i < nr; i++) {
            fxrx_frame f;
            // (a detection without its window cannot be handed out: it is dropped, counted and reported, never passed over in silence)
            if (fxrx_result(ctx, (unsigned)i, &f) != 0 || !f.framesyms || f.num_framesyms != FX_NFFT) { report("a detection's window", FXRX_ERR_STATE); continue; }
            pending.emplace_back();
            Det &d = pending.back();
            d.tau = f.tau; d.gamma = f.gamma; d.dphi = f.dphi; d.phi = f.phi;
            std::memcpy(d.win, f.framesyms, sizeof d.win);
        }
    }
    void poll()
    {
        const uint64_t age_limit = (uint64_t)(depth - 1) * block + block / 8;
        while (!submitted_at.empty() && (count - submitted_at.front() >= age_limit || fxrx_ready(ctx) == 1)) collect_one();
    }
};
extern "C" {
// /root/reference/lib/frame_detector_cc_impl.cc:54
qdetector_cccf qdetector_cccf_create_linear(fx_complex *seq, unsigned int len, int ftype, unsigned int k, unsigned int m, float beta)
{
    const fx::HostTables &T = fx::host_tables();
    if (!seq || len != FX_PN_LEN || ftype != LIQUID_FIRFILT_ARKAISER || k != FX_K || m != FX_M || std::fabs(beta - FX_BETA) > 1e-6f) return nullptr;
    for (unsigned i = 0; i < len; i++)
        if (std::fabs(seq[i].re - T.pn[i].re) > 1e-6f || std::fabs(seq[i].im - T.pn[i].im) > 1e-6f) return nullptr;
    std::unique_ptr<fxrx_qdet_s> q(new fxrx_qdet_s);
    if (const char *e = std::getenv("FXRX_QDET_BLOCK")) q->block = (unsigned)std::max(FX_NFFT, std::atoi(e));
    if (const char *e = std::getenv("FXRX_QDET_DEPTH")) q->depth = (unsigned)std::min(15, std::max(1, std::atoi(e)));
    if (!q->make_ctx() || !q->set_ring(q->block)) return nullptr;
    return q.release();
}
// /root/reference/lib/frame_detector_cc_impl.cc:63
void qdetector_cccf_destroy(qdetector_cccf q) { delete q; }
// /root/reference/lib/frame_detector_cc_impl.cc:55.  The detector starts over (what is queued or in flight is dropped), as before.
void qdetector_cccf_set_threshold(qdetector_cccf q, float t)
{
    if (!q || t != t) return;                // (a NaN is no threshold: the value stays, nothing is dropped or counted)
    const float old = q->threshold;
    q->threshold = t;
    if (!q->make_ctx()) q->threshold = old;
}
unsigned int fxrx_qdet_errors(qdetector_cccf q) { return q ? q->errors : 0; }
unsigned int fxrx_qdet_pending(qdetector_cccf q) { return q ? (unsigned)q->pending.size() : 0; }
fxrx_ctx *fxrx_qdet_context(qdetector_cccf q) { return q ? q->ctx : nullptr; }
void fxrx_qdet_flush(qdetector_cccf q) { if (q) q->flush(); }
void fxrx_qdet_set_block(qdetector_cccf q, unsigned int samples)
{
    if (!q || !q->ctx) return;
    const unsigned nb = samples < FX_NFFT ? (unsigned)FX_NFFT : samples;
    if (nb == q->block) return;
    q->flush();                              // what is queued runs at the old size (buffers move); pending detections are copies already
    (void)q->resize(nb, "fxrx_qdet_set_block");
}
// /root/reference/lib/frame_detector_cc_impl.cc:77
void *qdetector_cccf_execute(qdetector_cccf q, fx_complex x)
{
    if (!q || !q->ctx) return nullptr;
    q->bufs[q->cur][q->fill++] = x; q->count++;
    if (q->fill == q->block) q->submit_current();
    if (++q->since_poll >= kQdetPollEvery) { q->since_poll = 0; q->poll(); }
    if (q->pending.empty()) return nullptr;
    const fxrx_qdet_s::Det &d = q->pending.front();
    q->tau = d.tau; q->gamma = d.gamma; q->dphi = d.dphi; q->phi = d.phi;      // (estimates first, then the pointer: the order callers rely on)
    std::memcpy(q->window, d.win, sizeof q->window);
    q->pending.pop_front();
    return q->window;
}
// /root/reference/lib/frame_detector_cc_impl.cc:90-93 (commented-out getters)
float qdetector_cccf_get_tau(qdetector_cccf q) { return q ? q->tau : 0; }
float qdetector_cccf_get_gamma(qdetector_cccf q) { return q ? q->gamma : 0; }
float qdetector_cccf_get_dphi(qdetector_cccf q) { return q ? q->dphi : 0; }
float qdetector_cccf_get_phi(qdetector_cccf q) { return q ? q->phi : 0; }
unsigned int qdetector_cccf_get_buf_len(qdetector_cccf) { return FX_NFFT; }
}

// ------------------------------------------------------------------------------------------ flexframegen
struct fxrx_gen_s { fx::FrameGen g; bool assembled = false; };
extern "C" {
// /root/reference/lib/flex_tx_impl.cc:51
int flexframegenprops_init_default(flexframegenprops_s *p)
{
    if (!p) return -1;
    p->check = FX_CRC_32; p->fec0 = FX_FEC_NONE; p->fec1 = FX_FEC_NONE; p->mod_scheme = FX_MODEM_QPSK;
    return 0;
}
static int apply_props(fxrx_gen_s *q, const flexframegenprops_s *p)
{
    if (!fx::modem_bps(p->mod_scheme) || !fx::fec_supported(p->fec0) || !fx::fec_supported(p->fec1) ||
        p->check == FX_CRC_UNKNOWN || p->check > FX_CRC_32) return -1;
    q->g.check = p->check; q->g.fec0 = p->fec0; q->g.fec1 = p->fec1; q->g.ms = p->mod_scheme;
    return 0;
}
// /root/reference/lib/flex_tx_impl.cc:56
flexframegen flexframegen_create(flexframegenprops_s *props)
{
    fxrx_gen_s *q = new fxrx_gen_s;
    flexframegenprops_s d; flexframegenprops_init_default(&d);
    if (apply_props(q, props ? props : &d) != 0) { delete q; return nullptr; }
    return q;
}
// /root/reference/lib/flex_tx_impl.cc:72
void flexframegen_destroy(flexframegen q) { delete q; }
// /root/reference/lib/flex_tx_impl.cc:188
int flexframegen_setprops(flexframegen q, flexframegenprops_s *props) { if (!q || !props) return -1; return apply_props(q, props); }
// /root/reference/lib/flex_tx_impl.cc:198
int flexframegen_assemble(flexframegen q, const unsigned char *header, const unsigned char *payload, unsigned int n)
{
    if (!q || (!payload && n) || n > 65535) return -1;
    static const unsigned char z = 0;
    q->g.assemble(header, payload ? payload : &z, n); q->assembled = true;
    return 0;
}
// /root/reference/lib/flex_tx_impl.cc:199
unsigned int flexframegen_getframelen(flexframegen q) { return (q && q->assembled) ? FX_K * (unsigned)q->g.syms.size() : 0; }
// /root/reference/lib/flex_tx_impl.cc:201.  Returns 1 when the frame is complete (liquid's convention).
int flexframegen_write_samples(flexframegen q, fx_complex *buf, unsigned int len)
{
    if (!q || !q->assembled || !buf) return -1;
    unsigned need = FX_K * (unsigned)q->g.syms.size();
    if (len < need) return -1;
    q->g.write(reinterpret_cast<fx::cf *>(buf));
    for (unsigned i = need; i < len; i++) buf[i] = fx_complex{ 0, 0 };
    return 1;
}
void fxrx_gen_set_delay(flexframegen q, float dt) { if (q) q->g.dt = dt; }
}
