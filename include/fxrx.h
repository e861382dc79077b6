/*
 * fxrx.h -- C ABI of libfxrx.so, the MI355X-native flexframe receive path.
 *
 * Two layers:
 *
 *  (1) DROP-IN NAMES.  The exact liquid-dsp entry points that gr::liquiddsp's blocks call, with
 *      ABI-compatible signatures, so that gnuradio-liquiddsp can be linked against libfxrx.so for
 *      this path.  Each declaration cites the reference line it serves.
 *
 *  (2) BATCHED API (fxrx_*).  Many independent IQ streams per call, device or host pointers,
 *      results returned as plain records.  This is the throughput path (BASELINE configs 2-5);
 *      the reference has no counterpart (one flexframesync handle per block instance,
 *      /root/reference/lib/flex_rx_impl.cc:49).
 *
 * No torch / C++ types cross this boundary.  Nothing here throws; failures are status codes
 * (or NULL handles) and fxrx_last_error().  The library needs a HIP device: every constructor
 * fails loudly (NULL + error text) when none is usable -- there is no CPU fallback.
 */
#ifndef FXRX_H
#define FXRX_H
#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* liquid's `float complex` is two packed floats; gr_complex (std::complex<float>) likewise.  A caller that wants its own
 * spelling of that type in these prototypes defines FXRX_COMPLEX_TYPE before including this header (include/liquid/liquid.h
 * does: std::complex<float> in C++, float _Complex in C); layout and calling convention are the same. */
#ifdef FXRX_COMPLEX_TYPE
typedef FXRX_COMPLEX_TYPE fx_complex;
#else
typedef struct { float re, im; } fx_complex;
#endif

/* ------------------------------------------------------------------------------------------
 * (1) drop-in names
 * ------------------------------------------------------------------------------------------ */

/* framesyncstats_s -- read at /root/reference/lib/flex_rx_impl.cc:195,198,218,232-234 */
typedef struct {
    float        evm;            /* error vector magnitude [dB] */
    float        rssi;           /* received signal strength [dB] */
    float        cfo;            /* carrier offset estimate [rad/sample] */
    fx_complex  *framesyms;      /* payload symbols after carrier recovery */
    unsigned int num_framesyms;
    unsigned int mod_scheme;     /* LIQUID_MODEM_* value */
    unsigned int mod_bps;
    unsigned int check;          /* LIQUID_CRC_*   */
    unsigned int fec0;           /* LIQUID_FEC_* (first / "inner" in the reference's naming) */
    unsigned int fec1;           /* LIQUID_FEC_* (second / "outer") */
} framesyncstats_s;

/* callback type -- /root/reference/lib/flex_rx_impl.h:48-55 */
typedef int (*framesync_callback)(unsigned char *header, int header_valid, unsigned char *payload,
                                  unsigned int payload_len, int payload_valid, framesyncstats_s stats,
                                  void *userdata);

typedef struct fxrx_sync_s *flexframesync;

/* /root/reference/lib/flex_rx_impl.cc:49 */
flexframesync flexframesync_create(framesync_callback callback, void *userdata);
/* /root/reference/lib/flex_rx_impl.cc:71 */
void flexframesync_destroy(flexframesync q);
/* /root/reference/lib/flex_rx_impl.cc:213.  Samples are queued and run through the GPU in blocks
 * (fxrx_sync_set_block); at most ONE completed frame is handed to the callback per call, which is
 * what the reference's work() loop can consume (it tests a single flag after each call, :216).
 * Buffers passed to the callback stay valid until the next call on the same handle. */
void flexframesync_execute(flexframesync q, fx_complex *x, unsigned int n);
void flexframesync_reset(flexframesync q);
/* extensions (additive).  Samples are collected in page-locked buffers of `block` samples (default 2^20; FXRX_SYNC_BLOCK) and
 * run through the GPU as consecutive blocks of one continuing stream, up to FXRX_SYNC_DEPTH (default 3) of them in flight while
 * the next buffer fills: flexframesync_execute never waits for the GPU unless all of those are still busy.  Frames therefore
 * reach the callback in order, one per call, between one and `depth` + 1 blocks after their last sample was handed in.
 * fxrx_sync_flush: run whatever is queued now and wait for everything in flight (frames are then pending: n = 0 calls
 * deliver them).  fxrx_sync_set_block: flushes, then changes the block length. */
void fxrx_sync_flush(flexframesync q);
void fxrx_sync_set_block(flexframesync q, unsigned int samples);     /* (if the new buffers cannot be had, the old length stays and fxrx_sync_errors goes up) */
/* Streaming delivery (opt-in; off by default).  floor_samples > 0: whenever a call ends with nothing in flight on the GPU and at least
 * floor_samples queued, the partly filled buffer is run at once as the next, shorter, block of the continuing stream, and finished blocks
 * are looked for at least every floor_samples samples.  Frames then reach the callback without fxrx_sync_flush and without waiting for a
 * block to fill; block length follows the offered rate by itself (while one block runs the next gathers).  Still at most one frame per
 * call, buffers valid until the next call on the handle.  0: off.  A sensible floor is 8192.  Environment: FXRX_SYNC_STREAMING=<floor>,
 * read by flexframesync_create -- how an unmodified caller turns it on. */
void fxrx_sync_set_streaming(flexframesync q, unsigned int floor_samples);
void fxrx_sync_set_threshold(flexframesync q, float threshold);   /* values as fxrx_config.threshold; NaN: ignored */
void fxrx_sync_set_equalizer(flexframesync q, int on);   /* re-creates the context like fxrx_sync_set_threshold */
void fxrx_sync_set_soft(flexframesync q, int on);        /* likewise: soft-decision payload decoding */
/* soft-input block decoders (fxrx_config.soft_block), in force while soft payload decoding is on.  Re-creates the context; returns 0,
 * or -1 if that failed, in which case the previous setting stays */
int  fxrx_sync_set_soft_block(flexframesync q, int on);
/* soft values carried from a block fec1 into a convolutional fec0 (fxrx_config.soft_chain), in force while soft payload decoding and
 * soft_block are on.  Re-creates the context; returns 0, or -1 if that failed or if, with on != 0, soft payload decoding or soft_block
 * is off, in which case the previous setting stays */
int  fxrx_sync_set_soft_chain(flexframesync q, int on);
/* soft-decision Reed-Solomon decoding (fxrx_config.soft_rs), in force while soft payload decoding is on.  Re-creates the context; returns
 * 0, or -1 if that failed or if, with on != 0, soft payload decoding is off, in which case the previous setting stays */
int  fxrx_sync_set_soft_rs(flexframesync q, int on);
/* the bound on f of soft-decision Reed-Solomon decoding (fxrx_config.soft_rs_fmax, the same value: 0 for no bound, else the even bound
 * 0 .. 32 plus one) and its soft hand-over to a convolutional fec0 (fxrx_config.soft_rs_chain), in force while soft payload decoding and
 * soft_rs are on.  Each re-creates the context; returns 0, or -1 if that failed, if the value is none fxrx_create takes or if, with a
 * value other than 0, soft payload decoding or soft_rs is off, in which case the previous setting stays */
int  fxrx_sync_set_soft_rs_fmax(flexframesync q, int fmax_plus_1);
int  fxrx_sync_set_soft_rs_chain(flexframesync q, int on);
unsigned int fxrx_sync_pending(flexframesync q);     /* completed frames not yet delivered */
/* the liquid signatures return void: when a block fails on the GPU its samples (and those of the blocks in flight with it) are
 * dropped -- never fed twice --, the synchroniser restarts freshly reset behind the gap, the text stays in fxrx_last_error(),
 * one line goes to stderr and this counter goes up */
unsigned int fxrx_sync_errors(flexframesync q);
struct fxrx_ctx_s;
struct fxrx_ctx_s *fxrx_sync_context(flexframesync q);   /* the batched context underneath (tests, statistics) */

/* m-sequence -- /root/reference/lib/frame_detector_cc_impl.cc:47,49,50,52 */
typedef struct fxrx_mseq_s *msequence;
msequence    msequence_create(unsigned int m, unsigned int g, unsigned int a);
unsigned int msequence_advance(msequence ms);
void         msequence_destroy(msequence ms);

/* detector -- /root/reference/lib/frame_detector_cc_impl.cc:54,55,63,77,90-93 */
#define LIQUID_FIRFILT_ARKAISER 7
typedef struct fxrx_qdet_s *qdetector_cccf;
/* Only the flexframe preamble configuration the reference uses is accepted:
 * 64 symbols, ARKAISER, k=2, m=7, beta=0.3; anything else returns NULL. */
qdetector_cccf qdetector_cccf_create_linear(fx_complex *sequence, unsigned int sequence_len, int ftype,
                                            unsigned int k, unsigned int m, float beta);
void   qdetector_cccf_destroy(qdetector_cccf q);
void   qdetector_cccf_set_threshold(qdetector_cccf q, float threshold);   /* values as fxrx_config.threshold; NaN: ignored */
/* Per-sample entry kept for link compatibility.  A call stores the sample in a page-locked buffer; a full buffer (65 536 samples;
 * FXRX_QDET_BLOCK / fxrx_qdet_set_block, at least 512) is searched on the GPU as the next block of one continuing stream while the
 * next buffer fills, FXRX_QDET_DEPTH (default 1) blocks in flight.  Every detection is reported exactly once, one per call, later
 * than liquid would: at the latest an eighth of a block length (plus depth - 1 block lengths, and up to 1024 calls) after its block filled, earlier when a
 * poll finds the block done.  That bound holds whatever the GPU's timing because it is enforced by a wait: the call that reaches it
 * blocks in fxrx_collect, on the caller's thread, until the block is done.  tau, gamma, dphi, phi are set before the pointer is returned; the pointer is the handle's own buffer
 * of the 512 aligned samples (cut on the GPU, fxrx_config.want_framesyms), valid until the next call.  Block users should use the
 * batched API in detector mode instead. */
void  *qdetector_cccf_execute(qdetector_cccf q, fx_complex x);
float  qdetector_cccf_get_tau(qdetector_cccf q);
float  qdetector_cccf_get_gamma(qdetector_cccf q);
float  qdetector_cccf_get_dphi(qdetector_cccf q);
float  qdetector_cccf_get_phi(qdetector_cccf q);
unsigned int qdetector_cccf_get_buf_len(qdetector_cccf q);
unsigned int fxrx_qdet_errors(qdetector_cccf q);     /* as fxrx_sync_errors: a failed block's samples are dropped, never fed twice; the detector restarts freshly reset behind the gap */
/* extensions (additive).  fxrx_qdet_flush: submit what is queued, wait for everything in flight; detections are then pending (further
 * calls deliver them, one each).  fxrx_qdet_set_block: flushes, then changes the block length (unchanged, and an error counted, if the
 * buffers cannot be had).  fxrx_qdet_context: the batched detector context underneath (tests, statistics). */
void         fxrx_qdet_flush(qdetector_cccf q);
unsigned int fxrx_qdet_pending(qdetector_cccf q);
void         fxrx_qdet_set_block(qdetector_cccf q, unsigned int samples);
struct fxrx_ctx_s *fxrx_qdet_context(qdetector_cccf q);

/* frame generator (test / loopback source) -- /root/reference/lib/flex_tx_impl.cc:51,56,72,188,198-201 */
typedef struct { unsigned int check, fec0, fec1, mod_scheme; } flexframegenprops_s;
typedef struct fxrx_gen_s *flexframegen;
int          flexframegenprops_init_default(flexframegenprops_s *props);
flexframegen flexframegen_create(flexframegenprops_s *props);
void         flexframegen_destroy(flexframegen q);
int          flexframegen_setprops(flexframegen q, flexframegenprops_s *props);
int          flexframegen_assemble(flexframegen q, const unsigned char *header, const unsigned char *payload,
                                   unsigned int payload_len);
unsigned int flexframegen_getframelen(flexframegen q);
int          flexframegen_write_samples(flexframegen q, fx_complex *buffer, unsigned int buffer_len);
/* extension: design the pulse with a fractional-sample offset dt (channel emulation in tests/bench).  liquid's firdes
 * convention, tap i at t = i - (n-1)/2 + dt: dt is an ADVANCE -- the frame arrives dt samples early, the receiver's
 * start + tau comes out dt lower (tau ~ -dt; tests/test_ref_detect.py pins the sign). */
void         fxrx_gen_set_delay(flexframegen q, float dt);

/* ------------------------------------------------------------------------------------------
 * (2) batched API
 * ------------------------------------------------------------------------------------------ */
enum { FXRX_MODE_FLEX_RX = 0, FXRX_MODE_DETECTOR = 1 };
enum { FXRX_OK = 0, FXRX_ERR_ARG = -1, FXRX_ERR_HIP = -2, FXRX_ERR_NODEVICE = -3, FXRX_ERR_STATE = -4 };

typedef struct {
    int          device;         /* HIP device ordinal */
    int          mode;           /* FXRX_MODE_* */
    unsigned int n_streams;
    float        threshold;      /* <= 0 -> default (0.5 flex_rx like liquid's flexframesync, 0.45 detector like
                                    /root/reference/lib/frame_detector_cc_impl.cc:55).  Any other finite value, and +Inf, is taken as
                                    given: a hop detects when rxy > threshold.  rxy is the peak over the root of the window's energy
                                    taken as spread evenly over its 512 samples: near 1 at most in steady traffic, up to sqrt(512 / 156)
                                    = 1.81 for a preamble alone in a silent window (1.4 in a fresh detector's first, half-empty
                                    window), never more.  A threshold above that (2, +Inf) yields no results and no error; 1.5 is
                                    still reached by a strong frame behind much weaker traffic.  NaN: fxrx_create fails with
                                    FXRX_ERR_ARG (every comparison with it is false: it would silently detect nothing);
                                    fxrx_sync_set_threshold and qdetector_cccf_set_threshold then keep the previous value, re-create
                                    nothing and count no error */
    unsigned int segment_len;    /* speculation granularity in samples (0 -> auto) */
    int          want_framesyms; /* copy payload symbols back to the host with each result.  Detector mode: every detection carries its 512 aligned
                                    samples instead (fxrx_frame.framesyms, num_framesyms = 512): x[start, start + 512) of its stream, bit for bit,
                                    (0, 0) below the stream's zero-floor (index < 0 since create / fxrx_reset) -- what liquid's
                                    qdetector_cccf_execute returns.  Valid, like payloads, until the next fxrx_collect / fxrx_process */
    int          equalizer;      /* 1: optional equaliser stage on (liquid: FLEXFRAMESYNC_ENABLE_EQ, compiled out of a stock libliquid):
                                    13-tap eqlms at 2 samples/symbol behind the matched filter, trained on the 64 p/n symbols, frozen
                                    afterwards; symbol instants move 3 symbols later.  0 (default): what flexframesync executes */
    int          soft_decision;  /* 1: decode the payload from per-bit soft values (liquid: flexframesync_decode_payload_soft, which the
                                    reference never calls): soft-input Viterbi for the convolutional stage(s) nearest the channel.
                                    With want_framesyms the soft values themselves come back too (fxrx_frame.soft_bits).  0: hard */
    int          soft_header;    /* 1: decode the 20-byte frame header from per-bit soft values (liquid: flexframesync_decode_header_soft, which
                                    the reference never calls): the header's QPSK symbols, after pilot phase / frequency / gain correction,
                                    give two soft values each under the payload demapper's rule above, and the Hamming(8,4) stage next to the
                                    channel picks the maximum-likelihood codeword of every 8 soft values; SECDED(72,64) and CRC-32 follow as
                                    before.  The soft rule is this project's, not pinned to liquid's demapper.  Flex_rx mode only
                                    (fxrx_create fails with FXRX_ERR_ARG in detector mode).  0 (default): hard decisions */
    int          soft_block;     /* 1: a block code (Hamming, Golay, SECDED; not Reed-Solomon) in a stage that decodes from soft values -- fec1,
                                    or fec0 when fec1 is none -- decodes from them too, instead of from their hard decisions: Hamming(7,4) /
                                    (8,4) / (12,8) by exhaustive maximum likelihood (least cost sum_b (c_b ? 255 - s_b : s_b), ties to the
                                    smallest message), Golay(24,12) and SECDED by Chase-4 over the hard decoder (the four least reliable
                                    positions flipped in all 16 patterns, the cheapest re-encoded success, ties to the smallest pattern).
                                    These rules are this project's, not pinned to liquid's fec_decode_soft.  Needs soft_decision = 1 and
                                    flex_rx mode (fxrx_create fails with FXRX_ERR_ARG otherwise).  0 (default): hard decisions there */
    int          soft_chain;     /* 1: when fec1 is one of soft_block's codes and fec0 is convolutional, fec1's decoder emits one soft value per
                                    message bit (8 l0 of them, in the order of its output bytes, MSB first) instead of hard bytes; they pass
                                    the soft de-interleaver and fec0 decodes with the soft-input Viterbi.  Every other pair (fec1 none,
                                    convolutional or Reed-Solomon; a block fec0 behind a block fec1) decodes as under soft_block.
                                    The soft-output rule, integers only, is this project's, not liquid's.  With s_b the soft value of
                                    codeword position b (0 = surely 0, 255 = surely 1), C(c) = sum_b (c_b ? 255 - s_b : s_b) the cost of
                                    codeword c, d the message soft_block's decoder returns (same ties) and L_i >= 0 the margin of message
                                    bit i, the output is
                                        o_i = min(255, max(128, (255 + L_i + 1) >> 1))   if d_i = 1,
                                        o_i = max(0, min(127, (255 - L_i) >> 1))         if d_i = 0,
                                    so o_i > 127 exactly when d_i = 1, in the unit of the input (a channel value s has margin |2 s - 255|).
                                    Hamming(7,4) / (8,4) / (12,8): L_i = min{C(c) : m_i != d_i} - C(d) over all codewords (max-log-MAP).
                                    Golay, SECDED (Chase-4): the same minimum over the candidates, the successful re-encodings of the 16
                                    patterns; no candidate with m_i != d_i: L_i = 255 (the output saturates at 0 / 255); no candidate at
                                    all (the output is the hard decoder's on the hard word): o_i = d_i ? 192 : 64.  Positions a short last
                                    block does not transmit and padding bits past 8 l0 are not emitted.
                                    Needs soft_block = 1 (hence soft_decision = 1 and flex_rx mode; fxrx_create fails with FXRX_ERR_ARG
                                    otherwise).  0 (default): fec1 hands fec0 hard bytes */
    int          soft_rs;        /* 1: a Reed-Solomon code RS(255,223) in a stage that decodes from soft values -- fec1, or fec0 when fec1 is
                                    none -- decodes from them too, by generalized-minimum-distance decoding.  Per block of N = dl + 32
                                    bytes, with s the soft values in codeword order (MSB first): hard byte h_j (bit set iff s > 127), bit
                                    margin m = |2 s - 255|, byte reliability rho_j = the least margin of its bits; E_f = the first f
                                    positions ascending by (rho_j, j).  For f = 0, 2, ..., 32 the candidate c_f is the codeword of the
                                    shortened code that differs from h in at most (32 - f) / 2 positions outside E_f (unique if it exists;
                                    a locator root outside the N transmitted positions: none; f = 0 is the hard decoder).  The candidate
                                    with the least D(c) = sum of m over the bits where c and h differ wins, ties to the smallest f; its
                                    data bytes are the stage's output, hard bytes (nothing soft is handed on to a stage behind it).  The
                                    rule is this project's, integers only, not pinned to liquid.  It never gives up: c_32 always exists, so
                                    a block far beyond the code's reach is replaced by a far codeword where the hard decoder hands it on
                                    as received -- measured as a loss for Reed-Solomon in front of a convolutional fec0 at low SNR, a
                                    gain for Reed-Solomon alone.  Independent of soft_block / soft_chain;
                                    frames without a Reed-Solomon stage decode as with soft_rs = 0.  Needs soft_decision = 1 and flex_rx
                                    mode (fxrx_create fails with FXRX_ERR_ARG otherwise).  0 (default): the bounded-distance decoder on the
                                    hard decisions, radius 16 bytes */
    int          soft_rs_fmax;   /* a bound on f for soft_rs.  Encoding: 0 (default): no bound, fmax = 32, soft_rs's rule as above; otherwise
                                    fmax + 1 for an even fmax 0 .. 32 (1: f = 0 only; 17: fmax = 16; 33: the same as 0).  The rule is
                                    soft_rs's with the trials f = 0, 2, ..., fmax only: the winner is the least D among their candidates,
                                    ties to the smallest f.  With fmax < 32 a block may have no candidate; it is then passed on as
                                    received (the hard bytes h).  fmax = 0 is the bounded-distance hard decoder, radius 16.  Choosing
                                    fmax: trial f accepts any word within e = (32 - f) / 2 errors outside f erasures, so a word far from
                                    every codeword is accepted by it with probability about q(N, f) = C(N - f, e) 255^e / 256^(2 e), the
                                    share of the punctured code's space that its radius-e balls cover (N = 99: q(32) = 1, q(30) = 0.26,
                                    q(24) = 2.7e-4, q(16) = 2e-9; table in DESIGN.md section 8): pick fmax from the miscorrection rate
                                    you accept.  Needs soft_rs = 1; any other value: fxrx_create fails with FXRX_ERR_ARG */
    int          soft_rs_chain;  /* 1: when fec1 is RS(255,223) and fec0 is convolutional, the Reed-Solomon stage emits one soft value per
                                    data bit instead of hard bytes.  Per block, with len the data bytes the block really carries (the
                                    padded last block: fewer than dl), 8 len values, MSB first, in byte order: a block with a winning
                                    candidate c (a codeword as received is its own f = 0 candidate) emits o = c_bit ? 255 : 0 for its data
                                    bits; a block with no candidate (soft_rs_fmax) emits o = s, the channel's soft values of its data
                                    positions, unchanged; parity and pad positions are not emitted.  The 8 l0 values pass the soft
                                    de-interleaver and fec0 decodes with the soft-input Viterbi, as behind FEC_NONE or under soft_chain.
                                    With every block accepted the result is that of the hard hand-over.  Every other pair (Reed-Solomon
                                    as fec0 behind fec1 none, Reed-Solomon with fec0 none or a block code, no Reed-Solomon) decodes as
                                    with soft_rs_chain = 0.  The rule is this project's.  Needs soft_rs = 1 (fxrx_create fails with
                                    FXRX_ERR_ARG otherwise).  0 (default): hard bytes are handed on */
} fxrx_config;

typedef struct {
    unsigned int stream;
    int64_t      start;          /* absolute sample index (since create/reset) of aligned sample 0 */
    int          cfo_bin;        /* coarse CFO bin of the detector sweep */
    float        rxy, tau, gamma, dphi, phi;
    unsigned int pfb_index;
    float        pilot_dphi, pilot_phi, pilot_gain;
    int          header_valid, payload_valid;
    unsigned char header[20];    /* 14 user bytes + 6 protocol bytes */
    const unsigned char *payload; unsigned int payload_len;
    const fx_complex *framesyms; unsigned int num_framesyms;   /* host pointer or NULL (detector mode: the aligned window, see want_framesyms) */
    float        evm_db, rssi_db, cfo, evm_sum;
    unsigned int mod_scheme, mod_bps, check, fec0, fec1;
    const unsigned char *soft_bits; unsigned int num_soft_bits;   /* soft_decision + want_framesyms: one byte per coded bit in channel
                                                                     order, 0 = surely 0 ... 255 = surely 1; else NULL */
} fxrx_frame;

typedef struct fxrx_ctx_s fxrx_ctx;

const char *fxrx_last_error(void);
const char *fxrx_version(void);
int         fxrx_device_count(void);
/* page-locked host memory for input buffers: uploads from it run asynchronously (NULL + fxrx_last_error() on failure) */
void       *fxrx_pinned_alloc(size_t bytes);
void        fxrx_pinned_free(void *p);

fxrx_ctx *fxrx_create(const fxrx_config *cfg);
void      fxrx_destroy(fxrx_ctx *c);
void      fxrx_reset(fxrx_ctx *c);

/* Feed n_samples[s] new samples of every stream s.  iq[s] points at interleaved float32 (re,im);
 * on_device != 0 means the pointers are HIP device pointers on cfg.device (zero copy when the
 * stream has no carried-over tail).  Returns the number of results (frames, or detections in
 * detector mode) now readable through fxrx_result(), or a negative FXRX_ERR_*.  Results and
 * the buffers they point to stay valid until the next call on this context. */
int fxrx_process(fxrx_ctx *c, const void *const *iq, const uint64_t *n_samples, int on_device);
int fxrx_result(const fxrx_ctx *c, unsigned int i, fxrx_frame *out);

/* Pipelined form of fxrx_process (= submit + collect).  fxrx_submit enqueues the block's whole kernel chain on the block's
 * own HIP stream -- walkers, seek verification, chain (stitch / repair / resume state), plan, payload MF, PLL, packet decode,
 * results into pinned host memory -- and returns without waiting for any of it; what a stream carries from block to block
 * (resume state, unconsumed tail) stays on the device, so a block that continues the streams of the previous one simply
 * orders its first walkers behind that block's chain kernel.  fxrx_collect waits for the OLDEST submitted block and exposes
 * its results through fxrx_result / fxrx_last_timing.  With depth d (fxrx_set_depth, 1..32, default 1; 0 or more: FXRX_ERR_ARG; with blocks in flight: FXRX_ERR_STATE, the depth stays either way) up to d blocks may
 * be in flight; one more fxrx_submit fails with FXRX_ERR_STATE ("pipeline full") and changes nothing.  After fxrx_reset the next
 * block starts from a freshly reset synchroniser (positions count from 0 again, no carried tail, nothing in front of its first sample);
 * blocks in flight at that moment deliver what they would have delivered without it.  Blocks of one stream must be
 * submitted in order; input buffers, host or device, must stay valid until their block has been collected; results stay
 * valid until the next fxrx_collect / fxrx_process on the context (a submit in between does not touch them).  Returns 0
 * (submit) / result count (collect) or FXRX_ERR_*. */
int fxrx_set_depth(fxrx_ctx *c, unsigned int depth);
/* Any binary32 value is valid input: NaN, +-Inf and overflowing samples never make a call fail, never change another stream of
 * the batch, and change only the frames whose windows and filter spans read them ("Bad samples"). */
int fxrx_submit(fxrx_ctx *c, const void *const *iq, const uint64_t *n_samples, int on_device);
int fxrx_collect(fxrx_ctx *c);
/* Failure semantics.  A failing fxrx_submit (bad arguments, a batch too large for the arenas, an allocation that fails) leaves
 * the context exactly as it was: the same block, or another, can be submitted next and continues the streams from where they
 * stood.  Every argument check and reservation of a block, whatever its format, is done before anything is enqueued: nothing reads
 * the input buffers of a submit that failed, and they may be reused or freed at once.  A failing fxrx_collect drops every block in flight (their samples are never searched) and restarts all streams
 * from a freshly reset synchroniser with the next block submitted; sample positions keep counting.  Either way the context
 * stays usable -- unless the HIP runtime itself reports errors, which every later call will report again. */
/* Integer IQ (SDR-native samples).  A block may be handed over as interleaved 16-bit (sc16) or 8-bit (sc8) signed integer
 * (re, im) pairs instead of float32; the conversion happens on the device, inside the block's upload: host memory crosses the
 * bus raw, at 4 / 2 bytes a sample (asynchronously when it is page-locked), into a staging buffer of the block and is converted
 * behind the copy; a device buffer is read in place; a small page-locked block (up to FXRX_INGEST_KERNEL_MAX raw bytes per
 * stream, an environment variable, default 1 MiB) is read over the bus by the conversion kernel itself, which saves the host the
 * copy call.  Measured: up to 1 MB raw the two routes are equally fast, from 2 MB on the copy is faster.
 * Definition of a sample: re = (float)i_re * scale, im = (float)i_im * scale -- one exact
 * int -> float conversion and one IEEE binary32 multiply, no contraction -- which is what fxrx_iq_convert_host computes: results
 * for integer input are identical, field for field and bit for bit, to fxrx_submit on the float array that function produces.
 * The format is a property of a block, not of the context: the blocks of a continuing stream may change format; all streams of
 * one block share it.  sc16 samples must be 4-byte aligned, sc8 samples 2-byte aligned (FXRX_ERR_ARG otherwise); any such
 * alignment and any n_samples work.  fxrx_submit(c, ...) is fxrx_submit_fmt(c, ..., FXRX_IQ_FC32).  Failure semantics as for
 * fxrx_submit. */
enum { FXRX_IQ_FC32 = 0, FXRX_IQ_SC16 = 1, FXRX_IQ_SC8 = 2 };
unsigned int fxrx_iq_sample_bytes(int fmt);                 /* 8, 4, 2; 0 for an unknown fmt (no GPU needed) */
/* scale of an integer format: default 1/32768 (sc16), 1/128 (sc8).  Must be finite and > 0; applies from the next submit on.
 * FXRX_IQ_FC32 or an unknown format: FXRX_ERR_ARG */
int fxrx_set_iq_scale(fxrx_ctx *c, int fmt, float scale);
int fxrx_submit_fmt(fxrx_ctx *c, const void *const *iq, const uint64_t *n_samples, int on_device, int fmt);
int fxrx_process_fmt(fxrx_ctx *c, const void *const *iq, const uint64_t *n_samples, int on_device, int fmt);
/* the definition of the conversion, on the host (no GPU needed): n_samples integer pairs at `in` -> 2 n_samples floats at
 * out_re_im.  FXRX_IQ_FC32 copies.  Returns 0, or FXRX_ERR_ARG for an unknown format or a NULL pointer */
int fxrx_iq_convert_host(int fmt, float scale, const void *in, uint64_t n_samples, float *out_re_im);
/* 1: the oldest block in flight has finished (fxrx_collect will not wait), 0: not yet / nothing in flight, < 0: FXRX_ERR_* */
/* (a block whose tail waits in an open gang, FXRX_TAIL_GANG, is launched by this call: hence no const) */
int fxrx_ready(fxrx_ctx *c);
unsigned int fxrx_inflight(const fxrx_ctx *c);
/* tests: make the next `submits` calls of fxrx_submit / `collects` calls of fxrx_collect fail (FXRX_ERR_STATE) after they have
 * done their bookkeeping, to exercise the paths above */
int fxrx_debug_fail(fxrx_ctx *c, unsigned int submits, unsigned int collects);
/* tests: out[0] = tail launches so far that served more than one block in flight (the payload PLL and the decode front of up to four
 * blocks in one launch each: FXRX_TAIL_GANG, 1 = off; only with fxrx_set_depth >= 4), out[1] = the blocks they carried */
int fxrx_debug_gang_stats(const fxrx_ctx *c, uint64_t out[2]);
/* tests: of the last collected block -- out[0] = speculative segments whose first hops the pre-lock scan (fx_prescan_kernel) took
 * off their walkers (FXRX_PRESCAN=1; off by default; FXRX_PRESCAN_HOPS = hops scanned per segment, 0 = none), out[1] = those whose walker took its
 * first candidate preamble from the scan's table, out[2] = those whose table held none: their own scan carried on behind it */
int fxrx_debug_prescan_stats(const fxrx_ctx *c, uint64_t out[3]);
/* tests, no device needed: the walker's reading of a pre-lock scan table.  words: n_words chunk words (16 hops each; hop << 16 | lag of
 * the chunk's lowest hitting hop, or 0xFFFFFFFF); K: hops asked for; start / stop / n: the segment and the data.  Returns 1 when a word
 * holds a hit, 0 when none does; out[0] = position the walk goes on from, out[1] = hops added to the cheap-hop counter, out[2] = hops the
 * scan covers (new half inside the segment and the data, at most K) */
int fxrx_debug_prescan_words(const uint32_t *words, uint32_t n_words, uint32_t K, int64_t start, int64_t stop, int64_t n, int64_t out[3]);
/* tests: which of its reasons made fxrx_collect complete a block's decoding (fxrx_timing.late_decodes counts the blocks; a block may count
 * under several reasons).  out[0..5], cumulative since fxrx_create: plain frames beyond the decode launch | Reed-Solomon frames and no
 * Reed-Solomon launch | batch Viterbi frames beyond the launch | trellis work items beyond the launch | handed-back frames beyond the fallback
 * launch | frames that were not clean in a chain without the trellis kernels.  out[6..9], of the last collected block: frames on the
 * wave-per-frame list, on the batch Viterbi list, on the Reed-Solomon list, and trellis work items (class padding included).
 * (FXRX_DEBUG_CUS=<n>, read by fxrx_create: plan the launches as for a chip of n CUs, 1 <= n <= the real count) */
int fxrx_debug_late_stats(const fxrx_ctx *c, uint64_t out[10]);
/* tests: blocks in flight whose tails are deferred at this moment (the open gang's members; 0 .. 3) */
int fxrx_debug_gang_open(const fxrx_ctx *c);
/* tests: run the walker's header decoder on the GPU over n headers given in host memory.  soft != 0: `in` holds 432 soft values per
 * header (0 = surely 0 ... 255 = surely 1) in channel order, before the header's first de-interleaver; soft == 0: the 54 received bytes.
 * Writes 20 decoded bytes per header to out20 and the CRC-32 verdict (1 / 0) to valid[i].  Synchronous, on the current HIP device;
 * returns 0 or FXRX_ERR_* */
int fxrx_debug_header_decode(int soft, const uint8_t *in, unsigned int n, uint8_t *out20, int *valid);
/* tests: run the payload decoder's block decoder for `fec` (Hamming, Golay or SECDED), soft-input (soft != 0) or hard, on the GPU over
 * `count` packets of n message bytes given in host memory.  soft != 0: `in` holds 8 fec_enc_len(fec, n) soft values per packet in codeword
 * bit order (after the stage's de-interleaver); soft == 0: the fec_enc_len(fec, n) coded bytes.  Writes n bytes per packet to out.
 * Synchronous, on the current HIP device; returns 0 or FXRX_ERR_* */
int fxrx_debug_block_decode(unsigned int fec, int soft, unsigned int n, unsigned int count, const uint8_t *in, uint8_t *out);
/* tests: its soft-output twin (fxrx_config.soft_chain): `in` holds 8 fec_enc_len(fec, n) soft values per packet in codeword bit order,
 * out_soft receives 8 n soft values per packet, one per message bit, MSB first.  Synchronous, on the current HIP device; returns 0 or
 * FXRX_ERR_* */
int fxrx_debug_block_siso(unsigned int fec, unsigned int n, unsigned int count, const uint8_t *in, uint8_t *out_soft);
/* tests: the soft-decision Reed-Solomon decoder (fxrx_config.soft_rs) on the GPU over `count` packets of n message bytes: in_soft holds
 * 8 fec_enc_len(RS, n) soft values per packet in codeword bit order, out receives n bytes per packet, chosen_f the winning f of every
 * Reed-Solomon block (max(1, ceil(n / 223)) per packet; 255 would say "no candidate" and is never written: the f = 32
 * candidate always exists).  Synchronous, on the current HIP device; returns 0 or
 * FXRX_ERR_* */
int fxrx_debug_rs_soft(unsigned int n, unsigned int count, const uint8_t *in_soft, uint8_t *out, uint8_t *chosen_f);
/* tests: the same decoder under a bound on f (fmax itself: even, 0 .. 32; fxrx_config.soft_rs_fmax) and in either output form
 * (fxrx_config.soft_rs_chain).  chain = 0: out gets n bytes per packet, the hard output under the bound; chain = 1: out gets 8 n soft
 * values per packet.  in_soft and chosen_f as for fxrx_debug_rs_soft; a block given up on has chosen_f 255.  The same cap on n. */
int fxrx_debug_rs_chain(unsigned int n, unsigned int count, int fmax, int chain, const uint8_t *in_soft, uint8_t *out, uint8_t *chosen_f);
/* diagnostic builds (-DFX_STAMPS) only: shader-clock deltas of the decode phases of payload job i */
int fxrx_debug_stamps(const fxrx_ctx *c, unsigned int i, uint32_t out[8]);
int fxrx_debug_chain_stamps(const fxrx_ctx *c, uint32_t out[8]);  /* chain kernel phase clocks (stream 0) of the last collected block */
int fxrx_debug_walk_stamps(const fxrx_ctx *c, uint64_t out[4]);   /* summed walker phase clocks: coarse, seek, align, header */
int fxrx_debug_walk_maxjob(const fxrx_ctx *c, uint64_t out[8]);   /* slowest walk job: 4 phase clocks, hops, coarse hops, frames, total */
int fxrx_debug_walk_jobs(const fxrx_ctx *c, uint32_t *out, unsigned int cap_jobs);   /* per walk job 6 words: 4 stamps, hops, frames; returns the job count */
/* device-resident payload symbols / hard decisions of the last call (NULL if none) */
const void *fxrx_device_framesyms(const fxrx_ctx *c, uint64_t *n_symbols);

typedef struct {
    double   walk_ms, paymf_ms, paypll_ms, paydec_ms, total_ms;   /* HIP-event times of the block's kernels, on the stream they ran on */
    uint64_t hops, walk_jobs, repairs, frames, payload_symbols, samples, hops_cheap;
    double   host_submit_ms, host_walkwait_ms;   /* wall time inside fxrx_submit (descriptor build + enqueue) / always 0: the host no longer waits for the walkers */
    double   seekverify_ms;                      /* fx_seekverify_kernel (full detector over the hops the walkers skipped) */
    uint64_t verify_hops, verify_failures;       /* hops re-checked / runs on which the exact detector fired (those spans are walked again, exactly) */
    double   host_collectwait_ms;                /* wall time fxrx_collect waited for the block's results */
    uint64_t walk_mode;                          /* 0: all streams started freshly reset, 1: some continued the previous block (true walkers ordered behind its chain kernel) */
    double   chain_ms;                           /* fx_chain_kernel + fx_plan_kernel */
    uint64_t replays;                            /* carry-buffer overflows / chain repairs handled so far (blocks behind were enqueued again) */
    uint64_t vb_blocks, vb_repairs;              /* batch Viterbi: trellis blocks (incl. padding slots) / blocks run again because a hand-over check failed */
    uint64_t late_decodes;                       /* blocks whose decode launches had to be completed at collect (more frames than the grids were sized for) */
    uint64_t vb_fallbacks;                       /* batch Viterbi: frames handed back to the wave-per-frame decoder (a hand-over that stayed unverified) */
    uint64_t vb_clean;                           /* batch Viterbi: rate-1/2 frames whose coded bits were a codeword as received, decoded without a trellis (FXRX_VB_CLEAN=0: none) */
    uint64_t trellis_launched;                   /* batch Viterbi: 1 when the block's trellis kernels were launched with its chain, 0 when they were left out (clean
                                                  * frames finish in fx_vbpre_kernel; FXRX_VB_EARLY_TAIL=0: always 1) */
    uint64_t late_windows;                       /* detector mode with want_framesyms: blocks so far whose aligned windows had to be completed at collect (more
                                                  * detections than window slots were reserved from the previous block's count; FXRX_DETWIN_RESERVE sets the number) */
} fxrx_timing;
int fxrx_last_timing(const fxrx_ctx *c, fxrx_timing *t);
/* Stage times come from HIP events recorded between the kernels of a block, and every event is one more packet in the block's
 * queue -- with blocks in flight the queues' packet rate is what limits throughput.  level 2: all stages;
 * 1: the PLL only (paypll_ms; what bench.py quotes its roofline line for); 0: none (the *_ms fields read 0); -1 (default):
 * 2 with one block at a time, 0 with depth > 1.  Counters are always there.  Environment: FXRX_TIMING. */
int fxrx_set_timing(fxrx_ctx *c, int level);
/* diagnostics: of the last collected block, ms since a common origin: host time at fxrx_submit, GPU time of its first and of its
 * last event, host time when fxrx_collect returned it (needs timing level 2 from the first submit on) */
int fxrx_debug_block_times(const fxrx_ctx *c, double out[4]);
/* the HIP stream (hipStream_t as void*) of the first slot of the ring of blocks in flight; every block runs its whole kernel
 * chain on its slot's stream.  To order external work against a block, use fxrx_collect (it returns when the block's
 * results are on the host). */
void *fxrx_stream(const fxrx_ctx *c);

/* batched frame generator: one frame -> samples (host) */
unsigned int fxrx_gen_frame_len(unsigned int mod_scheme, unsigned int check, unsigned int fec0, unsigned int fec1,
                                unsigned int payload_len);

/* block-API index maps of the reference (lib/flex_tx_impl.cc:75-181, lib/flex_rx_impl.cc:74-179); -1 = unsupported */
int fxrx_mod_from_index(int idx);   int fxrx_mod_to_index(unsigned int mod_scheme);
int fxrx_inner_from_index(int idx); int fxrx_inner_to_index(unsigned int fec);
int fxrx_outer_from_index(int idx); int fxrx_outer_to_index(unsigned int fec);

/* ------------------------------------------------------------------------------------------
 * (3) batched frame generator on the GPU -- the flex_tx counterpart
 *
 * What /root/reference/lib/flex_tx_impl.cc:191-209 (send_pkt) does per PDU -- flexframegen_assemble (:200) and
 * flexframegen_write_samples (:203-205) with the properties of :51-56 / :183-189 -- for many frames in one call,
 * straight into a device buffer.  Packet encoding of header and payload (CRC, whitening, both code stages,
 * interleavers, bit packing), modulation and pulse shaping run on the GPU; the host lays out descriptors.  Samples are
 * bit-identical to flexframegen_write_samples.
 * ------------------------------------------------------------------------------------------ */
typedef struct fxtx_ctx_s fxtx_ctx;
typedef struct {
    flexframegenprops_s props;          /* check, fec0, fec1, mod_scheme of this frame */
    const unsigned char *header;        /* 14 user bytes, or NULL for zeros */
    const unsigned char *payload;       /* payload_len bytes (host memory) */
    unsigned int        payload_len;    /* 0 .. 65535 */
    float               dt;             /* fractional-sample offset the pulse is designed with (0 = none): an advance, tau ~ -dt */
    unsigned long long  out_offset;     /* first sample of the frame in the output buffer */
} fxtx_frame;
fxtx_ctx    *fxtx_create(int device);                        /* NULL + fxrx_last_error() without a usable GPU */
void         fxtx_destroy(fxtx_ctx *c);
unsigned int fxtx_frame_len(const fxtx_frame *f);            /* samples the frame occupies */
/* Writes every frame's samples to out_device[out_offset ...] (interleaved float32 re,im; out_len samples long).  Frames
 * must not overlap; samples between frames are left untouched (zero the buffer first).  Returns 0 or FXRX_ERR_*;
 * synchronous (the frames are in the buffer when the call returns). */
int          fxtx_generate(fxtx_ctx *c, const fxtx_frame *frames, unsigned int n_frames, void *out_device,
                           unsigned long long out_len);
/* The synthetic channel of the test / bench source on the device, so that hundreds of distinct streams
 * never exist on the host: stream s = samples [s n_per_stream, (s+1) n_per_stream) of iq_device becomes
 * gain x[n] exp(j (phase + n cfo)) + noise, noise white Gaussian with standard deviation sigma per real dimension, drawn from
 * a counter-based generator keyed by `seed` (every sample is a function of (seed, n) alone).  n_per_stream must be even.
 * Synchronous; returns 0 or FXRX_ERR_*. */
typedef struct { float cfo, phase, gain, sigma; unsigned long long seed; } fxtx_channel;
int          fxtx_apply_channel(fxtx_ctx *c, void *iq_device, unsigned int n_streams, unsigned long long n_per_stream,
                          const fxtx_channel *ch);

/* Float IQ -> integer IQ on the device (the inverse of the receive side's conversion, for signal sources and tools):
 * q = saturate(rintf(x * inv_scale)) per component (round half to even; NaN -> 0), to int16 (FXRX_IQ_SC16) or int8 (FXRX_IQ_SC8)
 * pairs; *saturated (may be NULL) = number of components that were clamped -- what tells a user the gain is wrong.  Synchronous.
 * in / out are device pointers on the context's device (8-byte / sample-size aligned); they may not overlap.
 * Returns 0 or FXRX_ERR_*. */
int          fxtx_quantize(fxtx_ctx *c, const void *iq_f32_device, void *out_device, unsigned long long n_samples,
                           int fmt, float inv_scale, unsigned long long *saturated);

#ifdef __cplusplus
}
#endif
#endif
