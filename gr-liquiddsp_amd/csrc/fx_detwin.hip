// fx_detwin.hip -- the aligned windows of detector mode (include/fxrx.h: fxrx_frame.framesyms with FXRX_MODE_DETECTOR and
// want_framesyms): for every detection of a block the 512 samples x[start, start + 512) of its stream, exactly as the walker
// read them, into page-locked host memory.  This is what liquid's qdetector_cccf_execute returns.
//
// fx_detwin_kernel runs on the block's stream behind the plan stage.  How many detections the block holds only the device
// knows (FxBlockHdr.n_frames of the payload-side header), so workgroups stride over the records; a workgroup of 256 threads
// moves one window as 256 pieces of 16 bytes.  A record's stream and block-local start come from the device-side twin of its
// result record (FxPayJob, same index) and the plan stage's stream_base; the source is the two-piece addressing of the chain
// (FxStreamDesc): index p >= 0 is x[p], p < 0 is xa_end[p] in the carried tail, and whatever lies below the stream's
// zero-floor (absolute index abs_base + p < 0) is (0, 0).  `start` may be odd, so a piece's two samples are loaded as two
// float2 (8-byte aligned) and stored as one 16-byte vector: every slot is 4096 bytes at a 4096-byte offset.
//
// Slots.  Window i of the records [0, reserved) goes to slot i of `out`.  The host reserves from the previous block's count,
// and completes a block with more detections when it is collected (fx_host.cpp: finish_windows), from the block's input --
// which the API keeps valid until then.  The carried tail is NOT kept that long (the chain kernel two blocks on writes over
// it), so the windows that reach into it are never left for later: a stream's record k (k = 0, 1) beyond the reservation whose
// start is negative goes to slot 2 s + k of `out_tail` now.  Two suffice: the previous block (n samples) left either because
// a window did not fit (a0 + 512 > n) or because its next hop did not (pos + 256 > n, tail kept from pos - 256), so the first
// detection that starts in the tail has a0 > n - 512; detections of a stream are at least 256 samples apart, so the second
// has a0 > n - 256 and a third would start behind n, not in the tail.  A third one sets *flag_host all
// the same, and the host fails the block rather than hand out a window nobody wrote.
//
// Bounds: every load is checked against [-carry_len, n) of its stream, so no descriptor can make it read outside the
// block's buffers; stores go to slot indices below `reserved` / 2 nstreams, which is what the host allocated.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "fx_common.h"
#include "fx_launch.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

#define DETWIN_THREADS 256
static_assert(2 * DETWIN_THREADS == FX_NFFT, "one 16-byte piece (two samples) per thread");

__device__ __forceinline__ float2 detwin_sample(const float2 *x, const float2 *xa_end, int64_t n, int64_t lowest, int64_t p)
{
    if (p < lowest || p >= n) return make_float2(0.0f, 0.0f);
    return p >= 0 ? x[p] : xa_end[p];
}

// window of record g (stream s) -> slot (256 x 16 bytes)
__device__ __forceinline__ void detwin_copy(const FxStreamDesc &sd, int64_t start, f32x4 *slot)
{
    // lowest readable index: the zero-floor, and never below the tail that is really there
    int64_t lowest = 0;
    if (start < 0) {
        const int64_t have = (sd.xa_end && sd.state_in) ? sd.state_in->carry_len : 0;
        lowest = max(-sd.abs_base, -have);
    }
    const int64_t p = start + 2 * (int64_t)threadIdx.x;
    const float2 a = detwin_sample(sd.x, sd.xa_end, sd.n, lowest, p), b = detwin_sample(sd.x, sd.xa_end, sd.n, lowest, p + 1);
    f32x4 v; v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
    __builtin_nontemporal_store(v, slot + threadIdx.x);
}

// records [first, min(n_frames, reserved)) -> out; with_tails: also the tail windows beyond the reservation -> out_tail.
// skip_tail (the launch at collect): records with a negative start are left alone -- their tail is gone, they were served before.
extern "C" __global__ __launch_bounds__(DETWIN_THREADS)
void fx_detwin_kernel(const FxStreamDesc *streams, uint32_t nstreams, const uint32_t *stream_base, const FxPayJob *pjobs, const FxBlockHdr *hdr,
                      uint32_t first, uint32_t reserved, f32x4 *out, f32x4 *out_tail, uint32_t *flag_host, int with_tails, int skip_tail)
{
    const uint32_t n = hdr->n_frames, end = min(n, reserved);
    for (uint32_t g = first + blockIdx.x; g < end; g += gridDim.x) {
        uint32_t lo = 0, hi = nstreams;                                          // stream_base[lo] <= g < stream_base[hi]
        while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (stream_base[mid] <= g) lo = mid; else hi = mid; }
        const int64_t start = pjobs[g].start;
        if (skip_tail && start < 0) continue;
        detwin_copy(streams[lo], start, out + (size_t)g * DETWIN_THREADS);
    }
    if (!with_tails || n <= reserved) return;
    for (uint32_t s = blockIdx.x; s < nstreams; s += gridDim.x) {
        const uint32_t b0 = stream_base[s], b1 = stream_base[s + 1];
        for (uint32_t k = 0; b0 + k < b1; k++) {
            const uint32_t g = b0 + k;
            const int64_t start = pjobs[g].start;
            if (start >= 0) break;                                               // (a stream's records are in order of position)
            if (g < reserved) continue;
            if (k >= 2) { if (threadIdx.x == 0) *flag_host = 1u; break; }
            detwin_copy(streams[s], start, out_tail + (size_t)(2 * s + k) * DETWIN_THREADS);
        }
    }
}

extern "C" hipError_t fx_launch_detwin(hipStream_t st, unsigned grid, const FxStreamDesc *streams, uint32_t nstreams, const uint32_t *stream_base, const FxPayJob *pjobs,
                                       const FxBlockHdr *hdr, uint32_t first, uint32_t reserved, float2 *out, float2 *out_tail, uint32_t *flag_host, int with_tails,
                                       int skip_tail)
{
    hipLaunchKernelGGL(fx_detwin_kernel, dim3(grid ? grid : 1u), dim3(DETWIN_THREADS), 0, st, streams, nstreams, stream_base, pjobs, hdr, first, reserved,
                       reinterpret_cast<f32x4 *>(out), reinterpret_cast<f32x4 *>(out_tail), flag_host, with_tails, skip_tail);
    return hipGetLastError();
}
