// fx_ingest.hip -- integer IQ at the edges of the receive path (include/fxrx.h: fxrx_submit_fmt, fxtx_quantize).
//
// fx_ingest_kernel<FMT>: 16-bit / 8-bit integer (re, im) pairs -> float2 in the block's staging buffer, from where the
// untouched chain reads them exactly as it reads an uploaded float block.  A sample is re = (float)i_re * scale,
// im = (float)i_im * scale: one exact conversion and one binary32 multiply (the build passes -ffp-contract=off), the same
// two operations fxrx_iq_convert_host performs, so results are bit-identical to the float path on that function's output.
//
// The source is page-locked host memory read over the bus, a caller's device buffer, or the slot's raw staging buffer.
// Like fx_upload_kernel this is a latency problem: 16-byte loads (4 sc16 / 8 sc8 samples), kIngestInFlight of them issued
// per thread before the first is used, non-temporal (every byte is read once), a grid of a few workgroups per CU striding
// over the vectors.  Vector loads touch only 16-byte-aligned addresses that lie entirely inside [src, src + n * bytes):
// the unaligned head (< 16 bytes) and the tail (< 16 bytes) go through one element load per sample.  Exactly n float2 are
// written.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include "../../include/fxrx.h"
#include "fx_launch.h"

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kIngestInFlight = 4;      // 16-byte loads per thread before the first conversion: 64 bytes, as the float upload keeps

template <int FMT> struct IqFmt;
template <> struct IqFmt<FXRX_IQ_SC16> { typedef uint32_t elem; static constexpr int per_vec = 4; };     // one sample = one 32-bit word
template <> struct IqFmt<FXRX_IQ_SC8>  { typedef uint16_t elem; static constexpr int per_vec = 8; };     // one sample = one 16-bit word

// sample k of a 32-bit word (little endian: re in the low half)
__device__ __forceinline__ float2 iq_sc16(uint32_t w, float scale)
{
    return make_float2((float)(int16_t)(w & 0xffffu) * scale, (float)(int16_t)(w >> 16) * scale);
}
__device__ __forceinline__ float2 iq_sc8(uint32_t w16, float scale)
{
    return make_float2((float)(int8_t)(w16 & 0xffu) * scale, (float)(int8_t)((w16 >> 8) & 0xffu) * scale);
}
template <int FMT> __device__ __forceinline__ float2 iq_elem(typename IqFmt<FMT>::elem w, float scale)
{
    if constexpr (FMT == FXRX_IQ_SC16) return iq_sc16((uint32_t)w, scale);
    else return iq_sc8((uint32_t)w, scale);
}

// the per_vec samples of one 16-byte vector -> dst[0 .. per_vec); pair: dst is 16-byte aligned (two samples per store)
template <int FMT, bool PAIR> __device__ __forceinline__ void iq_store_vec(u32x4 v, float scale, float2 *dst)
{
    constexpr int NV = IqFmt<FMT>::per_vec;
    float2 s[NV];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint32_t w = v[k];
        if constexpr (FMT == FXRX_IQ_SC16) s[k] = iq_sc16(w, scale);
        else { s[2 * k] = iq_sc8(w & 0xffffu, scale); s[2 * k + 1] = iq_sc8(w >> 16, scale); }
    }
    if (PAIR) {
        f32x4 *d4 = reinterpret_cast<f32x4 *>(dst);
#pragma unroll
        for (int k = 0; k < NV / 2; k++) { f32x4 o; o[0] = s[2 * k].x; o[1] = s[2 * k].y; o[2] = s[2 * k + 1].x; o[3] = s[2 * k + 1].y; d4[k] = o; }
    } else {
#pragma unroll
        for (int k = 0; k < NV; k++) dst[k] = s[k];
    }
}

template <int FMT, bool PAIR> __device__ __forceinline__ void ingest_body(const u32x4 *vsrc, float2 *vdst, size_t nvec, float scale)
{
    constexpr int NV = IqFmt<FMT>::per_vec;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (; i + (kIngestInFlight - 1) * stride < nvec; i += kIngestInFlight * stride) {
        u32x4 v[kIngestInFlight];
#pragma unroll
        for (int k = 0; k < kIngestInFlight; k++) v[k] = __builtin_nontemporal_load(vsrc + i + k * stride);
#pragma unroll
        for (int k = 0; k < kIngestInFlight; k++) iq_store_vec<FMT, PAIR>(v[k], scale, vdst + (i + k * stride) * NV);
    }
    for (; i < nvec; i += stride) iq_store_vec<FMT, PAIR>(__builtin_nontemporal_load(vsrc + i), scale, vdst + i * NV);
}

template <int FMT> __global__ __launch_bounds__(256)
void fx_ingest_kernel(const void *src, float2 *dst, size_t n, float scale)
{
    typedef typename IqFmt<FMT>::elem elem;
    constexpr size_t NV = IqFmt<FMT>::per_vec;
    const elem *e = reinterpret_cast<const elem *>(src);
    // head: samples in front of the first 16-byte boundary (src is a multiple of sizeof(elem): the host checked)
    const size_t mis = (size_t)(reinterpret_cast<uintptr_t>(src) & 15u);
    const size_t to_boundary = mis ? (16u - mis) / sizeof(elem) : 0u;
    const size_t head = n < to_boundary ? n : to_boundary;
    const size_t nvec = (n - head) / NV;                     // whole vectors inside the buffer
    const size_t tail0 = head + nvec * NV;                   // first sample behind them (n - tail0 < NV)
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid < head) dst[gid] = iq_elem<FMT>(e[gid], scale);
    if (gid < n - tail0) dst[tail0 + gid] = iq_elem<FMT>(e[tail0 + gid], scale);
    const u32x4 *vsrc = reinterpret_cast<const u32x4 *>(e + head);
    // dst is 16-byte aligned (the staging buffer's start), so the body's first output is when head is even
    if ((head & 1u) == 0) ingest_body<FMT, true>(vsrc, dst + head, nvec, scale);
    else ingest_body<FMT, false>(vsrc, dst + head, nvec, scale);
}

extern "C" hipError_t fx_launch_ingest(hipStream_t st, int fmt, const void *src, float2 *dst, size_t n, float scale, unsigned n_cus)
{
    if (n == 0) return hipSuccess;
    const size_t per_vec = fmt == FXRX_IQ_SC16 ? 4 : 8;
    const size_t nvec = n / per_vec + 1;                     // (an upper bound; at least one workgroup for head and tail)
    const unsigned grid = (unsigned)std::min<size_t>((nvec + 256 * kIngestInFlight - 1) / (256 * kIngestInFlight), 4u * (size_t)n_cus);
    if (fmt == FXRX_IQ_SC16) hipLaunchKernelGGL(fx_ingest_kernel<FXRX_IQ_SC16>, dim3(grid ? grid : 1u), dim3(256), 0, st, src, dst, n, scale);
    else if (fmt == FXRX_IQ_SC8) hipLaunchKernelGGL(fx_ingest_kernel<FXRX_IQ_SC8>, dim3(grid ? grid : 1u), dim3(256), 0, st, src, dst, n, scale);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

// ---- the inverse, for the generator side: q = saturate(rintf(x * inv_scale)) per component (round half to even; NaN -> 0).
// One sample per thread and pass: an 8-byte load, a 4-byte (sc16) / 2-byte (sc8) store.  Clamped components are counted per
// thread, summed over the wave and added with one atomic per wave.
template <int LO, int HI> __device__ __forceinline__ int quantize_one(float x, float inv_scale, unsigned &clamped)
{
    const float r = rintf(x * inv_scale);
    if (r > (float)HI) { clamped++; return HI; }
    if (r < (float)LO) { clamped++; return LO; }
    return (r == r) ? (int)r : 0;
}

template <int FMT> __global__ __launch_bounds__(256)
void fx_quantize_kernel(const float2 *in, void *out, size_t n, float inv_scale, unsigned long long *saturated)
{
    typedef typename IqFmt<FMT>::elem elem;
    elem *o = reinterpret_cast<elem *>(out);
    unsigned clamped = 0;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const float2 x = in[i];
        if constexpr (FMT == FXRX_IQ_SC16) {
            const int re = quantize_one<-32768, 32767>(x.x, inv_scale, clamped), im = quantize_one<-32768, 32767>(x.y, inv_scale, clamped);
            o[i] = (elem)(((uint32_t)re & 0xffffu) | ((uint32_t)im << 16));
        } else {
            const int re = quantize_one<-128, 127>(x.x, inv_scale, clamped), im = quantize_one<-128, 127>(x.y, inv_scale, clamped);
            o[i] = (elem)(((uint32_t)re & 0xffu) | (((uint32_t)im & 0xffu) << 8));
        }
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) clamped += (unsigned)__shfl_xor((int)clamped, m, 64);
    if ((threadIdx.x & 63) == 0 && clamped) atomicAdd(saturated, (unsigned long long)clamped);
}

extern "C" hipError_t fx_launch_quantize(hipStream_t st, int fmt, const float2 *in, void *out, size_t n, float inv_scale, unsigned long long *saturated,
                                         unsigned n_cus)
{
    if (n == 0) return hipSuccess;
    const unsigned grid = (unsigned)std::min<size_t>((n + 255) / 256, 8u * (size_t)n_cus);
    if (fmt == FXRX_IQ_SC16) hipLaunchKernelGGL(fx_quantize_kernel<FXRX_IQ_SC16>, dim3(grid), dim3(256), 0, st, in, out, n, inv_scale, saturated);
    else if (fmt == FXRX_IQ_SC8) hipLaunchKernelGGL(fx_quantize_kernel<FXRX_IQ_SC8>, dim3(grid), dim3(256), 0, st, in, out, n, inv_scale, saturated);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}
