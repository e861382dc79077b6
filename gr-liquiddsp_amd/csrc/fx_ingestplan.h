// fx_ingestplan.h -- how the new samples of one stream reach the float buffer a block's kernels read: six routes, chosen per stream
// from the block's format, where the samples lie, whether the device can read that memory, and two size limits.
//
//   format    source                                              route
//   fc32      device                                              kRouteInPlace        read where it lies, nothing to launch
//   fc32      host, page-locked, 8-byte aligned, <= upload limit  kRouteUploadKernel   fx_upload_kernel fetches it over the bus
//   fc32      host, otherwise                                     kRouteUploadCopy     the runtime's copy engines
//   sc16/sc8  device                                              kRouteConvertInPlace fx_ingest_kernel reads it in place
//   sc16/sc8  host, page-locked, <= ingest limit (raw bytes)      kRouteConvertBus     fx_ingest_kernel reads it over the bus
//   sc16/sc8  host, otherwise                                     kRouteConvertCopy    raw copy into the slot, then fx_ingest_kernel
//
// A stream without new samples has no route (kRouteNone).  fx_host.cpp:prepare_ingest asks ingest_route for every stream, reserves what
// the route writes to and leaves the jobs in the slot; enqueue_front launches them behind every check and reservation of the block.
// Host only and pure -- no HIP call, no allocation --, so that tests/cpp/ingestplan_check.cpp checks it with g++ alone.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/fxrx.h"

enum IngestRoute { kRouteNone = 0, kRouteInPlace, kRouteUploadKernel, kRouteUploadCopy, kRouteConvertInPlace, kRouteConvertBus, kRouteConvertCopy };

// bytes up to which a page-locked host block is read by a kernel instead of the copy engines, per stream and block
struct IngestLimits {
    size_t upload_kernel_max = 64u << 20;   // fc32: the launch costs microseconds where the copy call held the host thread for hundreds
    size_t ingest_kernel_max = 1u << 20;    // sc16 / sc8, raw bytes (FXRX_INGEST_KERNEL_MAX): equal to the copy up to 1 MB, slower from 2 MB on
};

inline unsigned iq_sample_bytes(int fmt) { return fmt == FXRX_IQ_FC32 ? 8u : fmt == FXRX_IQ_SC16 ? 4u : fmt == FXRX_IQ_SC8 ? 2u : 0u; }

// could a kernel read n samples at host address addr, were that memory page-locked?  (Asked first: whether it is page-locked takes a
// call into the runtime.)  Float IQ is fetched in 8-byte pieces; integer IQ may sit at any multiple of its sample size, which
// prepare_ingest has checked.
inline bool kernel_may_read_host(int fmt, uintptr_t addr, uint64_t n, const IngestLimits &lim)
{
    if (fmt == FXRX_IQ_FC32) return (addr & 7u) == 0 && n * 8u <= lim.upload_kernel_max;
    return n * iq_sample_bytes(fmt) <= lim.ingest_kernel_max;
}

// page_locked: the device can read the memory at addr (host sources only; not looked at where kernel_may_read_host says no)
inline IngestRoute ingest_route(int fmt, bool on_device, bool page_locked, uintptr_t addr, uint64_t n, const IngestLimits &lim)
{
    if (!n) return kRouteNone;
    const bool flt = fmt == FXRX_IQ_FC32;
    if (on_device) return flt ? kRouteInPlace : kRouteConvertInPlace;
    if (page_locked && kernel_may_read_host(fmt, addr, n, lim)) return flt ? kRouteUploadKernel : kRouteConvertBus;
    return flt ? kRouteUploadCopy : kRouteConvertCopy;
}
inline bool route_copies(IngestRoute r) { return r == kRouteUploadCopy || r == kRouteConvertCopy; }          // through the copy engines first
inline bool route_converts(IngestRoute r) { return r >= kRouteConvertInPlace; }                               // ends in fx_ingest_kernel
