// ingestplan_check.cpp -- the input routes of a block (gr-liquiddsp_amd/csrc/fx_ingestplan.h: ingest_route), compiled host-only with
// g++: tests/test_ingestplan.py.  Every row of the header's table, both sides of each size limit, the alignment rule of float IQ,
// and that a stream without new samples gets no route whatever else is said about it.
#include <cstdio>
#include <cstdint>
#include <initializer_list>
#include "../../gr-liquiddsp_amd/csrc/fx_ingestplan.h"

static int g_fail = 0, g_checks = 0;
#define CHECK(c, ...) do { g_checks++; if (!(c)) { if (++g_fail <= 20) { std::printf("FAIL %s: ", #c); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static const uintptr_t kAligned = 0x7f0000001000u;

static void table_rows(const IngestLimits &lim)
{
    const uint64_t n = 1000;        // 8000 / 4000 / 2000 bytes: below every limit used here
    for (bool locked : { false, true }) for (uintptr_t off : { 0u, 4u }) {
        CHECK(ingest_route(FXRX_IQ_FC32, true, locked, kAligned + off, n, lim) == kRouteInPlace, "fc32 device, locked %d offset %u", locked, (unsigned)off);
        for (int fmt : { FXRX_IQ_SC16, FXRX_IQ_SC8 })
            CHECK(ingest_route(fmt, true, locked, kAligned + off, n, lim) == kRouteConvertInPlace, "format %d device, locked %d offset %u", fmt, locked, (unsigned)off);
    }
    CHECK(ingest_route(FXRX_IQ_FC32, false, true, kAligned, n, lim) == kRouteUploadKernel, "fc32 page-locked");
    CHECK(ingest_route(FXRX_IQ_FC32, false, false, kAligned, n, lim) == kRouteUploadCopy, "fc32 pageable");
    for (int fmt : { FXRX_IQ_SC16, FXRX_IQ_SC8 }) for (uintptr_t off : { 0u, 2u, 4u, 6u }) {       // integer IQ: any multiple of the sample size
        if (fmt == FXRX_IQ_SC16 && (off & 3u)) continue;
        CHECK(ingest_route(fmt, false, true, kAligned + off, n, lim) == kRouteConvertBus, "format %d page-locked offset %u", fmt, (unsigned)off);
        CHECK(ingest_route(fmt, false, false, kAligned + off, n, lim) == kRouteConvertCopy, "format %d pageable offset %u", fmt, (unsigned)off);
    }
}

// at the limit a kernel reads page-locked memory, one byte (that is: the first whole sample) over it the copy engines do; pageable
// memory and device memory take their routes at either size
static void size_limits(const IngestLimits &lim)
{
    struct Row { int fmt; size_t max; IngestRoute kernel, copy, device; };
    const Row rows[3] = { { FXRX_IQ_FC32, lim.upload_kernel_max, kRouteUploadKernel, kRouteUploadCopy, kRouteInPlace },
                          { FXRX_IQ_SC16, lim.ingest_kernel_max, kRouteConvertBus, kRouteConvertCopy, kRouteConvertInPlace },
                          { FXRX_IQ_SC8, lim.ingest_kernel_max, kRouteConvertBus, kRouteConvertCopy, kRouteConvertInPlace } };
    for (const Row &r : rows) {
        const uint64_t b = iq_sample_bytes(r.fmt), at = r.max / b, over = (r.max + 1 + b - 1) / b;     // most samples within the limit / fewest beyond max + 1 bytes
        CHECK(at * b <= r.max && over * b >= r.max + 1 && over == at + 1, "format %d limit %zu", r.fmt, r.max);
        if (at) CHECK(ingest_route(r.fmt, false, true, kAligned, at, lim) == r.kernel, "format %d at the limit %zu", r.fmt, r.max);
        CHECK(ingest_route(r.fmt, false, true, kAligned, over, lim) == r.copy, "format %d over the limit %zu", r.fmt, r.max);
        CHECK(kernel_may_read_host(r.fmt, kAligned, at, lim) && !kernel_may_read_host(r.fmt, kAligned, over, lim), "format %d: the question asked first, limit %zu", r.fmt, r.max);
        for (uint64_t n : { at ? at : 1, over }) {
            CHECK(ingest_route(r.fmt, false, false, kAligned, n, lim) == r.copy, "format %d pageable, %llu samples", r.fmt, (unsigned long long)n);
            CHECK(ingest_route(r.fmt, true, false, kAligned, n, lim) == r.device, "format %d device, %llu samples", r.fmt, (unsigned long long)n);
        }
    }
}

static void float_alignment(const IngestLimits &lim)
{
    for (uintptr_t off = 1; off < 8; off++) {
        CHECK(ingest_route(FXRX_IQ_FC32, false, true, kAligned + off, 1000, lim) == kRouteUploadCopy, "fc32 page-locked at offset %u", (unsigned)off);
        CHECK(!kernel_may_read_host(FXRX_IQ_FC32, kAligned + off, 1000, lim), "fc32 at offset %u: the question asked first", (unsigned)off);
    }
    CHECK(ingest_route(FXRX_IQ_FC32, false, true, kAligned + 8, 1000, lim) == kRouteUploadKernel, "fc32 page-locked, one sample into the allocation");
}

static void empty_streams(const IngestLimits &lim)
{
    for (int fmt : { FXRX_IQ_FC32, FXRX_IQ_SC16, FXRX_IQ_SC8 }) for (bool dev : { false, true }) for (bool locked : { false, true }) for (uintptr_t addr : { (uintptr_t)0, kAligned, kAligned + 1 })
        CHECK(ingest_route(fmt, dev, locked, addr, 0, lim) == kRouteNone, "format %d device %d locked %d: no samples", fmt, dev, locked);
}

int main()
{
    CHECK(iq_sample_bytes(FXRX_IQ_FC32) == 8 && iq_sample_bytes(FXRX_IQ_SC16) == 4 && iq_sample_bytes(FXRX_IQ_SC8) == 2 && iq_sample_bytes(3) == 0 && iq_sample_bytes(-1) == 0, "sample sizes");
    IngestLimits def;
    CHECK(def.upload_kernel_max == (64u << 20) && def.ingest_kernel_max == (1u << 20), "default limits %zu %zu", def.upload_kernel_max, def.ingest_kernel_max);
    // the defaults; limits that are no multiple of a sample; an integer limit of 0 (FXRX_INGEST_KERNEL_MAX=0: always the copy engines) and a huge one
    const IngestLimits sets[] = { def, { 8000, 4000 }, { 8001, 4003 }, { 8007, 4001 }, { 64u << 20, 0 }, { 64u << 20, (size_t)1 << 40 } };
    for (const IngestLimits &lim : sets) {
        if (lim.upload_kernel_max >= 8000 && lim.ingest_kernel_max >= 4000) table_rows(lim);
        size_limits(lim); float_alignment(lim); empty_streams(lim);
    }
    std::printf("%d checks, %d failures\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
