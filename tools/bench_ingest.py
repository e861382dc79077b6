"""Rates of the receive path with the IQ starting in pinned host memory, per sample format (bench.py's value_with_h2d shape of
run: uploaded inside every submit, every frame of the last pass checked), plus the cost of the extra device pass.

    python tools/bench_ingest.py [--repeats 3] [--min-time 1.0] [--fc32-only] [--sweep]

The config-2 capture (bench.py's generator) is quantised once on the device (fxtx_quantize, RMS at 1/4 of full scale).  Legs:

  <fmt>_blocks      2^20-sample blocks of ONE continuing stream from pinned host memory, by the library's default route
  <fmt>_blocks_kernel / _copy   the same with the route forced for integer IQ (FXRX_INGEST_KERNEL_MAX = 2^40 / 0): the kernel
                    reads the host buffer over the bus / the copy engines move the raw bytes and the kernel converts on the device
  <fmt>_one, _one_kernel, _one_copy   the capture as one 20-Msample block per pass, likewise
  fc32_device / sc16_device   IQ resident in HBM (bench.py's headline shape); sc16 pays the conversion pass

Legs alternate inside this process, `--repeats` rounds, each leg in a timed region of its own that ends in a synchronise and lasts
at least --min-time seconds.  Every region runs on a context of its own, created for it, warmed up and closed afterwards, so that
only one context is alive at a time: HIP maps the streams of all live contexts onto a few hardware queues, and with many contexts
alive the rate of a latency-bound leg depended on which queues its streams happened to share (legs swapped places from job to job).  Prints one JSON line.  --fc32-only: the float legs alone (a library without the integer entry points).
--sweep: instead of the legs above, both routes for sc16 and sc8 over block sizes 2^14 .. 2^24 samples of one continuing stream
(where the limit FXRX_INGEST_KERNEL_MAX belongs).
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_SAMPLES = 20_000_000
BLOCK = 1 << 20
DEPTH = 12
LINK_GBPS = 63.0            # x16 Gen5 host link, usable


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--min-time", type=float, default=1.0)
    ap.add_argument("--samples", type=int, default=N_SAMPLES)
    ap.add_argument("--fc32-only", action="store_true")
    ap.add_argument("--sweep", action="store_true")
    a = ap.parse_args(argv)
    import torch
    fx = importlib.import_module("gr-liquiddsp_amd")
    if not torch.cuda.is_available():
        raise SystemExit("bench_ingest.py needs a HIP device")
    x, injected = fx.synth_stream(a.samples, stream_id=0)
    want = [pl for _, pl in injected]
    xd = torch.from_numpy(x).cuda()
    bytes_per = {"fc32": 8, "sc16": 4, "sc8": 2}
    host = {"fc32": torch.from_numpy(x).pin_memory()}
    dev = {"fc32": xd}
    fmt_id = {"fc32": 0}
    if not a.fc32_only:
        fmt_id.update(sc16=fx.IQ_SC16, sc8=fx.IQ_SC8)
        tx = fx.TxContext()
        for name, full in (("sc16", 32768.0), ("sc8", 128.0)):
            q, sat = tx.quantize(xd, fmt_id[name], 0.25 * full)
            if sat:
                raise SystemExit("bench_ingest: %d components clipped at 1/4 full scale" % sat)
            dev[name] = q
            host[name] = q.cpu().pin_memory()
        tx.close()
    torch.cuda.synchronize()

    def check(frames, what):
        got = [f["payload"] for f in frames if f["payload_valid"]]
        if got != want:
            raise SystemExit("bench_ingest: leg %s decoded %d of %d injected frames -- refusing to report a rate" % (what, len(got), len(want)))

    ROUTE = {"kernel": str(1 << 40), "copy": "0"}              # FXRX_INGEST_KERNEL_MAX (read when the context is created)

    def make_leg(name, fmt, shape, route=None, block=BLOCK):
        """returns (run(passes) -> frames of the last pass, close())"""
        before = os.environ.get("FXRX_INGEST_KERNEL_MAX")
        if route is not None:
            os.environ["FXRX_INGEST_KERNEL_MAX"] = ROUTE[route]
        ctx = fx.RxContext(1)
        if route is not None:
            if before is None:
                del os.environ["FXRX_INGEST_KERNEL_MAX"]
            else:
                os.environ["FXRX_INGEST_KERNEL_MAX"] = before
        ctx.set_depth(DEPTH); ctx.set_timing(0)
        on_dev = shape == "device"
        src = (dev if on_dev else host)[fmt]
        base, bps, n = src.data_ptr(), bytes_per[fmt], a.samples
        cuts = list(range(0, n, block)) + [n] if shape == "blocks" else [0, n]

        def submit(lo, hi):
            if fmt == "fc32":
                ctx.submit_raw([base + lo * bps], [hi - lo], on_dev)
            else:
                ctx.submit_raw([base + lo * bps], [hi - lo], on_dev, fmt_id[fmt])

        def run(passes):
            tags, last = [], []                                  # pass number of every block in flight, oldest first
            if shape == "blocks":
                ctx.reset()                                      # the passes follow each other as one continuing stream

            def collect():
                r = ctx.collect_raw()
                if tags.pop(0) == passes - 1:                    # (the capture ends in noise: no frame straddles two passes)
                    last.extend(ctx.results(r))
            for p in range(passes):
                for lo, hi in zip(cuts[:-1], cuts[1:]):
                    if len(tags) == DEPTH:
                        collect()
                    if shape != "blocks":
                        ctx.reset()
                    submit(lo, hi); tags.append(p)
            while tags:
                collect()
            return last
        return run, ctx.close

    legs = []
    if a.sweep:
        for fmt in ("sc16", "sc8"):
            for lg in (14, 16, 18, 20, 22, 24):
                for route in ("kernel", "copy"):
                    name = "%s_2^%d_%s" % (fmt, lg, route)
                    legs.append((name, (name, fmt, "blocks", route, 1 << lg), bytes_per[fmt]))
    else:
        for fmt in fmt_id:
            for shape in ("blocks", "one"):
                legs.append((fmt + "_" + shape, (fmt + "_" + shape, fmt, shape), bytes_per[fmt]))
                if fmt != "fc32":
                    for route in ("kernel", "copy"):
                        name = "%s_%s_%s" % (fmt, shape, route)
                        legs.append((name, (name, fmt, shape, route), bytes_per[fmt]))
        legs.append(("fc32_device", ("fc32_device", "fc32", "device"), 0))
        if not a.fc32_only:
            legs.append(("sc16_device", ("sc16_device", "sc16", "device"), 0))

    passes = {}
    rates = {name: [] for name, _, _ in legs}
    for _ in range(a.repeats):
        for name, spec, _ in legs:
            run, close = make_leg(*spec)                         # a context of this region's own (see above)
            check(run(2), name)                                  # warm-up, checked
            torch.cuda.synchronize()
            if name not in passes:                               # pass count of the timed regions from the warm rate
                t0 = time.perf_counter(); run(3); torch.cuda.synchronize()
                per = (time.perf_counter() - t0) / 3
                passes[name] = max(3, int(a.min_time / per * 1.15) + 1)
            while True:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                frames = run(passes[name])
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if dt >= a.min_time:
                    break
                passes[name] = int(passes[name] * a.min_time / dt * 1.2) + 1
            check(frames, name)
            rates[name].append(passes[name] * a.samples / dt / 1e6)
            close()
    out = {"metric": "Msamples/s through flex_rx by IQ sample format (QPSK r1/2 1024B, config 2)", "unit": "Msamples/s", "samples": a.samples,
           "block": BLOCK, "depth": DEPTH, "repeats": a.repeats, "min_time_s": a.min_time, "library": fx.lib().fxrx_version().decode(),
           "link_GBps_reference": LINK_GBPS, "legs": {}}
    for name, _, bps in legs:
        r = rates[name]; med = statistics.median(r)
        out["legs"][name] = dict(rates=[round(v, 1) for v in r], median=round(med, 1), spread_pct=round(100.0 * (max(r) - min(r)) / med, 2),
                                 bus_bytes_per_sample=bps, bus_GBps=round(med * 1e6 * bps / 1e9, 2), of_link=round(med * 1e6 * bps / 1e9 / LINK_GBPS, 3))
    L = out["legs"]
    for shape in ("blocks", "one"):
        for fmt in ("sc16", "sc8"):
            for sfx in ("", "_kernel", "_copy"):
                if fmt + "_" + shape + sfx in L:
                    L[fmt + "_" + shape + sfx]["vs_fc32_same_run"] = round(L[fmt + "_" + shape + sfx]["median"] / L["fc32_" + shape]["median"], 3)
    if "sc16_device" in L:
        L["sc16_device"]["vs_fc32_device"] = round(L["sc16_device"]["median"] / L["fc32_device"]["median"], 3)
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
