#!/usr/bin/env python
"""Frame latency of the drop-in boundary under a paced source.

Feeds a synthetic stream through flexframesync_execute in 256-sample calls at a wall-clock target rate (csrc/blocks/dropin_feed.cpp:
dropin_feed_paced) and reports, per setting, the delay between handing in a frame's last sample and its callback: median, p99, and
the frames that had not arrived when the input stopped.  Needs a GPU.

    python tools/dropin_latency.py --rates 10e6 100e6 --streaming 8192 --samples 4000000
    python tools/dropin_latency.py --streaming 0 --block 65536      # streaming off: frames arrive as blocks fill
"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rates", type=float, nargs="+", default=[10e6, 100e6], help="offered rates, samples per second")
    ap.add_argument("--streaming", type=int, default=8192, help="fxrx_sync_set_streaming floor (0: off)")
    ap.add_argument("--block", type=int, default=0, help="FXRX_SYNC_BLOCK (0: default)")
    ap.add_argument("--samples", type=int, default=4_000_000)
    ap.add_argument("--payload-len", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    if args.block:
        os.environ["FXRX_SYNC_BLOCK"] = str(args.block)
    fx = importlib.import_module("gr-liquiddsp_amd")
    F = fx._ffi.feed_lib()
    x, inj = fx.synth_stream(args.samples, stream_id=4242, payload_len=args.payload_len)
    flen = fx.lib().fxrx_gen_frame_len(2, fx.CRC_24, 11, 1, args.payload_len)
    ends = np.array([p + flen - 1 for p, _ in inj], np.uint64)
    for rate in args.rates:
        for rep in range(args.repeats):
            lat = np.zeros(len(ends), np.float64)
            und, ach = C.c_uint(0), C.c_double(0.0)
            n = F.dropin_feed_paced(x.ctypes.data, len(x), C.c_double(rate), args.streaming, ends.ctypes.data, len(ends), lat.ctypes.data,
                                    C.byref(und), C.byref(ach))
            if n == -2:
                raise SystemExit("dropin_feed_paced: the callbacks are not the injected frames, one each (latencies cannot be paired)")
            if n < 0:
                raise SystemExit("dropin_feed_paced failed: %s" % fx.lib().fxrx_last_error().decode())
            l = lat[:n] * 1e3
            print(json.dumps(dict(rate_msps=rate / 1e6, achieved_msps=round(ach.value / 1e6, 2), streaming_floor=args.streaming, block=args.block or (1 << 20),
                                  frames=len(ends), delivered_before_input_stopped=n, undelivered=und.value,
                                  median_ms=round(float(np.median(l)), 3) if n else None, p99_ms=round(float(np.percentile(l, 99)), 3) if n else None,
                                  max_ms=round(float(l.max()), 3) if n else None)), flush=True)


if __name__ == "__main__":
    main()
