"""Bounded soft Reed-Solomon decoding and its soft hand-over, sensitivity and cost (profiles/soft_rs_chain_sensitivity.txt): the legs
and the IQ of dev_soft_rs_sweep.py (same stream ids, so the first two columns repeat profiles/soft_rs_sensitivity.txt), valid payloads
with
  soft_decision alone | soft_rs (no bound) | soft_rs_fmax 0, 8, 16, 24 with the chain off | the same with soft_rs_chain on,
all with the soft header; then paydec_ms of one block of Reed-Solomon traffic at 20 dB and at 4 dB with soft_rs alone and with the
chain at fmax 0, 16, 32 (medians of --reps runs, same process).  A payload counts if it is valid and equal to the transmitted one."""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
fx = importlib.import_module("gr-liquiddsp_amd")
import dev_soft_rs_sweep as base                   # noqa: E402  (the legs' traffic: one definition)

FMAX = (0, 8, 16, 24)
COLUMNS = [("soft", dict()), ("soft_rs", dict(soft_rs=True))] + [("f%d" % f, dict(soft_rs=True, soft_rs_fmax=f)) for f in FMAX] + \
          [("f%d+c" % f, dict(soft_rs=True, soft_rs_fmax=f, soft_rs_chain=True)) for f in FMAX]


def every(xs, inj):
    res = []
    for _, kw in COLUMNS:
        ctx = fx.RxContext(len(xs), soft_header=True, soft_decision=True, **kw)
        res.append(base.valid_payloads(ctx.process(xs), inj))
        ctx.close()
    return res


def table(title, what, points, label, make):
    print(title)
    print("%-6s %-5s %-11s %5s   %s" % ("mod", what, "inner/outer", "sent", " ".join("%6s" % c for c, _ in COLUMNS)))
    for ms in (base.PSK4, base.QAM16):
        for i, (f0, f1) in enumerate(base.PAIRS):
            pts = points(ms, f0)
            xs, inj = [], []
            for j, p in enumerate(pts):
                x, fr = make(ms, i, f0, f1, j, p)
                xs.append(x); inj.append(fr)
            res = every(xs, inj)
            for j, p in enumerate(pts):
                print("%-6s %-5s %-11s %5d   %s" % ("psk4" if ms == base.PSK4 else "qam16", label % p, "%s/%s" % (base.NAMES[f0], base.NAMES[f1]), len(inj[j]),
                                                  " ".join("%6d" % r[j] for r in res)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=160_000, help="samples per stream and point")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--skip-cost", action="store_true")
    a = ap.parse_args()

    def awgn(ms, i, f0, f1, j, snr):
        return fx.synth_stream(a.samples, stream_id=int(100 * snr) + 1000 + 10 * i + ms, mod=ms, fec0=f0, fec1=f1, payload_len=base.PAYLOAD, snr_db=snr)

    def blank(ms, i, f0, f1, j, frac):
        npay = base.payload_samples(ms, f0)
        x, fr = fx.synth_stream(a.samples, stream_id=3000 + 100 * j + 10 * i + ms, mod=ms, fec0=f0, fec1=f1, payload_len=base.PAYLOAD, snr_db=20.0)
        rng = np.random.RandomState(77 + 100 * j + 10 * i + ms)
        span = int(round(frac * npay))
        for start, _ in fr:
            p = start + 2 * base.HEAD_SYMBOLS + int(rng.randint(0, npay - span))
            x[p:p + span] = 0
        return x, fr
    table("leg 1: AWGN", "snr", lambda ms, f0: base.SNRS[(ms, f0)], "%.1f", awgn)
    table("leg 2: blanking at 20 dB (one zeroed span inside every frame's payload)", "blank", lambda ms, f0: base.BLANK, "%.2f", blank)
    if a.skip_cost:
        return
    import torch
    legs = [("soft_rs", dict(soft_rs=True))] + [("chain fmax %d" % f, dict(soft_rs=True, soft_rs_fmax=f, soft_rs_chain=True)) for f in (0, 16, 32)]
    for snr in (20.0, 4.0):
        xs = [torch.from_numpy(fx.synth_stream(2_000_000, stream_id=90 + i, mod=base.PSK4, fec0=f0, fec1=base.RS, payload_len=base.PAYLOAD, snr_db=snr)[0]).cuda()
              for i, (f0, _) in enumerate(base.PAIRS)]
        ctxs = [fx.RxContext(2, soft_decision=True, **kw) for _, kw in legs]
        for c in ctxs:
            c.set_timing(2)
            c.process(xs)
        ms = [[] for _ in legs]
        for _ in range(a.reps):
            for k, c in enumerate(ctxs):
                c.reset()
                c.process(xs)
                ms[k].append(c.timing()["paydec_ms"])
        for k, (name, _) in enumerate(legs):
            v = np.array(ms[k])
            print("%g dB block (2 x 2e6 samples, rs alone + rs over v27, %d frames): %-13s paydec_ms median %.4f min %.4f max %.4f (%d runs)"
                  % (snr, ctxs[k].timing()["frames"], name, np.median(v), v.min(), v.max(), len(v)), flush=True)
        for c in ctxs:
            c.close()


if __name__ == "__main__":
    main()
