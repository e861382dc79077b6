"""Soft Reed-Solomon sensitivity (profiles/soft_rs_sensitivity.txt): valid payloads with soft payload decoding alone (soft_decision)
and with generalized-minimum-distance Reed-Solomon decoding on top (soft_rs), the same IQ for both, all with the soft header; then
paydec_ms of one block of Reed-Solomon traffic at 20 dB and at 4 dB with soft_rs off and on (medians of --reps runs).

Leg 1, AWGN across the waterfall: synth_stream (random payloads, CRC-24, 64-byte payloads), PSK4 and QAM16, Reed-Solomon alone
(fec0 none, fec1 RS) and Reed-Solomon over V27 (fec0 V27, fec1 RS).
Leg 2, blanking: the same traffic at 20 dB with one span of samples zeroed inside every frame's payload, 2 .. 12 % of the payload's
samples, at a position drawn per frame (seeded).
A payload counts if it is valid and equal to the transmitted one."""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
fx = importlib.import_module("gr-liquiddsp_amd")

PSK4, QAM16 = 2, 27
NONE, V27, RS = 1, 11, 27
NAMES = {NONE: "none", V27: "v27", RS: "rs"}
BPS = {PSK4: 2, QAM16: 4}
PAIRS = [(NONE, RS), (V27, RS)]
SNRS = {(PSK4, NONE): [2.0, 3.0, 3.5, 4.0, 4.5, 5.0, 6.0], (PSK4, V27): [-1.0, 0.0, 1.0, 2.0, 3.0, 4.0, 5.0],
        (QAM16, NONE): [8.0, 9.0, 10.0, 10.5, 11.0, 12.0, 13.0], (QAM16, V27): [5.0, 6.0, 7.0, 8.0, 9.0, 10.0, 11.0]}
BLANK = [0.02, 0.03, 0.05, 0.08, 0.12]
PAYLOAD, CRC_BYTES = 64, 3
HEAD_SYMBOLS = 64 + 231                       # preamble and header in front of the payload, 2 samples a symbol


def payload_samples(ms, fec0):
    k = PAYLOAD + CRC_BYTES
    l0 = k if fec0 == NONE else (2 * (8 * k + 6) + 7) // 8
    return 2 * ((8 * (l0 + 32) + BPS[ms] - 1) // BPS[ms])


def valid_payloads(frames, injected):
    sent = [set(p for _, p in inj) for inj in injected]
    n = [0] * len(injected)
    for f in frames:
        if f["payload_valid"] and f["payload"] in sent[f["stream"]]:
            n[f["stream"]] += 1
    return n


def both(xs, inj):
    res = []
    for on in (False, True):
        ctx = fx.RxContext(len(xs), soft_header=True, soft_decision=True, soft_rs=on)
        res.append(valid_payloads(ctx.process(xs), inj))
        ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=160_000, help="samples per stream and point")
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    print("leg 1: AWGN")
    print("%-6s %-5s %-11s %5s   %s" % ("mod", "snr", "inner/outer", "sent", "valid payloads: soft / soft_rs"))
    for ms in (PSK4, QAM16):
        for i, (f0, f1) in enumerate(PAIRS):
            xs, inj = [], []
            for snr in SNRS[(ms, f0)]:
                x, fr = fx.synth_stream(a.samples, stream_id=int(100 * snr) + 1000 + 10 * i + ms, mod=ms, fec0=f0, fec1=f1, payload_len=PAYLOAD, snr_db=snr)
                xs.append(x); inj.append(fr)
            res = both(xs, inj)
            for j, snr in enumerate(SNRS[(ms, f0)]):
                print("%-6s %-5.1f %-11s %5d   %4d %4d" % ("psk4" if ms == PSK4 else "qam16", snr, "%s/%s" % (NAMES[f0], NAMES[f1]), len(inj[j]),
                                                          res[0][j], res[1][j]), flush=True)
    print("leg 2: blanking at 20 dB (one zeroed span inside every frame's payload)")
    print("%-6s %-5s %-11s %5s   %s" % ("mod", "blank", "inner/outer", "sent", "valid payloads: soft / soft_rs"))
    for ms in (PSK4, QAM16):
        for i, (f0, f1) in enumerate(PAIRS):
            xs, inj = [], []
            npay = payload_samples(ms, f0)
            for j, frac in enumerate(BLANK):
                x, fr = fx.synth_stream(a.samples, stream_id=3000 + 100 * j + 10 * i + ms, mod=ms, fec0=f0, fec1=f1, payload_len=PAYLOAD, snr_db=20.0)
                rng = np.random.RandomState(77 + 100 * j + 10 * i + ms)
                span = int(round(frac * npay))
                for start, _ in fr:
                    p = start + 2 * HEAD_SYMBOLS + int(rng.randint(0, npay - span))
                    x[p:p + span] = 0
                xs.append(x); inj.append(fr)
            res = both(xs, inj)
            for j, frac in enumerate(BLANK):
                print("%-6s %-5.2f %-11s %5d   %4d %4d" % ("psk4" if ms == PSK4 else "qam16", frac, "%s/%s" % (NAMES[f0], NAMES[f1]), len(inj[j]),
                                                          res[0][j], res[1][j]), flush=True)
    # paydec_ms of one block (2 streams of 2e6 samples: PSK4, Reed-Solomon alone and over V27): at 20 dB, where every block is a
    # codeword and no trial runs, and at 4 dB, where the blocks of the first stream have errors and all 17 trials run
    import torch
    for snr in (20.0, 4.0):
        xs = [torch.from_numpy(fx.synth_stream(2_000_000, stream_id=90 + i, mod=PSK4, fec0=f0, fec1=RS, payload_len=PAYLOAD, snr_db=snr)[0]).cuda()
              for i, (f0, _) in enumerate(PAIRS)]
        ctxs = {on: fx.RxContext(2, soft_decision=True, soft_rs=on) for on in (False, True)}
        for c in ctxs.values():
            c.set_timing(2)
            c.process(xs)
        ms = {False: [], True: []}
        for _ in range(a.reps):
            for on, c in ctxs.items():
                c.reset()
                c.process(xs)
                ms[on].append(c.timing()["paydec_ms"])
        for on in (False, True):
            v = np.array(ms[on])
            print("%g dB block (2 x 2e6 samples, rs alone + rs over v27, %d frames): soft_decision=1 soft_rs=%d paydec_ms median %.4f min %.4f max %.4f (%d runs)"
                  % (snr, ctxs[on].timing()["frames"], on, np.median(v), v.min(), v.max(), len(v)))
        print("%g dB: soft_rs extra paydec_ms (median): %+.4f" % (snr, np.median(ms[True]) - np.median(ms[False])))
        for c in ctxs.values():
            c.close()

if __name__ == "__main__":
    main()
