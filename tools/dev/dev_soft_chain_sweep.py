"""Soft chain sensitivity (profiles/soft_chain_sensitivity.txt): valid payloads per SNR with hard payload decoding, soft decoding of
the convolutional stages only (soft_decision), soft block decoding on top (soft_block) and soft values carried from the block
decoder into the Viterbi decoder on top of that (soft_chain), all with the soft header; then paydec_ms of one 20 dB block of
Hamming(12,8) and Golay over V27 traffic with soft_chain off and on.

Traffic: synth_stream (random payloads, CRC-24, 64-byte payloads), PSK4 and QAM16, inner code V27, outer code Hamming(7,4),
Hamming(12,8), Golay(24,12) or SECDED(72,64), one stream per outer code, the streams of tools/dev/dev_block_soft_sweep.py (same
ids).  A payload counts if it is valid and equal to the transmitted one."""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
fx = importlib.import_module("gr-liquiddsp_amd")

PSK4, QAM16 = 2, 27
NONE, V27, H74, H128, GOLAY, SD72 = 1, 11, 4, 6, 7, 10
NAMES = {NONE: "none", V27: "v27", H74: "h74", H128: "h128", GOLAY: "golay", SD72: "sd72"}
PAIRS = [(f0, f1) for f0 in (NONE, V27) for f1 in (H74, H128, GOLAY, SD72)]      # (stream ids count over all eight; the V27 ones run)
SNRS = {PSK4: [0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0], QAM16: [5.0, 6.0, 7.0, 8.0, 9.0, 10.0, 11.0]}
SETTINGS = [("hard", dict()), ("soft", dict(soft_decision=True)), ("soft_block", dict(soft_decision=True, soft_block=True)),
            ("soft_chain", dict(soft_decision=True, soft_block=True, soft_chain=True))]


def valid_payloads(frames, injected):
    sent = [set(p for _, p in inj) for inj in injected]
    n = [0] * len(injected)
    for f in frames:
        if f["payload_valid"] and f["payload"] in sent[f["stream"]]:
            n[f["stream"]] += 1
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=160_000, help="samples per stream and point")
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    print("%-6s %-5s %-11s %5s   %s" % ("mod", "snr", "inner/outer", "sent", "valid payloads: hard / soft / soft_block / soft_chain"))
    for ms in (PSK4, QAM16):
        for snr in SNRS[ms]:
            xs, inj = [], []
            for i, (f0, f1) in enumerate(PAIRS):
                if f0 != V27:
                    continue
                x, fr = fx.synth_stream(a.samples, stream_id=int(100 * snr) + 10 * i + ms, mod=ms, fec0=f0, fec1=f1, payload_len=64, snr_db=snr)
                xs.append(x); inj.append(fr)
            res = []
            for _, kw in SETTINGS:
                ctx = fx.RxContext(len(xs), soft_header=True, **kw)
                res.append(valid_payloads(ctx.process(xs), inj))
                ctx.close()
            for i, (f0, f1) in enumerate(p for p in PAIRS if p[0] == V27):
                print("%-6s %-5.1f %-11s %5d   %4d %4d %4d %4d" % ("psk4" if ms == PSK4 else "qam16", snr, "%s/%s" % (NAMES[f0], NAMES[f1]),
                                                                len(inj[i]), res[0][i], res[1][i], res[2][i], res[3][i]), flush=True)
    # paydec_ms of one 20 dB block (2 streams of 2e6 samples: PSK4, Hamming(12,8) and Golay outer codes over V27)
    import torch
    xs = [torch.from_numpy(fx.synth_stream(2_000_000, stream_id=70 + i, mod=PSK4, fec0=V27, fec1=f1, payload_len=64, snr_db=20.0)[0]).cuda()
          for i, f1 in enumerate((H128, GOLAY))]
    ctxs = {sb: fx.RxContext(2, soft_decision=True, soft_block=True, soft_chain=sb) for sb in (False, True)}
    for c in ctxs.values():
        c.set_timing(2)
        c.process(xs)
    ms = {False: [], True: []}
    for _ in range(a.reps):
        for sb, c in ctxs.items():
            c.reset()
            c.process(xs)
            ms[sb].append(c.timing()["paydec_ms"])
    for sb in (False, True):
        v = np.array(ms[sb])
        print("20 dB block (2 x 2e6 samples, h128 + golay over v27, %d frames): soft_block=1 soft_chain=%d paydec_ms median %.4f min %.4f max %.4f (%d runs)"
              % (ctxs[sb].timing()["frames"], sb, np.median(v), v.min(), v.max(), len(v)))
    print("soft_chain extra paydec_ms (median): %+.4f" % (np.median(ms[True]) - np.median(ms[False])))


if __name__ == "__main__":
    main()
