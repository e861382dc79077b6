"""Soft header sensitivity (profiles/soft_header_sensitivity.txt): frames sent / detected / valid headers / valid payloads over
0-5 dB for hard or soft header decoding crossed with hard or soft payload decoding, and walk_ms of a lone 20 dB block with the
soft header off and on.

Traffic: PSK4, V27, CRC-24, 64-byte payloads, random 14-byte user headers, CFO 0.01 rad/sample, random phase and fractional delay,
AWGN with sigma^2 = 10^(-snr/10) per complex sample (as synth_stream).  A detection counts if it lies within 64 samples of a
transmitted frame; a valid header or payload counts only if it is the transmitted one."""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
fx = importlib.import_module("gr-liquiddsp_amd")


def traffic(n_frames, snr_db, seed, payload_len=64, cfo=0.01, gap=256):
    rng = np.random.RandomState(seed)
    g = fx.FrameGen(2, 11, 1, 5)
    parts, sent, p = [np.zeros(1000, np.complex64)], [], 1000
    for _ in range(n_frames):
        hd = rng.randint(0, 256, 14).astype(np.uint8)
        pl = rng.randint(0, 256, payload_len).astype(np.uint8)
        fr = g.frame(pl, header=hd, dt=rng.uniform(-0.5, 0.5))
        parts += [fr, np.zeros(gap, np.complex64)]
        sent.append((p, hd.tobytes(), pl.tobytes()))
        p += len(fr) + gap
    g.close()
    x = np.concatenate(parts + [np.zeros(4000, np.complex64)])
    n = np.arange(len(x), dtype=np.float64)
    x = (x * np.exp(1j * (cfo * n + rng.uniform(-np.pi, np.pi)))).astype(np.complex64)
    x += (np.float32(np.sqrt(0.5 * 10.0 ** (-snr_db / 10.0))) * rng.standard_normal(2 * len(x)).astype(np.float32)).view(np.complex64)
    return x, sent


def score(frames, sent):
    starts = np.array([s[0] for s in sent])
    det, hv, pv = set(), set(), set()
    for f in frames:
        j = int(np.argmin(np.abs(starts - f["start"])))
        if abs(int(starts[j]) - f["start"]) >= 64:
            continue
        det.add(j)
        if f["header_valid"] and f["header"][:14] == sent[j][1]:
            hv.add(j)
            if f["payload_valid"] and f["payload"] == sent[j][2]:
                pv.add(j)
    return len(det), len(hv), len(pv)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    print("frames per point %d; PSK4 V27 CRC-24, 64-byte payloads, CFO 0.01, random user headers" % a.frames)
    print("%-6s %-13s %6s %9s %13s %15s" % ("snr", "header/payld", "sent", "detected", "valid_header", "valid_payload"))
    for snr in (0.0, 1.0, 2.0, 3.0, 4.0, 5.0):
        x, sent = traffic(a.frames, snr, 9000 + int(snr))
        for sh in (False, True):
            for sd in (False, True):
                ctx = fx.RxContext(1, soft_header=sh, soft_decision=sd)
                d, h, p = score(ctx.process([x]), sent)
                ctx.close()
                print("%-6.1f %-13s %6d %9d %13d %15d" % (snr, "%s/%s" % ("soft" if sh else "hard", "soft" if sd else "hard"), len(sent), d, h, p),
                      flush=True)
    # walk_ms of a lone block (one block in flight, all stage events on), soft header off / on alternated
    import torch
    xb, _ = fx.synth_stream(4_000_000, stream_id=0, snr_db=20.0)
    xd = torch.from_numpy(xb).cuda()
    ctxs = {sh: fx.RxContext(1, soft_header=sh) for sh in (False, True)}
    for c in ctxs.values():
        c.process([xd])
    ms = {False: [], True: []}
    for _ in range(a.reps):
        for sh, c in ctxs.items():
            c.reset()
            c.process([xd])
            ms[sh].append(c.timing()["walk_ms"])
    for sh in (False, True):
        v = np.array(ms[sh])
        print("20 dB lone block (4e6 samples, %d frames): soft_header=%d walk_ms median %.4f min %.4f max %.4f (%d runs)"
              % (ctxs[sh].timing()["frames"], sh, np.median(v), v.min(), v.max(), len(v)))
    print("soft header extra walk_ms (median): %+.4f" % (np.median(ms[True]) - np.median(ms[False])))


if __name__ == "__main__":
    main()
