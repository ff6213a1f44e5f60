#!/usr/bin/env python3
"""Speed of the native codec (dia_hip/codec.py, csrc/codec.hip) at full size on synthetic weights, against the same network as
plain torch ops on torch-ROCm in fp32 (tests/codec_ref.py moved to the device).  Prints, per configuration, seconds of audio per
second, the time per frame and its ratio to the decode step's time per frame (README: 1 038 / 6 519 / 23 385 frames/s at batch
1 / 8 / 64), then the native path's time per layer shape.  --precision takes a comma list of decoder modes (fp32, bf16x2, bf16):
the modes' repetitions are interleaved (one of each per round), every mode is reported with its best, median and worst time and, in
bold, against the fp32 native path of the same run; the per-layer table is printed per mode.

    python scratch/codec_speed.py [--reps 3] [--no-torch] [--precision fp32,bf16x2,bf16]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "dia-tts-prune_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

from codec_ref import RefCodec, random_codes  # noqa: E402
from dia_hip import codec as K  # noqa: E402

DECODE_FPS = {1: 1038.0, 8: 6519.0, 64: 23385.0}
CASES = [(1, 860), (8, 860), (64, 430)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--window", type=int, default=128)
    ap.add_argument("--precision", type=str, default="fp32", help="comma list of fp32, bf16x2, bf16")
    args = ap.parse_args()
    modes = [m for m in args.precision.split(",") if m]
    dev = torch.device("cuda:0")
    cfg = K.CodecConfig()
    sd = K.synthetic_state_dict(cfg, seed=7)
    codecs = {m: K.DeviceCodec((cfg, sd), dev, window=args.window, precision=m) for m in modes}
    codec = codecs[modes[0]]
    print(f"codec_speed: full-size synthetic DAC decoder, window {codec.window} + 2 x {codec.ctx} context frames, "
          f"rows per pass <= {codec.rows_cap}, {torch.cuda.get_device_name(0)}")
    ref = None if args.no_torch else RefCodec(cfg, {k: v.to(dev) for k, v in sd.items()}, torch.float32)
    for B, T in CASES:
        rows = [random_codes(cfg, T, seed=100 + b) for b in range(B)]
        frames, audio_s = B * T, B * T * cfg.hop / cfg.sample_rate
        times = {m: [] for m in modes}
        outs_m = {}
        for m in modes:
            codecs[m].decode_batch(rows[:1])                                       # warm-up
        for _ in range(args.reps):                                                 # interleaved: one repetition of every mode per round
            for m in modes:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                outs_m[m] = codecs[m].decode_batch(rows)
                times[m].append(time.perf_counter() - t0)
        for m in modes:
            best, med, worst = min(times[m]), float(np.median(times[m])), max(times[m])
            line = (f"native {m:6s} {B:2d} x {T}: {best * 1e3:9.1f} ms (median {med * 1e3:.1f}, worst {worst * 1e3:.1f}, {len(times[m])} reps)  "
                    f"{audio_s / best:8.1f} s audio/s  {best / frames * 1e6:8.1f} us/frame  "
                    f"= {best / frames * DECODE_FPS[B]:6.2f} x the decode step's {1e6 / DECODE_FPS[B]:.1f} us/frame")
            if m != "fp32" and "fp32" in times:
                f32 = outs_m["fp32"][0].astype(np.float64)
                line += (f"  **{min(times['fp32']) / best:.2f} x the fp32 native path** (medians {float(np.median(times['fp32'])) / med:.2f} x); "
                         f"max |{m} - fp32| row 0 {float(np.abs(outs_m[m][0] - f32).max()):.2e}")
            print(line, flush=True)
        best, y = min(times[modes[0]]), outs_m[modes[0]]
        if ref is None:
            continue
        try:
            c = torch.from_numpy(np.stack(rows)).to(dev)
            tb = 1e30
            with torch.no_grad():
                for rep in range(args.reps + 1):                                    # the first run carries MIOpen's search
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    outs = [ref.decoder(ref.from_codes(c[b0:b0 + 8])).cpu() for b0 in range(0, B, 8)]
                    torch.cuda.synchronize()
                    if rep:
                        tb = min(tb, time.perf_counter() - t0)
            err = float(np.abs(outs[0][0, 0].numpy() - y[0]).max())
            print(f"torch         {B:2d} x {T}: {tb * 1e3:9.1f} ms  {audio_s / tb:8.1f} s audio/s  {tb / frames * 1e6:8.1f} us/frame  "
                  f"(whole utterances, 8 rows per pass; native {modes[0]} / torch time {best / tb:.2f}; max |native {modes[0]} - torch| row 0 {err:.2e})", flush=True)
        except Exception as e:                                                     # a layer MIOpen will not run
            print(f"torch         {B:2d} x {T}: failed: {type(e).__name__}: {str(e)[:300]}", flush=True)
    # per layer: one pass of 8 x 128-frame windows
    rows = [random_codes(cfg, 128, seed=b) for b in range(8)]
    per = {}
    for m in modes:
        codecs[m].decode_batch(rows)
    for _ in range(args.reps):                                                     # interleaved; the smallest time of every launch
        for m in modes:
            codecs[m].layer_events = []
            codecs[m].decode_batch(rows)
            torch.cuda.synchronize()
            ms = [(label, a.elapsed_time(b)) for label, a, b in codecs[m].layer_events]
            per[m] = ms if m not in per else [(l, min(t, u)) for (l, t), (_, u) in zip(ms, per[m])]
            codecs[m].layer_events = None
    print(f"native per launch, 8 rows x 128 frames (one window each, no context), ms, best of {args.reps}: " + " | ".join(modes))
    for i, (label, _) in enumerate(per[modes[0]]):
        print(f"  {label:28s} " + " | ".join(f"{per[m][i][1]:8.3f}" for m in modes))
    for m in modes:
        tot = sum(t for _, t in per[m])
        print(f"  total {m:6s} {tot:.3f} ms = {tot / (8 * 128) * 1e3:.1f} us/frame")


if __name__ == "__main__":
    main()
