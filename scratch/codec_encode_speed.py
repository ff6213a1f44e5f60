#!/usr/bin/env python3
"""Speed of the native codec's encode side (dia_hip/codec.py, csrc/codec.hip) at full size on synthetic weights, host to host
(float samples in host memory -> int64 codes in host memory), against the same network as plain torch ops on torch-ROCm in fp32
(tests/codec_enc_ref.py moved to the device, whole utterances).  Prints, per configuration, seconds of audio per second and the
time per frame, then the native path's time per layer class.

    python scratch/codec_encode_speed.py [--reps 3] [--no-torch]
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

from codec_enc_ref import RefEncoder, make_wave, whole_state  # noqa: E402
from dia_hip import codec as K  # noqa: E402

CASES = [(1, 5.0), (8, 10.0)]                                                      # rows x seconds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--window", type=int, default=128)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = K.CodecConfig()
    sd = whole_state(cfg, 7)
    codec = K.DeviceCodec((cfg, sd), dev, window=args.window)
    print(f"codec_encode_speed: full-size synthetic DAC encoder + RVQ search, window {codec.window} + 2 x {codec.enc_ctx} context frames, "
          f"rows per pass <= {codec.enc_rows_cap}, {torch.cuda.get_device_name(0)}")
    ref = None if args.no_torch else RefEncoder(cfg, {k: v.to(dev) for k, v in sd.items()}, torch.float32)
    for B, secs in CASES:
        rows = [make_wave(int(secs * cfg.sample_rate), seed=100 + b) for b in range(B)]
        frames = sum(-(-r.shape[0] // cfg.hop) for r in rows)
        audio_s = B * secs
        codec.encode_batch(rows[:1])                                               # warm-up
        best = 1e30
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = codec.encode_batch(rows)
            best = min(best, time.perf_counter() - t0)
        print(f"native  {B} x {secs:.0f} s: {best * 1e3:9.1f} ms  {audio_s / best:8.1f} s audio/s  {best / frames * 1e6:8.1f} us/frame", flush=True)
        if ref is None:
            continue
        try:
            tb = 1e30
            with torch.no_grad():
                for rep in range(args.reps + 1):                                    # the first run carries MIOpen's search
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    x = torch.stack([ref.preprocess(r)[0] for r in rows]).to(dev)
                    codes = ref.quantize(ref.encoder(x))[0].cpu()
                    torch.cuda.synchronize()
                    if rep:
                        tb = min(tb, time.perf_counter() - t0)
            same = float((codes[0].numpy() == got[0]).mean())
            print(f"torch   {B} x {secs:.0f} s: {tb * 1e3:9.1f} ms  {audio_s / tb:8.1f} s audio/s  {tb / frames * 1e6:8.1f} us/frame  "
                  f"(whole utterances in one pass; native / torch time {best / tb:.2f}; codes of row 0 equal at {100 * same:.1f} % of (stage, frame))", flush=True)
        except Exception as e:                                                     # a layer MIOpen will not run, or memory
            print(f"torch   {B} x {secs:.0f} s: failed: {type(e).__name__}: {str(e)[:300]}", flush=True)
    # per layer class: one pass of 8 x 128-frame rows (one window each, no context)
    rows = [make_wave(128 * cfg.hop, seed=b) for b in range(8)]
    codec.encode_batch(rows)
    codec.layer_events = []
    codec.encode_batch(rows)
    torch.cuda.synchronize()
    klass = {}
    for label, a, b in codec.layer_events:
        kind, _, rest = label.partition(" ")
        key = "quantize" if kind == "quantize" else ("strided k 2s" if kind == "convs" else ("k 3" if kind == "conv3" else f"conv {rest.split()[1]}" + (" (1 -> d)" if rest.startswith("1->") else "")))
        klass[key] = klass.get(key, 0.0) + a.elapsed_time(b)
    tot = sum(klass.values())
    print("native per layer class, 8 rows x 128 frames (device time between events):")
    for key, ms in sorted(klass.items(), key=lambda kv: -kv[1]):
        print(f"  {key:22s} {ms:9.3f} ms  {100 * ms / tot:5.1f} %")
    print(f"  total {tot:.3f} ms = {tot / (8 * 128) * 1e3:.1f} us/frame")
    codec.layer_events = None


if __name__ == "__main__":
    main()
