#!/usr/bin/env python3
"""Audio distance (dia_hip/spectral.py, csrc/spectral.hip): the default stft + mel metrics on 1 x 5 s and 8 x 10 s at 44.1 kHz, against
the same computation written with torch-ROCm ops (torch.stft + matmul + reductions, float32, on the same device).  Two figures
per side: device time of the launches (events around them, waveforms and plans resident) and host-to-host time (numpy in, Python
floats out).  Repetitions are interleaved: native, torch, native, torch, ...; the median is reported.

    python scratch/spectral_speed.py [--reps 7]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dia-tts-prune_amd"))

from dia_hip import spectral as S  # noqa: E402

RATE = 44100
DEV = torch.device("cuda:0")
SPECS = [(w, 0, 2, 1.0, 1.0) for w in S.STFT_DEFAULT["windows"]] + [(w, m, 1, 0.0, 1.0) for w, m in zip(S.MEL_DEFAULT["windows"], S.MEL_DEFAULT["n_mels"])]


def torch_terms(a, b, fbs, wins):
    """a, b fp32 [B, L] on the device -> [n_specs, B, 2] (mag_term, log_term)"""
    out = []
    for w, m, p, _, _ in SPECS:
        sa, sb = (torch.stft(x, n_fft=w, hop_length=w // 4, win_length=w, window=wins[w], center=True, pad_mode="constant", return_complex=True).abs().transpose(1, 2)
                  for x in (a, b))
        if m:
            sa, sb = sa @ fbs[(w, m)].T, sb @ fbs[(w, m)].T
        mag = (sa - sb).abs().mean(dim=(1, 2))
        log = (torch.log10(sa.clamp_min(S.EPS) ** p) - torch.log10(sb.clamp_min(S.EPS) ** p)).abs().mean(dim=(1, 2))
        out.append(torch.stack([mag, log], dim=1))
    return torch.stack(out)


def torch_distance(a, b, fbs, wins):
    t = torch_terms(a, b, fbs, wins).cpu().numpy().astype(np.float64)
    res = []
    for i in range(a.shape[0]):
        v = {"stft": 0.0, "mel": 0.0}
        for j, (w, m, p, mw, lw) in enumerate(SPECS):
            v["mel" if m else "stft"] += mw * t[j, i, 0] + lw * t[j, i, 1]
        res.append({"stft": v["stft"] / len(S.STFT_DEFAULT["windows"]), "mel": v["mel"] / len(S.MEL_DEFAULT["windows"])})
    return res


def timed_device(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def timed_host(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    dev = S.DeviceSpectral(DEV)
    wins = {w: torch.hann_window(w, periodic=True, dtype=torch.float32, device=DEV) for w, *_ in SPECS}
    fbs = {(w, m): torch.from_numpy(np.array(S.spectral_plan(w, RATE, m).fb32)).to(DEV) for w, m, *_ in SPECS if m}
    plans = [(S.spectral_plan(w, RATE, m), p) for w, m, p, _, _ in SPECS]
    props = torch.cuda.get_device_properties(0)
    print(f"device {props.name} ({getattr(props, 'gcnArchName', '?')}, {props.multi_processor_count} CUs); {len(SPECS)} resolutions (stft {S.STFT_DEFAULT['windows']}, mel {S.MEL_DEFAULT['windows']}); median of {args.reps}, interleaved")
    for B, secs in ((1, 5), (8, 10)):
        L = secs * RATE
        g = np.random.default_rng(B)
        a = [g.uniform(-1, 1, L).astype(np.float32) for _ in range(B)]
        b = [(x + 0.01 * g.uniform(-1, 1, L)).astype(np.float32) for x in a]
        da, db = dev._upload(a), dev._upload(b)
        parts = [torch.zeros(B, -(-S.n_frames(L, plan.window) // S.TILE_FRAMES), 2, dtype=torch.float64, device=DEV) for plan, _ in plans]

        def native_launches():
            for (plan, p), part in zip(plans, parts):
                dev.launch(plan, da, db, [L] * B, partial=part, power=p)

        native = dev.distance(a, b, RATE)                        # warms both sides, and the two must agree
        ref = torch_distance(da, db, fbs, wins)
        for i in range(B):
            for m in ("stft", "mel"):
                assert abs(native[i][m] - ref[i][m]) <= 1e-3 * abs(ref[i][m]), (i, m, native[i][m], ref[i][m])
        t = {k: [] for k in ("native device", "torch device", "native host", "torch host")}
        for _ in range(args.reps):
            t["native device"].append(timed_device(native_launches))
            t["torch device"].append(timed_device(lambda: torch_terms(da, db, fbs, wins)))
            t["native host"].append(timed_host(lambda: dev.distance(a, b, RATE)))
            t["torch host"].append(timed_host(lambda: torch_distance(torch.from_numpy(np.stack(a)).to(DEV), torch.from_numpy(np.stack(b)).to(DEV), fbs, wins)))
        med = {k: statistics.median(v) for k, v in t.items()}
        print(f"{B} x {secs} s: launches native {med['native device']:.3f} ms, torch {med['torch device']:.3f} ms (native / torch {med['native device'] / med['torch device']:.2f}); "
              f"host to host native {med['native host']:.3f} ms, torch {med['torch host']:.3f} ms (native / torch {med['native host'] / med['torch host']:.2f}); "
              f"stft {native[0]['stft']:.6f} mel {native[0]['mel']:.6f}")


if __name__ == "__main__":
    main()
