"""Speed of the loudness meter (DESIGN.md "Loudness"): the device time of dia_loudness's launches (between two events; samples,
table and bank already on the device) for 1 x 5 s, 8 x 10 s, 64 x 10 s and 1 x 30 s of 44.1 kHz audio, beside the same quantities
from torch-ROCm ops on the same GPU in the same run (repetitions interleaved, one of each per round).

torch, measure: torch has no recursive filter, so the K-weighting is applied in the frequency domain (rfft of the zero-padded row,
times the cascade's response, irfft: the recursion's output up to the padding), squared and summed per step in float64; the true
peak is one conv1d with the four phases of the same bank, abs, max.  torch, apply: (x.double() * g).float().

    python scratch/loudness_speed.py > profiles/r23_loudness_speed.txt
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "dia-tts-prune_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

from dia_hip import loudness as S

DEV = torch.device("cuda:0")
RATE = 44100
REPS = 7


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def torch_measure(xd, plan, H, kern, pad):
    B, N = xd.shape
    X = torch.fft.rfft(xd.double(), n=H.shape[0] * 2 - 2)
    y = torch.fft.irfft(X * H)[:, :N]
    ns = N // plan.step
    steps = (y[:, :ns * plan.step] ** 2).reshape(B, ns, plan.step).sum(dim=2)
    up = F.conv1d(F.pad(xd, pad)[:, None, :], kern)                            # [B, 4, N]
    return steps, torch.maximum(up.abs().amax(dim=(1, 2)), xd.abs().amax(dim=1))


def main():
    dev = S.DeviceLoudness(DEV)
    plan = S.loudness_plan(RATE)
    lo, hi = int(min(plan.first)), int(max(plan.first)) + plan.nt - 1
    kern = torch.zeros(4, 1, hi - lo + 1, device=DEV)
    for p in range(4):                                                         # conv1d correlates: tap k of phase p sits at first[p] + k - lo
        kern[p, 0, int(plan.first[p]) - lo:int(plan.first[p]) - lo + plan.nt] = torch.from_numpy(np.array(plan.bank32[p])).to(DEV)
    print(f"device: {torch.cuda.get_device_name(0)}; best / median of {REPS} interleaved rounds after 2 warm-up rounds; times in ms; "
          f"step {plan.step}, chunk {plan.chunk} x {plan.chunks}")
    for B, secs in ((1, 5), (8, 10), (64, 10), (1, 30)):
        N = RATE * secs
        g = np.random.default_rng(0)
        xd = torch.from_numpy((0.1 * g.standard_normal((B, N))).astype(np.float32)).to(DEV)
        nfft = 1 << int(np.ceil(np.log2(N + RATE)))                            # a second of decay for the 38 Hz high-pass
        w = torch.exp(-2j * np.pi * torch.arange(nfft // 2 + 1, dtype=torch.float64, device=DEV) / nfft)
        c = [float(v) for v in plan.coef]
        H = ((c[0] + c[1] * w + c[2] * w * w) / (1 + c[3] * w + c[4] * w * w)) * ((c[5] + c[6] * w + c[7] * w * w) / (1 + c[8] * w + c[9] * w * w))
        ns = N // plan.step
        steps = torch.zeros(B, ns, dtype=torch.float64, device=DEV)
        peaks = torch.zeros(B, 2, dtype=torch.float32, device=DEV)
        ws = torch.empty(S.ws_doubles(B, ns, plan.chunks), dtype=torch.float64, device=DEV)
        yd = torch.empty(B, N, dtype=torch.float32, device=DEV)
        lens, zero, gains = [N] * B, [0] * B, [0.5] * B
        fns = {
            "measure": lambda: dev.launch_measure(plan, xd, lens, steps, peaks, ws),
            "measure-torch": lambda: torch_measure(xd, plan, H, kern, (-lo, hi)),
            "apply": lambda: dev.launch_apply(xd, yd, lens, zero, lens, gains),
            "apply-torch": lambda: (xd.double() * 0.5).float(),
        }
        ts = {k: [] for k in fns}
        for r in range(REPS + 2):
            for k, fn in fns.items():
                t = timed(fn)
                if r >= 2:
                    ts[k].append(t)
        st, pk = torch_measure(xd, plan, H, kern, (-lo, hi))
        agree = float(((st - steps).abs() / steps).max())
        agree_pk = float((pk - peaks[:, 1]).abs().max())
        s = {k: (min(v), float(np.median(v))) for k, v in ts.items()}
        print(f"{B} x {secs} s: {ns} steps per row  |  measure {s['measure'][0]:8.4f} / {s['measure'][1]:8.4f}   torch rfft + conv1d "
              f"{s['measure-torch'][0]:8.4f} / {s['measure-torch'][1]:8.4f}  (native / torch {s['measure'][1] / s['measure-torch'][1]:.2f}; step sums "
              f"differ by {agree:.1e} relative, true peaks by {agree_pk:.1e})  |  apply {s['apply'][0]:8.4f} / {s['apply'][1]:8.4f}   torch "
              f"{s['apply-torch'][0]:8.4f} / {s['apply-torch'][1]:8.4f}  (native / torch {s['apply'][1] / s['apply-torch'][1]:.2f})", flush=True)


if __name__ == "__main__":
    main()
