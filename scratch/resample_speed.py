"""Speed of the resampler (DESIGN.md "Resampler"): DeviceResampler.resample host to host and the dia_resample launch alone, beside
the same filter as a torch strided conv1d over the FULL bank (torchaudio's formulation: one output channel per phase, stride o) on
the same GPU in the same run.  Host to host: a list of B arrays in, a list out (the conv1d column starts from one stacked [B, L]
array, which is what "from one [B, L] array" is for dia_resample); device: the launches alone, between two events.  1 x 5 s and 8 x 10 s, 48000 -> 44100 and 44100 -> 16000.

    python scratch/resample_speed.py > profiles/r13_resample_speed.txt
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "dia-tts-prune_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import resample_ref as R
from dia_hip import resample as S

DEV = torch.device("cuda:0")
REPS = 20


def median_ms(fn, reps=REPS):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ts))


def device_ms(fn, reps=REPS):
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


def conv_resample(x, f, o, n, width, m):
    """x [B, L] on the device -> [B, m]: pad, conv1d with the [n, 1, K] bank at stride o, interleave the phases"""
    xp = torch.nn.functional.pad(x[:, None, :], (width, width + o))
    y = torch.nn.functional.conv1d(xp, f, stride=o)
    return y.transpose(1, 2).reshape(x.shape[0], -1)[:, :m]


def main():
    dev = S.DeviceResampler(DEV)
    print(f"device: {torch.cuda.get_device_name(0)}; medians of {REPS} runs after 3 warm-up runs; times in ms")
    for rate_in, rate_out in ((48000, 44100), (44100, 16000)):
        plan = S.resample_plan(rate_in, rate_out)
        o, n, width, f64 = R.full_bank(rate_in, rate_out)
        f = torch.from_numpy(f64.astype(np.float32))[:, None, :].to(DEV)
        for B, secs in ((1, 5), (8, 10)):
            L = rate_in * secs
            m = plan.out_len(L)
            g = np.random.default_rng(0)
            rows = [g.uniform(-1, 1, size=L).astype(np.float32) for _ in range(B)]
            xh = np.stack(rows)
            xd = torch.from_numpy(xh).to(DEV)
            yd = torch.empty(B, m, dtype=torch.float32, device=DEV)
            zero, Ls, ms = [0] * B, [L] * B, [m] * B

            def native_host():
                return dev.resample(rows, rate_in, rate_out)

            def native_padded():
                return dev.resample_padded(xh, Ls, rate_in, rate_out)

            def native_launch():
                dev.launch(plan, xd, yd, zero, Ls, zero, ms, Ls)

            def conv_host():
                return conv_resample(torch.from_numpy(xh).to(DEV), f, o, n, width, m).cpu().numpy()

            def conv_launch():
                return conv_resample(xd, f, o, n, width, m)

            for fn in (native_host, native_padded, native_launch, conv_host, conv_launch):
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            got = np.stack(native_host())
            ref = conv_host()
            diff = float(np.abs(got - ref).max())
            print(f"{rate_in} -> {rate_out}  {B} x {secs} s  ({B * m} outputs, nt {plan.nt}, full K {f64.shape[1]}):  "
                  f"dia_resample host-to-host {median_ms(native_host):8.3f} (from one [B, L] array {median_ms(native_padded):8.3f})  device {device_ms(native_launch):7.4f}   |   "
                  f"torch conv1d host-to-host {median_ms(conv_host):8.3f}  device {device_ms(conv_launch):7.4f}   |   max |difference| {diff:.2e}")


if __name__ == "__main__":
    main()
