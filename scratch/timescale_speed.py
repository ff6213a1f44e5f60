"""Speed of the speed factor (DESIGN.md "Speed factor"): the device time of dia_timescale's launches (between two events; input,
window and centres already on the device) for 1 x 5 s, 8 x 10 s and 1 x 30 s of 44.1 kHz audio, both modes, speeds 0.8 / 0.94 /
1.25, beside the same computation as torch-ROCm ops on the same GPU in the same run (repetitions interleaved, one of each per
round) and the native codec's decode time (host to host, fp32) for the same audio.

torch, interp: F.interpolate(mode="linear", align_corners=True), which is the same positions in fp32.  torch, wsola: per frame a
gather of the template at the previous frame's offset, one grouped conv1d of the candidate span with it, argmax; the offsets stay
on the device.  Its tie rule is argmax's (the first maximum), and the overlap-add is not included: it is the search alone against
search + overlap-add.

    python scratch/timescale_speed.py > profiles/r22_timescale_speed.txt
"""
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "dia-tts-prune_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

from codec_ref import random_codes
from dia_hip import codec as K
from dia_hip import timescale as S

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


def torch_search(xp, plan, F_, off):
    """xp [B, off + N + off] zero-padded on the device -> delta int64 [B, F_] on the device"""
    B, W, D, Hs = xp.shape[0], plan.window, plan.tolerance, plan.hop
    cs = [plan.centre(k) for k in range(F_)]
    ar = torch.arange(W, device=xp.device)[None, :]
    delta = torch.zeros(B, F_, dtype=torch.int64, device=xp.device)
    prev = torch.zeros(B, 1, dtype=torch.int64, device=xp.device)
    for k in range(1, F_):
        t = torch.gather(xp, 1, off + cs[k - 1] + prev + ar)                   # [B, W]
        a = off + cs[k] - D - Hs
        corr = F.conv1d(xp[None, :, a:a + W + 2 * D], t[:, None, :], groups=B)[0]          # [B, 2 D + 1]
        prev = corr.argmax(dim=1, keepdim=True) - D
        delta[:, k] = prev[:, 0]
    return delta


def main():
    dev = S.DeviceTimescale(DEV)
    cfg = K.CodecConfig()
    codec = K.DeviceCodec((cfg, K.synthetic_state_dict(cfg, seed=7)), DEV)
    print(f"device: {torch.cuda.get_device_name(0)}; best / median of {REPS} interleaved rounds after 2 warm-up rounds; times in ms; "
          f"window 1024, tolerance 512")
    for B, secs in ((1, 5), (8, 10), (1, 30)):
        N = RATE * secs
        g = np.random.default_rng(0)
        # band-limited noise, so that the search has something to align
        rows = [np.convolve(g.standard_normal(N + 63), np.hanning(64) / 32.0, mode="valid").astype(np.float32) for _ in range(B)]
        xd = torch.from_numpy(np.stack(rows)).to(DEV)
        T = N // cfg.hop
        codes = [random_codes(cfg, T, seed=100 + b) for b in range(B)]
        codec.decode_batch(codes[:1])
        ct = []
        for _ in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            codec.decode_batch(codes)
            ct.append((time.perf_counter() - t0) * 1e3)
        print(f"{B} x {secs} s: native codec decode (fp32, host to host) of {B} x {T} frames: {min(ct):.1f} ms", flush=True)
        for speed in (0.8, 0.94, 1.25):
            pi, pw = S.TimescalePlan(speed, "interp"), S.TimescalePlan(speed, "wsola")
            M = pi.out_len(N)
            F_ = pw.frames(M)
            yd = torch.empty(B, M, dtype=torch.float32, device=DEV)
            zero, Ns, Ms, Fs = [0] * B, [N] * B, [M] * B, [F_] * B
            centre = torch.from_numpy(np.tile(np.concatenate([[0], pw.centres(0, F_)]).astype(np.int32), (B, 1))).to(DEV)
            delta = torch.zeros(B, F_, dtype=torch.int32, device=DEV)
            off = pw.window + pw.tolerance
            xp = F.pad(xd, (off, off + 2 * pw.window))

            fns = {
                "interp": lambda: dev.launch_interp(xd, yd, zero, Ns, zero, Ms, Ns, Ms),
                "interp-torch": lambda: F.interpolate(xd[:, None, :], size=M, mode="linear", align_corners=True),
                "wsola": lambda: dev.launch_wsola(pw, xd, yd, centre, delta, zero, Ns, zero, Fs, zero, zero, Ms, Ns),
                "wsola-torch": lambda: torch_search(xp, pw, F_, off),
            }
            ts = {k: [] for k in fns}
            for r in range(REPS + 2):
                for k, fn in fns.items():
                    t = timed(fn)
                    if r >= 2:
                        ts[k].append(t)
            agree = float((torch_search(xp, pw, F_, off) == delta.long()).float().mean())
            s = {k: (min(v), float(np.median(v))) for k, v in ts.items()}
            print(f"{B} x {secs} s  speed {speed}: {M} outputs, {F_} frames per row  |  "
                  f"interp {s['interp'][0]:8.4f} / {s['interp'][1]:8.4f}   torch F.interpolate {s['interp-torch'][0]:8.4f} / {s['interp-torch'][1]:8.4f}  "
                  f"(native / torch {s['interp'][1] / s['interp-torch'][1]:.2f})  |  "
                  f"wsola search + overlap-add {s['wsola'][0]:9.3f} / {s['wsola'][1]:9.3f}   torch conv1d + argmax search {s['wsola-torch'][0]:9.3f} / "
                  f"{s['wsola-torch'][1]:9.3f}  (native / torch {s['wsola'][1] / s['wsola-torch'][1]:.2f}; offsets equal in {agree:.3f} of the frames)  |  "
                  f"wsola / codec decode {s['wsola'][1] / min(ct):.3f}", flush=True)


if __name__ == "__main__":
    main()
