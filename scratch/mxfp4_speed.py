"""scratch/mxfp8_speed.py for the MXFP4 streams.
Decode speed of the MXFP4-quantised synthetic Dia-1.6B (synthetic_state_dict(seed=1234) -> mxfp4_quantize_state_dict): ONE
DeviceWeights(quant="mxfp4") holds the dense tiles and the MXFP4 streams of the same numbers; the knob mxfp4 picks per session
what the step streams (0 = dense tiles everywhere on the same checkpoint = the step without the feature, 0x7f7f = every class as MXFP4), so the A/B
runs in one process, interleaved, REPS times.  Batch 1 and batch 8 with mixed text lengths (32..512), K/V bf16 and f32.
Frames/s = decode steps x batch per second (graph replay).  Then per launch class the in-step time of one eager step
(dia_engine_time_step intervals: end of the previous launch -> end of this one, what rocprofv3 --kernel-trace reports as a
kernel's duration in a replayed graph), mean over the 18 layers and TS steps, per repetition.
  python scratch/mxfp4_speed.py [steps] [mask]     (mask: the MXFP4 side of the A/B, default 0x7f7f)
  python scratch/mxfp4_speed.py drift              (oracle on the synthetic checkpoint vs oracle on its quantised copy: recorded only,
                                                    synthetic weights say nothing about audio quality)
  rocprofv3 --kernel-trace --stats ... -- python scratch/mxfp4_speed.py prof BATCH MASK    (256 replayed steps of one session)"""
import sys, time
from collections import defaultdict
sys.path.insert(0, "dia-tts-prune_amd")
sys.path.insert(0, ".")
import numpy as np
import torch
from dia_hip import binding as hb
from dia_hip import config as C
from dia_hip.engine import DecodeSession, DeviceWeights
from dia_hip.quant import mxfp4_quantize_state_dict
from dia_hip.tokens import effective_text, encode_text, synthetic_text
from dia_hip.weights import synthetic_state_dict
TEXT = "[S1] Dia is an open weights text to dialogue model. [S2] You get full control over scripts and voices."
cfg = C.dia_1_6b_config()
if len(sys.argv) > 1 and sys.argv[1] == "drift":
    from oracle import dia_oracle as O
    torch.set_num_threads(16)
    sd = synthetic_state_dict(cfg, seed=1234, std=0.02)
    qsd = mxfp4_quantize_state_dict(cfg, sd)
    dm = O.Dims.of(cfg); mt = 5
    nz = O.exp_noise(42, mt - 1, dm.C, dm.tgt_vocab)
    a = O.generate(sd, cfg, TEXT, max_tokens=mt, noise=nz, mirror=False)
    b = O.generate(qsd, cfg, TEXT, max_tokens=mt, noise=nz, mirror=False)     # (free-running: steps after a differing sample diverge)
    for i in range(min(len(a.logits), len(b.logits))):
        d = np.abs(np.asarray(a.logits[i]) - np.asarray(b.logits[i]))
        print(f"step {i}: max |logit| {np.abs(np.asarray(a.logits[i])).max():.4f}, quantised - original: max {d.max():.4e}, rms {np.sqrt((d ** 2).mean()):.4e}, "
              f"samples equal {np.array_equal(a.preds[i], b.preds[i])}", flush=True)
    sys.exit(0)
dev = torch.device("cuda:0")
if len(sys.argv) > 3 and sys.argv[1] == "prof":
    B, mask = int(sys.argv[2]), int(sys.argv[3], 0)
    sd = mxfp4_quantize_state_dict(cfg, synthetic_state_dict(cfg, seed=1234, std=0.02, device=dev))
    w = DeviceWeights(cfg, sd, dev, quant="mxfp4")
    ids = [encode_text(effective_text(synthetic_text(L, cfg)), cfg) for L in (32, 64, 96, 128, 192, 256, 384, 512)][:B] if B > 1 else [encode_text(effective_text(TEXT), cfg)]
    hb.set_tuning("mxfp4", mask)
    s = DecodeSession(w, ids, kv_dtype="bf16", max_tokens=300, seeds=list(range(B)), ignore_eos=True)
    s.prefill(); s.sync()
    s.decode(256, True); s.sync()
    s.close()
    sys.exit(0)
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
MASK = int(sys.argv[2], 0) if len(sys.argv) > 2 else 0x7f7f
REPS, TS = 3, 4
sd = mxfp4_quantize_state_dict(cfg, synthetic_state_dict(cfg, seed=1234, std=0.02, device=dev))
ids1 = [encode_text(effective_text(TEXT), cfg)]
ids8 = [encode_text(effective_text(synthetic_text(L, cfg)), cfg) for L in (32, 64, 96, 128, 192, 256, 384, 512)]
w = DeviceWeights(cfg, sd, dev, quant="mxfp4")
del sd
NAMES = ["qkv", "attn_self", "o", "cq", "attn_cross", "co", "wi", "wo"]
CLS = ("qkv", "o", "cq", "co", "wi", "wo", "logits")
L = cfg.model.decoder.n_layer
for kv in ("bf16", "f32"):
    for ids in (ids1, ids8):
        B = len(ids)
        for rep in range(REPS):
            row = {}
            for tag, mask in (("dense", 0), ("mxfp4", MASK)):
                hb.set_tuning("mxfp4", mask)
                s = DecodeSession(w, ids, kv_dtype=kv, max_tokens=steps + 40 + TS, seeds=list(range(B)), ignore_eos=True)
                s.prefill(); s.sync()
                s.decode(16, True); s.sync()
                t0 = time.time(); s.decode(steps, True); s.sync(); dt = time.time() - t0
                print(f"K/V {kv:4s} batch {B} rep {rep} {tag:5s} (mask {mask:#06x}): decode {steps * B / dt:7.1f} frames/s ({dt / steps * 1e3:.3f} ms/step), "
                      f"weights {w.decode_weight_bytes(2 * B) / 1e9:.2f} GB per step", flush=True)
                per = defaultdict(float); names = {}
                for _ in range(TS):
                    s.time_step()
                    iv = s.last_intervals_ms
                    for i, ms in enumerate(iv[: 8 * L]):
                        per[NAMES[i % 8]] += ms * 1e3 / (L * TS)
                        names.setdefault(NAMES[i % 8], s.last_kernel_names[i])
                    per["logits"] += iv[8 * L] * 1e3 / TS; names["logits"] = s.last_kernel_names[8 * L]
                row[tag] = (per, names)
                s.close()
            for k in CLS:
                d, f = row["dense"][0][k], row["mxfp4"][0][k]
                print(f"    K/V {kv:4s} batch {B} rep {rep} {k:6s} in-step us per launch: dense {d:6.2f}  mxfp4 {f:6.2f}  ({'WIN ' if f < d else 'LOSS'} {100 * (f / d - 1):+5.1f} %)  "
                      f"{row['dense'][1][k].split('(')[0][-40:]} | {row['mxfp4'][1][k].split('(')[0][-40:]}", flush=True)
hb.set_tuning("mxfp4", -1)
