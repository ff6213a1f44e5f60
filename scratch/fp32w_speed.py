"""decode speed of a genuine fp32 Dia-1.6B checkpoint (perturbed synthetic weights, fp32 K/V) with its weights as one rounded
bf16 tile set (planes 1), hi + lo planes (2: Dia.fp32_weights = "bf16x2") and hi + mid + lo planes (3: "exact"), at batch 1 and
batch 8 with mixed text lengths, in one process.  Frames/s = decode steps x batch per second (graph replay)."""
import sys, time
sys.path.insert(0, "dia-tts-prune_amd")
import torch
from dia_hip import config as C
from dia_hip.engine import DecodeSession, DeviceWeights
from dia_hip.tokens import effective_text, encode_text, synthetic_text
from dia_hip.weights import synthetic_state_dict
cfg = C.dia_1_6b_config(); dev = torch.device("cuda:0")
sd = synthetic_state_dict(cfg, seed=1234, std=0.02, device=dev)
g = torch.Generator(device=dev).manual_seed(1)
sd = {k: (v + v.abs().mean() * 2.0 ** -10 * torch.randn(v.shape, generator=g, device=dev)) if v.ndim >= 2 and "embedding" not in k else v for k, v in sd.items()}
ids1 = [encode_text(effective_text("[S1] Dia is an open weights text to dialogue model. [S2] You get full control over scripts and voices."), cfg)]
ids8 = [encode_text(effective_text(synthetic_text(L, cfg)), cfg) for L in (32, 64, 96, 128, 192, 256, 384, 512)]
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 256
for planes in (1, 2, 3):
    w = DeviceWeights(cfg, sd, dev, weight_planes=planes)
    for ids in (ids1, ids8):
        B = len(ids)
        s = DecodeSession(w, ids, kv_dtype="f32", max_tokens=steps + 40, seeds=list(range(B)), ignore_eos=True)
        t0 = time.time(); s.prefill(); s.sync(); tp = time.time() - t0
        s.decode(16, True); s.sync()
        t0 = time.time(); s.decode(steps, True); s.sync(); dt = time.time() - t0
        print(f"weight planes {planes}, batch {B}: prefill {tp * 1e3:.1f} ms, decode {steps * B / dt:.1f} frames/s "
              f"({dt / steps * 1e3:.3f} ms/step), weights {w.decode_weight_bytes() / 1e9:.2f} GB per step", flush=True)
        s.close()
    del w
    torch.cuda.empty_cache()
