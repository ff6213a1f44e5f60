"""the two-plane decode step (Dia.fp32_weights = "bf16x2") on a perturbed fp32 Dia-1.6B checkpoint, fp32 K/V, eager launches —
run under rocprofv3 --kernel-trace --stats: python scratch/fp32w_prof.py BATCH [STEPS]"""
import sys
sys.path.insert(0, "dia-tts-prune_amd")
import torch
from dia_hip import config as C
from dia_hip.engine import DecodeSession, DeviceWeights
from dia_hip.tokens import effective_text, encode_text, synthetic_text
from dia_hip.weights import synthetic_state_dict
B = int(sys.argv[1]); steps = int(sys.argv[2]) if len(sys.argv) > 2 else 32
cfg = C.dia_1_6b_config(); dev = torch.device("cuda:0")
sd = synthetic_state_dict(cfg, seed=1234, std=0.02, device=dev)
g = torch.Generator(device=dev).manual_seed(1)
sd = {k: (v + v.abs().mean() * 2.0 ** -10 * torch.randn(v.shape, generator=g, device=dev)) if v.ndim >= 2 and "embedding" not in k else v for k, v in sd.items()}
w = DeviceWeights(cfg, sd, dev, weight_planes=2)
del sd
lens = [32, 64, 96, 128, 192, 256, 384, 512]
ids = [encode_text(effective_text(synthetic_text(lens[b % 8], cfg)), cfg) for b in range(B)]
s = DecodeSession(w, ids, kv_dtype="f32", max_tokens=steps + 8, seeds=list(range(B)), ignore_eos=True)
s.prefill(); s.sync()
s.decode(steps, False); s.sync()
s.close()
print(f"two-plane step, batch {B}: {steps} eager steps done")
