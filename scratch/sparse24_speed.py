"""decode speed of the 2:4-pruned synthetic Dia-1.6B (synthetic_state_dict(seed=1234) -> semi_structured_prune_state_dict): the
same checkpoint with its decoder streamed as dense tiles (sparse "off") and as 2:4 streams (sparse "2:4"), at batch 1 and batch 8
with mixed text lengths (32..512), K/V bf16 and f32, in one process.  Frames/s = decode steps x batch per second (graph replay).
Then the per-kernel times of one eager step (dispatch-level start / stop events, what rocprofv3 --kernel-trace reports), summed
per matrix over the 18 layers."""
import sys, time
from collections import defaultdict
sys.path.insert(0, "dia-tts-prune_amd")
import torch
from dia_hip import config as C
from dia_hip.engine import DecodeSession, DeviceWeights
from dia_hip.pruning import semi_structured_prune_state_dict
from dia_hip.tokens import effective_text, encode_text, synthetic_text
from dia_hip.weights import synthetic_state_dict
cfg = C.dia_1_6b_config(); dev = torch.device("cuda:0")
sd = semi_structured_prune_state_dict(cfg, synthetic_state_dict(cfg, seed=1234, std=0.02, device=dev))
ids1 = [encode_text(effective_text("[S1] Dia is an open weights text to dialogue model. [S2] You get full control over scripts and voices."), cfg)]
ids8 = [encode_text(effective_text(synthetic_text(L, cfg)), cfg) for L in (32, 64, 96, 128, 192, 256, 384, 512)]
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 256
ws = {sp: DeviceWeights(cfg, sd, dev, sparse=sp) for sp in ("off", "2:4")}
del sd
NAMES = ["qkv", "attn_self", "o", "cq", "attn_cross", "co", "wi", "wo"]
for kv in ("bf16", "f32"):
    for ids in (ids1, ids8):
        B = len(ids)
        for sp, w in ws.items():
            s = DecodeSession(w, ids, kv_dtype=kv, max_tokens=steps + 40, seeds=list(range(B)), ignore_eos=True)
            s.prefill(); s.sync()
            s.decode(16, True); s.sync()
            t0 = time.time(); s.decode(steps, True); s.sync(); dt = time.time() - t0
            print(f"K/V {kv:4s} batch {B}, sparse {sp:3s}: decode {steps * B / dt:7.1f} frames/s ({dt / steps * 1e3:.3f} ms/step), "
                  f"weights {w.decode_weight_bytes(2 * B) / 1e9:.2f} GB per step", flush=True)
            if kv == "f32":
                per = defaultdict(float); names = {}
                t = s.time_step()
                L = cfg.model.decoder.n_layer
                for i, ms in enumerate(t[: 8 * L]):
                    per[NAMES[i % 8]] += ms * 1e3
                    names.setdefault(NAMES[i % 8], s.last_kernel_names[i])
                per["logits"] = t[8 * L] * 1e3; names["logits"] = s.last_kernel_names[8 * L]
                for k in ("qkv", "o", "cq", "co", "wi", "wo", "logits"):
                    n = 1 if k == "logits" else L
                    print(f"    {k:6s} {per[k] / n:6.2f} us per launch  {names[k]}", flush=True)
            s.close()
