"""scratch/cross_fp8_speed.py for the FP8 self K/V caches (DESIGN.md "FP8 self K/V").
Decode speed of the synthetic Dia-1.6B (synthetic_state_dict(seed=1234)) with DecodeSession(self_kv="bf16") — the step of the parent
commit, launch for launch — against self_kv="fp8" on the same DeviceWeights, in one process, interleaved, REPS pairs per point:
batch 1 (one text), batch 8 and batch 64 with mixed text lengths (32..512 bytes), K/V bf16.  Every session first replays `depth`
steps (default 512; 2000 for the long point), so that the self caches are that long, then `steps` steps are timed.  Frames/s =
decode steps x batch per second (graph replay).  Then the self-attention launch's own time (dia_engine_time_step: kernel begin ->
end, and the in-step interval end of the previous launch -> end of this one), mean over the 18 layers and TS steps, per repetition.
  python scratch/self_fp8_speed.py [depth] [steps]   > profiles/r14_self_fp8_ab.txt
  python scratch/self_fp8_speed.py drift             largest logit deviation of the fp8 session from the bf16 session over 40 teacher-forced
                                                     steps (the scoring path: score=True sessions over the same forced rows), batch 2;
                                                     recorded only — synthetic weights say nothing about audio quality"""
import sys, time
sys.path.insert(0, "dia-tts-prune_amd")
sys.path.insert(0, ".")
import numpy as np
import torch
from dia_hip import config as C
from dia_hip.engine import DecodeSession, DeviceWeights
from dia_hip.tokens import effective_text, encode_text, synthetic_text
from dia_hip.weights import synthetic_state_dict
TEXT = "[S1] Dia is an open weights text to dialogue model. [S2] You get full control over scripts and voices."
cfg = C.dia_1_6b_config()
dev = torch.device("cuda:0")
w = DeviceWeights(cfg, synthetic_state_dict(cfg, seed=1234, std=0.02, device=dev), dev)
MIX = (32, 64, 96, 128, 192, 256, 384, 512)
L = cfg.model.decoder.n_layer
if len(sys.argv) > 1 and sys.argv[1] == "drift":
    V, Cn, steps = cfg.model.tgt_vocab_size, cfg.data.channels, 40
    ids = [encode_text(effective_text(TEXT), cfg), encode_text(effective_text(synthetic_text(384, cfg)), cfg)]
    rng = np.random.default_rng(5)
    teacher = [rng.integers(0, 1024, size=(steps + 2, Cn)).astype(np.int32) for _ in ids]
    ss = {sk: DecodeSession(w, ids, kv_dtype="bf16", max_tokens=steps + 2, temperature=0.0, teacher_tokens=teacher, score=True, self_kv=sk)
          for sk in ("bf16", "fp8")}
    for s in ss.values():
        s.prefill()
    worst, worst_abs = 0.0, 0.0
    for i in range(steps):
        lg = {}
        for sk, s in ss.items():
            s.decode(1, use_graph=False)
            lg[sk] = s.logits_host().astype(np.float64)
        d = np.abs(lg["fp8"] - lg["bf16"]).max()
        worst, worst_abs = max(worst, d), max(worst_abs, np.abs(lg["bf16"]).max())
        print(f"step {i + 1:2d}: max |logit fp8-self - bf16-self| {d:.4e}  (max |logit| {np.abs(lg['bf16']).max():.3f})", flush=True)
    sc = {sk: s.scores_host() for sk, s in ss.items()}
    m = np.isfinite(sc["bf16"][..., 0]) & np.isfinite(sc["fp8"][..., 0])
    print(f"largest logit deviation over {steps} teacher-forced steps (batch 2, texts of {len(ids[0])} and {len(ids[1])} bytes): {worst:.4e} "
          f"at logits up to {worst_abs:.3f}; dia_score lp_cond: max |difference| {np.abs(sc['fp8'][..., 0] - sc['bf16'][..., 0])[m].max():.4e} "
          f"over {int(m.sum())} scored positions", flush=True)
    print(f"self cache bytes (R = {ss['fp8'].R}, T = {ss['fp8'].T}): bf16 {ss['bf16'].self_cache_bytes}, fp8 {ss['fp8'].self_cache_bytes} "
          f"(x{ss['fp8'].self_cache_bytes / ss['bf16'].self_cache_bytes:.5f})", flush=True)
    for s in ss.values():
        s.close()
    sys.exit(0)
depth = int(sys.argv[1]) if len(sys.argv) > 1 else 512
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 256
batches = [int(b) for b in sys.argv[3].split(",")] if len(sys.argv) > 3 else [1, 8, 64]
REPS, TS = 3, 4
for B in batches:
    ids = [encode_text(effective_text(TEXT), cfg)] if B == 1 else [encode_text(effective_text(synthetic_text(n, cfg)), cfg) for n in MIX] * (B // 8)
    for rep in range(REPS):
        row = {}
        for sk in ("bf16", "fp8"):
            s = DecodeSession(w, ids, kv_dtype="bf16", max_tokens=depth + steps + 8 + TS, seeds=list(range(B)), ignore_eos=True, self_kv=sk)
            s.prefill(); s.sync()
            s.decode(depth, True); s.sync()
            t0 = time.time(); s.decode(steps, True); s.sync(); dt = time.time() - t0
            print(f"batch {B:2d} depth {depth} rep {rep} self_kv {sk:4s}: decode {steps * B / dt:8.1f} frames/s ({dt / steps * 1e3:.3f} ms/step), "
                  f"{s.launches_per_step()} launches per step, self cache {s.self_cache_bytes / 2 ** 20:.0f} MiB", flush=True)
            own = ivl = 0.0
            for _ in range(TS):
                ms = s.time_step()
                idx = [i for i, n in enumerate(s.last_kernel_names) if n.startswith("k_attn_self_f8") or n.startswith("k_attn_mfma<4, 1>")]
                assert len(idx) == L, s.last_kernel_names
                own += float(ms[idx].sum()) * 1e3 / (L * TS); ivl += float(s.last_intervals_ms[idx].sum()) * 1e3 / (L * TS)
            row[sk] = (steps * B / dt, own, ivl, s.last_kernel_names[idx[0]])
            s.close()
        a, b = row["bf16"], row["fp8"]
        print(f"    batch {B:2d} depth {depth} rep {rep}: frames/s fp8 / bf16 = {b[0] / a[0]:.4f};  self-attention launch, us: own time {a[1]:6.2f} -> {b[1]:6.2f} "
              f"({100 * (b[1] / a[1] - 1):+5.1f} %), in-step interval {a[2]:6.2f} -> {b[2]:6.2f} ({100 * (b[2] / a[2] - 1):+5.1f} %)   {a[3]} | {b[3]}", flush=True)
