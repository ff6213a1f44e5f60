"""scratch/mxfp4_speed.py for the FP8 cross K/V caches (DESIGN.md "FP8 cross K/V").
Decode speed of the synthetic Dia-1.6B (synthetic_state_dict(seed=1234)) with DecodeSession(cross_kv="bf16") — the step of the parent
commit, launch for launch — against cross_kv="fp8" on the same DeviceWeights, in one process, interleaved, REPS pairs per point:
batch 1 (one text), batch 8 and batch 64 with mixed text lengths (32..512 bytes), K/V bf16.  Frames/s = decode steps x batch per
second (graph replay).  Then the cross-attention launch's own time (dia_engine_time_step: kernel begin -> end, and the in-step
interval end of the previous launch -> end of this one), mean over the 18 layers and TS steps, per repetition.
  python scratch/cross_fp8_speed.py [steps]        > profiles/r10_cross_fp8_ab.txt
  python scratch/cross_fp8_speed.py drift          largest logit deviation of the fp8 session from the bf16 session over 40 teacher-forced
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
    ss = {ck: DecodeSession(w, ids, kv_dtype="bf16", max_tokens=steps + 2, temperature=0.0, teacher_tokens=teacher, score=True, cross_kv=ck)
          for ck in ("bf16", "fp8")}
    for s in ss.values():
        s.prefill()
    worst, worst_abs = 0.0, 0.0
    for i in range(steps):
        lg = {}
        for ck, s in ss.items():
            s.decode(1, use_graph=False)
            lg[ck] = s.logits_host().astype(np.float64)
        d = np.abs(lg["fp8"] - lg["bf16"]).max()
        worst, worst_abs = max(worst, d), max(worst_abs, np.abs(lg["bf16"]).max())
        print(f"step {i + 1:2d}: max |logit fp8-cross - bf16-cross| {d:.4e}  (max |logit| {np.abs(lg['bf16']).max():.3f})", flush=True)
    sc = {ck: s.scores_host() for ck, s in ss.items()}
    m = np.isfinite(sc["bf16"][..., 0]) & np.isfinite(sc["fp8"][..., 0])
    print(f"largest logit deviation over {steps} teacher-forced steps (batch 2, texts of {len(ids[0])} and {len(ids[1])} bytes): {worst:.4e} "
          f"at logits up to {worst_abs:.3f}; dia_score lp_cond: max |difference| {np.abs(sc['fp8'][..., 0] - sc['bf16'][..., 0])[m].max():.4e} "
          f"over {int(m.sum())} scored positions", flush=True)
    for s in ss.values():
        s.close()
    sys.exit(0)
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
REPS, TS = 3, 4
points = [[encode_text(effective_text(TEXT), cfg)]] + [[encode_text(effective_text(synthetic_text(n, cfg)), cfg) for n in MIX] * k for k in (1, 8)]
for ids in points:
    B = len(ids)
    for rep in range(REPS):
        row = {}
        for ck in ("bf16", "fp8"):
            s = DecodeSession(w, ids, kv_dtype="bf16", max_tokens=steps + 40 + TS, seeds=list(range(B)), ignore_eos=True, cross_kv=ck)
            s.prefill(); s.sync()
            s.decode(16, True); s.sync()
            t0 = time.time(); s.decode(steps, True); s.sync(); dt = time.time() - t0
            print(f"batch {B:2d} rep {rep} cross_kv {ck:4s}: decode {steps * B / dt:8.1f} frames/s ({dt / steps * 1e3:.3f} ms/step), "
                  f"{s.launches_per_step()} launches per step", flush=True)
            own = ivl = 0.0
            for _ in range(TS):
                ms = s.time_step()
                idx = [i for i, n in enumerate(s.last_kernel_names) if n == "k_attn_mfma_f8" or (n.startswith("k_attn_mfma<1, 1>"))]
                assert len(idx) == L, s.last_kernel_names
                own += float(ms[idx].sum()) * 1e3 / (L * TS); ivl += float(s.last_intervals_ms[idx].sum()) * 1e3 / (L * TS)
            row[ck] = (steps * B / dt, own, ivl, s.last_kernel_names[idx[0]])
            s.close()
        a, b = row["bf16"], row["fp8"]
        print(f"    batch {B:2d} rep {rep}: frames/s fp8 / bf16 = {b[0] / a[0]:.4f};  cross-attention launch, us: own time {a[1]:6.2f} -> {b[1]:6.2f} "
              f"({100 * (b[1] / a[1] - 1):+5.1f} %), in-step interval {a[2]:6.2f} -> {b[2]:6.2f} ({100 * (b[2] / a[2] - 1):+5.1f} %)   {a[3]} | {b[3]}", flush=True)
