"""What the scoring hook (dia_engine_set_score, DESIGN.md "Scoring") costs a decode step.
Synthetic Dia-1.6B (synthetic_state_dict(seed=1234)), ONE DeviceWeights; teacher-forced sessions over random codes with and
without score=True — the side without it launches exactly the step of a session that never heard of scoring — interleaved,
REPS times, batch 1 and batch 8 (mixed text lengths 32..512), K/V bf16.  ms/step of `steps` graph replays, then the in-step
time of the k_score launch itself (dia_engine_time_step intervals: end of the logits GEMM -> end of k_score), mean over TS steps.
  python scratch/score_speed.py [steps]  > profiles/r08_score_cost.txt"""
import sys, time
sys.path.insert(0, "dia-tts-prune_amd")
sys.path.insert(0, ".")
import numpy as np
import torch
from dia_hip import config as C
from dia_hip.engine import DecodeSession, DeviceWeights
from dia_hip.score import teacher_rows
from dia_hip.tokens import effective_text, encode_text, synthetic_text
from dia_hip.weights import synthetic_state_dict
TEXT = "[S1] Dia is an open weights text to dialogue model. [S2] You get full control over scripts and voices."
cfg = C.dia_1_6b_config()
dev = torch.device("cuda:0")
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
REPS, TS = 3, 4
w = DeviceWeights(cfg, synthetic_state_dict(cfg, seed=1234, std=0.02, device=dev), dev)
ids1 = [encode_text(effective_text(TEXT), cfg)]
ids8 = [encode_text(effective_text(synthetic_text(L, cfg)), cfg) for L in (32, 64, 96, 128, 192, 256, 384, 512)]
rs = np.random.RandomState(0)
mt = steps + 16 + TS + 2
for ids in (ids1, ids8):
    B = len(ids)
    rows = [teacher_rows(cfg, rs.randint(0, 1024, size=(mt, cfg.data.channels)))[:mt] for _ in range(B)]
    for rep in range(REPS):
        ms = {}
        for tag, score in (("plain", False), ("score", True)):
            s = DecodeSession(w, ids, kv_dtype="bf16", max_tokens=mt, temperature=0.0, teacher_tokens=rows, score=score)
            s.prefill(); s.sync()
            s.decode(16, True); s.sync()
            t0 = time.time(); s.decode(steps, True); s.sync(); dt = time.time() - t0
            ms[tag] = dt / steps * 1e3
            own = ""
            if score:
                us = []
                for _ in range(TS):
                    s.time_step()
                    i = s.last_kernel_names.index("k_score")
                    us.append(s.last_intervals_ms[i] * 1e3)
                own = f", k_score in-step {np.mean(us):.2f} us (launch {i} of {len(s.last_kernel_names)})"
            print(f"batch {B} rep {rep} {tag:5s}: {ms[tag]:.4f} ms/step, {steps * B / dt:7.1f} frames/s, {s.launches_per_step()} launches{own}", flush=True)
            s.close()
        print(f"    batch {B} rep {rep}: score - plain = {(ms['score'] - ms['plain']) * 1e3:+.2f} us/step ({100 * (ms['score'] / ms['plain'] - 1):+.2f} %)", flush=True)
