"""prompt_prefill="batched" at full size: stream time from admit() / prefill() to the first sampled frame of a prompted request,
against the replay ("auto" in these two configurations) — (a) admitted into a bf16 slot session of 8 slots with 7 live neighbours,
(b) a closed batch-1 self_kv="fp8" session, (c) the neighbours' frames/s during the admission window of (a).  Greedy requests: no
noise is drawn on the host, the times are the stream's.  Three interleaved pairs each."""
import sys, os, time
sys.path.insert(0, "dia-tts-prune_amd")
import numpy as np, torch
from dia_hip import config as C
from dia_hip.engine import DecodeSession, DeviceWeights, Request
from dia_hip.tokens import effective_text, encode_text
from dia_hip.weights import synthetic_state_dict
cfg = C.dia_1_6b_config(); dev = torch.device("cuda:0")
w = DeviceWeights(cfg, synthetic_state_dict(cfg, seed=1234, std=0.02, device=dev), dev)
text = "[S1] Dia is an open weights text to dialogue model. [S2] You get full control over scripts and voices."
tp, fs = 430, 431
ids = encode_text(effective_text(text, "[S1] prompt transcript."), cfg)
prompt = np.random.RandomState(0).randint(0, 1024, size=(tp, 9)).astype(np.int32)
MODES = ("auto", "batched")

# (a) + (c): 8 slots, 7 live neighbours, one prompted request admitted into the eighth
sess = {}
for mode in MODES:
    s = DecodeSession.open(w, 8, s_cap=len(ids), kv_dtype="bf16", ignore_eos=True, prompt_prefill=mode)
    s.admit([Request(encode_text(effective_text(text), cfg), temperature=0.0) for _ in range(7)])
    s.decode(32); s.sync()
    sess[mode] = s


def admission(s, mode):
    req = Request(ids, temperature=0.0, audio_prompt=prompt)
    s.sync(); t0 = time.time()
    b = s.admit([req])[0]
    n = 1 if mode == "batched" else fs             # decode steps up to and including the first sampled one
    left = n
    while left:
        k = min(64, left); s.decode(k); left -= k
    s.sync(); t1 = time.time()
    assert int(s.cur[b].item()) == fs + 1, (mode, int(s.cur[b].item()))
    s.release(b)
    return 1e3 * (t1 - t0), n


for mode in MODES:
    admission(sess[mode], mode)                    # warm (allocator, modules)
res = {m: [] for m in MODES}
for i in range(3):
    for mode in MODES:
        ms, n = admission(sess[mode], mode)
        res[mode].append(ms)
        print(f"(a) pair {i} bf16 8 slots, 7 live: prompt {tp} frames, {mode:7s}: admit() -> first sampled frame {ms:8.1f} ms ({n} decode steps); "
              f"(c) neighbours {7 * n / (ms / 1e3):7.1f} frames/s in that window", flush=True)
for mode in MODES:
    sess[mode].close()
a_auto, a_bat = np.median(res["auto"]), np.median(res["batched"])
print(f"(a) median: auto (replay) {a_auto:.1f} ms, batched {a_bat:.1f} ms, ratio {a_auto / a_bat:.1f}x; "
      f"(c) neighbours {7 * fs / (a_auto / 1e3):.1f} frames/s (replay window, {fs} steps) vs {7 / (a_bat / 1e3):.1f} frames/s (batched window, 1 step)", flush=True)

# (b) closed batch 1, self_kv="fp8"
sess = {m: DecodeSession(w, [ids], kv_dtype="bf16", self_kv="fp8", max_tokens=tp + 66, temperature=0.0, audio_prompts=[prompt], ignore_eos=True,
                         prompt_prefill=m) for m in MODES}


def closed(s, mode):
    s.cur.fill_(1); s.sync(); t0 = time.time()
    s.prefill()
    s.decode(1 if mode == "batched" else fs, True)
    s.sync(); t1 = time.time()
    assert int(s.cur[0].item()) == fs + 1
    return 1e3 * (t1 - t0)


for mode in MODES:
    closed(sess[mode], mode)
res = {m: [] for m in MODES}
for i in range(3):
    for mode in MODES:
        res[mode].append(closed(sess[mode], mode))
        print(f"(b) pair {i} closed batch 1 self_kv=fp8: prompt {tp} frames, {mode:7s}: prefill() -> first sampled frame {res[mode][-1]:8.1f} ms", flush=True)
for mode in MODES:
    sess[mode].close()
b_auto, b_bat = np.median(res["auto"]), np.median(res["batched"])
print(f"(b) median: auto (replay) {b_auto:.1f} ms, batched {b_bat:.1f} ms, ratio {b_auto / b_bat:.1f}x", flush=True)
