"""Continuous batching against closed batches on the synthetic Dia-1.6B (synthetic_state_dict(seed=1234)), bf16 K/V, ignore_eos:
64 requests with the benchmark's mixed text lengths (32..512) and max_tokens drawn once from RandomState(0) in [128, 1024].
  serve:   eight closed DecodeSessions of 8, each run to its longest member (the way without the feature), against ONE session
           of 8 slots served continuously; total frames (sum of the requests' lengths) per second of wall time, REPS interleaved
  admit:   stream time (HIP events) from the end of the last replay before admit() to the start of the first replay after it,
           for 1 and for 4 requests, beside prefill() of a closed session over the same texts
  sample:  k_sample per launch (dia_engine_time_step) in a closed batch of 8 and in 8 slots holding the same values
  parked:  ms per step of 8 slots with 1 live utterance, of a closed batch of 1 and of a closed batch of 8
  python scratch/slots_speed.py [serve|admit|sample|parked ...]     (default: all four)"""
import sys, time
sys.path.insert(0, "dia-tts-prune_amd")
sys.path.insert(0, ".")
import numpy as np
import torch
from dia_hip import config as C
from dia_hip.engine import DecodeSession, DeviceWeights, Request
from dia_hip.tokens import effective_text, encode_text, synthetic_text
from dia_hip.weights import synthetic_state_dict
what = sys.argv[1:] or ["serve", "admit", "sample", "parked"]
cfg = C.dia_1_6b_config()
dev = torch.device("cuda:0")
w = DeviceWeights(cfg, synthetic_state_dict(cfg, seed=1234, std=0.02, device=dev), dev)
MIXED_L = [32, 64, 96, 128, 192, 256, 384, 512]
N, SLOTS, REPS = 64, 8, 3
ids = [encode_text(effective_text(synthetic_text(MIXED_L[i % 8], cfg)), cfg) for i in range(N)]
mts = [int(v) for v in np.random.RandomState(0).randint(128, 1025, size=N)]
frames = sum(m - 1 for m in mts)                      # steps every request runs (ignore_eos: to its max_tokens)


def ev():
    return torch.cuda.Event(enable_timing=True)


if "serve" in what:
    closed_steps = sum(max(mts[i: i + SLOTS]) - 1 for i in range(0, N, SLOTS))
    print(f"{N} requests, {frames} frames; closed batches run {closed_steps} steps, ideal continuous {-(-frames // SLOTS)}", flush=True)
    for rep in range(REPS):
        t0 = time.time()
        for i in range(0, N, SLOTS):
            s = DecodeSession(w, ids[i: i + SLOTS], kv_dtype="bf16", max_tokens=max(mts[i: i + SLOTS]), seeds=list(range(i, i + SLOTS)),
                              ignore_eos=True)
            s.prefill(); s.run(use_graph=True); s.results(); s.close()
        dt_c = time.time() - t0
        t0 = time.time()
        s = DecodeSession.open(w, SLOTS, s_cap=512, kv_dtype="bf16", max_tokens=1024, ignore_eos=True)
        out = s.serve([Request(ids[i], seed=i, max_tokens=mts[i]) for i in range(N)], poll=64)
        steps = s._issued
        s.close()
        dt_s = time.time() - t0
        assert [r.last_step for r in out] == [m - 2 for m in mts], "a served request did not run to its max_tokens"
        print(f"rep {rep}: closed batches {frames / dt_c:8.1f} frames/s ({dt_c:6.2f} s)   8 slots served {frames / dt_s:8.1f} frames/s "
              f"({dt_s:6.2f} s, {steps} steps)   ratio {dt_c / dt_s:.3f}", flush=True)

if "admit" in what:
    for n in (1, 4):
        for rep in range(REPS):
            s = DecodeSession.open(w, SLOTS, s_cap=512, kv_dtype="bf16", max_tokens=256, ignore_eos=True)
            s.admit([Request(ids[i], seed=i, max_tokens=256) for i in range(SLOTS - n)])
            s.decode(32); s.sync()
            e0, e1, e2 = ev(), ev(), ev()
            with torch.cuda.stream(s.stream):
                s.decode(1); e0.record()
                t0 = time.time()
                s.admit([Request(ids[7 - i], seed=100 + i, max_tokens=256) for i in range(n)])
                host = time.time() - t0
                e1.record(); s.decode(1); e2.record()
            s.sync()
            c = DecodeSession(w, [ids[7 - i] for i in range(n)], kv_dtype="bf16", max_tokens=256, seeds=list(range(n)), ignore_eos=True)
            p0, p1 = ev(), ev()
            with torch.cuda.stream(c.stream):
                p0.record(); c.prefill(); p1.record()
            c.sync()
            print(f"admit {n} (texts of {[len(ids[7 - i]) for i in range(n)]} bytes) rep {rep}: stream time replay -> replay {e0.elapsed_time(e1):6.3f} ms "
                  f"(host enqueue {host * 1e3:6.3f} ms; the step behind it {e1.elapsed_time(e2):6.3f} ms)   closed prefill of the same texts "
                  f"{p0.elapsed_time(p1):6.3f} ms", flush=True)
            s.close(); c.close()

if "sample" in what:
    for rep in range(REPS):
        a = DecodeSession(w, ids[:SLOTS], kv_dtype="bf16", max_tokens=256, seeds=list(range(SLOTS)), ignore_eos=True)
        a.prefill()
        b = DecodeSession.open(w, SLOTS, s_cap=512, kv_dtype="bf16", max_tokens=256, ignore_eos=True)
        b.admit([Request(ids[i], seed=i, max_tokens=256) for i in range(SLOTS)])
        t = {}
        for tag, s in (("scalar", a), ("per-slot", b)):
            s.decode(32); s.sync()
            v = []
            for _ in range(16):
                ms = s.time_step()
                v.append(ms[-1] * 1e3)
            t[tag] = (np.median(v), min(v), max(v), s.last_kernel_names[-1])
        print(f"rep {rep}: k_sample per launch, batch 8: " + "   ".join(f"{k} median {m:5.2f} us (min {lo:5.2f}, max {hi:5.2f}) {nm}"
                                                                       for k, (m, lo, hi, nm) in t.items()), flush=True)
        a.close(); b.close()

if "parked" in what:
    K = 256
    for rep in range(REPS):
        row = {}
        s = DecodeSession.open(w, SLOTS, s_cap=512, kv_dtype="bf16", max_tokens=K + 64, ignore_eos=True)
        s.admit([Request(ids[3], seed=1, max_tokens=K + 64)])
        c1 = DecodeSession(w, [ids[3]], kv_dtype="bf16", max_tokens=K + 64, seeds=[1], ignore_eos=True); c1.prefill()
        c8 = DecodeSession(w, ids[:8], kv_dtype="bf16", max_tokens=K + 64, seeds=list(range(8)), ignore_eos=True); c8.prefill()
        for tag, x in (("8 slots, 1 live", s), ("closed batch 1", c1), ("closed batch 8", c8)):
            x.decode(16); x.ensure_noise(16 + K); x.sync()
            t0 = time.time(); x.decode(K); x.sync()
            row[tag] = (time.time() - t0) / K * 1e3
            x.close()
        print(f"rep {rep}: ms per step over {K} steps: " + "   ".join(f"{k} {v:.3f}" for k, v in row.items()), flush=True)
