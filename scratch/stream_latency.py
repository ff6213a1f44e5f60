"""Frame streaming against serve_iter on the synthetic Dia-1.6B (synthetic_state_dict(seed=1234)), bf16 K/V, ignore_eos,
max_tokens 1024; 1 slot with one request, and 8 slots with 8 requests of the benchmark's mixed text lengths (32..512) whose
max_tokens are drawn once from RandomState(0) in [512, 1024].  REPS repetitions, the variants interleaved.
  first:   wall time from the start of stream_iter / serve_iter to the first non-empty chunk on the host, against the time to
           the first result serve_iter yields (a whole utterance)
  rate:    total frames (steps of every request) per second of wall time: stream_iter(chunk=16) at lag 1 and lag 0, against
           serve_iter at poll 64 and poll 16
  emit:    stream time (HIP events) of one dia_emit_frames launch for 1 and for 8 slots, median of 32
  python scratch/stream_latency.py [first rate emit]     (default: all; first and rate come from the same runs)"""
import sys, time
sys.path.insert(0, "dia-tts-prune_amd")
sys.path.insert(0, ".")
import numpy as np
import torch
from dia_hip import config as C
from dia_hip.engine import DecodeSession, DeviceWeights, Request
from dia_hip.tokens import effective_text, encode_text, synthetic_text
from dia_hip.weights import synthetic_state_dict
what = sys.argv[1:] or ["first", "rate", "emit"]
cfg = C.dia_1_6b_config()
dev = torch.device("cuda:0")
w = DeviceWeights(cfg, synthetic_state_dict(cfg, seed=1234, std=0.02, device=dev), dev)
MIXED_L = [32, 64, 96, 128, 192, 256, 384, 512]
REPS, CHUNK, CAP = 3, 16, 64
ids = [encode_text(effective_text(synthetic_text(L, cfg)), cfg) for L in MIXED_L]
mts8 = [int(v) for v in np.random.RandomState(0).randint(512, 1025, size=8)]
CASES = {1: ([ids[3]], [1024]), 8: (ids, mts8)}


def requests(n):
    texts, mts = CASES[n]
    return [Request(t, seed=i, max_tokens=m) for i, (t, m) in enumerate(zip(texts, mts))]


def run(n, variant, arg):
    """(seconds to the first non-empty chunk or first result, frames per second) of one fresh session"""
    s = DecodeSession.open(w, n, s_cap=512, kv_dtype="bf16", max_tokens=1024, ignore_eos=True,
                           stream_cap=CAP if variant == "stream" else None)
    reqs = requests(n)
    frames = sum(r.max_tokens - 1 for r in reqs)
    first = None
    s.sync()
    t0 = time.time()
    if variant == "stream":
        got = [0] * n
        for i, start, codes, final in s.stream_iter(reqs, chunk=CHUNK, lag=arg):
            if first is None and codes.shape[-1]:
                first = time.time() - t0
            got[i] += codes.shape[-1]
        assert got == [m - 2 - 15 for m in CASES[n][1]], "a streamed request did not run to its max_tokens"
    else:
        for i, res in s.serve_iter(reqs, poll=arg):
            if first is None:
                first = time.time() - t0
    s.sync()
    dt = time.time() - t0
    s.close()
    return first, frames / dt


VARIANTS = [("stream", 1, "stream_iter lag 1"), ("stream", 0, "stream_iter lag 0"), ("serve", 64, "serve_iter poll 64"),
            ("serve", 16, "serve_iter poll 16")]

if "first" in what or "rate" in what:
    for n in (1, 8):
        run(n, "stream", 1)                               # warm-up: code objects, graph capture, the pinned allocator
        rows = {name: [] for _, _, name in VARIANTS}
        for rep in range(REPS):
            for variant, arg, name in VARIANTS:
                rows[name].append(run(n, variant, arg))
        print(f"{n} slot(s), {n} request(s), max_tokens {CASES[n][1]}, chunk {CHUNK}, stream_cap {CAP}:", flush=True)
        for name, v in rows.items():
            print(f"  {name:20s} first audio on the host after " + " ".join(f"{f * 1e3:8.1f}" for f, _ in v) + " ms    frames/s " +
                  " ".join(f"{r:8.1f}" for _, r in v), flush=True)
        base = [r for _, r in rows["serve_iter poll 64"]]
        mine = [r for _, r in rows["stream_iter lag 1"]]
        print(f"  stream_iter lag 1 / serve_iter poll 64: medians {np.median(mine) / np.median(base):.4f}; spread of serve_iter poll 64 "
              f"over its {REPS} repetitions {(max(base) - min(base)) / np.median(base):.4f}", flush=True)

if "emit" in what:
    for n in (1, 8):
        s = DecodeSession.open(w, n, s_cap=512, kv_dtype="bf16", max_tokens=1024, ignore_eos=True, stream_cap=CAP)
        s.admit(requests(n))
        s.decode(64)
        s._enqueue_emit(list(range(n)))
        s.sync()
        v = []
        for _ in range(32):
            s.decode(CHUNK)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s.stream)
            s._enqueue_emit(list(range(n)))
            e1.record(s.stream)
            s.sync()
            v.append(e0.elapsed_time(e1) * 1e3)
        for b in range(n):
            s.release(b)
        s.close()
        print(f"dia_emit_frames, {n} slot(s), {CHUNK} frames each: stream time median {np.median(v):6.2f} us (min {min(v):6.2f}, "
              f"max {max(v):6.2f})", flush=True)
