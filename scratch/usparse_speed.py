"""scratch/mxfp4_speed.py for the unstructured sparse streams (profiles/r21_usparse_speed.txt is this script's output).
  python scratch/usparse_speed.py [steps]      in-step A/B
  python scratch/usparse_speed.py launch       per-launch A/B
In-step: the synthetic Dia-1.6B (synthetic_state_dict(seed=1234)) pruned 50, 60 and 70 % with unstructured_prune_state_dict; ONE
DeviceWeights(sparse="unstructured") per sparsity holds the dense tiles and the streams of the same numbers, and the knob usparse
picks per session what the step streams: 0 = dense tiles everywhere on the same pruned checkpoint (the yardstick), one bit = one
launch class, 0x7f = every class.  Batch 1 and 2, K/V bf16, REPS repetitions with the configurations interleaved inside each.
Frames/s = decode steps x batch per second (graph replay).  Then per launch class the in-step time of one eager step
(dia_engine_time_step intervals, mean over the layers and TS steps) of the dense and the all-classes session, per repetition.
Per launch: dia_gemm_timed (dispatch-level begin -> end of the kernel) at 2 rows on a random bf16 matrix of the decode step's
shapes and epilogues, dense tiles against the stream of the same matrix at the rate the loader picks, alternating, a 512 MiB fill
between launches (cold caches), the first repetition dropped.  "cap" rows: every lane-tile holds exactly R non-zeros, so the
overflow list is empty and what remains beside the dense kernel's work is the expansion (mask, table read, permutes)."""
import ctypes as C_
import sys, time
from collections import defaultdict
sys.path.insert(0, "dia-tts-prune_amd")
sys.path.insert(0, ".")
import torch
from dia_hip import binding as hb
from dia_hip import config as C
from dia_hip import layout as lay
dev = torch.device("cuda:0")
CLS = ("qkv", "o", "cq", "co", "wi", "wo", "logits")


def launch_mode():
    L = hb.lib()

    def setup(K, N, epi, zeros, sk):
        gen = torch.Generator().manual_seed(K + N)
        M = 2
        X = torch.randn(M, K, generator=gen)
        w = (torch.randn(K, N, generator=gen) * 0.05).bfloat16().float()
        w[w == 0] = 0.05
        if isinstance(zeros, str):                              # "cap4" / "cap2": exactly R non-zeros in every lane-tile
            R = int(zeros[3:])
            order = torch.rand(K // 8, 8, N, generator=gen).argsort(dim=1).argsort(dim=1)
            w = w * (order < R).reshape(K, N)
        else:
            w = w * (torch.rand(K, N, generator=gen) >= zeros)
        A = lay.pack_f32_tiles(X.to(dev), ktiles=K // 32)
        pick = lay.us_choose(w.to(dev))
        Wd, kt, ns = lay.tile_weight(w.to(dev))
        keep = [A, Wd, pick[0]]
        um = hb.UsMat(stream=hb.ptr(pick[0]), rate=pick[1]); keep.append(um)
        out = []
        for fmt in (0, hb.W_USPARSE):
            g = hb.GemmArgs()
            g.A, g.a_ktiles, g.M, g.KT, g.nstrips, g.epi, g.act_f32, g.w_format, g.ssq_ld = hb.ptr(A), K // 32, M, kt, ns, epi, 3, fmt, 16
            g.W = C_.cast(C_.pointer(um), C_.c_void_p) if fmt else hb.ptr(Wd)
            sin = torch.ones(128, 16, device=dev); keep.append(sin)
            if epi != hb.EPI_RESID_EMIT:
                g.ssq_in, g.ssq_in_n, g.inv_d, g.eps = hb.ptr(sin), 128, 1.0 / 2048, 1e-5
            if epi == hb.EPI_SCALE_STORE:
                o = torch.zeros(M, N, device=dev); keep.append(o); g.out, g.ldo = hb.ptr(o), N
            elif epi == hb.EPI_RESID_EMIT:
                o = torch.zeros(M, N, device=dev); P = torch.zeros(1, N // 32, 64, 8, device=dev)
                sso = torch.zeros(ns, 16, device=dev); gn = torch.ones(N, device=dev)
                keep += [o, P, sso, gn]
                g.out, g.ldo, g.gnext, g.P, g.p_ktiles, g.ssq_out = hb.ptr(o), N, hb.ptr(gn), hb.ptr(P), N // 32, hb.ptr(sso)
            else:
                P = torch.zeros(1, N // 64, 64, 8, device=dev); keep.append(P); g.P, g.p_ktiles = hb.ptr(P), N // 64
            if sk:
                scr = torch.zeros(ns * sk * 256, device=dev); tk = torch.zeros(ns, dtype=torch.int32, device=dev); keep += [scr, tk]
                g.sk_scratch, g.sk_tickets, g.sk, g.sk_scratch_floats = hb.ptr(scr), hb.ptr(tk), sk, scr.numel()
            out.append(g)
        return out, keep, pick[1], pick[4] / pick[5]

    def flush():
        torch.empty(512 << 20, dtype=torch.uint8, device=dev).fill_(1)      # push the weights out of the caches between launches
        torch.cuda.synchronize()
    for name, K, N, epi, sk in (("qkv", 2048, 3072, 0, 0), ("o", 2048, 2048, 1, 0), ("wi", 2048, 16384, 2, 0), ("wo", 8192, 2048, 1, 2)):
        for zeros in (0.5, 0.6, 0.7, "cap4", "cap2"):
            gs, keep, rate, ratio = setup(K, N, epi, zeros, sk)
            ms = C_.c_float()
            ts = ([], [])
            for rep in range(7):
                for i in (0, 1):
                    flush()
                    hb.check(L.dia_gemm_timed(C_.byref(gs[i]), None, C_.byref(ms)), "dia_gemm_timed")
                    if rep:
                        ts[i].append(ms.value * 1e3)
            print(f"launch {name:3s} K={K} N={N} zeros={zeros} R={rate} bytes={ratio:.3f}  dense us {' '.join('%5.1f' % t for t in ts[0])}   "
                  f"stream us {' '.join('%5.1f' % t for t in ts[1])}", flush=True)


def step_mode(steps):
    from dia_hip.engine import DEC_MATS, DecodeSession, DeviceWeights
    from dia_hip.pruning import unstructured_prune_state_dict
    from dia_hip.tokens import effective_text, encode_text, synthetic_text
    from dia_hip.weights import synthetic_state_dict
    TEXT = "[S1] Dia is an open weights text to dialogue model. [S2] You get full control over scripts and voices."
    cfg = C.dia_1_6b_config()
    REPS, TS = 3, 2
    NAMES = ["qkv", "attn_self", "o", "cq", "attn_cross", "co", "wi", "wo"]
    NL = cfg.model.decoder.n_layer
    ids_of = {1: [encode_text(effective_text(TEXT), cfg)],
              2: [encode_text(effective_text(TEXT), cfg), encode_text(effective_text(synthetic_text(64, cfg)), cfg)]}
    raw = synthetic_state_dict(cfg, seed=1234, std=0.02, device=dev)
    for amount in (0.5, 0.6, 0.7):
        sd = unstructured_prune_state_dict(cfg, raw, amount)
        w = DeviceWeights(cfg, sd, dev, sparse="unstructured", compact="off")
        del sd
        for k in CLS:                                           # byte ratios and rates per class
            mats = [w.logits_us] if k == "logits" else [L[k + "us"] for L in w.dec_layers]
            names = ["decoder.logits_dense"] if k == "logits" else [f"decoder.layers.{i}.{k}" for i in range(NL)]
            ub, db = sum(w.us_bytes[n] or w.dense_bytes[n] for n in names), sum(w.dense_bytes[n] for n in names)
            print(f"zeros {amount:.0%} class {k:6s}: stream / dense bytes {ub / db:.3f}, streams {sum(m is not None for m in mats)}/{len(mats)}, "
                  f"rates {sorted(set(m.rate for m in mats if m is not None))}", flush=True)
        configs = [("dense", 0)] + [(k, 1 << i) for i, k in enumerate(CLS)] + [("all", 0x7f)]
        for B in (1, 2):
            for rep in range(REPS):
                row = {}
                for tag, mask in configs:
                    hb.set_tuning("usparse", mask)
                    s = DecodeSession(w, ids_of[B], kv_dtype="bf16", max_tokens=steps + 40 + TS, seeds=list(range(B)), ignore_eos=True)
                    s.prefill(); s.sync()
                    s.decode(16, True); s.sync()
                    t0 = time.time(); s.decode(steps, True); s.sync(); dt = time.time() - t0
                    print(f"zeros {amount:.0%} batch {B} rep {rep} {tag:6s} (mask {mask:#04x}): decode {steps * B / dt:7.1f} frames/s ({dt / steps * 1e3:.3f} ms/step), "
                          f"weights {w.decode_weight_bytes(2 * B) / 1e9:.2f} GB per step", flush=True)
                    if tag in ("dense", "all"):
                        per = defaultdict(float); names = {}
                        for _ in range(TS):
                            s.time_step()
                            iv = s.last_intervals_ms
                            for i, ms in enumerate(iv[: 8 * NL]):
                                per[NAMES[i % 8]] += ms * 1e3 / (NL * TS)
                                names.setdefault(NAMES[i % 8], s.last_kernel_names[i])
                            per["logits"] += iv[8 * NL] * 1e3 / TS; names["logits"] = s.last_kernel_names[8 * NL]
                        row[tag] = (per, names)
                    s.close()
                for k in CLS:
                    d, f = row["dense"][0][k], row["all"][0][k]
                    print(f"    zeros {amount:.0%} batch {B} rep {rep} {k:6s} in-step us per launch: dense {d:6.2f}  stream {f:6.2f}  ({'WIN ' if f < d else 'LOSS'} {100 * (f / d - 1):+5.1f} %)  "
                          f"{row['dense'][1][k].split('(')[0][-36:]} | {row['all'][1][k].split('(')[0][-36:]}", flush=True)
        del w
        torch.cuda.empty_cache()
    hb.set_tuning("usparse", -1)


if len(sys.argv) > 1 and sys.argv[1] == "launch":
    launch_mode()
else:
    step_mode(int(sys.argv[1]) if len(sys.argv) > 1 else 384)
