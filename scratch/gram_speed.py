"""Cost of a calibrating decode step with Gram matrices (DESIGN.md "Gram matrices and GPTQ"), synthetic Dia-1.6B, teacher-forced.
Three sessions per batch size, interleaved REPS times in one process: calibrate="gram" (one dia_act_gram in front of every GEMM),
calibrate=True (dia_act_stats) and a plain scoring session.  ms per step under graph replay, and beside the Gram number the step's
lower bound 2 x packed bytes of all taps / HBM peak (every launch reads and writes all of G) with the achieved fraction.
  python scratch/gram_speed.py [steps]
  python scratch/gram_speed.py solver      (no GPU: wall time of the host solver, gptq_factor + gptq_apply, at the model's own
                                             wi [2048, 8192] and wo [8192, 2048], format by format)"""
import sys, time
sys.path.insert(0, "dia-tts-prune_amd")
sys.path.insert(0, ".")
import numpy as np
import torch
from dia_hip import config as C
cfg = C.dia_1_6b_config()
if len(sys.argv) > 1 and sys.argv[1] == "solver":
    import os
    from dia_hip import quant as Q
    rs = np.random.RandomState(0)
    print(f"host threads: {len(os.sched_getaffinity(0))}", flush=True)
    for K, N in ((2048, 8192), (8192, 2048)):
        X = rs.randn(K + 512, K).astype(np.float32).astype(np.float64)
        G = X.T @ X
        w = torch.from_numpy((rs.randn(K, N) * 0.02).astype(np.float32))
        t0 = time.time(); U = Q.gptq_factor(G, K + 512); tf = time.time() - t0
        print(f"K={K}: gptq_factor (damp, inverse, Cholesky) {tf:.1f} s", flush=True)
        for fmt, rnd in (("mxfp4", Q.mxfp4_round_2d), ("mxfp8", Q.mxfp8_round_2d)):
            t0 = time.time(); q = Q.gptq_apply(w, U, fmt); ta = time.time() - t0
            r = Q.calibration_error(G, q - w) / Q.calibration_error(G, rnd(w) - w)
            print(f"K={K} N={N} {fmt}: gptq_apply {ta:.1f} s (error on the calibration rows {r:.3f} of round-to-nearest's; random inputs)", flush=True)
    sys.exit(0)
from dia_hip import calib as CAL
from dia_hip import score as S
from dia_hip.engine import DecodeSession, DeviceWeights
from dia_hip.tokens import effective_text, encode_text, synthetic_text
from dia_hip.weights import param_shapes, synthetic_state_dict
HBM_PEAK = 8.0e12                      # bytes/s, MI355X data sheet
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 48
REPS = 3
dev = torch.device("cuda:0")
w = DeviceWeights(cfg, synthetic_state_dict(cfg, seed=1234, std=0.02, device=dev), dev)
shp = param_shapes(cfg)
packed = sum(CAL.gram_tiles(CAL.contraction_size(t[0], shp[t[0]])) * 8192 for t in CAL.decoder_tap_names(cfg))
bound_ms = 2 * packed / HBM_PEAK * 1e3
print(f"packed Gram matrices of all {len(CAL.decoder_tap_names(cfg))} taps: {packed / 1e9:.2f} GB; lower bound of a step's Gram traffic {bound_ms:.3f} ms at {HBM_PEAK / 1e12:.1f} TB/s", flush=True)
rs = np.random.RandomState(3)
for B in (1, 8):
    ids = [encode_text(effective_text(synthetic_text(L, cfg)), cfg) for L in (128, 32, 64, 96, 192, 256, 384, 512)][:B]
    rows = [S.teacher_rows(cfg, rs.randint(0, 1024, size=(steps + 17, cfg.data.channels)))[: steps + 18] for _ in ids]
    mt = rows[0].shape[0]
    for rep in range(REPS):
        ms = {}
        for tag, kw in (("gram", dict(calibrate="gram")), ("stats", dict(calibrate=True)), ("plain", dict())):
            s = DecodeSession(w, ids, kv_dtype="bf16", max_tokens=mt, cfg_scale=3.0, temperature=0.0, teacher_tokens=rows, score=True, **kw)
            s.prefill(); s.sync()
            s.decode(16, True); s.sync()
            t0 = time.time(); s.decode(steps, True); s.sync(); ms[tag] = (time.time() - t0) / steps * 1e3
            launches = s.launches_per_step()
            s.close()
            print(f"batch {B} rep {rep} {tag:5s}: {ms[tag]:8.3f} ms/step ({launches} launches)", flush=True)
        extra = ms["gram"] - ms["plain"]
        print(f"    batch {B} rep {rep}: Gram taps cost {extra:.3f} ms/step over the plain scoring step ({ms['stats'] - ms['plain']:.3f} for dia_act_stats); "
              f"bound {bound_ms:.3f} ms, achieved {bound_ms / extra:.2f} of HBM peak", flush=True)
