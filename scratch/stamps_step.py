"""Workgroup timelines of the 1-4-row GEMV kinds INSIDE a graph-replayed batch-1 step of the 18-layer model (bench.py's weights).
Needs the stamp build with the table grouped by kind:
  make -C dia-tts-prune_amd/csrc BUILD=build_dbg OUT=../../scratch/libdia_dbg.so EXTRA="-DDIA_DBG_STAMPS -DDIA_DBG_STAMP_KINDS"
  DIA_HIP_LIB=scratch/libdia_dbg.so [DIA_TUNE=gemv_spec=0] python scratch/stamps_step.py
Each kind keeps the stamps of its LAST launch in the step (layer 17's; the logits head).  The stamps cost a few stores per workgroup:
the step is slower than the product's, the differences between kinds and knobs are what is read."""
import ctypes as C, sys
sys.path.insert(0, "dia-tts-prune_amd")
import numpy as np, torch
from dia_hip import binding as hb, config as CF
from dia_hip.engine import DecodeSession, DeviceWeights
from dia_hip.tokens import effective_text, encode_text, synthetic_text
from dia_hip.weights import synthetic_state_dict

d = torch.device("cuda:0"); L = hb.lib()
L.dia_dbg_stamps.argtypes = [C.c_void_p, C.c_int]
cfg = CF.dia_1_6b_config()
w = DeviceWeights(cfg, synthetic_state_dict(cfg, seed=1234, std=0.02, device=d), d)
s = DecodeSession(w, [encode_text(effective_text(synthetic_text(64, cfg)), cfg)], kv_dtype="bf16", max_tokens=80, seeds=[42], ignore_eos=True)
s.prefill()
s.decode(32, use_graph=True)
KINDS = {1: "cq   <2, ScaleStore>", 2: "o/co <2, ResidEmit>", 3: "qkv  deferred consumer <8, 8, 2, .., 2>", 4: "wo   producer <16, 8, 2, .., 1>",
         5: "logits consumer, several strips", 6: "wi   <16, 4, 2, true, ..>", 7: "other k_gemv_small"}
rows = {k: [] for k in KINDS}
for rep in range(5):
    s.decode(4, use_graph=True); s.sync()
    buf = np.zeros(4096 * 8, dtype=np.int64)
    assert L.dia_dbg_stamps(buf.ctypes.data_as(C.c_void_p), 4096 * 8) == 0
    tab = buf.reshape(8, 512, 8)[:, :, :6].astype(np.float64)
    for k in KINDS:
        st = tab[k]; st = st[st[:, 0] > 0]
        if not len(st): continue
        st = st[st[:, 0] > st[:, 0].max() - 2000]           # the last launch of this kind only (20 us window)
        us = (st - st[:, 0].min()) / 100.0
        rel = lambda a, b: us[:, a] - us[:, b]
        q = {"wgs": len(st), "spread": us[:, 0].max(), "to_w": rel(1, 0), "to_a": rel(2, 0), "tail": rel(5, 3), "life": rel(5, 0), "whole": us[:, 5].max()}
        rows[k].append(q)
f = lambda v: f"{v.min():5.2f}/{v.mean():5.2f}/{v.max():5.2f}"
print("tune gemv_spec =", L.dia_get_tuning(b"gemv_spec"), " (us; min/mean/max over the workgroups of the launch, then over 5 replays the median replay is printed)")
for k, name in KINDS.items():
    if not rows[k]: continue
    r = sorted(rows[k], key=lambda q: q["whole"])[len(rows[k]) // 2]
    sp = [q["spread"] for q in rows[k]]
    print(f"{name:42s} wgs {r['wgs']:3d}  start spread {r['spread']:4.2f} (5 replays {min(sp):4.2f}..{max(sp):4.2f})  start->weights issued {f(r['to_w'])}  "
          f"start->operand staged {f(r['to_a'])}  last MFMA->end {f(r['tail'])}  workgroup life {f(r['life'])}  first start->last end {r['whole']:5.2f}")
s.close()
