"""Decode with the MXFP4 weight streams (DeviceWeights quant="mxfp4") on a real MI355X: the mid model with an MXFP4-quantised
checkpoint, f32 K/V, teacher-forced against the oracle ON THE SAME quantised state dict (logits <= 1e-3, the north-star bound;
samples identical) — parity of a second encoding of the same numbers, not "how lossy is fp4" —, free runs with the streams on
and off, a slot session, the deferred wo merge beside MXFP4 streams on a model wide enough to take it, and Dia-1.6B shapes."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from dia_hip import binding as hb
from dia_hip import config as C
from dia_hip.engine import DecodeSession, DeviceWeights, Request
from dia_hip.quant import mxfp4_quantize_state_dict
from dia_hip.tokens import effective_text, encode_text, synthetic_text
from dia_hip.weights import synthetic_state_dict
from oracle import dia_oracle as O

TEXT = "[S1] Dia is an open weights text to dialogue model. [S2] You get full control over scripts and voices."
EVERY = 0x7f7f


@pytest.fixture(autouse=True)
def knobs_restored():
    yield
    hb.set_tuning("mxfp4", -1)
    hb.set_tuning("wo_defer", -1)


@pytest.fixture(scope="module")
def mid_f4():
    cfg = C.mid_config()
    sd = mxfp4_quantize_state_dict(cfg, synthetic_state_dict(cfg, seed=1234, std=0.02))
    return cfg, sd, DeviceWeights(cfg, sd, torch.device("cuda:0"), quant="mxfp4")


def _teacher_forced(cfg, sd, w, texts, mt):
    try:
        torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
    except Exception:
        pass
    dm = O.Dims.of(cfg)
    runs, noises = [], []
    for b, t in enumerate(texts):
        nz = O.exp_noise(42 + b, mt - 1, dm.C, dm.tgt_vocab)
        runs.append(O.generate(sd, cfg, t, max_tokens=mt, noise=nz, mirror=False))
        noises.append(nz)
    ids = [encode_text(effective_text(t), cfg) for t in texts]
    s = DecodeSession(w, ids, kv_dtype="f32", max_tokens=mt, noise=torch.stack(noises), teacher_tokens=[r.tokens for r in runs])
    s.prefill()
    worst = 0.0
    for i in range(mt - 1):
        s.decode(1, use_graph=False)
        lg = s.logits_host()
        for b, r in enumerate(runs):
            if i < len(r.logits):
                worst = max(worst, float(np.abs(lg[b] - r.logits[i]).max()))
    res = s.results()
    s.close()
    print(f"batch {len(texts)}: logits vs oracle {worst:.3e}")
    assert worst <= 1e-3, worst
    for b, r in enumerate(runs):
        for i, p in enumerate(r.preds):
            assert np.array_equal(res[b].preds[1 + i], p), (b, i)


def _free_run(cfg, w, B, steps=12, **kw):
    ids = [encode_text(effective_text(synthetic_text(32 + 16 * b, cfg)), cfg) for b in range(B)]
    s = DecodeSession(w, ids, kv_dtype="f32", max_tokens=steps + 4, seeds=list(range(B)), ignore_eos=True, **kw)
    s.prefill()
    s.decode(steps, use_graph=True)
    s.sync()
    out = [r.tokens.copy() for r in s.results()]
    s.close()
    return out


@pytest.mark.parametrize("B", [1, 3, 8])
def test_mid_mxfp4_vs_oracle(mid_f4, B):
    cfg, sd, w = mid_f4
    hb.set_tuning("mxfp4", EVERY)
    texts = [TEXT] + [synthetic_text(24 + 24 * b, cfg) for b in range(1, B)]
    _teacher_forced(cfg, sd, w, texts, 13)


@pytest.mark.parametrize("B", [1, 8])
def test_mid_mxfp4_step_runs_the_mxfp4_kernel(mid_f4, B):
    """the step really streams MXFP4: its GEMMs are k_gemm_mx<Fp4, ...> launches with every class on, and none with the knob at 0"""
    cfg, sd, w = mid_f4
    ids = [encode_text(effective_text(synthetic_text(32 + 16 * b, cfg)), cfg) for b in range(B)]
    for mask, expect in ((EVERY, True), (0, False)):
        hb.set_tuning("mxfp4", mask)
        s = DecodeSession(w, ids, kv_dtype="f32", max_tokens=8, seeds=list(range(B)), ignore_eos=True)
        s.prefill()
        s.time_step()
        # (an MX launch keeps its format: "k_gemm_mx<Fp4, 8, 4, false>" -> "k_gemm_mx<Fp4")
        names = set(n.split(",")[0] if n.startswith("k_gemm_mx<") else n.split("<")[0].split("::")[-1] for n in s.last_kernel_names)
        s.close()
        assert ("k_gemm_mx<Fp4" in names) == expect, names
        assert "k_gemm_mx<Fp8" not in names
        if expect:
            assert not any(n.startswith(("k_gemv_small", "k_gemm16")) for n in names), names


@pytest.mark.parametrize("B", [1, 8])
def test_mid_mxfp4_default_mask_equals_dense_tiles(mid_f4, B):
    """a 12-step free run with the default classes as MXFP4 == the same run over the dense tiles of the same checkpoint"""
    cfg, sd, w = mid_f4
    hb.set_tuning("mxfp4", -1)
    on = _free_run(cfg, w, B)
    hb.set_tuning("mxfp4", 0)
    off = _free_run(cfg, w, B)
    for a, b in zip(on, off):
        assert np.array_equal(a, b)


# ---- the deferred wo merge (knob wo_defer) beside MXFP4 streams: a 3-layer model of Dia-1.6B widths, the smallest on which the
# ---- engine takes the deferred form at all (D = 2048, wo K = 8192 in two slices)
def _wide_cfg():
    c = C.dia_1_6b_config()
    m = c.model
    return c.model_copy(update={
        "model": m.model_copy(update={"encoder": m.encoder.model_copy(update={"n_layer": 1}), "decoder": m.decoder.model_copy(update={"n_layer": 3})}),
        "data": c.data.model_copy(update={"text_length": 128, "audio_length": 128})})


@pytest.fixture(scope="module")
def wide_f4():
    cfg = _wide_cfg()
    dev = torch.device("cuda:0")                                    # (quantised and checked on the GPU: seconds less than on the CPU)
    sd = mxfp4_quantize_state_dict(cfg, synthetic_state_dict(cfg, seed=1234, std=0.02, device=dev))
    return cfg, DeviceWeights(cfg, sd, dev, quant="mxfp4")


def _deferred_forms_and_tokens(cfg, w, wo_defer):
    """(wo launches in the deferred producer form, launches in the deferred consumer form) of one step, the GEMM kernels of the
    step, and the tokens of a 12-step graph-replayed free run at batch 1"""
    hb.set_tuning("wo_defer", wo_defer)
    ids = [encode_text(effective_text(synthetic_text(32, cfg)), cfg)]
    s = DecodeSession(w, ids, kv_dtype="f32", max_tokens=20, seeds=[0], ignore_eos=True)
    s.prefill()
    s.time_step()
    names = list(s.last_kernel_names)
    s.close()
    small = [n for n in names if "k_gemv_small<" in n]
    forms = (sum(n.endswith(", 1>") for n in small), sum(n.endswith(", 2>") for n in small))
    return forms, sum("k_gemm_mx<Fp4," in n for n in names), _free_run(cfg, w, 1)[0]


@pytest.mark.parametrize("mask,f4_launches", [(-1, 7), (1 << 5, 3), (1 << 6, 1), (1 << 0, 3), (0, 0)],
                         ids=["default", "wo", "logits", "qkv", "none"])
def test_wide_mxfp4_on_either_side_keeps_the_in_launch_merge(wide_f4, mask, f4_launches):
    """An MXFP4 stream on wo (the default classes, or wo alone) or on a launch behind a wo (the logits head, the next layer's
    q/k/v projection) keeps wo's in-launch merge for the whole model, as an MXFP8 one does: no launch takes a deferred form
    whatever wo_defer says, and the tokens are those of wo_defer = 0.  With no class on (mask 0: dense tiles, the streams merely
    resident) the same weights DO take the deferred form — so the counts above are not zero for want of a model that could."""
    cfg, w = wide_f4
    nl = cfg.model.decoder.n_layer
    hb.set_tuning("mxfp4", mask)
    f_off, n_off, t_off = _deferred_forms_and_tokens(cfg, w, 0)
    f_on, n_on, t_on = _deferred_forms_and_tokens(cfg, w, -1)
    assert n_off == n_on == f4_launches                 # default: wi, wo of 3 layers + logits
    assert f_off == (0, 0)
    assert f_on == ((nl, nl) if mask == 0 else (0, 0))
    assert np.array_equal(t_on, t_off)


def test_dia16b_mxfp4_vs_oracle():
    """Dia-1.6B shapes (synthetic weights), every class as MXFP4, batch 1, 3 teacher-forced steps: the K = 8192 wo split two ways,
    the 16 384-column wi and the logits head in their persistent forms inside a step"""
    cfg = C.dia_1_6b_config()
    dev = torch.device("cuda:0")
    sd_gpu = mxfp4_quantize_state_dict(cfg, synthetic_state_dict(cfg, seed=1234, std=0.02, device=dev))
    w = DeviceWeights(cfg, sd_gpu, dev, quant="mxfp4")
    sd = {k: v.cpu() for k, v in sd_gpu.items()}
    del sd_gpu
    hb.set_tuning("mxfp4", EVERY)
    _teacher_forced(cfg, sd, w, [TEXT], 4)


def test_mid_mxfp4_slot_session_equals_closed_batch(mid_f4):
    cfg, sd, w = mid_f4
    hb.set_tuning("mxfp4", EVERY)
    mt, seeds, s_cap = 9, [42, 7], 128
    ids = [encode_text(effective_text(t), cfg) for t in (TEXT, synthetic_text(40, cfg))]
    a = DecodeSession(w, ids, kv_dtype="f32", max_tokens=mt, seeds=seeds, cfg_scale=2.5, temperature=1.1, top_p=0.9, top_k=50, s_cap=s_cap)
    a.prefill()
    a.decode(mt - 1)
    want = a.results()
    a.close()
    b = DecodeSession.open(w, 2, s_cap=s_cap, kv_dtype="f32", max_tokens=mt)
    try:
        b.admit([Request(i, seed=sd_, max_tokens=mt, cfg_scale=2.5, temperature=1.1, top_p=0.9, top_k=50) for i, sd_ in zip(ids, seeds)])
        b.decode(mt - 1)
        got = [b.collect(0), b.collect(1)]
    finally:
        b.close()
    for g, w_ in zip(got, want):
        assert np.array_equal(g.tokens, w_.tokens) and g.last_step == w_.last_step
