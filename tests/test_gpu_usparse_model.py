"""Decode with the unstructured sparse weight streams (DeviceWeights sparse="unstructured") on a real MI355X: the mid model pruned
60 % unstructured, f32 K/V, teacher-forced against the oracle ON THE SAME pruned state dict (logits <= 1e-3, the north-star bound;
samples identical), the launch classes of the knob usparse, and a 2-layer decoder of Dia-1.6B widths (wo's split-K at K = 8192)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from dia_hip import binding as hb
from dia_hip import config as C
from dia_hip.engine import DecodeSession, DeviceWeights, Request
from dia_hip.pruning import unstructured_prune_state_dict
from dia_hip.tokens import effective_text, encode_text, synthetic_text
from dia_hip.weights import synthetic_state_dict
from oracle import dia_oracle as O

TEXT = "[S1] Dia is an open weights text to dialogue model. [S2] You get full control over scripts and voices."
EVERY = 0x7f


@pytest.fixture(autouse=True)
def knobs_restored():
    yield
    hb.set_tuning("usparse", -1)
    hb.set_tuning("wo_defer", -1)


@pytest.fixture(scope="module")
def mid_us():
    cfg = C.mid_config()
    sd = unstructured_prune_state_dict(cfg, synthetic_state_dict(cfg, seed=1234, std=0.02), 0.6)
    w = DeviceWeights(cfg, sd, torch.device("cuda:0"), sparse="unstructured", compact="off")
    assert sum(L[k + "us"] is not None for L in w.dec_layers for k in ("qkv", "o", "cq", "co", "wi", "wo")) > 0
    return cfg, sd, w


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


def _free_run(cfg, w, B, steps=12):
    ids = [encode_text(effective_text(synthetic_text(32 + 16 * b, cfg)), cfg) for b in range(B)]
    s = DecodeSession(w, ids, kv_dtype="f32", max_tokens=steps + 4, seeds=list(range(B)), ignore_eos=True)
    s.prefill()
    s.decode(steps, use_graph=True)
    s.sync()
    out = [r.tokens.copy() for r in s.results()]
    s.close()
    return out


def _step_names(cfg, w, B):
    ids = [encode_text(effective_text(synthetic_text(32 + 16 * b, cfg)), cfg) for b in range(B)]
    s = DecodeSession(w, ids, kv_dtype="f32", max_tokens=8, seeds=list(range(B)), ignore_eos=True)
    s.prefill()
    s.time_step()
    names = list(s.last_kernel_names)
    s.close()
    return names


@pytest.mark.parametrize("B", [1, 2])
def test_mid_usparse_vs_oracle(mid_us, B):
    cfg, sd, w = mid_us
    hb.set_tuning("usparse", EVERY)
    texts = [TEXT] + [synthetic_text(24 + 24 * b, cfg) for b in range(1, B)]
    _teacher_forced(cfg, sd, w, texts, 13)


def test_mid_usparse_launch_classes(mid_us):
    """every class on: one k_gemm_us launch per matrix that has a stream; knob 0: none, and the tokens of the plain dense session;
    batch 3 (6 rows): no stream launch"""
    cfg, sd, w = mid_us
    have = sum(L[k + "us"] is not None for L in w.dec_layers for k in ("qkv", "o", "cq", "co", "wi", "wo")) + (w.logits_us is not None)
    hb.set_tuning("usparse", EVERY)
    assert sum("k_gemm_us<" in n for n in _step_names(cfg, w, 1)) == have
    assert sum("k_gemm_us<" in n for n in _step_names(cfg, w, 3)) == 0
    on = _free_run(cfg, w, 2)
    hb.set_tuning("usparse", 0)
    assert sum("k_gemm_us<" in n for n in _step_names(cfg, w, 1)) == 0
    off = _free_run(cfg, w, 2)
    dense = _free_run(cfg, DeviceWeights(cfg, sd, torch.device("cuda:0"), compact="off"), 2)
    for a, b in zip(off, dense):
        assert np.array_equal(a, b)
    for a, b in zip(on, dense):                              # the same numbers in another summation order: the same samples here
        assert np.array_equal(a, b)


def test_wide_decoder_usparse_tokens_equal_dense():
    """2 layers of Dia-1.6B widths (D = 2048, hidden 8192): wo streams at K = 8192 in two K slices and the whole model keeps wo's
    in-launch merge (no launch takes a deferred form, k_gemv_small<.., 1> / <.., 2>), while the same weights with no class on DO
    take it; the tokens are those of a plain dense DeviceWeights of the same checkpoint"""
    c = C.dia_1_6b_config()
    m = c.model
    cfg = c.model_copy(update={
        "model": m.model_copy(update={"encoder": m.encoder.model_copy(update={"n_layer": 1}), "decoder": m.decoder.model_copy(update={"n_layer": 2})}),
        "data": c.data.model_copy(update={"text_length": 128, "audio_length": 128})})
    dev = torch.device("cuda:0")
    sd = unstructured_prune_state_dict(cfg, synthetic_state_dict(cfg, seed=1234, std=0.02, device=dev), 0.6)
    w = DeviceWeights(cfg, sd, dev, sparse="unstructured", compact="off")
    assert all(L["wous"] is not None for L in w.dec_layers)
    hb.set_tuning("usparse", EVERY)
    names = _step_names(cfg, w, 1)
    assert sum("k_gemm_us<" in n and ", 16, false>" in n for n in names) == 2, names     # wo: 16 k-tiles per wave, one strip per workgroup

    def deferred(ns):                                        # (producer, consumer) launches of the deferred wo merge
        small = [n for n in ns if "k_gemv_small<" in n]
        return sum(n.endswith(", 1>") for n in small), sum(n.endswith(", 2>") for n in small)
    assert deferred(names) == (0, 0), names
    on = _free_run(cfg, w, 1)
    hb.set_tuning("usparse", 0)
    assert deferred(_step_names(cfg, w, 1)) == (2, 2)        # the streams merely resident: the deferred form is taken
    off = _free_run(cfg, w, 1)
    plain = _free_run(cfg, DeviceWeights(cfg, sd, dev, compact="off"), 1)
    assert np.array_equal(off[0], plain[0])
    assert np.array_equal(on[0], plain[0])


def test_mid_usparse_slot_session_equals_closed_batch(mid_us):
    """every class forced on (the closed batch's step is checked to run k_gemm_us): the requests admitted to a two-slot session
    return the tokens of their closed-batch run"""
    cfg, sd, w = mid_us
    hb.set_tuning("usparse", EVERY)
    mt, seeds, s_cap = 9, [42, 7], 128
    ids = [encode_text(effective_text(t), cfg) for t in (TEXT, synthetic_text(40, cfg))]
    kw = dict(cfg_scale=2.5, temperature=1.1, top_p=0.9, top_k=50)
    a = DecodeSession(w, ids, kv_dtype="f32", max_tokens=mt, seeds=seeds, s_cap=s_cap, **kw)
    a.prefill()
    a.time_step()
    assert any("k_gemm_us<" in n for n in a.last_kernel_names)
    a.close()
    a = DecodeSession(w, ids, kv_dtype="f32", max_tokens=mt, seeds=seeds, s_cap=s_cap, **kw)
    a.prefill()
    a.decode(mt - 1)
    want = a.results()
    a.close()
    b = DecodeSession.open(w, 2, s_cap=s_cap, kv_dtype="f32", max_tokens=mt)
    try:
        b.admit([Request(i, seed=sd_, max_tokens=mt, **kw) for i, sd_ in zip(ids, seeds)])
        b.decode(mt - 1)
        got = [b.collect(0), b.collect(1)]
    finally:
        b.close()
    for g, w_ in zip(got, want):
        assert np.array_equal(g.tokens, w_.tokens) and g.last_step == w_.last_step
