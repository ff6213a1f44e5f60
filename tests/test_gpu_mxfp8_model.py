"""Decode with the MXFP8 weight streams (DeviceWeights quant="mxfp8") on a real MI355X: the mid model and Dia-1.6B with an
MXFP8-quantised checkpoint, f32 K/V, teacher-forced against the oracle ON THE SAME quantised state dict (logits <= 1e-3, the
north-star bound; samples identical) — parity of a second encoding of the same numbers, not "how lossy is fp8" —, free-running
token buffers identical between graph replay and eager steps, and one bf16-K/V free run.  Every launch class streams MXFP8 here
(knob mxfp8 = 0x7f7f), whatever the measured default enables."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from dia_hip import binding as hb
from dia_hip import config as C
from dia_hip.engine import DecodeSession, DeviceWeights
from dia_hip.quant import mxfp8_quantize_state_dict
from dia_hip.tokens import effective_text, encode_text, synthetic_text
from dia_hip.weights import synthetic_state_dict
from oracle import dia_oracle as O

TEXT = "[S1] Dia is an open weights text to dialogue model. [S2] You get full control over scripts and voices."


@pytest.fixture(autouse=True)
def every_class_streams_mxfp8():
    hb.set_tuning("mxfp8", 0x7f7f)
    yield
    hb.set_tuning("mxfp8", -1)


def _kernels_of_a_step(s):
    s.time_step()
    # (an MX launch keeps its format: "k_gemm_mx<Fp8, 8, 4, false>" -> "k_gemm_mx<Fp8")
    return set(n.split(",")[0] if n.startswith("k_gemm_mx<") else n.split("<")[0].split("::")[-1] for n in s.last_kernel_names)


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
    return worst


@pytest.fixture(scope="module")
def mid_f8():
    cfg = C.mid_config()
    sd = mxfp8_quantize_state_dict(cfg, synthetic_state_dict(cfg, seed=1234, std=0.02))
    return cfg, sd, DeviceWeights(cfg, sd, torch.device("cuda:0"), quant="mxfp8")


@pytest.mark.parametrize("B", [1, 3, 8])
def test_mid_mxfp8_vs_oracle(mid_f8, B):
    cfg, sd, w = mid_f8
    texts = [TEXT] + [synthetic_text(24 + 24 * b, cfg) for b in range(1, B)]
    _teacher_forced(cfg, sd, w, texts, 9)


@pytest.mark.parametrize("B", [1, 8])
def test_mid_mxfp8_step_runs_the_mxfp8_kernel(mid_f8, B):
    """the step really streams MXFP8: its GEMMs are k_gemm_mx<Fp8, ...> launches, and none with the knob at 0"""
    cfg, sd, w = mid_f8
    ids = [encode_text(effective_text(synthetic_text(32 + 16 * b, cfg)), cfg) for b in range(B)]
    for mask, expect in ((0x7f7f, True), (0, False)):
        hb.set_tuning("mxfp8", mask)
        s = DecodeSession(w, ids, kv_dtype="f32", max_tokens=8, seeds=list(range(B)), ignore_eos=True)
        s.prefill()
        names = _kernels_of_a_step(s)
        s.close()
        assert ("k_gemm_mx<Fp8" in names) == expect, names
        if expect:
            assert not any(n.startswith(("k_gemv_small", "k_gemm16")) for n in names), names


@pytest.mark.parametrize("B", [1, 8])
def test_mid_mxfp8_graph_equals_eager(mid_f8, B):
    cfg, sd, w = mid_f8
    ids = [encode_text(effective_text(synthetic_text(32 + 16 * b, cfg)), cfg) for b in range(B)]
    out = []
    for graph in (True, False):
        s = DecodeSession(w, ids, kv_dtype="f32", max_tokens=24, seeds=list(range(B)), ignore_eos=True)
        s.prefill()
        s.decode(20, use_graph=graph)
        s.sync()
        out.append([r.tokens.copy() for r in s.results()])
        s.close()
    for a, b in zip(*out):
        assert np.array_equal(a, b)


def test_mid_mxfp8_bf16_kv_free_run(mid_f8):
    """the default cache format (bf16 K/V, MFMA attention) with the MXFP8 streams: a free run fills the token buffer with codes"""
    cfg, sd, w = mid_f8
    ids = [encode_text(effective_text(synthetic_text(32 + 16 * b, cfg)), cfg) for b in range(2)]
    s = DecodeSession(w, ids, kv_dtype="bf16", max_tokens=24, seeds=[0, 1], ignore_eos=True)
    s.prefill()
    s.decode(20, use_graph=True)
    s.sync()
    res = s.results()
    s.close()
    V = cfg.model.tgt_vocab_size
    for r in res:
        rows = r.tokens[1:21]
        assert rows.min() >= 0 and rows.max() < V


def test_dia16b_mxfp8_vs_oracle():
    """Dia-1.6B shapes, MXFP8 checkpoint, a few teacher-forced steps at batch 1 and at batch 8 mixed (texts 32..512 bytes)"""
    cfg = C.dia_1_6b_config()
    sd = mxfp8_quantize_state_dict(cfg, synthetic_state_dict(cfg, seed=1234, std=0.02))
    w = DeviceWeights(cfg, sd, torch.device("cuda:0"), quant="mxfp8")
    for texts in ([TEXT], [synthetic_text(L, cfg) for L in (32, 64, 96, 128, 192, 256, 384, 512)]):
        _teacher_forced(cfg, sd, w, texts, 4)
