"""Decode with the 2:4 sparse weight streams (DeviceWeights sparse="2:4") on a real MI355X: the mid model and Dia-1.6B with a 2:4
checkpoint, f32 K/V, teacher-forced against the oracle on the same zero-holding state dict (logits <= 1e-3, samples identical), and
free-running token buffers identical between graph replay and eager steps."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from dia_hip import config as C
from dia_hip.engine import DecodeSession, DeviceWeights
from dia_hip.pruning import semi_structured_prune_state_dict
from dia_hip.tokens import effective_text, encode_text, synthetic_text
from dia_hip.weights import synthetic_state_dict
from oracle import dia_oracle as O

TEXT = "[S1] Dia is an open weights text to dialogue model. [S2] You get full control over scripts and voices."


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
    assert worst <= 1e-3, worst
    for b, r in enumerate(runs):
        for i, p in enumerate(r.preds):
            assert np.array_equal(res[b].preds[1 + i], p), (b, i)
    return worst


@pytest.fixture(scope="module")
def mid24():
    cfg = C.mid_config()
    sd = semi_structured_prune_state_dict(cfg, synthetic_state_dict(cfg, seed=1234, std=0.02))
    return cfg, sd, DeviceWeights(cfg, sd, torch.device("cuda:0"), sparse="2:4")


@pytest.mark.parametrize("B", [1, 3, 8])
def test_mid_2of4_vs_oracle(mid24, B):
    cfg, sd, w = mid24
    texts = [TEXT] + [synthetic_text(24 + 24 * b, cfg) for b in range(1, B)]
    worst = _teacher_forced(cfg, sd, w, texts, 9)
    print(f"mid 2:4, batch {B}: logits vs oracle {worst:.3e}")


@pytest.mark.parametrize("B", [1, 8])
def test_mid_2of4_graph_equals_eager(mid24, B):
    cfg, sd, w = mid24
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


def test_dia16b_2of4_vs_oracle():
    """Dia-1.6B shapes, 2:4 checkpoint, a few teacher-forced steps at batch 1 and at batch 8 mixed (texts 32..512 bytes)"""
    cfg = C.dia_1_6b_config()
    sd = semi_structured_prune_state_dict(cfg, synthetic_state_dict(cfg, seed=1234, std=0.02))
    w = DeviceWeights(cfg, sd, torch.device("cuda:0"), sparse="2:4")
    for texts in ([TEXT], [synthetic_text(L, cfg) for L in (32, 64, 96, 128, 192, 256, 384, 512)]):
        worst = _teacher_forced(cfg, sd, w, texts, 4)
        print(f"Dia-1.6B 2:4, batch {len(texts)}: logits vs oracle {worst:.3e}")
