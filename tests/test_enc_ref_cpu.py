"""tests/enc_ref.py pinned on the CPU: the float64 encoder and cross-K/V restatements against the vectors recorded from the
reference (tests/golden/ref_mid.npz, the 1e-5 of test_oracle_golden.py), the packed attention reference against oracle.sdpa
evaluated in float64 on a ragged batch, and its RoPE tables against the ones the device is given."""
import numpy as np
import torch

import enc_ref as R
from dia_hip import config as C
from dia_hip import layout as lay
from dia_hip.weights import synthetic_state_dict
from oracle import dia_oracle as O


def test_encoder_and_cross_kv_refs_match_the_golden_vectors(golden):
    g = golden("ref_mid.npz")
    cfg = C.mid_config()
    sd = R.device_weights(synthetic_state_dict(cfg, seed=int(g["weight_seed"]), std=float(g["weight_std"])))
    L = int(g["L"])
    enc = R.encoder_ref(sd, cfg, g["text_ids"][:L])
    assert enc.dtype == torch.float64 and tuple(enc.shape) == (L, cfg.model.encoder.n_embd)
    assert np.abs(enc.numpy() - g["enc_out_cond"]).max() <= 1e-5
    kv = R.cross_kv_ref(sd, cfg, enc)
    assert len(kv) == cfg.model.decoder.n_layer
    for (k, v), kk, vv in ((kv[0], "cross_k_first", "cross_v_first"), (kv[-1], "cross_k_last", "cross_v_last")):
        assert k.dtype == torch.float64 and v.dtype == torch.float64
        assert np.abs(k.numpy() - g[kk]).max() <= 1e-5
        assert np.abs(v.numpy() - g[vv]).max() <= 1e-5


def test_device_weights_round_the_dense_kernels_only():
    sd = {"encoder.layers.0.self_attention.q_proj.weight": torch.tensor([1.0 + 2.0 ** -10]),
          "encoder.layers.0.pre_sa_norm.weight": torch.tensor([1.0 + 2.0 ** -10]),
          "encoder.embedding.weight": torch.tensor([1.0 + 2.0 ** -10])}
    w = R.device_weights(sd)
    assert all(t.dtype == torch.float64 for t in w.values())
    assert w["encoder.layers.0.self_attention.q_proj.weight"].item() == 1.0          # bf16: 8 significand bits
    assert w["encoder.layers.0.pre_sa_norm.weight"].item() == 1.0 + 2.0 ** -10
    assert w["encoder.embedding.weight"].item() == 1.0 + 2.0 ** -10


def test_rope_tables_are_the_device_tables():
    cos, sin = R.rope_tables64(1025, 128, 1, 10000)
    c32, s32 = lay.rope_tables(1025, 128, 1, 10000)
    assert cos.dtype == torch.float64 and torch.equal(cos, c32.double()) and torch.equal(sin, s32.double())


def test_enc_attn_ref_equals_oracle_sdpa_in_float64():
    """a ragged packed batch (an empty utterance, one key, a partial and several whole 32-row blocks, garbage in the padding
    rows) against oracle.rope / oracle.sdpa fed float64 per utterance"""
    torch.manual_seed(3)
    H, lens = 3, [45, 0, 1, 64, 130]
    offs, tot = [], 0
    for n in lens:
        offs.append(tot); tot += (n + 31) // 32 * 32
    qkv = torch.randn(tot, 3 * H * 128 + 8)                      # (columns behind q | k | v are not read)
    live = torch.zeros(tot, dtype=torch.bool)
    for o, n in zip(offs, lens):
        live[o: o + n] = True
    qkv[~live] = float("nan")
    cos, sin = lay.rope_tables(131, 128, 1, 10000)
    out = R.enc_attn_ref(qkv, H, offs, lens, cos, sin)
    assert out.dtype == torch.float64 and tuple(out.shape) == (tot, H, 128)
    assert (out[~live] == 0).all()
    c64, s64 = cos.double(), sin.double()
    for o, n in zip(offs, lens):
        if n == 0:
            continue
        x = qkv[o: o + n, : 3 * H * 128].double().reshape(n, 3, H, 128)

        def rope(t):       # oracle.rope's formula (it casts x to float32; the float64 statement of it)
            c, s = c64[:n, None], s64[:n, None]
            return torch.cat((t[..., :64] * c - t[..., 64:] * s, t[..., :64] * s + t[..., 64:] * c), dim=-1)

        q, k, v = rope(x[:, 0]), rope(x[:, 1]), x[:, 2]
        want = O.sdpa(q.transpose(0, 1)[None], k.transpose(0, 1)[None], v.transpose(0, 1)[None], None)[0].transpose(0, 1)
        assert want.dtype == torch.float64
        assert (out[o: o + n] - want).abs().max().item() <= 1e-13
    # the float32 statement of the same formula is what the GPU tests size their tolerance with
    out32 = R.enc_attn_ref(qkv, H, offs, lens, cos, sin, dtype=torch.float32)
    assert out32.dtype == torch.float32 and (out32.double() - out).abs().max().item() <= 2e-5
