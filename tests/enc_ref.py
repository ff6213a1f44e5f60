"""float64 references of the text encoder, plain torch on the CPU: the packed bidirectional attention that
dia_enc_attn computes, the encoder pass and the cross K/V precompute.

The formulas are those of oracle/dia_oracle.py (encoder_forward, cross_kv, rope, rmsnorm), restated so that EVERY
operation runs in float64, the norm included (the oracle's rmsnorm casts to float32).  The weights are taken as the
device holds them (device_weights): DeviceWeights streams every DenseGeneral kernel as one bf16 plane, embeddings and
norm weights as fp32.  The RoPE tables are part of the model's definition: cos / sin of the fp32 angle
fp32(pos) * fp32(inv_freq), the op sequence of the reference that dia_hip.layout.rope_tables also follows; the
references take them as given and only widen them to float64."""
import math

import numpy as np
import torch

HD = 128


def rope_tables64(npos, head_dim, min_ts, max_ts):
    """cos / sin [npos, head_dim / 2]: fp32 tables (oracle.rope_inv_freq, oracle.rope), widened to float64"""
    half = head_dim // 2
    fraction = (2.0 * torch.arange(0, half)) / head_dim
    inv_freq = (1.0 / (min_ts * (max_ts / min_ts) ** fraction)).to(torch.float32)
    f = torch.arange(npos, dtype=torch.float32).unsqueeze(-1) * inv_freq
    return torch.cos(f.to(torch.float32)).double(), torch.sin(f.to(torch.float32)).double()


def rope_ref(x, cos, sin):
    """half-split rotary embedding of x [T, N, H] at positions 0..T-1; cos / sin [>= T, H / 2] in x's dtype"""
    T, h = x.shape[0], x.shape[-1] // 2
    c, s = cos[:T, None, :], sin[:T, None, :]
    x1, x2 = x[..., :h], x[..., h:]
    return torch.cat((x1 * c - x2 * s, x1 * s + x2 * c), dim=-1)


def enc_attn_ref(qkv, H, offs, lens, cos, sin, dtype=torch.float64):
    """Per-utterance, per-head bidirectional attention of a packed batch.  qkv [rows, >= 3 * H * 128] holds q | k | v of H
    heads in its first 3 * H * 128 columns; utterance b occupies rows offs[b] .. offs[b] + lens[b] - 1 and its RoPE
    positions are 0 .. lens[b] - 1.  Returns [rows, H, 128] in `dtype` (float64; float32 gives the same formula in
    single precision, the yardstick of a tolerance): softmax(RoPE(q) RoPE(k)^T / sqrt(128)) v in the live rows, zeros
    in the others.  Rows outside the utterances are never read."""
    qkv = qkv.detach().cpu()
    cos, sin = cos.detach().cpu().to(dtype), sin.detach().cpu().to(dtype)
    out = torch.zeros(qkv.shape[0], H, HD, dtype=dtype)
    scale = 1.0 / math.sqrt(HD)
    for o, L in zip(offs, lens):
        if L == 0:
            continue
        x = qkv[o: o + L, : 3 * H * HD].to(dtype).reshape(L, 3, H, HD)
        q, k, v = rope_ref(x[:, 0], cos, sin), rope_ref(x[:, 1], cos, sin), x[:, 2]
        s = torch.einsum("qhd,khd->hqk", q, k) * scale
        out[o: o + L] = torch.einsum("hqk,khd->qhd", torch.softmax(s, dim=-1), v)
    return out


def device_weights(sd):
    """the checkpoint as the device holds it, in float64: DenseGeneral kernels rounded to bf16 (DeviceWeights with
    weight_planes = 1), embeddings and norm weights fp32"""
    out = {}
    for k, v in sd.items():
        v = v.detach().cpu().float()
        if not (k.endswith("norm.weight") or "embedding" in k):
            v = v.bfloat16().float()
        out[k] = v.double()
    return out


def rmsnorm_ref(x, g, eps):
    return x * torch.rsqrt((x * x).mean(dim=-1, keepdim=True) + eps) * g


def encoder_ref(sd, cfg, ids):
    """oracle.encoder_forward for ONE utterance without padding: ids [L] (the non-pad byte tokens) -> [L, n_embd] float64.
    sd is device_weights(checkpoint) (float64 tensors)."""
    m, e = cfg.model, cfg.model.encoder
    eps = float(m.normalization_layer_epsilon)
    ids = torch.as_tensor(np.asarray(ids), dtype=torch.long)
    L = int(ids.shape[0])
    cos, sin = rope_tables64(max(L, 1), e.head_dim, m.rope_min_timescale, m.rope_max_timescale)
    scale = 1.0 / math.sqrt(e.head_dim)
    x = sd["encoder.embedding.weight"][ids]
    for i in range(e.n_layer):
        p = f"encoder.layers.{i}."
        h = rmsnorm_ref(x, sd[p + "pre_sa_norm.weight"], eps)
        q = rope_ref(torch.einsum("te,enh->tnh", h, sd[p + "self_attention.q_proj.weight"]), cos, sin)
        k = rope_ref(torch.einsum("te,enh->tnh", h, sd[p + "self_attention.k_proj.weight"]), cos, sin)
        v = torch.einsum("te,enh->tnh", h, sd[p + "self_attention.v_proj.weight"])
        a = torch.einsum("nqk,knh->qnh", torch.softmax(torch.einsum("qnh,knh->nqk", q, k) * scale, dim=-1), v)
        x = x + torch.einsum("tnh,nhe->te", a, sd[p + "self_attention.o_proj.weight"])
        h = rmsnorm_ref(x, sd[p + "post_sa_norm.weight"], eps)
        f = torch.einsum("te,egf->tgf", h, sd[p + "mlp.wi_fused.weight"])
        x = x + (torch.nn.functional.silu(f[:, 0]) * f[:, 1]) @ sd[p + "mlp.wo.weight"]
    return rmsnorm_ref(x, sd["encoder.norm.weight"], eps)


def cross_kv_ref(sd, cfg, enc_out):
    """oracle.cross_kv for one utterance: enc_out [L, n_embd] float64 -> per decoder layer (K, V), each
    [cross_query_heads, L, 128] float64 (K = RoPE(k_proj(enc_out)) at positions 0..L-1, V = v_proj(enc_out))."""
    m, d = cfg.model, cfg.model.decoder
    L = int(enc_out.shape[0])
    cos, sin = rope_tables64(max(L, 1), d.cross_head_dim, m.rope_min_timescale, m.rope_max_timescale)
    out = []
    for i in range(d.n_layer):
        p = f"decoder.layers.{i}.cross_attention."
        k = rope_ref(torch.einsum("te,enh->tnh", enc_out, sd[p + "k_proj.weight"]), cos, sin).transpose(0, 1)
        v = torch.einsum("te,enh->tnh", enc_out, sd[p + "v_proj.weight"]).transpose(0, 1)
        out.append((k.contiguous(), v.contiguous()))
    return out
