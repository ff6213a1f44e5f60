"""One self-attention step on an FP8 self cache (DESIGN.md "FP8 self K/V"), stated in numpy float64: RoPE the new key, quantise it
and the new value with dia_hip/quant.py quantize_kv_fp8 (e4m3 bytes, one power-of-two scale per key), put them into slot cur - 1,
and attend with the G query heads of the kv head over the dequantised keys 0 .. cur - 1.  Everything is per (cache row, kv head):
k8 / v8 are uint8 [T, 128] (V in key order, not blocked), ks / vs float32 [T]."""
import numpy as np
import torch

from dia_hip.quant import dequantize_kv_fp8, quantize_kv_fp8


def rope(x, cos, sin):
    """x [..., 128] float64, cos / sin [64] of the position: the reference's half-split rotation (dia/layers.py:161-173)"""
    x = np.asarray(x, dtype=np.float64)
    c, s = np.asarray(cos, dtype=np.float64), np.asarray(sin, dtype=np.float64)
    x1, x2 = x[..., :64], x[..., 64:]
    return np.concatenate([x1 * c - x2 * s, x1 * s + x2 * c], axis=-1)


def quantize(x):
    """[..., 128] float64 -> (bytes uint8 [..., 128], scales float32 [...]) by quantize_kv_fp8"""
    q, s = quantize_kv_fp8(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)))
    return q.numpy(), s.numpy()


def dequantize(q, s):
    return dequantize_kv_fp8(torch.from_numpy(np.ascontiguousarray(q)), torch.from_numpy(np.ascontiguousarray(s))).double().numpy()


def attend(q_roped, k8, ks, v8, vs, n):
    """softmax(q K^T / sqrt(128)) V over the dequantised keys 0 .. n - 1: q_roped [G, 128] -> [G, 128] float64"""
    K, V = dequantize(k8[:n], ks[:n]), dequantize(v8[:n], vs[:n])
    s = (np.asarray(q_roped, dtype=np.float64) @ K.T) / np.sqrt(128.0)
    p = np.exp(s - s.max(axis=-1, keepdims=True))
    return (p / p.sum(axis=-1, keepdims=True)) @ V


def step(q, k_new, v_new, cos, sin, k8, ks, v8, vs, cur):
    """q [G, 128], k_new / v_new [128] as the projections leave them, cos / sin [64] of position cur, the cache of one (row, kv
    head) and cur = the number of keys once the new one is in.  Returns (out [G, 128], k8, ks, v8, vs), the cache as copies with
    slot cur - 1 written and nothing else touched."""
    k8, ks, v8, vs = (np.array(t, copy=True) for t in (k8, ks, v8, vs))
    k8[cur - 1], ks[cur - 1] = quantize(rope(k_new, cos, sin))
    v8[cur - 1], vs[cur - 1] = quantize(np.asarray(v_new, dtype=np.float64))
    return attend(rope(q, cos, sin), k8, ks, v8, vs, cur), k8, ks, v8, vs
