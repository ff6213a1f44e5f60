"""MXFP8 and MXFP4 weight-only quantisation (OCP MX, element type e4m3fn or e2m1, block = 32 consecutive K of one column).

A block of a ``[K, N]`` kernel (K the contraction axis, as DeviceWeights flattens it: ``pruning._kernel_2d``) shares one
power-of-two scale ``X = 2^e`` with ``e = floor(log2(max|w|)) - 8`` (an all-zero block: ``e = 0``), clamped to [-100, 100] and
stored as E8M0 (``e + 127``); an element is ``w / X`` clamped to +-448 and rounded to nearest-even e4m3.  The clamp comes
BEFORE the cast: the block maximum can land in (448, 512), and ``tensor.to(torch.float8_e4m3fn)`` does not saturate.

An e4m3 value times a power of two is exactly a bf16 value, so a dequantised checkpoint is an ordinary state dict that the
dense bf16 tiles, the oracle and the reference run exactly; the fp8 stream (layout.tile_weight_fp8, csrc/gemm_mx.hip) is a
second encoding of the same numbers.  "Is MXFP8-representable" is ``dequantise(quantise(w)) == w`` (``is_mxfp8``), which
holds for everything the quantiser emits (quantise(dequantise(q)) reproduces elements and scales bit for bit).

MXFP4 (``mxfp4_*``) is the same scheme with e2m1 elements: magnitudes {0, 0.5, 1, 1.5, 2, 3, 4, 6} (codes 0..7) and a sign bit
(code bit 3), ``e = floor(log2(max|w|)) - 2``, ``w / X`` clamped to +-6 and rounded to the nearest magnitude, a tie to the code with
an even mantissa bit (the even code).  The rounding is a comparison against the seven midpoints, no cast to an fp4 dtype.  An e2m1
value times a power of two is a bf16 value as well, so everything above holds for ``is_mxfp4`` and the fp4 stream
(layout.tile_weight_fp4) too.
"""

from __future__ import annotations

from collections import OrderedDict
from typing import Dict, List, Tuple

import torch

from .config import DiaConfig
from .pruning import _kernel_2d

MX_BLOCK = 32            # K per scale
E4M3_MAX = 448.0
E8M0_BIAS = 127
E_MIN, E_MAX = -100, 100  # every dequantised value stays a normal bf16


def _blocks(w2d: torch.Tensor) -> torch.Tensor:
    """[K, N] -> fp32 [ceil(K/32), 32, N], K zero-padded to whole blocks"""
    K, N = w2d.shape
    Kp = (K + MX_BLOCK - 1) // MX_BLOCK * MX_BLOCK
    wp = torch.zeros(Kp, N, dtype=torch.float32, device=w2d.device)
    wp[:K] = w2d.float()
    return wp.reshape(Kp // MX_BLOCK, MX_BLOCK, N)


def mxfp8_quantize_2d(w2d: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """[K, N] float -> (elements uint8 [Kp, N] (e4m3fn bits), scales uint8 [Kp/32, N] (E8M0)), Kp = K zero-padded to 32"""
    b = _blocks(w2d)
    amax = b.abs().amax(dim=1)                                            # [KB, N]
    # amax = m * 2^ex with m in [0.5, 1): floor(log2 amax) = ex - 1
    e = torch.frexp(amax)[1].to(torch.int32) - 1 - 8
    e = torch.where(amax > 0, e, torch.zeros_like(e)).clamp_(E_MIN, E_MAX)
    scaled = torch.ldexp(b, -e[:, None, :]).clamp_(-E4M3_MAX, E4M3_MAX)  # exact: a power-of-two factor
    elems = scaled.to(torch.float8_e4m3fn).view(torch.uint8).reshape(-1, b.shape[2])
    return elems.contiguous(), (e + E8M0_BIAS).to(torch.uint8).contiguous()


def mxfp8_dequantize_2d(elements: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """inverse of mxfp8_quantize_2d on the padded shape: fp32 [Kp, N] = element x 2^(scale - 127)"""
    Kp, N = elements.shape
    v = elements.contiguous().view(torch.float8_e4m3fn).float().reshape(Kp // MX_BLOCK, MX_BLOCK, N)
    e = scales.to(torch.int32) - E8M0_BIAS
    return torch.ldexp(v, e[:, None, :]).reshape(Kp, N)


def mxfp8_round_2d(w2d: torch.Tensor) -> torch.Tensor:
    """[K, N] -> fp32 [K, N]: the nearest MXFP8-representable matrix (dequantise(quantise(w)))"""
    return mxfp8_dequantize_2d(*mxfp8_quantize_2d(w2d))[: w2d.shape[0]]


def is_mxfp8(w2d: torch.Tensor) -> bool:
    """True when every value of [K, N] is its block's e4m3 element times the block's power-of-two scale"""
    return bool(torch.equal(mxfp8_round_2d(w2d), w2d.float()))


E2M1_MAX = 6.0
E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)                 # magnitude of code c (bits e e m), bit 3 = sign
E2M1_MIDPOINTS = (0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0)              # midpoint i lies between codes i and i + 1


def mxfp4_quantize_2d(w2d: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """[K, N] float -> (codes uint8 [Kp, N] (e2m1 in the low 4 bits, one per element), scales uint8 [Kp/32, N] (E8M0)), Kp = K
    zero-padded to 32"""
    b = _blocks(w2d)
    amax = b.abs().amax(dim=1)
    e = torch.frexp(amax)[1].to(torch.int32) - 1 - 2
    e = torch.where(amax > 0, e, torch.zeros_like(e)).clamp_(E_MIN, E_MAX)
    scaled = torch.ldexp(b, -e[:, None, :]).clamp_(-E2M1_MAX, E2M1_MAX)
    mag = scaled.abs()
    code = torch.zeros_like(mag, dtype=torch.uint8)
    for i, m in enumerate(E2M1_MIDPOINTS):                               # a tie stays on an even code i, leaves an odd one
        code += (mag > m if i % 2 == 0 else mag >= m).to(torch.uint8)
    code |= ((scaled < 0) & (code > 0)).to(torch.uint8) << 3             # (no negative zero: one code per value)
    return code.reshape(-1, b.shape[2]).contiguous(), (e + E8M0_BIAS).to(torch.uint8).contiguous()


def mxfp4_dequantize_2d(codes: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """inverse of mxfp4_quantize_2d on the padded shape: fp32 [Kp, N] = e2m1 value x 2^(scale - 127)"""
    Kp, N = codes.shape
    lut = torch.tensor(E2M1_VALUES + tuple(-v for v in E2M1_VALUES), dtype=torch.float32, device=codes.device)
    v = lut[(codes & 15).long()].reshape(Kp // MX_BLOCK, MX_BLOCK, N)
    e = scales.to(torch.int32) - E8M0_BIAS
    return torch.ldexp(v, e[:, None, :]).reshape(Kp, N)


def mxfp4_round_2d(w2d: torch.Tensor) -> torch.Tensor:
    """[K, N] -> fp32 [K, N]: the nearest MXFP4-representable matrix (dequantise(quantise(w)))"""
    return mxfp4_dequantize_2d(*mxfp4_quantize_2d(w2d))[: w2d.shape[0]]


def is_mxfp4(w2d: torch.Tensor) -> bool:
    """True when every value of [K, N] is its block's e2m1 element times the block's power-of-two scale"""
    return bool(torch.equal(mxfp4_round_2d(w2d), w2d.float()))


def mxfp8_names(cfg: DiaConfig) -> List[str]:
    """the DenseGeneral kernels a decode step streams: q/k/v, o, cross-q, cross-o, wi, wo of every decoder layer and the
    logits head (the encoder and the cross K/V projections run in the prefill only and stay as they are)"""
    names = []
    for i in range(cfg.model.decoder.n_layer):
        p = f"decoder.layers.{i}."
        names += [p + f"self_attention.{n}_proj.weight" for n in "qkvo"]
        names += [p + "cross_attention.q_proj.weight", p + "cross_attention.o_proj.weight"]
        names += [p + "mlp.wi_fused.weight", p + "mlp.wo.weight"]
    return names + ["decoder.logits_dense.weight"]


mx_names = mxfp8_names        # the same matrices whatever the MX element type


def mxfp8_quantize_state_dict(cfg: DiaConfig, sd: Dict[str, torch.Tensor]) -> "OrderedDict[str, torch.Tensor]":
    """An ordinary fp32 state dict holding the dequantised MXFP8 values of every kernel of ``mxfp8_names(cfg)``, each blocked
    along the K axis of its [K, N] form; everything else untouched.  Idempotent."""
    out: "OrderedDict[str, torch.Tensor]" = OrderedDict((k, v.clone()) for k, v in sd.items())
    for name in mxfp8_names(cfg):
        w = sd[name]
        out[name] = mxfp8_round_2d(_kernel_2d(name, w.float())).reshape(w.shape)
    return out


def mxfp4_quantize_state_dict(cfg: DiaConfig, sd: Dict[str, torch.Tensor]) -> "OrderedDict[str, torch.Tensor]":
    """As mxfp8_quantize_state_dict with e2m1 elements: the dequantised MXFP4 values of every kernel of ``mx_names(cfg)``."""
    out: "OrderedDict[str, torch.Tensor]" = OrderedDict((k, v.clone()) for k, v in sd.items())
    for name in mx_names(cfg):
        w = sd[name]
        out[name] = mxfp4_round_2d(_kernel_2d(name, w.float())).reshape(w.shape)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# FP8 cross K/V (DESIGN.md "FP8 cross K/V"): e4m3 elements with ONE scale per key (the 128 values of a head's K or V row), the
# reference dia_kv_quantize_fp8 (csrc/attn.hip) is pinned to.  The scale is the smallest power of two 2^e with amax / 2^e <= 448
# (so amax / scale lies in (224, 448] and nothing saturates), e >= KV_E_MIN (the smallest normal fp32), 1 for an all-zero key;
# elements round to nearest even.  An e4m3 value times a power of two is a bf16 value: the dequantised cache is an ordinary bf16
# cache, and quantising it again returns the same bytes and scales.
KV_E_MIN = -126


def quantize_kv_fp8(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """[..., 128] (any float dtype; keys in the second-to-last position or flattened into the lead) -> (bytes uint8 [..., 128]
    (e4m3fn bits), scales float32 [...]), one scale per row of the last axis"""
    xf = x.float()
    amax = xf.abs().amax(dim=-1)
    m, ex = torch.frexp(amax)                                             # amax = m * 2^ex, m in [0.5, 1); 448 = 0.875 * 2^9
    e = ex.to(torch.int32) - 9 + (m > 0.875).to(torch.int32)
    e = torch.where(amax > 0, e, torch.zeros_like(e)).clamp_(min=KV_E_MIN)
    scaled = torch.ldexp(xf, -e[..., None]).clamp_(-E4M3_MAX, E4M3_MAX)   # exact: a power-of-two factor (the clamp never bites)
    q = scaled.to(torch.float8_e4m3fn).view(torch.uint8)
    return q.contiguous(), torch.ldexp(torch.ones_like(amax), e).contiguous()


def dequantize_kv_fp8(q: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """inverse of quantize_kv_fp8: float32 [..., 128] = e4m3(byte) x scale, every value bf16-representable"""
    return q.contiguous().view(torch.float8_e4m3fn).float() * scales[..., None].float()
