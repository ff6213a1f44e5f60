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
# GPTQ (Frantar et al. 2022) onto the MX grids (DESIGN.md "Gram matrices and GPTQ"): walk the contraction axis and push every
# element's rounding error into the weights not rounded yet, weighted by the Hessian of the layer's output error H = X^T X / rows,
# which calib.GramStats supplies (csrc/gram.hip measures it on the running model).  Offline host code, float64 NumPy.  The grid is
# the one of the functions above: the block's E8M0 exponent by the same rule, taken from the block as the updates so far have left
# it, and the element rule restated in float64 (a float64 -> float32 -> e4m3 cast would round twice).  No activation reordering:
# the MX blocks are fixed runs of 32 K and a permutation would cut across them.
_MX_FMT = {"mxfp4": (2, E2M1_MAX), "mxfp8": (8, E4M3_MAX)}


def _mx_exponent_np(blk, ebias: int):
    """int [N]: the E8M0 exponent of one block [<= 32, N] (float64), the rule of mxfp8_quantize_2d / mxfp4_quantize_2d"""
    import numpy as np
    amax = np.abs(blk).max(axis=0)
    e = np.frexp(amax)[1].astype(np.int64) - 1 - ebias
    return np.clip(np.where(amax > 0, e, 0), E_MIN, E_MAX)


def _mx_round_row_np(v, e, fmt: str):
    """float64 [N] -> the nearest element of the format times 2^e: clamp first, then the ties of mxfp4_quantize_2d (the even code) /
    of the e4m3 cast (nearest even)"""
    import numpy as np
    s = np.clip(np.ldexp(v, -e), -_MX_FMT[fmt][1], _MX_FMT[fmt][1])
    mag = np.abs(s)
    if fmt == "mxfp4":
        code = np.zeros(mag.shape, dtype=np.int64)
        for i, m in enumerate(E2M1_MIDPOINTS):
            code += (mag > m) if i % 2 == 0 else (mag >= m)
        q = np.asarray(E2M1_VALUES)[code]
    else:
        # e4m3fn: 3 mantissa bits, normals from 2^-6, subnormals in steps of 2^-9; rint is nearest-even on the scaled mantissa
        p = np.maximum(np.frexp(mag)[1].astype(np.int64) - 1, -6)
        q = np.ldexp(np.rint(np.ldexp(mag, 3 - p)), p - 3)
    q = np.copysign(q, s)
    if fmt == "mxfp4":
        q = q + 0.0                   # one code per value: no negative zero (the e4m3 cast keeps it)
    return np.ldexp(q, e)


def gptq_factor(gram, rows: int, damp: float = 0.01):
    """float64 [K, K] upper triangular U with H^-1 = U^T U, for H = gram / rows: a channel with H_kk == 0 decoupled (H_kk = 1, its
    row and column zero: it was silent in calibration and keeps its plain rounding), damp * mean(diag H) added to the diagonal"""
    import numpy as np
    if rows <= 0:
        raise ValueError("gptq: the Gram matrix counted no row")
    H = np.array(gram, dtype=np.float64) / float(rows)
    if H.ndim != 2 or H.shape[0] != H.shape[1]:
        raise ValueError("gptq: the Gram matrix must be square")
    d = np.diagonal(H).copy()
    dead = d == 0
    H[dead, :] = 0
    H[:, dead] = 0
    H[dead, dead] = 1.0
    mean = float(d.mean())
    H[np.diag_indices_from(H)] += damp * (mean if mean > 0 else 1.0)
    return np.ascontiguousarray(np.linalg.cholesky(np.linalg.inv(H)).T)


def gptq_apply(w2d: torch.Tensor, U, fmt: str, block: int = 128) -> torch.Tensor:
    """[K, N] -> fp32 [K, N] on the grid of ``fmt`` by GPTQ with the factor of gptq_factor.  k ascending; at every k % 32 == 0 the
    block's exponent is fixed from the current block; err = (w_k - q_k) / U_kk goes into the rows behind, eagerly inside a run of
    ``block`` rows and as one matrix product behind it"""
    import numpy as np
    if fmt not in _MX_FMT:
        raise ValueError(f"gptq: fmt is mxfp4 or mxfp8, not {fmt!r}")
    if block <= 0 or block % MX_BLOCK:
        raise ValueError(f"gptq: block must be a positive multiple of {MX_BLOCK}")
    K, N = w2d.shape
    if U.shape != (K, K):
        raise ValueError(f"gptq: the Gram matrix has {U.shape[0]} channels, the kernel contracts {K}")
    W = w2d.detach().cpu().double().numpy().copy()
    Q = np.empty_like(W)
    e = None
    for i1 in range(0, K, block):
        i2 = min(i1 + block, K)
        W1, U1 = W[i1:i2], U[i1:i2, i1:i2]
        err = np.empty((i2 - i1, N))
        for i in range(i2 - i1):
            k = i1 + i
            if k % MX_BLOCK == 0:
                e = _mx_exponent_np(W[k: min(k + MX_BLOCK, K)], _MX_FMT[fmt][0])
            Q[k] = _mx_round_row_np(W1[i], e, fmt)
            err[i] = (W1[i] - Q[k]) / U1[i, i]
            if i + 1 < i2 - i1:
                W1[i + 1:] -= np.outer(U1[i, i + 1:], err[i])
        if i2 < K:
            W[i2:] -= U[i1:i2, i2:].T @ err
    out = torch.from_numpy(Q.astype(np.float32))
    # the exponent was fixed before the block's rows moved: where a block's largest value has dropped a binade since, the quantiser
    # reads a smaller exponent from the result, and an e4m3 value of mantissa 1.875 then lands on 480 > 448.  Such a block takes the
    # nearest representable values (uncompensated), so that dequantise(quantise(out)) == out always holds
    proj = (mxfp4_round_2d if fmt == "mxfp4" else mxfp8_round_2d)(out)
    return out if torch.equal(proj, out) else proj


def gptq_quantize_2d(w2d: torch.Tensor, gram, rows: int, fmt: str, damp: float = 0.01, block: int = 128) -> torch.Tensor:
    """[K, N] -> fp32 [K, N]: the MXFP4 / MXFP8-representable matrix GPTQ finds for the Gram matrix ``gram`` (float64 [K, K], the sum of
    x x^T over ``rows`` calibration rows).  With a diagonal ``gram`` this is mxfp4_round_2d / mxfp8_round_2d."""
    return gptq_apply(w2d, gptq_factor(gram, rows, damp), fmt, block)


def gptq_quantize_state_dict(cfg: DiaConfig, sd: Dict[str, torch.Tensor], gram_stats, fmt: str, damp: float = 0.01,
                             block: int = 128) -> "OrderedDict[str, torch.Tensor]":
    """As mxfp4_quantize_state_dict / mxfp8_quantize_state_dict with GPTQ in the place of round-to-nearest: every kernel of
    ``mx_names(cfg)`` against the Gram matrix of its input (``gram_stats``: a calib.GramStats covering all of them); the kernels of
    one tap (q/k/v) share one factorisation.  Everything else untouched."""
    gram_stats.check_against(cfg, mx_names(cfg))
    out: "OrderedDict[str, torch.Tensor]" = OrderedDict((k, v.clone()) for k, v in sd.items())
    tap, U = None, None
    for name in sorted(mx_names(cfg), key=gram_stats.tap_of):
        if gram_stats.tap_of(name) != tap:
            tap = gram_stats.tap_of(name)
            U = gptq_factor(gram_stats.dense(name), gram_stats.rows[tap], damp)
        w = sd[name]
        out[name] = gptq_apply(_kernel_2d(name, w.float()), U, fmt, block).reshape(w.shape)
    return out


def calibration_error(gram, delta: torch.Tensor) -> float:
    """tr(delta^T G delta) = ||X delta||_F^2: the squared output error of a kernel changed by ``delta`` [K, N] on the calibration rows"""
    import numpy as np
    d = delta.detach().cpu().double().numpy()
    return float(np.einsum("kn,kn->", d, np.asarray(gram, dtype=np.float64) @ d))


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
