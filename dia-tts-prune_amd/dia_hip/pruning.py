"""Structured pruning of a Dia checkpoint and detection of pruned structure for repacking.

``structured_prune_state_dict`` restates what the reference's ``offline_prune.py`` does in
``--prune-mode structured`` (offline_prune.py:82-156 -> dia/pruning_utils.py:64-151): for every
DenseGeneral kernel, rank the slices along ``dim`` by their L_n norm and zero the
``round(amount * n_slices)`` weakest (``torch.nn.utils.prune.ln_structured`` followed by
``prune.remove``) — the result is a same-shape checkpoint with zero slices and no mask.

``kept_slices`` recovers the structure from the zeros (the checkpoint carries no mask,
pruning_utils.py:145), which is what the loader uses to build physically smaller tensors.
"""

from __future__ import annotations

from collections import OrderedDict
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from .config import DiaConfig
from .weights import param_shapes


def prunable_names(cfg: DiaConfig):
    """DenseGeneral kernels = everything the reference's get_prunable_modules finds in DiaModel
    (pruning_utils.py:13-40): projections, MLP matrices and the logits head; embeddings and RMSNorm
    weights are not DenseGeneral/Linear/Conv1d and stay untouched."""
    return [k for k in param_shapes(cfg) if not (k.endswith("norm.weight") or "embedding" in k)]


def _channel_rms(cfg: DiaConfig, act_stats) -> Dict[str, torch.Tensor]:
    """{name: fp32 [K]} = sqrt(sum_k / rows) of a calib.ActStats, after checking that it covers every prunable kernel of this model
    with the right length (ValueError names the offending tensor)"""
    act_stats.check_against(cfg)
    return {k: torch.from_numpy(act_stats.rms(k)).to(torch.float32) for k in prunable_names(cfg)}


def _scaled_kernel(name: str, w: torch.Tensor, rms: torch.Tensor) -> torch.Tensor:
    """W[k, n] * rms[k] on the _kernel_2d view, in the kernel's own shape: the Wanda score is its absolute value"""
    w2 = _kernel_2d(name, w)
    return (w2 * rms.to(w2.device)[:, None]).reshape(w.shape)


def structured_prune_state_dict(cfg: DiaConfig, sd: Dict[str, torch.Tensor], amount: float, dim: int = 0,
                                n: int = 2, act_stats=None) -> Tuple["OrderedDict[str, torch.Tensor]", Dict[str, np.ndarray]]:
    """Returns (pruned state_dict, {name: kept slice indices along `dim`}).
    act_stats (calib.ActStats): slices are ranked by the L_n norm of the kernel scaled by its input channels' RMS
    (W[k, n] * sqrt(sum_k / rows) on the _kernel_2d view) instead of the kernel's own."""
    if not (0.0 < amount < 1.0):
        raise ValueError("--prune-amount must be between 0.0 and 1.0 (exclusive).")   # offline_prune.py:58-60
    rms = _channel_rms(cfg, act_stats) if act_stats is not None else None
    out: "OrderedDict[str, torch.Tensor]" = OrderedDict((k, v.clone()) for k, v in sd.items())
    kept: Dict[str, np.ndarray] = {}
    for name in prunable_names(cfg):
        w = out[name].float()
        if dim >= w.dim():                      # pruning_utils.py:84-87: module skipped
            continue
        size = w.shape[dim]
        n_prune = int(round(amount * size))
        n_keep = size - n_prune
        other = [a for a in range(w.dim()) if a != dim]
        norm = torch.norm(w if rms is None else _scaled_kernel(name, w, rms[name]), p=n, dim=other)
        keep_idx = torch.topk(norm, k=n_keep, largest=True).indices
        mask = torch.zeros(size, dtype=torch.bool, device=w.device)
        mask[keep_idx] = True
        shape = [1] * w.dim()
        shape[dim] = size
        out[name] = (w * mask.view(shape)).to(sd[name].dtype)
        kept[name] = torch.nonzero(mask).flatten().cpu().numpy().astype(np.int32)
    return out, kept


def unstructured_prune_state_dict(cfg: DiaConfig, sd: Dict[str, torch.Tensor], amount: float, act_stats=None) -> "OrderedDict[str, torch.Tensor]":
    """``offline_prune.py --prune-mode unstructured`` (offline_prune.py:101-103 -> pruning_utils.py:42-62):
    GLOBAL L1 magnitude pruning over all DenseGeneral kernels — the ``round(amount * N)`` entries of smallest
    absolute value across the concatenation of every prunable kernel (``prune.global_unstructured`` with
    ``L1Unstructured``: top-k of -|w| over the flattened concatenation, in module order) are zeroed.  The result
    has no exploitable structure: it loads as dense tensors whose zeros stream like any other value.
    act_stats (calib.ActStats): Wanda's comparison group instead of the global one — PER OUTPUT COLUMN of every kernel's _kernel_2d
    view the ``round(amount * K)`` entries of lowest score |W[k, n]| * sqrt(sum_k / rows) are zeroed, ties going to the lower k."""
    if not (0.0 < amount < 1.0):
        raise ValueError("--prune-amount must be between 0.0 and 1.0 (exclusive).")   # offline_prune.py:58-60
    if act_stats is not None:
        rms = _channel_rms(cfg, act_stats)
        res: "OrderedDict[str, torch.Tensor]" = OrderedDict((k, v.clone()) for k, v in sd.items())
        for name in prunable_names(cfg):
            w = sd[name]
            w2 = _kernel_2d(name, w.float())
            n_prune = int(round(amount * w2.shape[0]))
            if n_prune == 0:
                continue
            score = w2.abs() * rms[name].to(w2.device)[:, None]
            order = torch.sort(score, dim=0, descending=False, stable=True).indices     # among equals the lower k comes first: it goes
            mask = torch.ones_like(w2, dtype=torch.bool)
            mask.scatter_(0, order[:n_prune], False)
            res[name] = (w2 * mask).reshape(w.shape).to(w.dtype)
        return res
    names = prunable_names(cfg)
    flat = torch.cat([sd[k].detach().float().reshape(-1) for k in names])
    n_prune = int(round(amount * flat.numel()))
    out: "OrderedDict[str, torch.Tensor]" = OrderedDict((k, v.clone()) for k, v in sd.items())
    if n_prune == 0:
        return out
    idx = torch.topk(flat.abs(), k=n_prune, largest=False).indices
    mask = torch.ones_like(flat, dtype=torch.bool)
    mask[idx] = False
    off = 0
    for k in names:
        n = sd[k].numel()
        out[k] = (sd[k].float() * mask[off: off + n].reshape(sd[k].shape)).to(sd[k].dtype)
        off += n
    return out


def _kernel_2d(name: str, w: torch.Tensor) -> torch.Tensor:
    """a DenseGeneral kernel as [K, N] with K the contraction axis, as DeviceWeights flattens it: o_proj [heads, hd, D] and
    wo [F, D] keep their leading axes as K, every other kernel ([D, heads, hd], wi_fused [D, 2, F], logits [D, C, V]) its first"""
    if name.endswith("o_proj.weight"):
        return w.reshape(-1, w.shape[-1])
    return w.reshape(w.shape[0], -1)


def _prune_2of4_2d(w2d: torch.Tensor, rms: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[K, N] -> same shape: in every group of 4 consecutive K rows of each column the 2 largest |w| stay, the others become 0
    (ties: the lower K index stays).  A trailing partial group (K % 4 != 0) is treated as zero-padded.
    rms [K]: the 2 largest |w[k, n]| * rms[k] stay instead (same groups, same tie rule)."""
    K, N = w2d.shape
    Kp = (K + 3) // 4 * 4
    wp = torch.zeros(Kp, N, dtype=w2d.dtype, device=w2d.device)
    wp[:K] = w2d
    g = wp.reshape(Kp // 4, 4, N)
    score = g.abs()
    if rms is not None:
        rp = torch.zeros(Kp, dtype=w2d.dtype, device=w2d.device)
        rp[:K] = rms.to(device=w2d.device, dtype=w2d.dtype)
        score = score * rp.reshape(Kp // 4, 4, 1)
    # stable descending sort of the score keeps the lower index first among equals
    order = torch.sort(score, dim=1, descending=True, stable=True).indices
    mask = torch.zeros_like(g, dtype=torch.bool)
    mask.scatter_(1, order[:, :2], True)
    return (g * mask).reshape(Kp, N)[:K]


def semi_structured_prune_state_dict(cfg: DiaConfig, sd: Dict[str, torch.Tensor], act_stats=None) -> "OrderedDict[str, torch.Tensor]":
    """2:4 semi-structured pruning (``offline_prune.py --prune-mode 2:4``): every kernel of ``prunable_names(cfg)``, flattened
    to [K, N] (``_kernel_2d``), keeps the 2 largest |w| of every group of 4 consecutive K rows of each column; ties keep the
    lower K index.  Half of every kernel becomes zero, in the pattern the sparse MFMA of gfx950 consumes
    (layout.tile_weight_24).  Idempotent; embeddings and norms are untouched.
    act_stats (calib.ActStats): the rank of an entry is |W[k, n]| * sqrt(sum_k / rows), Wanda's score, instead of |W[k, n]|."""
    rms = _channel_rms(cfg, act_stats) if act_stats is not None else None
    out: "OrderedDict[str, torch.Tensor]" = OrderedDict((k, v.clone()) for k, v in sd.items())
    for name in prunable_names(cfg):
        w = sd[name]
        out[name] = _prune_2of4_2d(_kernel_2d(name, w.float()), None if rms is None else rms[name]).reshape(w.shape).to(w.dtype)
    return out


def is_2of4(w2d: torch.Tensor) -> bool:
    """True when every group of 4 consecutive rows (K) of every column of [K, N] holds at most 2 non-zeros
    (a trailing partial group counts as zero-padded)"""
    K, N = w2d.shape
    Kp = (K + 3) // 4 * 4
    nz = torch.zeros(Kp, N, dtype=torch.int32, device=w2d.device)
    nz[:K] = (w2d != 0).to(torch.int32)
    return bool((nz.reshape(Kp // 4, 4, N).sum(dim=1) <= 2).all().item())


def kept_slices(w: torch.Tensor, dim: int = 0) -> np.ndarray:
    """Indices along `dim` whose slice is not identically zero."""
    moved = w.movedim(dim, 0).reshape(w.shape[dim], -1)
    return torch.nonzero((moved != 0).any(dim=1)).flatten().cpu().numpy().astype(np.int32)


def sparsity(cfg: DiaConfig, sd: Dict[str, torch.Tensor]) -> float:
    """Global zero fraction over the prunable kernels (pruning_utils.py:153-179)."""
    tot = zero = 0
    for k in prunable_names(cfg):
        tot += sd[k].numel()
        zero += int((sd[k] == 0).sum().item())
    return zero / max(tot, 1)
