"""LoRA adapters, two ways.

Offline merge (``merge_lora_state_dict``): adapters are folded into the dense kernels before tiling, so the
decode path streams exactly the same bytes as without adapters — one voice per process.

Unmerged, per request (``AdapterBank``; DESIGN.md "Per-request adapters"): the q/k/v projections' adapters of several voices stay
resident beside ONE base model as fp32 ``A`` / ``B`` matrices, and every slot of a decode session picks its own (csrc/lora.hip).

The reference attaches adapters at run time through PEFT (cli.py:166-174, model.py:598-625), which is not
installed here and which, as far as its Linear-only LoRA layers go, cannot wrap this model's DenseGeneral
modules at all — parity for this file is therefore UNPINNED; it follows PEFT's published LoRA arithmetic
for a Linear layer: ``W[out, in] += (lora_alpha / r) * B[out, r] @ A[r, in]``.  A DenseGeneral kernel is
stored ``[in..., out...]`` (layers.py:47-51), i.e. the transpose of that W once both sides are flattened.

Adapter directory layout (PEFT's): ``adapter_config.json`` with ``r``, ``lora_alpha`` (+ optional
``rank_pattern`` / ``alpha_pattern``, ``fan_in_fan_out``) and ``adapter_model.safetensors`` or
``adapter_model.bin`` with keys ``<prefix>.<module path>.lora_A.weight`` / ``.lora_B.weight`` (an optional
adapter name segment such as ``.default`` is accepted).
"""

from __future__ import annotations

import json
import os
import re
from typing import Dict, Iterator, List, Optional, Tuple, Union

import torch

_KEY = re.compile(r"^(?:base_model\.model\.)?(?P<mod>.+?)\.lora_(?P<ab>[AB])(?:\.[^.]+)?\.weight$")


def load_adapter(adapter_dir: str):
    cfg_path = os.path.join(adapter_dir, "adapter_config.json")
    if not os.path.isfile(cfg_path):
        raise FileNotFoundError(f"adapter_config.json not found in {adapter_dir}")
    with open(cfg_path) as f:
        acfg = json.load(f)
    st = os.path.join(adapter_dir, "adapter_model.safetensors")
    bn = os.path.join(adapter_dir, "adapter_model.bin")
    if os.path.isfile(st):
        from safetensors.torch import load_file
        tensors = load_file(st)
    elif os.path.isfile(bn):
        tensors = torch.load(bn, map_location="cpu", weights_only=True)
    else:
        raise FileNotFoundError(f"adapter_model.safetensors / adapter_model.bin not found in {adapter_dir}")
    return acfg, tensors


def iter_adapter_modules(acfg: dict, tensors: Dict[str, torch.Tensor], adapter_dir: str) -> Iterator[Tuple[str, torch.Tensor, torch.Tensor, float, int]]:
    """The adapter's modules as (module path, lora_A [r, in], lora_B [out, r], alpha, rank stated by adapter_config) — key
    pattern, ``.default`` name segment, ``rank_pattern`` / ``alpha_pattern``: the one parser of merge_lora_state_dict and
    AdapterBank.  A module with only one of the two matrices raises when it is reached."""
    r_default, alpha_default = int(acfg.get("r", 8)), float(acfg.get("lora_alpha", 8))
    rank_pat, alpha_pat = acfg.get("rank_pattern") or {}, acfg.get("alpha_pattern") or {}
    pairs: Dict[str, Dict[str, torch.Tensor]] = {}
    for k, v in tensors.items():
        m = _KEY.match(k)
        if not m:
            continue
        pairs.setdefault(m.group("mod"), {})[m.group("ab")] = v
    if not pairs:
        raise RuntimeError(f"no lora_A / lora_B tensors found in {adapter_dir}")
    for mod, ab in pairs.items():
        if "A" not in ab or "B" not in ab:
            raise RuntimeError(f"adapter for {mod} lacks lora_{'B' if 'A' in ab else 'A'}")
        leaf = mod.rsplit(".", 1)[-1]
        alpha = float(next((v for p, v in alpha_pat.items() if mod.endswith(p) or leaf == p), alpha_default))
        r_cfg = int(next((v for p, v in rank_pat.items() if mod.endswith(p) or leaf == p), r_default))
        yield mod, ab["A"].float(), ab["B"].float(), alpha, r_cfg


def merge_lora_state_dict(sd: Dict[str, torch.Tensor], adapter_dir: str) -> Dict[str, torch.Tensor]:
    """Returns a new state dict with every adapted kernel replaced by ``kernel + scale * (B @ A)^T`` (fp32
    arithmetic, original dtype and shape kept).  Unknown modules raise: a silently ignored adapter would
    look like a working one."""
    acfg, tensors = load_adapter(adapter_dir)
    out = dict(sd)
    for mod, A, B, alpha, r_cfg in iter_adapter_modules(acfg, tensors, adapter_dir):      # A [r, in], B [out, r]
        name = mod + ".weight"
        if name not in sd:
            raise RuntimeError(f"adapter targets {mod}, which is not a module of this model")
        r = A.shape[0]
        if r_cfg != r:
            raise RuntimeError(f"{mod}: adapter rank {r} does not match adapter_config ({r_cfg})")
        w = sd[name]
        delta = (B @ A) * (alpha / r)                                # [out, in]
        if acfg.get("fan_in_fan_out"):
            delta = delta.t()
        n_in, n_out = A.shape[1], B.shape[0]
        if n_in * n_out != w.numel():           # kernel is [in..., out...] (layers.py:47-51): both sides flatten
            raise RuntimeError(f"{mod}: adapter shapes A{tuple(A.shape)} B{tuple(B.shape)} do not fit kernel {tuple(w.shape)}")
        flat = w.float().reshape(n_in, n_out)
        out[name] = (flat + delta.t()).reshape(w.shape).to(w.dtype)
    return out


# ------------------------------------------------------------------------------------------------ unmerged, per request
MAX_RANK = 64                                              # DIA_LORA_MAX_RANK
_SITE = re.compile(r"^(?P<side>encoder|decoder)\.layers\.(?P<l>\d+)\.(?P<att>self_attention|cross_attention)\.(?P<p>[qkv])_proj$")


class AdapterBank:
    """Several LoRA adapters resident beside one base model, for sessions whose requests pick one each.

    ``add(name, adapter_dir)`` parses a PEFT adapter directory (the parser of merge_lora_state_dict) into host tables;
    ``upload()`` — called by the first session that takes the bank, after which the bank is fixed — moves them to the device as
    ONE fp32 arena plus, per module, the tables the kernels index by adapter: pointers to ``A`` [r, in] and ``B`` flattened like
    a DenseGeneral kernel ([in = r, out...]), rank, scale = alpha / r.  A module an adapter does not touch has rank 0 there.

    A module is (block, layer, proj): block "enc" (encoder self-attention), "self" / "cross" (decoder), proj "q" / "k" / "v".
    Only those can be corrected behind their GEMM; an adapter on o_proj, wi_fused, wo, logits_dense or an embedding is refused
    here — merge it at load (``adapter_path=``), which takes every module."""

    def __init__(self, cfg, device: Union[str, torch.device] = "cpu"):
        from .weights import param_shapes
        self.cfg, self.device = cfg, torch.device(device)
        self._shapes = param_shapes(cfg)
        self.names: List[str] = []
        self.host: List[Dict[Tuple[str, int, str], dict]] = []      # per adapter: module -> dict(A [r, in], B [r, out], rank, scale)
        self.frozen = False
        self.arena: Optional[torch.Tensor] = None
        e, d = cfg.model.encoder, cfg.model.decoder
        self.modules: List[Tuple[str, int, str]] = ([("enc", l, p) for l in range(e.n_layer) for p in "qkv"] +
                                                    [("self", l, p) for l in range(d.n_layer) for p in "qkv"] +
                                                    [("cross", l, p) for l in range(d.n_layer) for p in "qkv"])
        self._mod_index = {m: i for i, m in enumerate(self.modules)}

    def __len__(self) -> int:
        return len(self.names)

    def module_of(self, path: str) -> Tuple[str, int, str]:
        """PEFT module path -> (block, layer, proj); raises for what the bank cannot serve and for what the model does not have"""
        m = _SITE.match(path)
        if m and path + ".weight" in self._shapes:
            block = "enc" if m.group("side") == "encoder" else ("self" if m.group("att") == "self_attention" else "cross")
            if not (block == "enc" and m.group("att") != "self_attention"):
                return block, int(m.group("l")), m.group("p")
        if path + ".weight" in self._shapes:
            raise RuntimeError(f"adapter targets {path}: only q_proj / k_proj / v_proj can stay unmerged (the GEMMs of o_proj, wi_fused, "
                               f"wo, logits_dense and the embeddings fuse what follows them); merge this adapter at load with adapter_path=")
        raise RuntimeError(f"adapter targets {path}, which is not a module of this model")

    def shape_of(self, mod: Tuple[str, int, str]) -> Tuple[int, int]:
        """(fan-in, fan-out) of a module's DenseGeneral kernel"""
        e, d = self.cfg.model.encoder, self.cfg.model.decoder
        block, _, p = mod
        if block == "enc":
            return e.n_embd, e.n_head * e.head_dim
        if block == "self":
            return d.n_embd, (d.gqa_query_heads if p == "q" else d.kv_heads) * d.gqa_head_dim
        return (d.n_embd if p == "q" else e.n_embd), d.cross_query_heads * d.cross_head_dim

    def add(self, name: str, adapter_dir: str) -> int:
        """Parse one adapter into the bank; returns its index (what Request.adapter / adapter_ids may also name it by)."""
        if self.frozen:
            raise RuntimeError("the adapter bank is fixed once a session has been opened with it: load every adapter first")
        if name in self.names:
            raise ValueError(f"adapter name {name!r} is already in the bank")
        acfg, tensors = load_adapter(adapter_dir)
        fifo = bool(acfg.get("fan_in_fan_out"))
        mods: Dict[Tuple[str, int, str], dict] = {}
        for path, A, B, alpha, r_cfg in iter_adapter_modules(acfg, tensors, adapter_dir):
            mod = self.module_of(path)
            r = A.shape[0]
            if r_cfg != r:
                raise RuntimeError(f"{path}: adapter rank {r} does not match adapter_config ({r_cfg})")
            if not 1 <= r <= MAX_RANK:
                raise RuntimeError(f"{path}: rank {r} is outside 1..{MAX_RANK} (the unmerged path's bound; merge it at load with adapter_path=)")
            n_in, n_out = self.shape_of(mod)
            if B.shape[1] != r or A.shape[1] * B.shape[0] != n_in * n_out:
                raise RuntimeError(f"{path}: adapter shapes A{tuple(A.shape)} B{tuple(B.shape)} do not fit kernel {tuple(self._shapes[path + '.weight'])}")
            # merge_lora_state_dict adds (scale * B @ A)^T to the kernel flattened [in, out]; with fan_in_fan_out it adds scale * B @ A
            # itself, i.e. the two matrices change roles (and the kernel must be square)
            down, up = (B.t(), A) if fifo else (A, B.t())               # [r, in], [r, out]
            if tuple(down.shape) != (r, n_in) or tuple(up.shape) != (r, n_out):
                raise RuntimeError(f"{path}: adapter shapes A{tuple(A.shape)} B{tuple(B.shape)} do not fit kernel {tuple(self._shapes[path + '.weight'])}")
            mods[mod] = dict(A=down.contiguous(), B=up.contiguous(), rank=r, scale=alpha / r)
        self.names.append(name)
        self.host.append(mods)
        return len(self.names) - 1

    def index_of(self, adapter: Union[None, str, int]) -> int:
        """name or index -> index; None -> -1 (the base model)"""
        if adapter is None:
            return -1
        if isinstance(adapter, str):
            if adapter not in self.names:
                raise ValueError(f"unknown adapter {adapter!r}; the bank holds {self.names}")
            return self.names.index(adapter)
        i = int(adapter)
        if not -1 <= i < len(self.names):
            raise ValueError(f"adapter index {i} outside the bank's {len(self.names)} adapters")
        return i

    def max_rank(self, mod: Tuple[str, int, str]) -> int:
        return max([h[mod]["rank"] for h in self.host if mod in h] + [0])

    def freeze(self):
        """Called by a session that takes the bank: uploads on first use, and add() raises from now on."""
        if not self.names:
            raise RuntimeError("the adapter bank is empty")
        self.frozen = True
        if self.arena is None:
            self.upload()

    def upload(self):
        """host tables -> one fp32 arena (16-byte aligned runs) + [module][adapter] pointer / rank / scale tables on the device"""
        n_ad, n_mod = len(self.names), len(self.modules)
        offs, tot = {}, 0
        for a, mods in enumerate(self.host):
            for mod, h in mods.items():
                for k in ("A", "B"):
                    offs[(a, mod, k)] = tot
                    tot += (h[k].numel() + 3) // 4 * 4
        flat = torch.zeros(max(tot, 4), dtype=torch.float32)
        for (a, mod, k), o in offs.items():
            t = self.host[a][mod][k]
            flat[o: o + t.numel()] = t.reshape(-1)
        self.arena = flat.to(self.device)
        base = self.arena.data_ptr()
        pa, pb = torch.zeros(n_mod, n_ad, dtype=torch.int64), torch.zeros(n_mod, n_ad, dtype=torch.int64)
        rk, sc = torch.zeros(n_mod, n_ad, dtype=torch.int32), torch.zeros(n_mod, n_ad, dtype=torch.float32)
        for a, mods in enumerate(self.host):
            for mod, h in mods.items():
                i = self._mod_index[mod]
                pa[i, a], pb[i, a] = base + 4 * offs[(a, mod, "A")], base + 4 * offs[(a, mod, "B")]
                rk[i, a], sc[i, a] = h["rank"], h["scale"]
        self.ptr_a, self.ptr_b, self.rank, self.scale = (t.to(self.device) for t in (pa, pb, rk, sc))

    def seg(self, mod: Tuple[str, int, str], col_off: int):
        """binding.LoraSeg of one module at output column `col_off` (n_cols 0 when no adapter of the bank touches it)"""
        from . import binding as hb
        s = hb.LoraSeg()
        mr = self.max_rank(mod)
        if mr == 0:
            return s
        i, n_ad = self._mod_index[mod], len(self.names)
        s.col_off, s.n_cols, s.max_rank = int(col_off), self.shape_of(mod)[1], mr
        s.A, s.B = self.ptr_a.data_ptr() + 8 * i * n_ad, self.ptr_b.data_ptr() + 8 * i * n_ad
        s.rank, s.scale = self.rank.data_ptr() + 4 * i * n_ad, self.scale.data_ptr() + 4 * i * n_ad
        return s
