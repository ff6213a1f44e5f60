"""Host side of activation statistics (DESIGN.md "Activation statistics"): per prunable kernel the sum of squares of every input
channel over the rows a calibration run counted, and the row count — what Wanda (Sun et al. 2023) needs beside the weights:
it ranks an entry by ``|W[k, n]| * ||x_k||_2``.

The device accumulates one float64 vector per tap (csrc/calib.hip, ``dia_act_stats``): seven kinds of tap in the decode step
(``dia_engine_set_calib``), six per encoder layer and one in front of the cross-K/V projection (``DecodeSession._encode``).
One tap serves every kernel that contracts with its rows (q/k/v; both halves of wi_fused; the cross k/v of all decoder layers):
the same vector is stored under each name.  ``ActStats`` itself is NumPy only.
"""

from __future__ import annotations

from typing import Dict, List, Sequence

import numpy as np

from .config import DiaConfig
from .weights import param_shapes

DEC_TAPS = ("qkv", "o", "cq", "co", "wi", "wo")       # the taps of a decoder layer, in the order of engine.DEC_MATS (enum dia_step_mat)
ENC_TAPS = ("qkv", "o", "wi", "wo")                   # the taps of an encoder layer, in launch order


def prunable_names(cfg: DiaConfig) -> List[str]:
    """as pruning.prunable_names (kept here too: this module does not import torch)"""
    return [k for k in param_shapes(cfg) if not (k.endswith("norm.weight") or "embedding" in k)]


def contraction_size(name: str, shape: Sequence[int]) -> int:
    """K of pruning._kernel_2d: o_proj [heads, hd, D] and wo [F, D] contract their leading axes, every other kernel its first"""
    if name.endswith("o_proj.weight"):
        return int(np.prod(shape[:-1]))
    return int(shape[0])


def _layer_tap_names(prefix: str, attn: str, tap: str) -> List[str]:
    if tap == "qkv":
        return [f"{prefix}self_attention.{p}_proj.weight" for p in "qkv"]
    return {"o": [prefix + "self_attention.o_proj.weight"], "cq": [prefix + "cross_attention.q_proj.weight"],
            "co": [prefix + "cross_attention.o_proj.weight"], "wi": [prefix + "mlp.wi_fused.weight"],
            "wo": [prefix + "mlp.wo.weight"]}[tap]


def decoder_tap_names(cfg: DiaConfig) -> List[List[str]]:
    """the kernels behind every tap of a calibrating step, in the engine's tap order: 6 * layer + DEC_TAPS index, the logits head last"""
    out = [_layer_tap_names(f"decoder.layers.{l}.", "self", t) for l in range(cfg.model.decoder.n_layer) for t in DEC_TAPS]
    return out + [["decoder.logits_dense.weight"]]


def encoder_tap_names(cfg: DiaConfig) -> List[List[str]]:
    """the kernels behind every tap of the encoder pass: 4 * layer + ENC_TAPS index, then the cross-K/V tap (the k and v projections of
    every decoder layer read the encoder output)"""
    out = [_layer_tap_names(f"encoder.layers.{l}.", "self", t) for l in range(cfg.model.encoder.n_layer) for t in ENC_TAPS]
    ckv = [f"decoder.layers.{l}.cross_attention.{p}_proj.weight" for l in range(cfg.model.decoder.n_layer) for p in "kv"]
    return out + [ckv]


def _shape_fields(cfg: DiaConfig) -> Dict[str, int]:
    m, e, d = cfg.model, cfg.model.encoder, cfg.model.decoder
    return dict(enc_n_layer=e.n_layer, enc_n_embd=e.n_embd, enc_n_hidden=e.n_hidden, enc_n_head=e.n_head, enc_head_dim=e.head_dim,
                dec_n_layer=d.n_layer, dec_n_embd=d.n_embd, dec_n_hidden=d.n_hidden, dec_gqa_query_heads=d.gqa_query_heads,
                dec_kv_heads=d.kv_heads, dec_gqa_head_dim=d.gqa_head_dim, dec_cross_query_heads=d.cross_query_heads,
                dec_cross_head_dim=d.cross_head_dim, channels=cfg.data.channels, tgt_vocab_size=m.tgt_vocab_size)


class ActStats:
    """``sums[name]``: float64 [K], the sum over counted rows of the squared input of channel k of kernel ``name`` (K the contraction
    axis of ``pruning._kernel_2d``); ``rows[name]``: how many rows that is.  ``shape_fields`` names the model the numbers belong to."""

    def __init__(self, sums: Dict[str, np.ndarray], rows: Dict[str, int], shape_fields: Dict[str, int]):
        if set(sums) != set(rows):
            raise ValueError("ActStats: sums and rows must hold the same names")
        self.sums = {k: np.ascontiguousarray(v, dtype=np.float64).reshape(-1) for k, v in sums.items()}
        self.rows = {k: int(v) for k, v in rows.items()}
        self.shape_fields = {k: int(v) for k, v in shape_fields.items()}

    @classmethod
    def zeros(cls, cfg: DiaConfig) -> "ActStats":
        shp = param_shapes(cfg)
        names = prunable_names(cfg)
        return cls({k: np.zeros(contraction_size(k, shp[k])) for k in names}, {k: 0 for k in names}, _shape_fields(cfg))

    @classmethod
    def ones(cls, cfg: DiaConfig) -> "ActStats":
        """every channel at RMS 1: pruning with it ranks by |w| alone"""
        s = cls.zeros(cfg)
        for k in s.sums:
            s.sums[k][:] = 1.0
            s.rows[k] = 1
        return s

    def names(self) -> List[str]:
        return list(self.sums)

    def rms(self, name: str) -> np.ndarray:
        """float64 [K]: sqrt(sum / rows), the channel's root mean square over the counted rows"""
        if self.rows[name] <= 0:
            raise ValueError(f"ActStats.rms({name}): no row was counted")
        return np.sqrt(self.sums[name] / float(self.rows[name]))

    def merge(self, other: "ActStats") -> "ActStats":
        """adds the other run's sums and counts into this one (same model, same names); returns self"""
        if other.shape_fields != self.shape_fields:
            raise ValueError("ActStats.merge: the statistics belong to models of different shapes")
        for k in self.sums:
            if k not in other.sums or other.sums[k].shape != self.sums[k].shape:
                raise ValueError(f"ActStats.merge: {k} is missing from the other statistics or has another length")
        for k in self.sums:
            self.sums[k] = self.sums[k] + other.sums[k]
            self.rows[k] += other.rows[k]
        return self

    def check_against(self, cfg: DiaConfig) -> None:
        """ValueError naming the first tensor of ``prunable_names(cfg)`` these statistics do not cover with the right length"""
        shp = param_shapes(cfg)
        for k in prunable_names(cfg):
            if k not in self.sums:
                raise ValueError(f"activation statistics hold nothing for {k}")
            K = contraction_size(k, shp[k])
            if self.sums[k].shape[0] != K:
                raise ValueError(f"activation statistics of {k} have {self.sums[k].shape[0]} channels, the kernel contracts {K}")
            if self.rows[k] <= 0:
                raise ValueError(f"activation statistics of {k} counted no row")
        extra = sorted(set(self.sums) - set(prunable_names(cfg)))
        if extra:
            raise ValueError(f"activation statistics name {extra[0]}, which this checkpoint does not have")

    def save(self, path: str) -> None:
        """one .npz: ``sum/<name>`` float64 arrays, ``rows/<name>`` int64 scalars, ``shape/<field>`` int64 scalars — arrays only, loaded
        with allow_pickle=False"""
        arrs = {}
        for k, v in self.sums.items():
            arrs["sum/" + k] = v
            arrs["rows/" + k] = np.int64(self.rows[k])
        for k, v in self.shape_fields.items():
            arrs["shape/" + k] = np.int64(v)
        with open(path, "wb") as f:
            np.savez(f, **arrs)

    @classmethod
    def load(cls, path: str) -> "ActStats":
        with np.load(path, allow_pickle=False) as z:
            sums = {k[4:]: z[k] for k in z.files if k.startswith("sum/")}
            rows = {k[5:]: int(z[k]) for k in z.files if k.startswith("rows/")}
            shape = {k[6:]: int(z[k]) for k in z.files if k.startswith("shape/")}
        return cls(sums, rows, shape)
