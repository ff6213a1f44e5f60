"""Host side of activation statistics (DESIGN.md "Activation statistics"): per prunable kernel the sum of squares of every input
channel over the rows a calibration run counted, and the row count — what Wanda (Sun et al. 2023) needs beside the weights:
it ranks an entry by ``|W[k, n]| * ||x_k||_2``.

The device accumulates one float64 vector per tap (csrc/calib.hip, ``dia_act_stats``): seven kinds of tap in the decode step
(``dia_engine_set_calib``), six per encoder layer and one in front of the cross-K/V projection (``DecodeSession._encode``).
One tap serves every kernel that contracts with its rows (q/k/v; both halves of wi_fused; the cross k/v of all decoder layers):
the same vector is stored under each name.  ``ActStats`` itself is NumPy only.

``GramStats`` (DESIGN.md "Gram matrices and GPTQ") holds what GPTQ needs instead: per tap of the decode step the full Gram matrix
of the input rows, as the device packs it (csrc/gram.hip, ``dia_act_gram``), stored once per tap however many kernels it serves.
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


# ---------------------------------------------------------------------------------------------------------------------------
# Gram matrices (DESIGN.md "Gram matrices and GPTQ").  The packed layout of dia_act_gram: the lower triangle of 32 x 32 tiles, tile
# (ti, tj), tj <= ti, at index ti (ti + 1) / 2 + tj, each tile row-major; diagonal tiles whole.
GRAM_TILE = 32


def gram_tiles(K: int) -> int:
    """tiles of the packed Gram matrix of K channels (K a multiple of 32)"""
    if K <= 0 or K % GRAM_TILE:
        raise ValueError(f"a packed Gram matrix has a multiple of {GRAM_TILE} channels, not {K}")
    T = K // GRAM_TILE
    return T * (T + 1) // 2


def gram_channels(tiles: int) -> int:
    """inverse of gram_tiles"""
    T = int((np.sqrt(8.0 * tiles + 1.0) - 1.0) / 2.0 + 0.5)
    if T * (T + 1) // 2 != tiles or T <= 0:
        raise ValueError(f"{tiles} tiles are no packed lower triangle")
    return T * GRAM_TILE


def pack_gram(dense: np.ndarray) -> np.ndarray:
    """symmetric [K, K] -> float64 [T (T + 1) / 2, 32, 32] (the lower triangle of tiles; the upper one is not looked at)"""
    dense = np.asarray(dense, dtype=np.float64)
    K = dense.shape[0]
    if dense.shape != (K, K):
        raise ValueError("pack_gram takes a square matrix")
    out = np.empty((gram_tiles(K), GRAM_TILE, GRAM_TILE), dtype=np.float64)
    T = K // GRAM_TILE
    blocks = dense.reshape(T, GRAM_TILE, T, GRAM_TILE).transpose(0, 2, 1, 3)
    for ti in range(T):
        out[ti * (ti + 1) // 2: ti * (ti + 1) // 2 + ti + 1] = blocks[ti, : ti + 1]
    return out


def unpack_gram(packed: np.ndarray) -> np.ndarray:
    """float64 [T (T + 1) / 2, 32, 32] -> symmetric [K, K]: the strict upper triangle of tiles mirrors the lower one"""
    packed = np.asarray(packed, dtype=np.float64).reshape(-1, GRAM_TILE, GRAM_TILE)
    K = gram_channels(packed.shape[0])
    T = K // GRAM_TILE
    blocks = np.empty((T, T, GRAM_TILE, GRAM_TILE), dtype=np.float64)
    for ti in range(T):
        row = packed[ti * (ti + 1) // 2: ti * (ti + 1) // 2 + ti + 1]
        blocks[ti, : ti + 1] = row
        blocks[:ti, ti] = row[:ti].transpose(0, 2, 1)
    return np.ascontiguousarray(blocks.transpose(0, 2, 1, 3).reshape(K, K))


def gram_diagonal(packed: np.ndarray) -> np.ndarray:
    """float64 [K]: the diagonal of a packed Gram matrix, without unpacking it"""
    packed = np.asarray(packed, dtype=np.float64).reshape(-1, GRAM_TILE, GRAM_TILE)
    T = gram_channels(packed.shape[0]) // GRAM_TILE
    return np.concatenate([np.diagonal(packed[ti * (ti + 1) // 2 + ti]) for ti in range(T)])


def gram_tap_keys(cfg: DiaConfig) -> List[str]:
    """one key per tap of the decode step, in the engine's tap order (index 6 * layer + DEC_TAPS index, the logits head last)"""
    return [f"decoder.layers.{l}.{t}" for l in range(cfg.model.decoder.n_layer) for t in DEC_TAPS] + ["decoder.logits_dense"]


def gram_layer_taps(cfg: DiaConfig, layers=None) -> List[int]:
    """tap indices of the selected layers: None = every decoder layer and the logits head; else layer indices (or a (first, end)
    range as a tuple), where index n_layer stands for the logits head"""
    n = cfg.model.decoder.n_layer
    if layers is None:
        sel = list(range(n + 1))
    elif isinstance(layers, tuple) and len(layers) == 2:
        sel = list(range(int(layers[0]), int(layers[1])))
    else:
        sel = sorted({int(l) for l in layers})
    if not sel or sel[0] < 0 or sel[-1] > n:
        raise ValueError(f"gram_layers selects {sel or 'nothing'}: layers are 0 .. {n - 1}, {n} is the logits head")
    return [6 * l + m for l in sel if l < n for m in range(6)] + ([6 * n] if n in sel else [])


class GramStats:
    """Per tap of the decode step (``gram_tap_keys``): ``packed[tap]`` float64 [T (T + 1) / 2, 32, 32], the Gram matrix of the tap's
    input rows in the layout of dia_act_gram; ``rows[tap]``, how many rows it sums; ``kernels[tap]``, the names of the kernels that
    contract with those rows (q/k/v share one array, both halves of wi_fused share one).  Only the kernels of ``quant.mx_names`` are
    covered: the encoder and the cross-K/V projections are not MX-streamed.  A tap may be absent (``gram_layers``)."""

    def __init__(self, packed: Dict[str, np.ndarray], rows: Dict[str, int], kernels: Dict[str, Sequence[str]], shape_fields: Dict[str, int]):
        if set(packed) != set(rows) or set(packed) != set(kernels):
            raise ValueError("GramStats: packed, rows and kernels must hold the same taps")
        self.packed = {k: np.ascontiguousarray(v, dtype=np.float64).reshape(-1, GRAM_TILE, GRAM_TILE) for k, v in packed.items()}
        for k, v in self.packed.items():
            gram_channels(v.shape[0])
        self.rows = {k: int(v) for k, v in rows.items()}
        self.kernels = {k: [str(n) for n in v] for k, v in kernels.items()}
        self.shape_fields = {k: int(v) for k, v in shape_fields.items()}

    @classmethod
    def zeros(cls, cfg: DiaConfig, layers=None) -> "GramStats":
        shp = param_shapes(cfg)
        keys, names = gram_tap_keys(cfg), decoder_tap_names(cfg)
        sel = gram_layer_taps(cfg, layers)
        packed = {keys[i]: np.zeros((gram_tiles(contraction_size(names[i][0], shp[names[i][0]])), GRAM_TILE, GRAM_TILE)) for i in sel}
        return cls(packed, {keys[i]: 0 for i in sel}, {keys[i]: names[i] for i in sel}, _shape_fields(cfg))

    def taps(self) -> List[str]:
        return list(self.packed)

    def names(self) -> List[str]:
        return [n for t in self.packed for n in self.kernels[t]]

    def tap_of(self, name: str) -> str:
        for t, ks in self.kernels.items():
            if name in ks:
                return t
        raise KeyError(f"no Gram matrix covers {name}")

    def channels(self, tap: str) -> int:
        return gram_channels(self.packed[tap].shape[0])

    def dense(self, name: str) -> np.ndarray:
        """symmetric float64 [K, K]: the Gram matrix of the input rows of kernel ``name``"""
        return unpack_gram(self.packed[self.tap_of(name)])

    def rows_of(self, name: str) -> int:
        return self.rows[self.tap_of(name)]

    def to_act_stats(self, into: "ActStats" = None) -> "ActStats":
        """the diagonals as activation statistics: the decoder names and the logits head these matrices cover, written into ``into``
        (replacing what it holds under those names) or into a new ActStats of those names alone"""
        out = into if into is not None else ActStats({}, {}, self.shape_fields)
        if out.shape_fields != self.shape_fields:
            raise ValueError("GramStats.to_act_stats: the statistics belong to models of different shapes")
        for t, ks in self.kernels.items():
            d = gram_diagonal(self.packed[t])
            for k in ks:
                out.sums[k] = d.copy()
                out.rows[k] = self.rows[t]
        return out

    def merge(self, other: "GramStats") -> "GramStats":
        """adds the other run's matrices and counts into this one; a tap only the other holds (another ``gram_layers``) is taken over.
        Returns self"""
        if other.shape_fields != self.shape_fields:
            raise ValueError("GramStats.merge: the matrices belong to models of different shapes")
        for t in other.packed:
            if t in self.packed and (other.packed[t].shape != self.packed[t].shape or other.kernels[t] != self.kernels[t]):
                raise ValueError(f"GramStats.merge: {t} has another size or other kernels in the other statistics")
        for t in other.packed:
            if t in self.packed:
                self.packed[t] = self.packed[t] + other.packed[t]
                self.rows[t] += other.rows[t]
            else:
                self.packed[t], self.rows[t], self.kernels[t] = other.packed[t].copy(), other.rows[t], list(other.kernels[t])
        return self

    def check_against(self, cfg: DiaConfig, names: Sequence[str] = None) -> None:
        """ValueError naming the first kernel of ``names`` (default: every MX-streamed kernel, quant.mx_names(cfg)) that no matrix
        covers with the right size and at least one row"""
        shp = param_shapes(cfg)
        if self.shape_fields != _shape_fields(cfg):
            raise ValueError("the Gram matrices belong to a model of another shape")
        for k in (names if names is not None else [n for tap in decoder_tap_names(cfg) for n in tap]):
            try:
                t = self.tap_of(k)
            except KeyError:
                raise ValueError(f"the Gram matrices hold nothing for {k}") from None
            K = contraction_size(k, shp[k])
            if self.channels(t) != K:
                raise ValueError(f"the Gram matrix of {k} has {self.channels(t)} channels, the kernel contracts {K}")
            if self.rows[t] <= 0:
                raise ValueError(f"the Gram matrix of {k} counted no row")

    def save(self, path: str) -> None:
        """one .npz: ``gram/<tap>`` float64 [tiles, 32, 32] (each tap's array once), ``rows/<tap>`` int64, ``kernels/<tap>`` a
        fixed-width string array, ``shape/<field>`` int64 — arrays only, loaded with allow_pickle=False"""
        arrs = {}
        for t, v in self.packed.items():
            arrs["gram/" + t] = v
            arrs["rows/" + t] = np.int64(self.rows[t])
            arrs["kernels/" + t] = np.array(self.kernels[t], dtype=np.str_)
        for k, v in self.shape_fields.items():
            arrs["shape/" + k] = np.int64(v)
        with open(path, "wb") as f:
            np.savez(f, **arrs)

    @classmethod
    def load(cls, path: str) -> "GramStats":
        with np.load(path, allow_pickle=False) as z:
            packed = {k[5:]: z[k] for k in z.files if k.startswith("gram/")}
            rows = {k[5:]: int(z[k]) for k in z.files if k.startswith("rows/")}
            kernels = {k[8:]: [str(n) for n in z[k]] for k in z.files if k.startswith("kernels/")}
            shape = {k[6:]: int(z[k]) for k in z.files if k.startswith("shape/")}
        return cls(packed, rows, kernels, shape)
