"""Host side of the MI355X decode path: weight residency, prefill, and the decode loop.

Everything numerical happens in ``libdia_hip.so``; torch tensors are storage (``data_ptr()``),
streams and events.  The call sequence mirrors the reference's ``Dia._prepare_generation``
(dia/model.py:355-427) and the ``while`` loop of ``Dia.generate`` (model.py:748-807):

  prefill(b):  text ids -> encoder (12 layers) -> per-decoder-layer cross K/V     [model.py:382-397]
  decode:      one hipGraph replay per step; token state machine on the device     [model.py:748-807]

Rows of every activation buffer are ordered ``2*b + {0: uncond, 1: cond}`` (model.py:362).  The
uncond row never sees text, so the encoder runs on the packed non-pad tokens of
the cond row only — exact, SURVEY.md App. B3.
"""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from functools import partial
from typing import Dict, List, Optional, Sequence, Union

import numpy as np
import torch

from . import binding as hb
from . import compact as cpt
from . import layout as lay
from .config import DiaConfig
from .pruning import is_2of4
from .quant import is_mxfp4, is_mxfp8
from .tokens import CODEBOOK_SIZE

HEAD_DIM = 128
_TILERS = {1: lay.tile_weight, 2: lay.tile_weight_bf16x2, 3: lay.tile_weight_planes}       # weight_planes -> layout of a DenseGeneral kernel


def _ceil(v: int, m: int) -> int:
    return (v + m - 1) // m * m


DEC_MATS = ("qkv", "o", "cq", "co", "wi", "wo")       # the matrices of a decoder layer that a decode step streams (DecLayer w_* / kt_* / ns_*)
STEP_MATS = DEC_MATS + ("logits",)                    # ... and the head: launch order and MXFP8 class bits (enum dia_step_mat, include/dia_hip.h)


@dataclass
class TiledW:
    """One weight in a kernel layout.  With two-plane weights `kt` counts hi and lo tiles."""
    t: torch.Tensor
    kt: int
    ns: int
    planes: int = 1

    @property
    def nbytes(self) -> int:
        return self.t.numel() * self.t.element_size()

    @property
    def a_kt(self) -> int:
        """k-tiles of the activation this weight multiplies"""
        return self.kt // 2 if self.planes == 2 else self.kt


@dataclass
class UsW:
    """One matrix as an unstructured sparse stream (layout.tile_weight_us): the uint8 stream, its rate, K/32 and N/16"""
    t: torch.Tensor
    rate: int
    kt: int
    ns: int

    @property
    def nbytes(self) -> int:
        return self.t.numel()


# a matrix keeps a stream only when it is smaller than this share of its dense tiles (1.0 = smaller at all: the stream reached no
# break-even at any measured ratio, profiles/r21_usparse_speed.txt)
US_MAX_RATIO = 1.0


def _plane_set(P: torch.Tensor, kt: int):
    """(pointer, plane stride, k-tiles) of an activation plane set [plane][m-tile][kt][64][8]"""
    return hb.ptr(P), P[0].numel(), kt


def pack_segments(lengths: Sequence[int]):
    """Variable-length segments as runs of whole 32-row blocks (m-tiles and key blocks) of one packed batch:
    (offset of every segment, total rows, int32 row -> segment with -1 in the padding rows)."""
    offs, tot = [], 0
    for n in lengths:
        offs.append(tot)
        tot += _ceil(n, 32)
    row_seg = np.full((tot,), -1, dtype=np.int32)
    for i, n in enumerate(lengths):
        row_seg[offs[i]: offs[i] + n] = i
    return offs, tot, row_seg


def _compact_mlp(wi3, wo, live_hidden, keep_wi):
    """The MLP of a structured-pruned layer: the live hidden units (padded to the kernels' granule, compact.pad_hidden_keep; a padding
    unit is a zero row of wo) and the kept input rows of wi."""
    hid = cpt.pad_hidden_keep(live_hidden).to(wi3.device)
    wi3 = torch.stack([cpt.take_cols_idx(wi3[:, 0, :], hid), cpt.take_cols_idx(wi3[:, 1, :], hid)], dim=1)
    wi3 = wi3[keep_wi.to(wi3.device)]
    wo = wo[hid.clamp(min=0)].clone()
    wo[hid < 0] = 0
    return wi3, wo


def _launch_gemm(st, A, a_kt, W: TiledW, epi, *, M, ssq, ssq_ld, width, eps, w_planes, ssq_in=False, out=None, ldo=0, gnext=None,
                 P=None, p_kt=0, ssq_out=False, cmap=None, strip_map=None, kv=None, kv_layers=None, row_map=None, sk=None):
    """One dia_gemm over the M packed rows of a prefill.  `ssq` holds the strip sums of squares of the `width`-wide residual stream.
    kv: (kc, vc, kv_dtype, kv_heads, kv_cap, kv_batch_index, kv_vblocked, kv_plane_stride, cos_t, sin_t) of the cross-K/V epilogue,
    kv_layers: (strips, cache stride) per layer of a merged launch; row_map: (row_b, seg_off); sk: (splits, scratch, tickets)."""
    g = hb.GemmArgs()
    g.A, g.a_plane_stride, g.a_ktiles = _plane_set(A, a_kt)
    g.M = M
    g.W, g.KT, g.nstrips, g.epi = hb.ptr(W.t), W.kt, W.ns, epi
    g.w_planes = w_planes
    if ssq_in:
        g.ssq_in, g.ssq_in_n, g.inv_d, g.eps = hb.ptr(ssq), width // 16, 1.0 / width, eps
    g.ssq_ld = ssq_ld
    g.out, g.ldo, g.gnext = hb.ptr(out), ldo, hb.ptr(gnext)
    if P is not None:
        g.P, g.p_plane_stride, g.p_ktiles = _plane_set(P, p_kt)
    if ssq_out:
        g.ssq_out = hb.ptr(ssq)
    g.strip_map, g.cmap = hb.ptr(strip_map), hb.ptr(cmap)
    if kv is not None:
        g.kc, g.vc, g.kv_dtype, g.kv_heads, g.kv_cap, g.kv_batch_index, g.kv_vblocked, g.kv_plane_stride, g.cos_t, g.sin_t = kv
        if kv_layers is not None:
            g.kv_layer_strips, g.kv_layer_stride = kv_layers
    if row_map is not None:
        g.row_b, g.seg_off = (hb.ptr(t) for t in row_map)
    if sk is not None:      # split-K over workgroups through the session's slab scratch (short prompts: the z-form needs K <= 2048 per workgroup)
        g.sk, scratch, tickets = sk
        g.sk_scratch, g.sk_tickets, g.sk_scratch_floats = hb.ptr(scratch), hb.ptr(tickets), scratch.numel()
    hb.check(hb.lib().dia_gemm(C.byref(g), st), "dia_gemm")


class DeviceWeights:
    """Checkpoint -> kernel layouts, resident in HBM (bf16 tiles; norms / embeddings fp32)."""

    def __init__(self, cfg: DiaConfig, sd: Dict[str, torch.Tensor], device: torch.device, compact: str = "auto",
                 weight_planes: int = 1, seg: str = "off", sparse: str = "off", quant: str = "off"):
        """compact: "auto" = drop structure that a structured-pruned checkpoint zeroed (decoder only),
        "off" = keep every matrix at its checkpoint shape (zeros are streamed).
        weight_planes: 1 = every DenseGeneral kernel as ONE bf16 tile set (exact for bf16-representable checkpoints, the fast
        kernels); 2 = the hi / lo bf16 planes of the fp32 weights interleaved per k-tile (layout.tile_weight_bf16x2: relative
        error <= 2^-17, 2x the bytes, the tuned decode kernels); 3 = the hi / mid / lo bf16
        planes of the fp32 weights (exact for any checkpoint, 3x the bytes, the generic kernel: the parity configuration of a
        genuine fp32 checkpoint).
        seg: "on" = a dense Dia-1.6B-shaped decoder on a GPU also carries the ring arenas of the persistent MLP segments
        (layout.seg_ring; + 2.2 GB: co, wi, wo and the following layer's qkv once more, per CU in consumption order), which
        batch 1-2 sessions then run instead of four launches per layer when the knob seg=1 is set.  EXPERIMENT, default "off":
        measured 43 us per segment against 31 us for the four launches it replaces.
        sparse: "2:4" = a 2:4-pruned checkpoint (offline_prune.py --prune-mode 2:4) also carries every decoder q/k/v, o, cross-q,
        cross-o, wi and wo matrix and the logits head as a 2:4 sparse stream (layout.tile_weight_24, 0.5625 of the dense bytes),
        which decode steps of at most 4 rows (batch 1-2) stream instead of the dense tiles.  The dense tiles stay
        resident for the encoder, the cross K/V projections, both prefills and larger batches: the decoder's weights take about
        1.56x the memory of the dense model's decoder.  Every such matrix must hold at most 2 non-zeros in every group of 4
        consecutive K (pruning.is_2of4) and every K must be a multiple of 512; not with weight_planes != 1, a compacted
        checkpoint or seg="on".
        quant: "mxfp8" = an MXFP8-representable checkpoint (offline_quantize.py; quant.is_mxfp8) also carries the same matrices as
        MXFP8 streams (layout.tile_weight_fp8: e4m3 elements + one E8M0 scale per 32 K of a column, 0.516 of the dense bytes),
        which decode steps of at most 16 rows (batch 1-8) stream instead of the dense tiles.  The dense tiles stay resident for the
        encoder, the cross K/V projections, both prefills and larger batches and hold the same numbers, so results do not depend on
        which form a step used beyond summation order.  Every K must be a multiple of 512; not with sparse="2:4",
        weight_planes != 1, a compacted checkpoint or seg="on".
        "mxfp4" = the same for an MXFP4-representable checkpoint (offline_quantize.py --format mxfp4; quant.is_mxfp4) and MXFP4
        streams (layout.tile_weight_fp4: e2m1 elements, 0.266 of the dense bytes), under the same conditions.
        sparse: "unstructured" = an unstructured-pruned checkpoint (offline_prune.py --prune-mode unstructured) also carries the
        same matrices as lossless lane-local fixed-rate streams (layout.tile_weight_us: an 8-bit mask and a window of 4 or 2 bf16
        values per lane and k-tile plus an overflow list; the rate is chosen per matrix by the smaller stream), which decode steps
        of at most 4 rows (batch 1-2) stream for the launch classes the knob usparse enables (binding.usparse_mask).  A matrix
        whose stream is not smaller than US_MAX_RATIO of its dense tiles carries none (its entry is None) and stays dense.
        us_bytes / dense_bytes map every matrix name to its stream's bytes (0: none) and its dense tiles' bytes.  Every K must be a
        multiple of 512; not with weight_planes != 1, seg="on", quant != "off" or a compacted checkpoint.  The stream sizes
        depend on the data, so such a model is not broadcast (dist.broadcast_weights): every rank loads and tiles the checkpoint."""
        if weight_planes not in _TILERS:
            raise ValueError("weight_planes must be 1, 2 or 3")
        if sparse not in ("off", "2:4", "unstructured"):
            raise ValueError('sparse must be "off", "2:4" or "unstructured"')
        if sparse == "unstructured" and weight_planes != 1:
            raise hb.DiaHipError("sparse='unstructured': the stream holds one bf16 weight plane (weight_planes must be 1)")
        if sparse == "unstructured" and seg == "on":
            raise hb.DiaHipError("sparse='unstructured': the persistent MLP segments stream dense ring arenas (seg must be 'off')")
        if sparse == "unstructured" and quant != "off":
            raise hb.DiaHipError(f"sparse='unstructured': the unstructured sparse stream and the {quant.upper()} stream exclude each other "
                                 "(quant must be 'off')")
        if sparse == "2:4" and weight_planes != 1:
            raise hb.DiaHipError("sparse='2:4': the 2:4 stream holds one bf16 weight plane (weight_planes must be 1)")
        if sparse == "2:4" and seg == "on":
            raise hb.DiaHipError("sparse='2:4': the persistent MLP segments stream dense ring arenas (seg must be 'off')")
        if quant not in ("off", "mxfp8", "mxfp4"):
            raise ValueError('quant must be "off", "mxfp8" or "mxfp4"')
        mx = quant.upper()
        if quant != "off" and sparse == "2:4":
            raise hb.DiaHipError(f"quant='{quant}': the {mx} stream and the 2:4 sparse stream exclude each other (sparse must be 'off')")
        if quant != "off" and weight_planes != 1:
            raise hb.DiaHipError(f"quant='{quant}': an {mx} value is one bf16 value (weight_planes must be 1)")
        if quant != "off" and seg == "on":
            raise hb.DiaHipError(f"quant='{quant}': the persistent MLP segments stream dense ring arenas (seg must be 'off')")
        self.sparse = sparse
        self.quant = quant
        self.us_bytes: Dict[str, int] = {}              # sparse="unstructured": matrix name -> bytes of its stream (0: none) ...
        self.dense_bytes: Dict[str, int] = {}           # ... and of its dense tiles
        self.weight_planes = weight_planes
        m, e, d = cfg.model, cfg.model.encoder, cfg.model.decoder
        if d.gqa_head_dim != HEAD_DIM or d.cross_head_dim != HEAD_DIM or e.head_dim != HEAD_DIM:
            raise hb.DiaHipError("the HIP attention kernels are built for head_dim 128 (Dia-1.6B)")
        if d.n_embd % 32 or d.n_hidden % 32 or e.n_embd % 32 or e.n_hidden % 32:
            raise hb.DiaHipError("embedding / hidden sizes must be multiples of 32")
        self.cfg, self.device = cfg, device
        self.max_weight_rounding = 0.0                  # largest |w - bf16(w)| / max|w| over the DenseGeneral kernels

        self._build_encoder(sd, compact)
        keep_logits = self._build_decoder(sd, compact)
        self._build_seg(sd, seg)
        self.dec_norm = self._dev(sd, "decoder.norm.weight").contiguous()
        lw = self._dev(sd, "decoder.logits_dense.weight").reshape(d.n_embd, -1)
        self.logits = self._tile(lw[keep_logits.to(device)] if keep_logits is not None else lw)
        self.logits_cols = lw.shape[1]
        self.logits24 = self._tile24("decoder.logits_dense", lw) if sparse == "2:4" else None
        self.logits_us = self._tile_us("decoder.logits_dense", lw) if sparse == "unstructured" else None
        self.logits_f8 = self._tile_mx("decoder.logits_dense", lw, quant) if quant == "mxfp8" else None
        self.logits_f4 = self._tile_mx("decoder.logits_dense", lw, quant) if quant == "mxfp4" else None
        npos = max(cfg.data.audio_length, cfg.data.text_length) + 1
        cos, sin = lay.rope_tables(npos, HEAD_DIM, m.rope_min_timescale, m.rope_max_timescale)
        self.cos_t, self.sin_t = cos.to(device), sin.to(device)
        # strip map of the merged cross-K/V launch of a compacted decoder: layer l's compact strip s -> l * (CH * 16) + original strip
        self.smap_ckv_all = None
        if any(L["smap_ckv"] is not None for L in self.dec_layers):
            per_layer = d.cross_query_heads * 16
            full = torch.arange(per_layer, dtype=torch.int32, device=device)
            self.smap_ckv_all = torch.cat([(L["smap_ckv"] if L["smap_ckv"] is not None else full) + i * per_layer
                                           for i, L in enumerate(self.dec_layers)]).to(torch.int32).contiguous()
        self.flat = None
        self.pack_flat()

    def _dev(self, sd, name) -> torch.Tensor:
        return sd[name].to(device=self.device, dtype=torch.float32)

    def _i32(self, t) -> torch.Tensor:
        return t.to(device=self.device, dtype=torch.int32).contiguous()

    def _tile(self, w2d) -> TiledW:
        t, kt, ns = _TILERS[self.weight_planes](w2d)
        if w2d.numel() and self.weight_planes == 1:
            err = (w2d - w2d.to(torch.bfloat16).to(w2d.dtype)).abs().max()
            scale = w2d.abs().max()
            if float(scale) > 0.0:
                self.max_weight_rounding = max(self.max_weight_rounding, float(err / scale))
        return TiledW(t, kt, ns, self.weight_planes)

    @staticmethod
    def _tile24(name, w2d) -> TiledW:
        if w2d.shape[0] % 512:
            raise hb.DiaHipError(f"sparse='2:4': {name}: K = {w2d.shape[0]} is not a multiple of 512")
        if not is_2of4(w2d):
            raise hb.DiaHipError(f"sparse='2:4': {name} is not 2:4 sparse (more than 2 non-zeros in a group of 4 consecutive K)")
        return TiledW(*lay.tile_weight_24(w2d))

    def _tile_us(self, name, w2d) -> Optional["UsW"]:
        """the unstructured sparse stream of a matrix at the rate that makes it smaller, or None when it is not smaller than
        US_MAX_RATIO of the dense tiles"""
        if w2d.shape[0] % 512:
            raise hb.DiaHipError(f"sparse='unstructured': {name}: K = {w2d.shape[0]} is not a multiple of 512")
        pick = lay.us_choose(w2d, US_MAX_RATIO)
        self.dense_bytes[name] = (w2d.shape[0] // 32) * ((w2d.shape[1] + 15) // 16) * 1024
        self.us_bytes[name] = pick[4] if pick is not None else 0
        return UsW(pick[0], pick[1], pick[2], pick[3]) if pick is not None else None

    @staticmethod
    def _tile_mx(name, w2d, quant) -> TiledW:
        """the MXFP8 / MXFP4 stream of a matrix that holds nothing but such values"""
        pred, tiler = (is_mxfp8, lay.tile_weight_fp8) if quant == "mxfp8" else (is_mxfp4, lay.tile_weight_fp4)
        if w2d.shape[0] % 512:
            raise hb.DiaHipError(f"quant='{quant}': {name}: K = {w2d.shape[0]} is not a multiple of 512")
        if not pred(w2d):
            raise hb.DiaHipError(f"quant='{quant}': {name} is not {quant.upper()}-representable (quantise the checkpoint with "
                                 f"offline_quantize.py --format {quant})")
        return TiledW(*tiler(w2d))

    def _build_encoder(self, sd, compact: str):
        e, device = self.cfg.model.encoder, self.device
        E, EH = e.n_embd, e.n_head
        self.enc_emb = self._dev(sd, "encoder.embedding.weight").contiguous()
        plans = []
        for i in range(e.n_layer):
            pl = cpt.plan_encoder_layer({k: v for k, v in sd.items() if k.startswith(f"encoder.layers.{i}.")},
                                        f"encoder.layers.{i}.", EH)
            plans.append(pl if (compact != "off" and cpt.enc_is_pruned(pl)) else None)
        self.enc_layers = []
        for i, P in enumerate(plans):
            p = f"encoder.layers.{i}."
            wq, wk, wv = (self._dev(sd, p + f"self_attention.{n}_proj.weight").reshape(E, -1) for n in "qkv")
            o = self._dev(sd, p + "self_attention.o_proj.weight").reshape(-1, E)
            wi3 = self._dev(sd, p + "mlp.wi_fused.weight")
            wo = self._dev(sd, p + "mlp.wo.weight")
            L = dict(g_sa=self._dev(sd, p + "pre_sa_norm.weight").contiguous(), g_mlp=self._dev(sd, p + "post_sa_norm.weight").contiguous(),
                     heads=EH, cmap_mlp=None, cmap_next=None)
            nxt = plans[i + 1] if i + 1 < e.n_layer else None
            if nxt is not None:
                L["cmap_next"] = self._i32(cpt._cmap(nxt.keep_qkv))
            if P is not None:
                hc = P.live_heads.to(device).repeat_interleave(HEAD_DIM)            # live head columns
                kq = P.keep_qkv.to(device)
                wq, wk, wv = wq[kq][:, hc], wk[kq][:, hc], wv[kq][:, hc]
                o = cpt.pad_rows(o[hc])
                wi3, wo = _compact_mlp(wi3, wo, P.live_hidden, P.keep_wi)
                L.update(heads=int(P.live_heads.sum()), cmap_mlp=self._i32(cpt._cmap(P.keep_wi)))
            L.update(qkv=self._tile(torch.cat([wq, wk, wv], dim=1)), o=self._tile(o), wi=self._tile(lay.interleave_gate_up(wi3)),
                     wo=self._tile(wo))
            self.enc_layers.append(L)
        self.enc_cmap_first = self._i32(cpt._cmap(plans[0].keep_qkv)) if plans and plans[0] is not None else None
        self.enc_compacted = any(pl is not None for pl in plans)
        self.enc_norm = self._dev(sd, "encoder.norm.weight").contiguous()

    def _build_decoder(self, sd, compact: str) -> Optional[torch.Tensor]:
        """Returns the kept input rows of the logits head when compaction dropped some (None: all of them)."""
        cfg, device = self.cfg, self.device
        e, d = cfg.model.encoder, cfg.model.decoder
        D = d.n_embd
        QH, KVH, CH = d.gqa_query_heads, d.kv_heads, d.cross_query_heads
        perm = lay.rope_pair_perm(HEAD_DIM).to(device)
        self.dec_emb = torch.stack([self._dev(sd, f"decoder.embeddings.{c}.weight") for c in range(cfg.data.channels)]).contiguous()
        plans = []
        for i in range(d.n_layer):
            pl = cpt.plan_decoder_layer({k: v for k, v in sd.items() if k.startswith(f"decoder.layers.{i}.")},
                                        f"decoder.layers.{i}.", QH, KVH, CH)
            plans.append(pl if (compact != "off" and cpt.is_pruned(pl)) else None)
        keep_logits = cpt.pad_keep(cpt.nonzero_rows(sd["decoder.logits_dense.weight"].reshape(D, -1)))
        if compact == "off" or bool(keep_logits.all()):
            keep_logits = None
        self.compacted = any(p is not None for p in plans) or keep_logits is not None or self.enc_compacted
        if self.sparse == "2:4" and self.compacted:
            raise hb.DiaHipError("sparse='2:4': a compacted (structured-pruned) checkpoint has no 2:4 form; load it with compact='off' "
                                 "or prune with --prune-mode 2:4")
        if self.sparse == "unstructured" and self.compacted:
            raise hb.DiaHipError("sparse='unstructured': a compacted (structured-pruned) checkpoint has no unstructured sparse stream; "
                                 "load it with compact='off'")
        if self.quant != "off" and self.compacted:
            raise hb.DiaHipError(f"quant='{self.quant}': a compacted (structured-pruned) checkpoint has no {self.quant.upper()} stream; "
                                 "load it with compact='off'")
        i32 = self._i32
        self.dec_layers = []
        for i, P in enumerate(plans):
            p = f"decoder.layers.{i}."
            qkv = torch.cat([self._dev(sd, p + f"self_attention.{n}_proj.weight").reshape(D, -1) for n in "qkv"], dim=1)
            o = self._dev(sd, p + "self_attention.o_proj.weight").reshape(-1, D)
            cq = self._dev(sd, p + "cross_attention.q_proj.weight").reshape(D, -1)
            co = self._dev(sd, p + "cross_attention.o_proj.weight").reshape(-1, D)
            ck = self._dev(sd, p + "cross_attention.k_proj.weight")[:, :, perm].reshape(e.n_embd, -1)
            cv = self._dev(sd, p + "cross_attention.v_proj.weight").reshape(e.n_embd, -1)
            ckv = torch.cat([ck, cv], dim=1)
            wi3 = self._dev(sd, p + "mlp.wi_fused.weight")
            wo = self._dev(sd, p + "mlp.wo.weight")
            L = dict(g_sa=self._dev(sd, p + "pre_sa_norm.weight").contiguous(), g_ca=self._dev(sd, p + "pre_ca_norm.weight").contiguous(),
                     g_mlp=self._dev(sd, p + "pre_mlp_norm.weight").contiguous(),
                     cmap_ca=None, cmap_mlp=None, cmap_next=None, smap_qkv=None, smap_cq=None, smap_ckv=None,
                     hmap_self=None, hmap_cross=None)
            if i + 1 < d.n_layer:          # input order of what consumes this layer's wo output
                nk = plans[i + 1].keep_qkv if plans[i + 1] is not None else None
            else:
                nk = keep_logits
            if nk is not None:
                L["cmap_next"] = i32(cpt._cmap(nk))
            if P is not None:
                cols = lambda strips: (torch.tensor(strips, dtype=torch.long)[:, None] * 16 + torch.arange(16)[None, :]).reshape(-1).to(device)
                s_qkv = (cpt.strips_of_heads(P.live_q_heads, 0) + cpt.strips_of_heads(P.live_kv_heads, QH * 128)
                         + cpt.strips_of_heads(P.live_kv_heads, (QH + KVH) * 128))
                qkv = qkv[P.keep_qkv.to(device)][:, cols(s_qkv)]
                o = cpt.pad_rows(o[P.live_q_heads.to(device).repeat_interleave(128)])
                s_cq = cpt.strips_of_heads(P.live_c_heads, 0)
                cq = cq[P.keep_cq.to(device)][:, cols(s_cq)]
                co = cpt.pad_rows(co[P.live_c_heads.to(device).repeat_interleave(128)])
                s_ckv = cpt.strips_of_heads(P.live_c_heads, 0) + cpt.strips_of_heads(P.live_c_heads, CH * 128)
                ckv = ckv[:, cols(s_ckv)]
                wi3, wo = _compact_mlp(wi3, wo, P.live_hidden, P.keep_wi)
                L.update(cmap_ca=i32(cpt._cmap(P.keep_cq)), cmap_mlp=i32(cpt._cmap(P.keep_wi)),
                         smap_qkv=i32(torch.tensor(s_qkv)), smap_cq=i32(torch.tensor(s_cq)), smap_ckv=i32(torch.tensor(s_ckv)),
                         hmap_self=i32(cpt.head_map(P.live_q_heads)), hmap_cross=i32(cpt.head_map(P.live_c_heads)))
            mats = dict(qkv=qkv, o=o, cq=cq, co=co, wi=lay.interleave_gate_up(wi3), wo=wo)
            L["ckv"] = self._tile(ckv)
            for k in DEC_MATS:
                L[k] = self._tile(mats[k])
                L[k + "24"] = self._tile24(p + k, mats[k]) if self.sparse == "2:4" else None
                L[k + "us"] = self._tile_us(p + k, mats[k]) if self.sparse == "unstructured" else None
                L[k + "f8"] = self._tile_mx(p + k, mats[k], self.quant) if self.quant == "mxfp8" else None
                L[k + "f4"] = self._tile_mx(p + k, mats[k], self.quant) if self.quant == "mxfp4" else None
            # experiment (knob wo_diag=1): wo once more in the diagonal layout (4-column groups: 256 workgroups with the whole K each)
            L["wo_diag"] = None
            if (hb.get_tuning("wo_diag") == 1 and P is None and self.weight_planes == 1 and device.type == "cuda" and wo.shape[0] % 1024 == 0
                    and wo.shape[0] <= 8192 and wo.shape[1] % 8 == 0 and nk is None):
                L["wo_diag"] = lay.diag_tile_weight(wo)
            self.dec_layers.append(L)
        self.cmap_first = i32(cpt._cmap(plans[0].keep_qkv)) if plans[0] is not None else None
        return keep_logits

    def _build_seg(self, sd, seg: str):
        """Ring arenas of the persistent MLP segments (experiment, seg="on"): Dia-1.6B-shaped dense decoders on a GPU only."""
        d = self.cfg.model.decoder
        D, QH, KVH, CH = d.n_embd, d.gqa_query_heads, d.kv_heads, d.cross_query_heads
        self.seg_layers: List[torch.Tensor] = []
        if not (seg == "on" and self.device.type == "cuda" and self.weight_planes == 1 and not self.compacted and D == 2048
                and d.n_hidden == 8192 and QH * HEAD_DIM == 2048 and CH * HEAD_DIM == 2048 and (QH + 2 * KVH) * HEAD_DIM == 3072):
            return
        for i in range(d.n_layer):
            p = f"decoder.layers.{i}."
            wi3 = self._dev(sd, p + "mlp.wi_fused.weight")
            qn = None
            if i + 1 < d.n_layer:
                pn = f"decoder.layers.{i + 1}."
                qn = torch.cat([self._dev(sd, pn + f"self_attention.{n_}_proj.weight").reshape(D, -1) for n_ in "qkv"], dim=1)
            self.seg_layers.append(lay.seg_ring(self._dev(sd, p + "cross_attention.o_proj.weight").reshape(-1, D), wi3[:, 0, :], wi3[:, 1, :],
                                                self._dev(sd, p + "mlp.wo.weight"), qn))
            del wi3, qn

    def ckv_all(self) -> Optional[TiledW]:
        """The cross-K/V tile sets of every decoder layer as ONE weight of sum(ns) strips, when they are one bf16 tile set each with
        the same K and sit back to back in the arena (pack_flat); None otherwise (three-plane weights: one launch per layer)."""
        ts = [L["ckv"] for L in self.dec_layers]
        if self.weight_planes != 1 or not ts or any(t.kt != ts[0].kt for t in ts):
            return None
        p0 = ts[0].t.data_ptr()
        for t in ts:
            if t.t.data_ptr() != p0:
                return None
            p0 += t.nbytes
        n = sum(t.t.numel() for t in ts)
        base = ts[0].t
        whole = torch.empty(0, dtype=base.dtype, device=base.device).set_(base.untyped_storage(), base.storage_offset(), (n,))
        return TiledW(whole, ts[0].kt, sum(t.ns for t in ts))

    def tensors(self) -> List[torch.Tensor]:
        """Every device tensor of the model, in a deterministic order (the layout of the flat arena)."""
        out: List[torch.Tensor] = [self.enc_emb]
        for L in self.enc_layers:
            out += [L["g_sa"], L["g_mlp"], L["qkv"].t, L["o"].t, L["wi"].t, L["wo"].t]
            out += [L[k] for k in ("cmap_mlp", "cmap_next") if L[k] is not None]
        out += [self.enc_norm, self.dec_emb]
        for L in self.dec_layers:
            out += [L["g_sa"], L["g_ca"], L["g_mlp"]] + [L[k].t for k in DEC_MATS]
            out += [L[k] for k in ("cmap_ca", "cmap_mlp", "cmap_next", "smap_qkv", "smap_cq", "smap_ckv", "hmap_self", "hmap_cross", "wo_diag")
                    if L[k] is not None]
        # the cross-K/V projections of ALL layers back to back (whole KiB each, so the 256-byte slots leave no gaps): the prefill runs them
        # as ONE GEMM over their common input (ckv_all)
        out += [L["ckv"].t for L in self.dec_layers]
        if self.smap_ckv_all is not None:
            out.append(self.smap_ckv_all)
        out += [self.dec_norm, self.logits.t, self.cos_t, self.sin_t]
        out += [t for t in (self.cmap_first, self.enc_cmap_first) if t is not None]
        out += self.seg_layers
        if self.sparse == "2:4":                    # the 2:4 streams (sparse="2:4"), after everything the dense model holds
            for L in self.dec_layers:
                out += [L[k + "24"].t for k in DEC_MATS]
            out.append(self.logits24.t)
        if self.sparse == "unstructured":           # the unstructured sparse streams, in the same place (the matrices that have one)
            for L in self.dec_layers:
                out += [L[k + "us"].t for k in DEC_MATS if L[k + "us"] is not None]
            if self.logits_us is not None:
                out.append(self.logits_us.t)
        if self.quant == "mxfp8":                   # the MXFP8 streams (quant="mxfp8"), after everything the dense model holds
            for L in self.dec_layers:
                out += [L[k + "f8"].t for k in DEC_MATS]
            out.append(self.logits_f8.t)
        if self.quant == "mxfp4":                   # the MXFP4 streams (quant="mxfp4"), in the same place
            for L in self.dec_layers:
                out += [L[k + "f4"].t for k in DEC_MATS]
            out.append(self.logits_f4.t)
        return out

    def pack_flat(self):
        """Move every tensor into ONE contiguous byte arena (256-byte aligned slots, order of tensors()): the model is a
        single HBM allocation, and the multi-GPU weight distribution is a single broadcast of it (one
        ncclBroadcast of the repacked weights).  Tensor objects keep their identity; only their storage moves."""
        ts = self.tensors()
        offs, tot = [], 0
        for t in ts:
            offs.append(tot)
            tot += (t.numel() * t.element_size() + 255) // 256 * 256
        flat = torch.zeros(tot, dtype=torch.uint8, device=self.device)
        for t, o in zip(ts, offs):
            nb = t.numel() * t.element_size()
            v = flat[o: o + nb].view(t.dtype).view(t.shape)
            v.copy_(t)
            t.data = v
        self.flat = flat

    @classmethod
    def empty_like_config(cls, cfg: DiaConfig, device: torch.device, weight_planes: int = 1, seg: str = "off",
                          sparse: str = "off", quant: str = "off") -> "DeviceWeights":
        """Same tensors, zero-filled: the receive side of the multi-GPU weight broadcast (dense layout;
        a compacted, i.e. structured-pruned, model has checkpoint-dependent shapes: every rank then
        loads the checkpoint itself instead of receiving a broadcast).  `weight_planes` must be the sender's
        (dist.broadcast_weights checks it on every rank before the arena travels)."""
        from .weights import param_shapes
        if sparse == "unstructured":
            raise hb.DiaHipError("sparse='unstructured': the stream sizes depend on the checkpoint, so there is no arena to receive; "
                                 "load and tile the checkpoint on every rank")
        sd = {k: torch.zeros(shp, dtype=torch.float32, device=device) for k, shp in param_shapes(cfg).items()}
        return cls(cfg, sd, device, compact="off", weight_planes=weight_planes, seg=seg, sparse=sparse, quant=quant)

    def prefill_weight_bytes(self) -> int:
        """bf16 bytes the prefill streams once per batch: the encoder and the cross K/V projections"""
        n = sum(L[k].nbytes for L in self.enc_layers for k in ("qkv", "o", "wi", "wo"))
        return n + sum(L["ckv"].nbytes for L in self.dec_layers)

    def decode_weight_bytes(self, rows: int = 2) -> int:
        """bf16 bytes one decode step of `rows` rows (2 per utterance) streams (SURVEY.md §8d 'W'): every decoder matrix except
        the prefill-only cross K/V projections, plus the logits head — the 2:4 streams where the step uses them (sparse="2:4",
        at most 4 rows) and the MXFP8 streams for the matrices of STEP_MATS the library enables at this row count (quant="mxfp8",
        at most 16 rows: binding.mxfp8_mask; quant="mxfp4": the MXFP4 streams, binding.mxfp4_mask)."""
        every = self.sparse == "2:4" and rows <= 4
        us = hb.usparse_mask(rows) if self.sparse == "unstructured" else 0
        mx = {"mxfp8": hb.mxfp8_mask, "mxfp4": hb.mxfp4_mask}[self.quant](rows) if self.quant != "off" else 0
        sfx = "f4" if self.quant == "mxfp4" else "f8"
        logits_mx = self.logits_f4 if self.quant == "mxfp4" else self.logits_f8

        def w(L, k):
            if us >> STEP_MATS.index(k) & 1 and L[k + "us"] is not None:
                return L[k + "us"].nbytes
            if mx >> STEP_MATS.index(k) & 1:
                return L[k + sfx].nbytes
            return L[k + "24"].nbytes if every else L[k].nbytes
        if us >> STEP_MATS.index("logits") & 1 and self.logits_us is not None:
            n = self.logits_us.nbytes
        else:
            n = logits_mx.nbytes if mx >> STEP_MATS.index("logits") & 1 else (self.logits24.nbytes if every else self.logits.nbytes)
        for L in self.dec_layers:
            n += sum(w(L, k) for k in DEC_MATS)
        return n


@dataclass
class Request:
    """One utterance for a continuously batched session (DecodeSession.open / admit / serve): what the reference's generate()
    takes per call (model.py:631-646).  max_tokens None = the session's."""
    text_ids: np.ndarray
    seed: Optional[int] = None
    max_tokens: Optional[int] = None
    cfg_scale: float = 3.0
    temperature: float = 1.3
    top_p: float = 0.95
    top_k: int = 35
    audio_prompt: Optional[np.ndarray] = None      # codes [Tp, C]; the prompt rows are replayed through the decode step (prompt_prefill="batched": prefilled)
    adapter: Optional[Union[str, int]] = None      # name or index in the session's AdapterBank; None = the base model


@dataclass
class UtteranceResult:
    tokens: np.ndarray          # int32 [T, C] token buffer (DecoderOutput.generated_tokens)
    codes: np.ndarray           # rows [prefill_step : last_step+1]   (model.py:831)
    last_step: int
    preds: np.ndarray           # int32 [T, C] raw samples per step row (before the EOS state machine)
    text_len: int


class KvFp8Cache:
    """An e4m3 K/V cache, all layers in one allocation per tensor: bytes k8 [n_layer, rows, heads, cap, 128] and v8 (the blocked V layout,
    [.., cap / 32, 128, 32]), fp32 scales per key ks / vs [n_layer, rows, heads, cap].  Zeroed once: a key that was never written, or is
    left over in a re-used slot, is finite bytes times a finite scale."""

    def __init__(self, n_layer: int, rows: int, heads: int, cap: int, device=None):
        z = lambda *s, dt: torch.zeros(n_layer, rows, heads, *s, dtype=dt, device=device)
        self.k8, self.v8 = z(cap, HEAD_DIM, dt=torch.uint8), z(cap // 32, HEAD_DIM, 32, dt=torch.uint8)
        self.ks, self.vs = z(cap, dt=torch.float32), z(cap, dt=torch.float32)

    def ptrs(self, layer: Optional[int] = None) -> hb.KvFp8Ptrs:        # the whole allocation, or one layer's view of it
        k8, v8, ks, vs = (t if layer is None else t[layer] for t in (self.k8, self.v8, self.ks, self.vs))
        return hb.KvFp8Ptrs(k8=hb.ptr(k8), v8=hb.ptr(v8), ks=hb.ptr(ks), vs=hb.ptr(vs))

    def ptr_array(self):        # every layer's pointers, as dia_engine_set_cross_fp8 / _self_fp8 take them (the engine copies the array)
        return (hb.KvFp8Ptrs * len(self.k8))(*[self.ptrs(i) for i in range(len(self.k8))])

    @property
    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in (self.k8, self.v8, self.ks, self.vs))


class DecodeSession:
    """Buffers + engine for one batch of utterances."""

    prompt_prefill = "auto"                      # (set per session; "batched" also prefills at slot admission and onto fp8 self caches)

    def __init__(self, w: DeviceWeights, text_ids: Sequence[np.ndarray], *, kv_dtype: str = "bf16",
                 max_tokens: Optional[int] = None, cfg_scale: float = 3.0, temperature: float = 1.3,
                 top_p: float = 0.95, top_k: int = 35, seeds: Optional[Sequence[Optional[int]]] = None,
                 noise: Optional[torch.Tensor] = None, ignore_eos: bool = False,
                 teacher_tokens: Optional[Sequence[np.ndarray]] = None, stream: Optional[torch.cuda.Stream] = None,
                 s_cap: Optional[int] = None, audio_prompts: Optional[Sequence[Optional[np.ndarray]]] = None,
                 prompt_prefill: str = "auto", attention: str = "auto", score: bool = False,
                 adapters=None, adapter_ids: Optional[Sequence[Union[None, str, int]]] = None, cross_kv: str = "bf16",
                 self_kv: str = "bf16", calibrate: Union[bool, str] = False, gram_layers=None, _slotted: bool = False):
        """audio_prompts: per utterance None or int codes [Tp, C] (reference model.py:311-353).  The prompt
        rows are replayed through the decode step before sampling starts (semantics: oracle.generate), or — with
        bf16 caches — prefilled as one packed MFMA batch; prompt_prefill="replay" forces the replay.
        prompt_prefill="batched" (opt-in; DESIGN.md "Prompt prefill at admission and onto fp8 caches"): every prompt of more than
        one frame is prefilled as a packed batch — also at slot admission (admit / serve / stream_iter) and onto self_kv="fp8"
        caches, which "auto" leaves to the replay.  Whatever the prefill kernels cannot serve raises ValueError here: fp32 or
        two-plane K/V, attention="valu", adapters=, teacher_tokens= / score=True, a compacted decoder, weight_planes != 1.
        attention="valu" keeps bf16 V caches row-major and runs the VALU attention kernel (comparison runs).
        score=True (with teacher_tokens): every step also reduces its logits to the log-probability of the forced row, on the
        device (dia_score; DESIGN.md "Scoring"); scores_host() downloads the [B, T, C, 3] result once at the end.
        adapters: a lora.AdapterBank whose adapters stay UNMERGED beside the base weights (DESIGN.md "Per-request adapters");
        adapter_ids[b] = name or index of utterance b's adapter, None = base model.  The bank is fixed from here on.  Such a session
        replays audio prompts through the decode step (no batched prompt prefill), and refuses a compacted model and seg="on".
        cross_kv="fp8": the decode step's cross-attention reads an e4m3 copy of the cross caches with one power-of-two scale per key
        and head (DESIGN.md "FP8 cross K/V"), quantised from the bf16 caches behind every encoder pass; needs bf16 K/V with the
        blocked V layout.  "bf16" (default): nothing of it exists.
        self_kv="fp8": the SELF caches are e4m3 bytes with one power-of-two scale per key and head (DESIGN.md "FP8 self K/V"): the step's
        self-attention quantises the new key as it appends it, k_self / v_self are not allocated (self_cache_bytes is 0.516 of the
        bf16 session's) and audio prompts replay through the decode step unless prompt_prefill="batched".  Needs bf16 K/V with the blocked V layout and
        audio_length % 32 == 0; independent of cross_kv.  "bf16" (default): nothing of it exists.
        calibrate=True (with teacher_tokens): the encoder pass and every step also accumulate, in front of each GEMM, the per-channel
        sum of squares of its input rows on the device (dia_act_stats; DESIGN.md "Activation statistics"); act_stats() downloads them
        once at the end.  Closed teacher-forced sessions only: slots, adapters=, a compacted checkpoint and seg="on" raise ValueError.
        So do forced rows of unequal lengths or a max_tokens other than their length: teacher forcing acts on no EOS, so the rows behind
        a shorter utterance would be counted.  Goes together with score=True.
        calibrate="gram": everything calibrate=True does, except that the decode step's taps run dia_act_gram (DESIGN.md "Gram matrices
        and GPTQ") and accumulate the full Gram matrix of each GEMM input, for the layers of gram_layers (None: every decoder layer and the
        logits head; else layer indices or a (first, end) tuple, index n_layer standing for the logits head — T (T + 1) / 2 * 8 KiB per tap of
        T k-tiles).  gram_stats() downloads the matrices; act_stats() keeps working, the diagonals supplying the step's sums (an
        unselected layer's names then hold no row).  The same refusals."""
        if calibrate not in (False, True, "gram"):
            raise ValueError(f"calibrate is False, True or 'gram', not {calibrate!r}")
        if gram_layers is not None and calibrate != "gram":
            raise ValueError("gram_layers needs calibrate='gram'")
        if calibrate:
            why = None
            if teacher_tokens is None:
                why = "it measures teacher-forced rows: pass teacher_tokens"
            elif _slotted:
                why = "slots: a slot session admits and retires requests while it runs, calibration is for closed batches"
            elif adapters is not None:
                why = "adapters=: the statistics are the base model's, an adapter's correction is not part of any pruned kernel"
            elif w.compacted:
                why = "a compacted checkpoint: its kernels contract permuted, shortened channel lists (load it with compact='off')"
            elif w.seg_layers:
                why = "seg='on': the persistent MLP segments keep the inputs of co, wi and wo inside their launch"
            elif len({int(np.asarray(t).shape[0]) for t in teacher_tokens}) != 1 or (max_tokens is not None and int(max_tokens) != int(np.asarray(teacher_tokens[0]).shape[0])):
                why = ("forced rows of different lengths (or another max_tokens): every step counts the rows of every utterance, and a "
                       "teacher-forced utterance does not end before max_tokens")
            if why is not None:
                raise ValueError(f"calibrate={calibrate!r} is not served with {why}")
        if adapter_ids is not None and adapters is None:
            raise ValueError("adapter_ids needs adapters= (an AdapterBank)")
        if score and (teacher_tokens is None or _slotted):
            raise ValueError("score=True scores teacher-forced rows of a closed batch: pass teacher_tokens (and no slots)")
        if prompt_prefill not in ("auto", "replay", "batched") or attention not in ("auto", "valu"):
            raise ValueError("prompt_prefill must be 'auto', 'replay' or 'batched', attention 'auto' or 'valu'")
        if cross_kv not in ("bf16", "fp8"):
            raise ValueError("cross_kv must be 'bf16' or 'fp8'")
        if self_kv not in ("bf16", "fp8"):
            raise ValueError("self_kv must be 'bf16' or 'fp8'")
        self.prompt_prefill = prompt_prefill
        cfg, dev = w.cfg, w.device
        self.w, self.cfg, self.dev = w, cfg, dev
        d, da = cfg.model.decoder, cfg.data
        self.B = B = len(text_ids)
        self.R = 2 * B
        self.rows_pad = _ceil(self.R, 16)
        self.T = da.audio_length
        self.C, self.V, self.D, self.F = da.channels, cfg.model.tgt_vocab_size, d.n_embd, d.n_hidden
        self.max_tokens = self.T if max_tokens is None else int(max_tokens)
        if not (2 <= self.max_tokens <= self.T):
            raise ValueError(f"max_tokens must be in [2, {self.T}]")
        # "bf16x2": every K / V value as hi + lo bf16 in two planes of the bf16 layouts (16 significand bits, the bytes of the fp32
        # caches): the MFMA attention kernel with logits inside the 1e-3 parity bound
        self.kv_code = {"f32": hb.KV_F32, "float32": hb.KV_F32, "bf16": hb.KV_BF16, "bfloat16": hb.KV_BF16, "bf16x2": hb.KV_BF16X2}[kv_dtype]
        if self.kv_code == hb.KV_BF16X2 and attention == "valu":
            raise ValueError("kv_dtype 'bf16x2' is served by the MFMA attention kernel only")
        # bf16 caches keep V blocked as [key/32][128][32] for the MFMA attention kernel
        self.v_blocked = int(self.kv_code in (hb.KV_BF16, hb.KV_BF16X2) and attention != "valu")
        if cross_kv == "fp8":
            if self.kv_code != hb.KV_BF16:
                raise ValueError(f"cross_kv='fp8' is quantised from one-plane bf16 cross caches: kv_dtype '{kv_dtype}' (fp32 or two-plane K/V) "
                                 "is not served")
            if attention == "valu" or not self.v_blocked:
                raise ValueError("cross_kv='fp8' needs the blocked V layout of the MFMA attention kernel (attention='valu' keeps V row-major)")
        self.cross_kv = cross_kv
        if self_kv == "fp8":
            if self.kv_code != hb.KV_BF16:
                raise ValueError(f"self_kv='fp8' replaces one-plane bf16 self caches: kv_dtype '{kv_dtype}' (fp32 or two-plane K/V) is not served")
            if attention == "valu" or not self.v_blocked:
                raise ValueError("self_kv='fp8' needs the blocked V layout of the MFMA attention kernel (attention='valu' keeps V row-major)")
            if self.T % 32 != 0:
                raise ValueError(f"self_kv='fp8' needs audio_length % 32 == 0 (whole 32-key granules), not {self.T}")
        self.self_kv = self_kv
        if prompt_prefill == "batched":              # everything the dia_dec_prefill_* kernels cannot serve, by name, before anything is allocated
            why = None
            if self.kv_code != hb.KV_BF16:
                why = f"kv_dtype '{kv_dtype}' (fp32 or two-plane K/V): the prefill kernels write and read one-plane bf16 or fp8 self caches"
            elif not self.v_blocked:
                why = "attention='valu' keeps V row-major: the prefill kernels need the blocked V layout"
            elif adapters is not None:
                why = "adapters=: the batched prefill's projections carry no adapter correction"
            elif teacher_tokens is not None or score:
                why = "teacher_tokens= / score=True: forced rows are scored step by step"
            elif w.compacted:
                why = "a compacted decoder: the prefill GEMMs address the uncompacted columns"
            elif w.weight_planes != 1:
                why = f"weight_planes = {w.weight_planes}: the prefill GEMMs read one-plane weights"
            if why is not None:
                raise ValueError(f"prompt_prefill='batched' is not served with {why}")
        kvt = torch.float32 if self.kv_code == hb.KV_F32 else torch.bfloat16
        self.kv_planes = 2 if self.kv_code == hb.KV_BF16X2 else 1
        self.stream = stream if stream is not None else torch.cuda.Stream(device=dev)
        self.lens = [int(len(t)) for t in text_ids]
        self.S = s_cap if s_cap is not None else max(32, _ceil(max(self.lens + [1]), 32))
        if self.S > da.text_length and s_cap is None:
            self.S = da.text_length
        self.text_ids = [np.asarray(t, dtype=np.int32) for t in text_ids]
        self.teacher = teacher_tokens is not None
        self.ignore_eos = ignore_eos
        md = max(da.delay_pattern)
        self.max_delay = md

        z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)
        mt = self.rows_pad // 16
        self.xkt, self.akt, self.hkt = self.D // 32, max(d.gqa_query_heads, d.cross_query_heads) * HEAD_DIM // 32, self.F // 32
        self.x = z(self.rows_pad, self.D)
        # <= 4 rows: handed to the engine for the case that it lets the launch behind a wo merge wo's split-K slices (dia_engine_set_x_alt:
        # then the residual stream of odd layers).  The engine decides per model; two-plane, 2:4, MXFP8 and compacted models and the
        # knob wo_defer=0 keep the in-launch merge and leave this buffer (128 KB) unused
        self.x_alt = z(self.rows_pad, self.D) if self.R <= 4 else None
        # activations between the kernels of a step travel as fp32 tiles in these buffers (the fragment order of one plane, 4-byte
        # values: 4 instead of the 6 bytes of three bf16 planes hi + mid + lo == fp32); every consumer splits the planes itself — the
        # M <= 4 GEMV while staging its image through LDS, the 16-row GEMM in registers — same arithmetic bit for bit.
        # Tuning knob act_f32=0 keeps the planes between the kernels.
        t_ = hb.get_tuning("act_f32")
        self.act_f32 = int(t_ != 0)
        # persistent MLP segments (csrc/seg.hip, experiment): batch 1-2 on a model that carries the ring arenas, knob seg=1
        self.seg = bool(self.R <= 4 and w.seg_layers and self.act_f32 and hb.get_tuning("seg") == 1)
        self.seg_ws = None
        if self.seg:
            self.seg_ws = torch.zeros(int(hb.lib().dia_seg_workspace_bytes()), dtype=torch.uint8, device=dev)
        self.planes_x = z(3, mt, self.xkt, 64, 8, dt=torch.bfloat16)
        self.planes_a = z(3, mt, self.akt, 64, 8, dt=torch.bfloat16)
        self.planes_h = z(3, mt, self.hkt, 64, 8, dt=torch.bfloat16)
        self.ssq = z(self.D // 8, self.rows_pad)          # strip sums of squares: D / 16 per row, D / 8 behind the diagonal-layout wo
        self.nqkv = (d.gqa_query_heads + 2 * d.kv_heads) * HEAD_DIM
        self.qkv = z(self.rows_pad, self.nqkv)
        self.qc = z(self.rows_pad, d.cross_query_heads * HEAD_DIM)
        self.ld_logits = w.logits.ns * 16
        self.logits = z(self.rows_pad, self.ld_logits)
        pl = (self.kv_planes,) if self.kv_planes > 1 else ()           # two-plane caches: [plane][...]
        # self_kv="fp8": the self caches ARE an e4m3 cache, no bf16 cache beside it
        self.f8_self = KvFp8Cache(d.n_layer, self.R, d.kv_heads, self.T, dev) if self_kv == "fp8" else None
        self.k_self = [None if self.f8_self else z(*pl, self.R, d.kv_heads, self.T, HEAD_DIM, dt=kvt) for _ in range(d.n_layer)]
        self.v_self = [None if self.f8_self else z(*pl, self.R, d.kv_heads, self.T, HEAD_DIM, dt=kvt) for _ in range(d.n_layer)]
        # cross caches of all layers in ONE allocation each (per-layer views): the prefill's merged cross-K/V launch addresses a layer
        # as kc + layer * kv_layer_stride
        self.k_cross_all = z(d.n_layer, *pl, B, d.cross_query_heads, self.S, HEAD_DIM, dt=kvt)
        self.v_cross_all = z(d.n_layer, *pl, B, d.cross_query_heads, self.S, HEAD_DIM, dt=kvt)
        self.k_cross = [self.k_cross_all[i] for i in range(d.n_layer)]
        self.v_cross = [self.v_cross_all[i] for i in range(d.n_layer)]
        # cross_kv="fp8": the e4m3 copy the step's cross-attention reads, beside the bf16 caches (which stay: +50 % cross-cache memory);
        # zero bytes and zero scales until dia_kv_quantize_fp8 writes a row's granules
        self.f8_cross = KvFp8Cache(d.n_layer, B, d.cross_query_heads, self.S, dev) if cross_kv == "fp8" else None
        self.kv_plane_self = self.R * d.kv_heads * self.T * HEAD_DIM if self.kv_planes > 1 else 0
        self.kv_plane_cross = B * d.cross_query_heads * self.S * HEAD_DIM if self.kv_planes > 1 else 0
        self.text_len = torch.tensor(self.lens, dtype=torch.int32, device=dev)
        nsc = max(hb.lib().dia_attn_scratch_floats(self.R, d.kv_heads, self.T),
                  hb.lib().dia_attn_scratch_floats(B, d.cross_query_heads, self.S))
        self.attn_scratch = z(max(nsc, 1))
        self.attn_tickets = z(max(self.R * d.kv_heads, B * d.cross_query_heads), dt=torch.int32)
        # split-K slabs: up to 4 splits of wo (one or two m-tiles); with 17..32 rows every GEMM splits K in two
        ns_max = max([self.D // 16, w.logits.ns] + [DL[k].ns for DL in w.dec_layers for k in DEC_MATS])
        n_scr = max((self.D // 16) * 4 * 512, ns_max * 2 * 512 if 16 < self.R <= 32 else 0)
        if 16 < self.R <= 128:   # 2..8 m-tiles: wo splits K four ways for every m-tile (k_gemm16 over gridDim.z)
            n_scr = max(n_scr, 2 * -(-self.R // 32) * (self.D // 16) * 4 * 256)       # (whole PAIRS of m-tiles: k_gemm2t hands two tiles over together)
        if 16 < self.R <= 32:    # k_gemm_blk32: column blocks x K ranges of >= 8 k-tiles, 512 floats per strip and range
            n_scr = max([n_scr, w.logits.ns * -(-w.logits.kt // 8) * 512] +
                        [DL[k].ns * -(-DL[k].kt // 8) * 512 for DL in w.dec_layers for k in DEC_MATS])
        if self.R <= 4:          # room for the two K slices of a wo whose merge is deferred (if the engine defers): one padded m-tile of x each
            n_scr = max(n_scr, 2 * self.rows_pad * self.D)
        self.sk_scratch = z(n_scr)
        self.sk_tickets = z(max(ns_max, 8 * (self.D // 16)), dt=torch.int32)
        self.mlp_barrier = z(2, dt=torch.int32)          # dia_mlp_fused: arrivals, error flag

        # token buffer + state machine (state.py:178-208; model.py:736-741)
        from .tokens import delayed_prefill
        tok = np.full((B, self.T, self.C), -1, dtype=np.int32)
        self.first_steps = []
        for b in range(B):
            pr = None if audio_prompts is None else audio_prompts[b]
            if pr is not None:
                pr = np.asarray(pr)
                if pr.ndim == 3 and pr.shape[0] == 1:
                    pr = pr[0]
                if pr.ndim != 2 or pr.shape[1] != self.C:
                    raise ValueError(f"Unexpected audio_prompt shape: {pr.shape}. Expected [T, C] or [1, T, C].")   # model.py:316
            prefill, pstep = delayed_prefill(cfg, pr)
            if prefill.shape[0] > self.T:
                raise ValueError(f"audio prompt of {pstep - 1} frames does not fit audio_length {self.T}")
            tok[b, : prefill.shape[0]] = prefill
            self.first_steps.append(int(pstep))
        if self.teacher:
            for b in range(B):
                tt = np.asarray(teacher_tokens[b], dtype=np.int32)
                tok[b, : tt.shape[0]] = tt
        self.prefill_step = 1                     # every utterance starts at step 1; steps < first_step replay the prompt
        self.first_step = torch.tensor(self.first_steps, dtype=torch.int32, device=dev)
        self.tokens = torch.from_numpy(tok).to(dev)
        self.pred = torch.full((B, self.T, self.C), -1, dtype=torch.int32, device=dev)
        self.cur = torch.full((B,), 1, dtype=torch.int32, device=dev)
        fsm = np.zeros((B, 8), dtype=np.int32)
        fsm[:, 1] = -1
        fsm[:, 2] = md
        self.fsm = torch.from_numpy(fsm).to(dev)
        self.delay = torch.tensor(list(da.delay_pattern), dtype=torch.int32, device=dev)

        # Exp(1) variates for the multinomial draw: the reference's generator stream after
        # torch.manual_seed(seed) (model.py:679-683), one [C,V] draw per sampled step.  Drawing 3071 rows takes
        # 0.7 s per utterance on the host, so they are drawn in chunks as the decode advances (the stream of a
        # generator is the same whether it is consumed in one draw or in pieces) and uploaded ahead of the steps
        # that read them; a generation that ends early never draws the rest.
        self.noise_steps = self.max_tokens - 1
        self._noise_rows = 0                    # rows [0, _noise_rows) are on the device
        self._issued = 0                        # decode steps enqueued so far
        self._gens = None
        if temperature != 0.0:
            if noise is not None:
                nz = noise.to(torch.float32)
                if tuple(nz.shape) != (B, self.noise_steps, self.C, self.V):
                    raise ValueError(f"noise must be [B,{self.noise_steps},{self.C},{self.V}]")
                self.noise = nz.to(dev)
                self._noise_rows = self.noise_steps
            else:
                self.noise = torch.empty(B, self.noise_steps, self.C, self.V, dtype=torch.float32, device=dev)
                self._gens = []
                for b in range(B):
                    g = torch.Generator()
                    sd = None if seeds is None else seeds[b]
                    if sd is None:
                        g.seed()
                    else:
                        g.manual_seed(int(sd))
                    self._gens.append(g)
        else:
            self.noise = None
            self._noise_rows = self.noise_steps

        self.sample_params = dict(cfg_scale=float(cfg_scale), temperature=float(temperature), top_p=float(top_p),
                                  top_k=int(top_k or 0))
        self._pinned: List[torch.Tensor] = []    # pinned host buffers of asynchronous copies still in the stream (dropped at sync())
        self.slotted = bool(_slotted)
        if self.slotted:
            self._init_slots()
        self.adapters = adapters
        if adapters is not None:
            self._init_adapters(adapter_ids)
        # teacher-forced scoring: lp_cond, lp_cfg, H_cfg per row and channel; NaN = no step has scored this position
        self.scores = torch.full((B, self.T, self.C, 3), float("nan"), dtype=torch.float32, device=dev) if score else None
        self._calib = None
        if calibrate:
            self._init_calib(gram=calibrate == "gram", gram_layers=gram_layers)
        self._engine = C.c_void_p()
        self._build_engine()
        self.prefilled = self.slotted            # slots are prefilled one by one, at admission

    # ------------------------------------------------------------------ per-request adapters (DESIGN.md "Per-request adapters")
    def _init_adapters(self, adapter_ids):
        """adapter_of_slot on the device (-1 = base model) + the bank's tables; everything the unmerged path cannot serve raises here"""
        w, bank = self.w, self.adapters
        if w.compacted:
            raise hb.DiaHipError("adapters=: a compacted (structured-pruned) checkpoint permutes the columns the corrections address; "
                                 "load it with compact='off' or merge the adapter at load (adapter_path=)")
        if w.seg_layers:
            raise hb.DiaHipError("adapters=: the persistent MLP segments run the q/k/v projection inside their launch (seg must be 'off')")
        if bank.cfg.model != self.cfg.model:
            raise hb.DiaHipError("adapters=: the bank was built for another model configuration")
        if adapter_ids is not None and (self.slotted or len(adapter_ids) != self.B):
            raise ValueError("adapter_ids: one entry per utterance of a closed batch (slot sessions take Request.adapter)")
        ids = [bank.index_of(a) for a in (adapter_ids if adapter_ids is not None else [None] * self.B)]
        bank.freeze()
        if bank.arena.device != self.x.device:       # (tensors' own devices: "cuda" and "cuda:0" name the same one)
            raise hb.DiaHipError(f"adapters=: the bank lives on {bank.arena.device}, the session on {self.x.device}")
        self._adapter_host = np.asarray(ids, dtype=np.int32)
        self.adapter_of_slot = torch.from_numpy(self._adapter_host.copy()).to(self.dev)

    def _push_adapter_slots(self):
        """the host's adapter_of_slot -> the device, in stream order (pinned + asynchronous, like every table of an admission)"""
        pin = torch.from_numpy(self._adapter_host.copy()).pin_memory()
        self._pinned.append(pin)
        with torch.cuda.stream(self.stream):
            self.adapter_of_slot.copy_(pin, non_blocking=True)

    def _zero_ranks(self) -> torch.Tensor:
        if getattr(self, "_zero_rank_t", None) is None:
            self._zero_rank_t = torch.zeros(len(self.adapters), dtype=torch.int32, device=self.dev)
        return self._zero_rank_t

    def _lora_common(self, a, x, ldx, D, gain, M):
        a.x, a.ldx, a.D, a.gain, a.eps, a.M = x, ldx, D, hb.ptr(gain), float(self.cfg.model.normalization_layer_epsilon), M
        a.adapter_of_slot, a.n_slots, a.n_adapters = hb.ptr(self.adapter_of_slot), self.B, len(self.adapters)

    # ------------------------------------------------------------------ activation statistics (DESIGN.md "Activation statistics")
    def _init_calib(self, gram=False, gram_layers=None):
        """one float64 accumulator per tap (the decode step's 6 * n_layer + 1, then the encoder pass's 4 * n_layer + 1) and one row
        counter each; a tap's width is the contraction size of the kernels behind it.  gram: the decode step's taps get a packed Gram
        matrix instead (the selected ones) and no vector"""
        from . import calib as cal
        from .weights import param_shapes
        shp = param_shapes(self.cfg)
        taps = cal.decoder_tap_names(self.cfg) + cal.encoder_tap_names(self.cfg)
        kt = []
        for names in taps:
            Ks = {cal.contraction_size(k, shp[k]) for k in names}
            if len(Ks) != 1 or next(iter(Ks)) % 32 != 0:
                raise ValueError(f"calibrate=True: the kernels behind the tap of {names[0]} contract {sorted(Ks)} channels (one size, a multiple of 32)")
            kt.append(next(iter(Ks)) // 32)
        n_dec = len(cal.decoder_tap_names(self.cfg))
        sel = set(cal.gram_layer_taps(self.cfg, gram_layers)) if gram else set()
        self._calib = dict(names=taps, kt=kt, n_dec=n_dec,
                           acc=[None if gram and j < n_dec else torch.zeros(32 * k, dtype=torch.float64, device=self.dev) for j, k in enumerate(kt)],
                           counters=torch.zeros(len(taps), dtype=torch.int64, device=self.dev))
        if gram:
            self._calib["gram"] = [torch.zeros(cal.gram_tiles(32 * kt[j]) * 1024, dtype=torch.float64, device=self.dev) if j in sel else None
                                   for j in range(n_dec)]

    def _enc_tap(self, st, i, P, kt, row_mask, M, ssq=None, width=0, eps=0.0):
        """dia_act_stats over the encoder pass's plane set P in front of the GEMM of encoder tap i (bf16 planes; ssq: the normed stream)"""
        c = self._calib
        j = c["n_dec"] + i
        a = hb.ActStatsArgs()
        a.x, a.plane_stride, a.ktiles = _plane_set(P, kt)
        a.ktiles_used, a.M, a.rows_pad, a.act_f32 = c["kt"][j], M, M, 0
        if ssq is not None:
            a.ssq_in, a.ssq_in_n, a.ssq_ld, a.inv_d, a.eps = hb.ptr(ssq), width // 16, M, 1.0 / width, eps
        a.row_mask = hb.ptr(row_mask)
        a.acc, a.counter = hb.ptr(c["acc"][j]), c["counters"].data_ptr() + 8 * j
        hb.check(hb.lib().dia_act_stats(C.byref(a), st), "dia_act_stats")

    def act_stats(self):
        """calib.ActStats of everything this session has counted so far (calibrate=True); synchronises"""
        from . import calib as cal
        if self._calib is None:
            raise hb.DiaHipError("act_stats(): the session was not built with calibrate=True")
        self.sync()
        c = self._calib
        counts = c["counters"].cpu().numpy()
        out = cal.ActStats.zeros(self.cfg)
        if "gram" in c:                        # the step's sums are the diagonals of its Gram matrices
            self._gram_stats(counts).to_act_stats(into=out)
        for j, names in enumerate(c["names"]):
            if c["acc"][j] is None:
                continue
            v = c["acc"][j].cpu().numpy()
            for k in names:
                out.sums[k] = v.copy()
                out.rows[k] = int(counts[j])
        return out

    def _gram_stats(self, counts):
        from . import calib as cal
        c = self._calib
        keys = cal.gram_tap_keys(self.cfg)
        sel = [j for j, g in enumerate(c["gram"]) if g is not None]
        return cal.GramStats({keys[j]: c["gram"][j].cpu().numpy() for j in sel}, {keys[j]: int(counts[j]) for j in sel},
                             {keys[j]: c["names"][j] for j in sel}, cal._shape_fields(self.cfg))

    def gram_stats(self):
        """calib.GramStats of everything the selected taps have counted so far (calibrate="gram"); synchronises"""
        if self._calib is None or "gram" not in self._calib:
            raise hb.DiaHipError("gram_stats(): the session was not built with calibrate='gram'")
        self.sync()
        return self._gram_stats(self._calib["counters"].cpu().numpy())

    # ------------------------------------------------------------------ engine descriptor
    def _embed_args(self) -> hb.EmbedArgs:
        e = hb.EmbedArgs()
        e.tokens, e.cur = hb.ptr(self.tokens), hb.ptr(self.cur)
        e.B, e.T, e.C, e.V, e.D = self.B, self.T, self.C, self.V, self.D
        e.emb, e.g, e.x = hb.ptr(self.w.dec_emb), hb.ptr(self.w.dec_layers[0]["g_sa"]), hb.ptr(self.x)
        e.P, e.p_plane_stride, e.p_ktiles = _plane_set(self.planes_x, self.xkt)
        e.ssq_ld, e.ssq = self.rows_pad, hb.ptr(self.ssq)
        e.cmap = hb.ptr(self.w.cmap_first)
        e.act_f32 = self.act_f32
        return e

    def _sample_args(self) -> hb.SampleArgs:
        da = self.cfg.data
        s = hb.SampleArgs()
        s.logits, s.ld_logits, s.B, s.T, s.C, s.V = hb.ptr(self.logits), self.ld_logits, self.B, self.T, self.C, self.V
        s.max_tokens = self.max_tokens
        s.cfg_scale, s.temperature, s.top_p = (self.sample_params[k] for k in ("cfg_scale", "temperature", "top_p"))
        s.top_k = self.sample_params["top_k"]
        s.eos, s.pad, s.bos, s.max_delay = da.audio_eos_value, da.audio_pad_value, da.audio_bos_value, self.max_delay
        s.ignore_eos, s.teacher = int(self.ignore_eos), int(self.teacher)
        s.delay, s.noise, s.noise_steps = hb.ptr(self.delay), hb.ptr(self.noise), self.noise_steps
        s.tokens, s.pred, s.cur, s.fsm = hb.ptr(self.tokens), hb.ptr(self.pred), hb.ptr(self.cur), hb.ptr(self.fsm)
        s.first_step = hb.ptr(self.first_step) if self.slotted or any(f != 1 for f in self.first_steps) else None
        s.embed = self._embed_args()
        if self.slotted:
            s.slot_cfg_scale, s.slot_temperature, s.slot_top_p = (hb.ptr(self.slot_f32[i]) for i in range(3))
            s.slot_top_k, s.slot_max_tokens = hb.ptr(self.slot_i32[0]), hb.ptr(self.slot_i32[1])
        return s

    def _build_engine(self):
        d = self.cfg.model.decoder
        w = self.w
        n = d.n_layer
        self._layers = (hb.DecLayer * n)()
        for i, L in enumerate(w.dec_layers):
            dl = self._layers[i]
            for f in DEC_MATS:
                setattr(dl, "w_" + f, hb.ptr(L[f].t))
                setattr(dl, "kt_" + f, L[f].kt)
                setattr(dl, "ns_" + f, L[f].ns)
                sp = L[f + "24"]                                            # 2:4 stream (sparse="2:4"), NULL = dense only
                setattr(dl, "w_" + f + "_24", hb.ptr(sp.t) if sp is not None else None)
                f8 = L[f + "f8"]                                            # MXFP8 stream (quant="mxfp8"), NULL = dense only
                setattr(dl, "w_" + f + "_f8", hb.ptr(f8.t) if f8 is not None else None)
            dl.g_sa, dl.g_ca, dl.g_mlp = hb.ptr(L["g_sa"]), hb.ptr(L["g_ca"]), hb.ptr(L["g_mlp"])
            dl.k_self, dl.v_self = hb.ptr(self.k_self[i]), hb.ptr(self.v_self[i])
            dl.k_cross, dl.v_cross = hb.ptr(self.k_cross[i]), hb.ptr(self.v_cross[i])
            for f in ("cmap_ca", "cmap_mlp", "cmap_next", "smap_qkv", "smap_cq", "hmap_self", "hmap_cross"):
                setattr(dl, f, hb.ptr(L[f]))
            dl.w_wo_diag = hb.ptr(L["wo_diag"])
        ed = hb.EngineDesc()
        ed.n_layer, ed.D, ed.F = n, self.D, self.F
        ed.q_heads, ed.kv_heads, ed.cq_heads = d.gqa_query_heads, d.kv_heads, d.cross_query_heads
        ed.C, ed.V, ed.B, ed.T, ed.S = self.C, self.V, self.B, self.T, self.S
        ed.kv_dtype, ed.rows_pad, ed.ld_logits = self.kv_code, self.rows_pad, self.ld_logits
        ed.v_blocked = self.v_blocked
        ed.kv_plane_self, ed.kv_plane_cross = self.kv_plane_self, self.kv_plane_cross
        ed.eps = float(self.cfg.model.normalization_layer_epsilon)
        ed.layers = C.cast(self._layers, C.POINTER(hb.DecLayer))
        ed.w_logits, ed.kt_logits, ed.ns_logits = hb.ptr(w.logits.t), w.logits.kt, w.logits.ns
        ed.w_logits_24 = hb.ptr(w.logits24.t) if w.logits24 is not None else None
        ed.w_logits_f8 = hb.ptr(w.logits_f8.t) if w.logits_f8 is not None else None
        ed.g_final = hb.ptr(w.dec_norm)
        ed.x, ed.planes_x, ed.planes_a, ed.planes_h = hb.ptr(self.x), hb.ptr(self.planes_x), hb.ptr(self.planes_a), hb.ptr(self.planes_h)
        ed.ssq, ed.qkv, ed.qc, ed.logits = hb.ptr(self.ssq), hb.ptr(self.qkv), hb.ptr(self.qc), hb.ptr(self.logits)
        ed.cos_t, ed.sin_t, ed.text_len = hb.ptr(w.cos_t), hb.ptr(w.sin_t), hb.ptr(self.text_len)
        ed.attn_scratch, ed.attn_tickets = hb.ptr(self.attn_scratch), hb.ptr(self.attn_tickets)
        ed.sk_scratch, ed.sk_tickets = hb.ptr(self.sk_scratch), hb.ptr(self.sk_tickets)
        ed.sk_scratch_floats = self.sk_scratch.numel()
        ed.mlp_barrier = hb.ptr(self.mlp_barrier)
        ed.act_f32 = self.act_f32
        ed.w_planes = w.weight_planes
        ed.sample = self._sample_args()
        if self.seg:
            self._seg_w = (C.c_void_p * n)(*[hb.ptr(t) for t in w.seg_layers])
            ed.seg_w = C.cast(self._seg_w, C.POINTER(C.c_void_p))
            ed.seg_ws = hb.ptr(self.seg_ws)
        self._desc = ed
        hb.check(hb.lib().dia_engine_create(C.byref(ed), C.c_void_p(self.stream.cuda_stream), C.byref(self._engine)),
                 "dia_engine_create")
        if self.x_alt is not None:
            hb.check(hb.lib().dia_engine_set_x_alt(self._engine, hb.ptr(self.x_alt)), "dia_engine_set_x_alt")
        if self.f8_cross is not None:                                       # the step's cross-attention reads the e4m3 copy
            hb.check(hb.lib().dia_engine_set_cross_fp8(self._engine, self.f8_cross.ptr_array()), "dia_engine_set_cross_fp8")
        if self.f8_self is not None:                                        # the step's self-attention appends to and reads the e4m3 caches
            hb.check(hb.lib().dia_engine_set_self_fp8(self._engine, self.f8_self.ptr_array()), "dia_engine_set_self_fp8")
        if w.quant == "mxfp4":                                              # MXFP4 streams (quant="mxfp4"): beside the description
            f4_layers = (hb.Mxfp4Layer * n)()                               # (the engine copies the array)
            for i, L in enumerate(w.dec_layers):
                for f in DEC_MATS:
                    setattr(f4_layers[i], "w_" + f, hb.ptr(L[f + "f4"].t))
            f4 = hb.Mxfp4Streams(n_layer=n, layers=C.cast(f4_layers, C.POINTER(hb.Mxfp4Layer)), w_logits=hb.ptr(w.logits_f4.t))
            hb.check(hb.lib().dia_engine_set_mxfp4(self._engine, C.byref(f4)), "dia_engine_set_mxfp4")
        if w.sparse == "unstructured":                                      # unstructured sparse streams: beside the description
            us_layers = (hb.UsLayer * n)()                                  # (the engine copies the array)
            mat = lambda u: hb.UsMat(stream=hb.ptr(u.t), rate=u.rate) if u is not None else hb.UsMat()
            for i, L in enumerate(w.dec_layers):
                for f in DEC_MATS:
                    setattr(us_layers[i], "w_" + f, mat(L[f + "us"]))
            us = hb.UsStreams(n_layer=n, layers=C.cast(us_layers, C.POINTER(hb.UsLayer)), w_logits=mat(w.logits_us))
            hb.check(hb.lib().dia_engine_set_usparse(self._engine, C.byref(us)), "dia_engine_set_usparse")
        if self.scores is not None:
            sp, sc = ed.sample, hb.ScoreArgs()
            sc.logits, sc.ld_logits, sc.B, sc.T, sc.C, sc.V = sp.logits, sp.ld_logits, sp.B, sp.T, sp.C, sp.V
            sc.cfg_scale, sc.eos, sc.pad, sc.bos = sp.cfg_scale, sp.eos, sp.pad, sp.bos
            sc.tokens, sc.cur, sc.first_step, sc.fsm, sc.out = sp.tokens, sp.cur, sp.first_step, sp.fsm, hb.ptr(self.scores)
            hb.check(hb.lib().dia_engine_set_score(self._engine, C.byref(sc)), "dia_engine_set_score")
        if self._calib is not None and "gram" in self._calib:               # one dia_act_gram in front of every GEMM of the selected layers
            c = self._calib
            nd = c["n_dec"]
            gp = (C.c_void_p * nd)(*[hb.ptr(t) for t in c["gram"]])         # (the engine copies both arrays; None = no launch)
            kts = (C.c_int32 * nd)(*c["kt"][:nd])
            ga = hb.GramArgs(n_layer=n, gram=C.cast(gp, C.POINTER(C.c_void_p)), kt=C.cast(kts, C.POINTER(C.c_int32)),
                             counters=c["counters"].data_ptr())
            hb.check(hb.lib().dia_engine_set_gram(self._engine, C.byref(ga)), "dia_engine_set_gram")
        elif self._calib is not None:                                       # one dia_act_stats in front of every GEMM of the step
            c = self._calib
            nd = c["n_dec"]
            acc = (C.c_void_p * nd)(*[hb.ptr(t) for t in c["acc"][:nd]])   # (the engine copies both arrays)
            kts = (C.c_int32 * nd)(*c["kt"][:nd])
            ca = hb.CalibArgs(n_layer=n, acc=C.cast(acc, C.POINTER(C.c_void_p)), kt=C.cast(kts, C.POINTER(C.c_int32)),
                              counters=c["counters"].data_ptr())
            hb.check(hb.lib().dia_engine_set_calib(self._engine, C.byref(ca)), "dia_engine_set_calib")
        if self.adapters is not None:                                       # unmerged adapters: two more launches per layer
            bank, QH, KVH = self.adapters, d.gqa_query_heads, d.kv_heads
            ll = (hb.LoraLayer * n)()                                       # (the engine copies the array)
            for i in range(n):
                ll[i].q, ll[i].k = bank.seg(("self", i, "q"), 0), bank.seg(("self", i, "k"), QH * HEAD_DIM)
                ll[i].v, ll[i].cq = bank.seg(("self", i, "v"), (QH + KVH) * HEAD_DIM), bank.seg(("cross", i, "q"), 0)
            ls = hb.LoraStep(n_layer=n, n_adapters=len(bank), layers=C.cast(ll, C.POINTER(hb.LoraLayer)),
                             adapter_of_slot=hb.ptr(self.adapter_of_slot))
            hb.check(hb.lib().dia_engine_set_lora(self._engine, C.byref(ls)), "dia_engine_set_lora")

    def close(self):
        """Tear the engine down: the stream is drained first (queued graph replays read the executable graph's own
        argument blocks), then dia_engine_destroy releases the graph, its side stream and events."""
        if self._engine:
            eng, self._engine = self._engine, C.c_void_p()
            self.stream.synchronize()
            hb.check(hb.lib().dia_engine_destroy(eng), "dia_engine_destroy")

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ prefill
    def prefill(self, keep_encoder_out: bool = False):
        """Encoder + cross-K/V precompute for every utterance, then the first input embedding.
        Replaces model.py:382-397 (Encoder.forward layers.py:445-462; precompute_cross_attn_cache 632-669).

        All utterances run as ONE packed batch: utterance b occupies rows [off_b, off_b + L_b) of every
        activation buffer, off_b a multiple of 32 (whole m-tiles and key blocks), padding rows zero.  The dense layers
        (qkv, o, wi, wo) are single GEMMs over all rows — weights are read once per batch and the row count
        is what the MFMA-tiled kernel wants — and so are the bidirectional attention (dia_enc_attn) and the cross-K/V projection, which find a row's
        utterance and RoPE position through row_b / seg_off; only the embedding runs per utterance.  Only the non-pad tokens of the cond row are computed (exact)."""
        L = hb.lib()
        st = C.c_void_p(self.stream.cuda_stream)
        self.enc_out = [None] * self.B
        self._encode(list(enumerate(self.text_ids)), keep_encoder_out)
        with torch.cuda.stream(self.stream):
            if self._prompt_prefill_batched():
                self._prompt_prefill(st)
            ea = self._embed_args()
            hb.check(L.dia_embed_tokens(C.byref(ea), st), "dia_embed_tokens")
        self.prefilled = True

    def _encode(self, pairs, keep_encoder_out: bool = False):
        """The packed encoder pass + cross-K/V precompute of prefill() for a list of (utterance index, text ids): the utterances of
        a closed batch, or the requests admitted into free slots of a running session.  row_b / seg_off / seg_len carry the
        utterance index, so the encoder attention and the cross-K/V launch write the rows of exactly these utterances' caches.
        Everything is enqueued on the session's stream."""
        L = hb.lib()
        cfg, w, dev = self.cfg, self.w, self.dev
        e, d = cfg.model.encoder, cfg.model.decoder
        st = C.c_void_p(self.stream.cuda_stream)
        E, Fe = e.n_embd, e.n_hidden
        eps = float(cfg.model.normalization_layer_epsilon)
        utt = [int(b) for b, _ in pairs]
        lens = [int(len(t)) for _, t in pairs]
        # unmerged adapters: the corrections of the encoder's q/k/v and of the cross K/V caches, for the utterances that have one
        bank = self.adapters if self.adapters is not None and any(self._adapter_host[b] >= 0 for b in utt) else None
        offs, tot, row_seg = pack_segments(lens)              # whole 32-key blocks per utterance (blocked V planes)
        with torch.cuda.stream(self.stream):
            if tot > 0:
                Mp, mt = tot, tot // 16
                Hmax = max(EL["heads"] for EL in w.enc_layers)
                ekt = E // 32
                akt = max(max(1, Hmax * HEAD_DIM // 32), max(EL["o"].a_kt for EL in w.enc_layers))   # o rows may be zero-padded
                hkt = max(EL["wo"].a_kt for EL in w.enc_layers)               # (compacted) hidden width in k-tiles
                # every buffer of the pass is a view of ONE zero-filled allocation (one memset instead of nine), every small integer
                # table one host array (one copy instead of 3 + B): the chain is ~80 launches, each of these was one more
                nq_max = 3 * Hmax * HEAD_DIM
                shapes = [((Mp, E), torch.float32), ((3, mt, ekt, 64, 8), torch.bfloat16), ((3, mt, akt, 64, 8), torch.bfloat16),
                          ((3, mt, hkt, 64, 8), torch.bfloat16), ((E // 16, Mp), torch.float32), ((Mp, nq_max), torch.float32),
                          ((3, Hmax, Mp, HEAD_DIM), torch.bfloat16), ((3, Hmax, Mp, HEAD_DIM), torch.bfloat16)]
                sizes = [_ceil(int(np.prod(sh)) * (4 if dt == torch.float32 else 2), 256) for sh, dt in shapes]
                ws = torch.zeros(sum(sizes), dtype=torch.uint8, device=dev)
                views, o_ = [], 0
                for (sh, dt), nb in zip(shapes, sizes):
                    n_el = int(np.prod(sh))
                    views.append(ws[o_: o_ + n_el * (4 if dt == torch.float32 else 2)].view(dt).view(*sh))
                    o_ += nb
                x, px, pa, ph, ssq, qkv, kp, vp = views          # (kp / vp: K / V planes of the attention, scratch)
                live = [i for i in range(len(pairs)) if lens[i] > 0]      # (positions in `pairs`; utt[i] = the utterance)
                id_off, n_ids = {}, 0
                for i in live:
                    id_off[i] = n_ids
                    n_ids += _ceil(lens[i], 4)                     # (16-byte aligned runs)
                tab = np.zeros((Mp + 2 * _ceil(self.B, 4) + n_ids,), dtype=np.int32)
                tab[:Mp] = np.where(row_seg >= 0, np.asarray(utt, dtype=np.int32)[np.maximum(row_seg, 0)], -1)
                o_so, o_sl = Mp, Mp + _ceil(self.B, 4)
                tab[o_so + np.asarray(utt)] = offs
                tab[o_sl + np.asarray(utt)] = lens
                o_id = Mp + 2 * _ceil(self.B, 4)
                for i in live:
                    tab[o_id + id_off[i]: o_id + id_off[i] + lens[i]] = pairs[i][1]
                # pinned + asynchronous: a pageable copy blocks the host until the stream has drained, and every launch behind it starts late
                self._pf_tab_host = torch.from_numpy(tab).pin_memory()        # (kept until the next prefill: the copy reads it in stream order)
                self._pinned.append(self._pf_tab_host)
                tab_d = self._pf_tab_host.to(dev, non_blocking=True)
                row_b, seg_off, seg_len = tab_d[:Mp], tab_d[o_so: o_so + self.B], tab_d[o_sl: o_sl + self.B]

                def rows(t, i, width):              # device pointer of row off_i of a [Mp, width] fp32 buffer
                    return t.data_ptr() + offs[i] * width * 4

                def planes_at(P, i, kt_):           # device pointer of m-tile off_i/16 of a plane set (bf16)
                    return P.data_ptr() + (offs[i] // 16) * kt_ * 512 * 2

                for i in live:
                    ids = tab_d[o_id + id_off[i]: o_id + id_off[i] + lens[i]]
                    hb.check(L.dia_embed_text(hb.ptr(ids), lens[i], hb.ptr(w.enc_emb), E, hb.ptr(w.enc_layers[0]["g_sa"]),
                                              rows(x, i, E), planes_at(px, i, ekt), px[0].numel(), ekt,
                                              ssq.data_ptr() + offs[i] * 4, Mp, hb.ptr(w.enc_cmap_first), st), "dia_embed_text")

                gemm = partial(_launch_gemm, st, M=Mp, ssq=ssq, ssq_ld=Mp, width=E, eps=eps, w_planes=w.weight_planes)
                # calibrate=True: the statistics of the rows in front of every GEMM; every packed row of an utterance counts, no padding row
                tap = None
                if self._calib is not None:
                    live_rows = (row_b >= 0).to(torch.uint8)
                    tap = partial(self._enc_tap, st, row_mask=live_rows, M=Mp)

                def cross_kv(kc, vc):               # the cross-K/V epilogue writes every utterance's rows of these caches (row_b / seg_off)
                    return (hb.ptr(kc), hb.ptr(vc), self.kv_code, d.cross_query_heads, self.S, 0, self.v_blocked, self.kv_plane_cross,
                            hb.ptr(w.cos_t), hb.ptr(w.sin_t))

                for i, EL in enumerate(w.enc_layers):
                    Hl = EL["heads"]                 # live heads of this layer (all of them unless the checkpoint was pruned)
                    nq = 3 * Hl * HEAD_DIM
                    if Hl > 0:
                        if tap:
                            tap(4 * i, px, ekt, ssq=ssq, width=E, eps=eps)
                        gemm(px, ekt, EL["qkv"], hb.EPI_SCALE_STORE, ssq_in=True, out=qkv, ldo=nq)
                        segs = [bank.seg(("enc", i, p_), j * Hl * HEAD_DIM) for j, p_ in enumerate("qkv")] if bank is not None else []
                        segs = [s_ for s_ in segs if s_.n_cols]
                        if segs:                     # x is still the row this GEMM's input was normed from (g_sa), o_proj has not run
                            la = hb.LoraArgs()
                            self._lora_common(la, hb.ptr(x), E, E, EL["g_sa"], Mp)
                            la.row_slot, la.rows_per_slot, la.n_segs, la.out, la.ldo = hb.ptr(row_b), 1, len(segs), hb.ptr(qkv), nq
                            for j, s_ in enumerate(segs):
                                la.seg[j] = s_
                            hb.check(L.dia_lora_apply(C.byref(la), st), "dia_lora_apply")
                        ea_ = hb.EncAttnArgs()
                        ea_.qkv, ea_.ldq, ea_.q_off, ea_.k_off, ea_.v_off = hb.ptr(qkv), nq, 0, Hl * HEAD_DIM, 2 * Hl * HEAD_DIM
                        ea_.heads, ea_.rows = Hl, Mp
                        ea_.row_b, ea_.seg_off, ea_.seg_len = hb.ptr(row_b), hb.ptr(seg_off), hb.ptr(seg_len)
                        ea_.cos_t, ea_.sin_t, ea_.kp, ea_.vp = hb.ptr(w.cos_t), hb.ptr(w.sin_t), hb.ptr(kp), hb.ptr(vp)
                        ea_.P, ea_.p_plane_stride, ea_.p_ktiles = _plane_set(pa, akt)
                        hb.check(L.dia_enc_attn(C.byref(ea_), st), "dia_enc_attn")
                        if tap:
                            tap(4 * i + 1, pa, akt)
                        gemm(pa, akt, EL["o"], hb.EPI_RESID_EMIT, out=x, ldo=E, gnext=EL["g_mlp"], P=px, p_kt=ekt, ssq_out=True,
                             cmap=EL["cmap_mlp"])
                    else:
                        raise hb.DiaHipError("encoder layer with every attention head pruned is not supported")
                    if tap:
                        tap(4 * i + 2, px, ekt, ssq=ssq, width=E, eps=eps)
                    gemm(px, ekt, EL["wi"], hb.EPI_SWIGLU_EMIT, ssq_in=True, P=ph, p_kt=hkt)
                    if tap:
                        tap(4 * i + 3, ph, hkt)
                    gnext = w.enc_layers[i + 1]["g_sa"] if i + 1 < len(w.enc_layers) else w.enc_norm
                    # 17..128 rows: wo (K = 4096) as two K halves per strip, so that it rides the z-form of the 16-row kernel instead
                    # of the generic one (whose 4-m-tile form spills)
                    wo_sk = None
                    kt_wo, ns_wo = EL["wo"].kt, EL["wo"].ns
                    if (16 < Mp <= 128 and kt_wo % 16 == 0 and kt_wo // 2 <= 64 and w.weight_planes == 1 and EL["cmap_next"] is None
                            and self.sk_scratch.numel() >= mt * ns_wo * 2 * 256 and self.sk_tickets.numel() >= mt * ns_wo):
                        wo_sk = (2, self.sk_scratch, self.sk_tickets)
                    gemm(ph, hkt, EL["wo"], hb.EPI_RESID_EMIT, out=x, ldo=E, gnext=gnext, P=px, p_kt=ekt, ssq_out=True,
                         cmap=EL["cmap_next"], sk=wo_sk)
                # px now holds planes(x * encoder.norm.weight); ssq the row sums of squares of x
                if tap:
                    tap(4 * len(w.enc_layers), px, ekt, ssq=ssq, width=E, eps=eps)
                ckv_all = w.ckv_all() if hb.get_tuning("ckv_merge") != 0 else None
                if ckv_all is not None:             # ONE launch for the 18 layers: their input is the same (18 x 13.8 -> 1 x ~100 us at 98 rows)
                    gemm(px, ekt, ckv_all, hb.EPI_CROSSKV, ssq_in=True, kv=cross_kv(self.k_cross_all, self.v_cross_all),
                         strip_map=w.smap_ckv_all, row_map=(row_b, seg_off), kv_layers=(d.cross_query_heads * 16, self.k_cross[0].numel()))
                else:
                    for i, DL in enumerate(w.dec_layers):
                        gemm(px, ekt, DL["ckv"], hb.EPI_CROSSKV, ssq_in=True, kv=cross_kv(self.k_cross[i], self.v_cross[i]),
                             strip_map=DL["smap_ckv"], row_map=(row_b, seg_off))
                for i in range(len(w.dec_layers) if bank is not None else 0):
                    # RoPE is linear: RoPE(dK) and dV are added to what the CROSSKV epilogue stored, for the rows of these utterances
                    # only (row_b).  x holds the encoder's last residual rows, encoder.norm is the consumer's weight
                    ks, vs = bank.seg(("cross", i, "k"), 0), bank.seg(("cross", i, "v"), 0)
                    if not (ks.n_cols or vs.n_cols):
                        continue
                    ca = hb.LoraCrossKvArgs()
                    self._lora_common(ca, hb.ptr(x), E, E, w.enc_norm, Mp)
                    ca.row_b, ca.seg_off = hb.ptr(row_b), hb.ptr(seg_off)
                    for s_ in (ks, vs):              # a module no adapter touches: an all-zero rank table of the right width
                        if not s_.n_cols:
                            o_ = ks if ks.n_cols else vs
                            s_.n_cols, s_.A, s_.B, s_.scale = d.cross_query_heads * HEAD_DIM, o_.A, o_.B, o_.scale
                            s_.rank = hb.ptr(self._zero_ranks())
                    ca.k, ca.v = ks, vs
                    (ca.kc, ca.vc, ca.kv_dtype, ca.kv_heads, ca.kv_cap, ca.kv_batch_index, ca.kv_vblocked, ca.kv_plane_stride, ca.cos_t,
                     ca.sin_t) = cross_kv(self.k_cross[i], self.v_cross[i])
                    ca.rope_rows = w.cos_t.shape[0]
                    hb.check(L.dia_lora_crosskv(C.byref(ca), st), "dia_lora_crosskv")
                if self.cross_kv == "fp8":         # behind the CROSSKV epilogue AND the adapters' corrections: the copy the step reads
                    self._quantize_cross(utt, lens)
                if keep_encoder_out:
                    for i in live:
                        Lb, o = lens[i], offs[i]
                        inv = torch.rsqrt(ssq[:, o: o + Lb].sum(dim=0) / E + eps)
                        self.enc_out[utt[i]] = (x[o: o + Lb] * inv[:, None] * w.enc_norm[None, :]).clone()

    def _quantize_cross(self, utt: Sequence[int], lens: Sequence[int]):
        """dia_kv_quantize_fp8 for exactly these utterances' rows of the cross caches: ONE launch over all decoder layers per
        DIA_SLOTS_PER_CALL rows, on the session's stream (the caller holds it)."""
        d = self.cfg.model.decoder
        st = C.c_void_p(self.stream.cuda_stream)
        for i0 in range(0, len(utt), hb.SLOTS_PER_CALL):
            rows, ln = list(utt[i0: i0 + hb.SLOTS_PER_CALL]), list(lens[i0: i0 + hb.SLOTS_PER_CALL])
            a = hb.KvFp8Args()
            a.kc, a.vc = hb.ptr(self.k_cross_all), hb.ptr(self.v_cross_all)
            a.out = self.f8_cross.ptrs()
            a.B, a.heads, a.S, a.n = self.B, d.cross_query_heads, self.S, len(rows)
            a.row, a.len = (C.c_int32 * len(rows))(*rows), (C.c_int32 * len(rows))(*ln)
            a.n_layer = d.n_layer
            a.kv_layer_stride = a.f8_layer_stride = self.k_cross[0].numel()
            hb.check(hb.lib().dia_kv_quantize_fp8(C.byref(a), st), "dia_kv_quantize_fp8")

    # ------------------------------------------------------------------ audio-prompt prefill, batched
    def _prompt_prefill_batched(self) -> bool:
        """The batched MFMA prefill of the prompt rows needs bf16 caches with the blocked V layout and an
        uncompacted decoder; everything else replays the prompt rows through the decode step (first_step).  A session with
        adapters= always replays: the batched prefill's projections carry no adapter correction, the decode step's do.  So does
        self_kv="fp8" under "auto": the replay quantises every prompted key exactly like a generated one; and so does a slot
        session, whose admissions replay.  prompt_prefill="batched" (checked at construction) prefills in all of these."""
        if self.prompt_prefill == "batched":
            return any(f > 2 for f in self.first_steps)
        return (not self.slotted and self.self_kv != "fp8" and self.adapters is None and any(f > 2 for f in self.first_steps) and self.v_blocked == 1 and self.kv_code == hb.KV_BF16 and not self.w.compacted and not self.teacher
                and self.prompt_prefill != "replay" and self.w.weight_planes == 1)

    def _prompt_prefill(self, st, slots=None):
        """Decoder.forward in prefill mode (layers.py:722-766) for the audio prompts of the given (utterance / slot b, first_step)
        pairs at once (None: every utterance of a closed batch), with the replay's semantics (token row r -> slot r, position
        r + 1): packed rows = both CFG rows of every prompted utterance; dense layers on the MFMA-tiled GEMM, K/V append / causal
        self-attention / cross attention over the caches by the dia_dec_prefill_* kernels (the _fp8 entry points over e4m3 self
        caches).  Afterwards cur[b] = first_step[b]: the whole tensor for a closed batch; for admitted slots an indexed device
        write of exactly those slots (a live slot's cur is the device's), from one pinned table with the packing — no host wait."""
        L = hb.lib()
        cfg, w, dev = self.cfg, self.w, self.dev
        d = cfg.model.decoder
        D, F = self.D, self.F
        QH, KVH, CH = d.gqa_query_heads, d.kv_heads, d.cross_query_heads
        eps = float(cfg.model.normalization_layer_epsilon)
        closed = slots is None
        pairs = list(enumerate(self.first_steps)) if closed else [(int(b), int(fs)) for b, fs in slots]
        pairs = [(b, fs) for b, fs in pairs if fs > 2]       # rows 0..fs-2 are prefilled; fs == 2 (one frame) is left to the replay path
        if not pairs:
            return
        segs = []                                   # (cache row 2b+c, prompt rows)
        for b, fs in pairs:
            segs += [(2 * b, fs - 1), (2 * b + 1, fs - 1)]
        offs, Mp, rs = pack_segments([n for _, n in segs])
        mt = Mp // 16
        if closed:
            i32 = lambda a: torch.tensor(a, dtype=torch.int32, device=dev)
            row_seg = torch.from_numpy(rs).to(dev)
            seg_off, seg_len, seg_row = i32(offs), i32([n for _, n in segs]), i32([r for r, _ in segs])
        else:                                       # one pinned table, one asynchronous copy: packing, then the slots and their cur
            ns, nb = _ceil(len(segs), 4), _ceil(len(pairs), 4)
            tab = np.zeros((Mp + 3 * ns + 2 * nb,), dtype=np.int32)
            tab[:Mp] = rs
            for j, col in enumerate((offs, [n for _, n in segs], [r for r, _ in segs])):
                tab[Mp + j * ns: Mp + j * ns + len(segs)] = col
            o_b = Mp + 3 * ns
            tab[o_b: o_b + len(pairs)] = [b for b, _ in pairs]
            tab[o_b + nb: o_b + nb + len(pairs)] = [fs for _, fs in pairs]
            pin = torch.from_numpy(tab).pin_memory()
            self._pinned.append(pin)
            tab_d = pin.to(dev, non_blocking=True)
            row_seg, seg_off, seg_len, seg_row = (tab_d[:Mp], tab_d[Mp: Mp + len(segs)], tab_d[Mp + ns: Mp + ns + len(segs)],
                                                  tab_d[Mp + 2 * ns: Mp + 2 * ns + len(segs)])
            cur_idx, cur_val = tab_d[o_b: o_b + len(pairs)], tab_d[o_b + nb: o_b + nb + len(pairs)]
        fp8 = self.self_kv == "fp8"
        z = lambda *sh, dt=torch.float32: torch.zeros(*sh, dtype=dt, device=dev)
        xkt, akt, hkt = D // 32, max(QH, CH) * HEAD_DIM // 32, F // 32
        x = z(Mp, D)
        px, pa, ph = (z(3, mt, kt_, 64, 8, dt=torch.bfloat16) for kt_ in (xkt, akt, hkt))
        ssq = z(D // 16, Mp)
        qkv, qc = z(Mp, self.nqkv), z(Mp, CH * HEAD_DIM)

        def pargs():
            a = hb.DecPrefillArgs()
            a.row_seg, a.seg_off, a.seg_len, a.seg_row, a.rows = hb.ptr(row_seg), hb.ptr(seg_off), hb.ptr(seg_len), hb.ptr(seg_row), Mp
            a.cos_t, a.sin_t = hb.ptr(w.cos_t), hb.ptr(w.sin_t)
            return a

        gemm = partial(_launch_gemm, st, M=Mp, ssq=ssq, ssq_ld=Mp, width=D, eps=eps, w_planes=w.weight_planes)

        a = pargs()
        a.tokens, a.T, a.C, a.V, a.D = hb.ptr(self.tokens), self.T, self.C, self.V, D
        a.emb, a.g, a.x = hb.ptr(w.dec_emb), hb.ptr(w.dec_layers[0]["g_sa"]), hb.ptr(x)
        a.P, a.p_plane_stride, a.p_ktiles = _plane_set(px, xkt)
        a.ssq, a.ssq_ld = hb.ptr(ssq), Mp
        hb.check(L.dia_dec_prefill_embed(C.byref(a), st), "dia_dec_prefill_embed")
        for i, DL in enumerate(w.dec_layers):
            gemm(px, xkt, DL["qkv"], hb.EPI_SCALE_STORE, ssq_in=True, out=qkv, ldo=self.nqkv)
            a = pargs()
            a.q, a.ldq, a.q_off, a.k_off, a.v_off = hb.ptr(qkv), self.nqkv, 0, QH * HEAD_DIM, (QH + KVH) * HEAD_DIM
            a.q_heads, a.kv_heads, a.kv_cap, a.causal = QH, KVH, self.T, 1
            a.P, a.p_plane_stride, a.p_ktiles = _plane_set(pa, akt)
            if fp8:                                 # kc == vc == NULL: the e4m3 caches are the only self caches
                f8 = self.f8_self.ptrs(i)
                hb.check(L.dia_dec_prefill_kv_fp8(C.byref(a), C.byref(f8), st), "dia_dec_prefill_kv_fp8")
                hb.check(L.dia_dec_prefill_attn_fp8(C.byref(a), C.byref(f8), st), "dia_dec_prefill_attn_fp8")
            else:
                a.kc, a.vc = hb.ptr(self.k_self[i]), hb.ptr(self.v_self[i])
                hb.check(L.dia_dec_prefill_kv(C.byref(a), st), "dia_dec_prefill_kv")
                hb.check(L.dia_dec_prefill_attn(C.byref(a), st), "dia_dec_prefill_attn(self)")
            gemm(pa, akt, DL["o"], hb.EPI_RESID_EMIT, out=x, ldo=D, gnext=DL["g_ca"], P=px, p_kt=xkt, ssq_out=True)
            gemm(px, xkt, DL["cq"], hb.EPI_SCALE_STORE, ssq_in=True, out=qc, ldo=CH * HEAD_DIM)
            a = pargs()
            a.q, a.ldq, a.q_off = hb.ptr(qc), CH * HEAD_DIM, 0
            a.q_heads, a.kv_heads, a.kv_cap, a.causal = CH, CH, self.S, 0
            a.kc, a.vc, a.text_len = hb.ptr(self.k_cross[i]), hb.ptr(self.v_cross[i]), hb.ptr(self.text_len)
            a.P, a.p_plane_stride, a.p_ktiles = _plane_set(pa, akt)
            hb.check(L.dia_dec_prefill_attn(C.byref(a), st), "dia_dec_prefill_attn(cross)")
            gemm(pa, akt, DL["co"], hb.EPI_RESID_EMIT, out=x, ldo=D, gnext=DL["g_mlp"], P=px, p_kt=xkt, ssq_out=True)
            gemm(px, xkt, DL["wi"], hb.EPI_SWIGLU_EMIT, ssq_in=True, P=ph, p_kt=hkt)
            gnext = w.dec_layers[i + 1]["g_sa"] if i + 1 < len(w.dec_layers) else w.dec_norm
            gemm(ph, hkt, DL["wo"], hb.EPI_RESID_EMIT, out=x, ldo=D, gnext=gnext, P=px, p_kt=xkt, ssq_out=True)
        if closed:
            cur = [fs if fs > 2 else 1 for fs in self.first_steps]
            self.cur.copy_(torch.tensor(cur, dtype=torch.int32))
        else:
            self.cur.index_copy_(0, cur_idx.long(), cur_val)

    # ------------------------------------------------------------------ decode
    def ensure_noise(self, rows: int):
        """Make the Exp(1) rows [0, rows) resident (no-op for explicit noise / greedy sampling).  Step number s of
        an utterance reads row s - first_step, so `rows` = decode steps enqueued so far is always enough."""
        if self.slotted:
            return self._ensure_slot_noise(int(rows) - self._issued)
        rows = min(int(rows), self.noise_steps)
        if self._gens is None or rows <= self._noise_rows:
            return
        r0, n = self._noise_rows, rows - self._noise_rows

        def draw(b):
            t = torch.empty(n, self.C, self.V, dtype=torch.float32)
            t.exponential_(1.0, generator=self._gens[b])
            return t

        if self.B > 1:
            from concurrent.futures import ThreadPoolExecutor
            with ThreadPoolExecutor(max_workers=min(self.B, 8)) as pool:      # torch releases the GIL while it draws
                parts = list(pool.map(draw, range(self.B)))
        else:
            parts = [draw(0)]
        host = torch.stack(parts)
        with torch.cuda.stream(self.stream):
            self.noise[:, r0:rows].copy_(host, non_blocking=False)
        self._noise_rows = rows

    def decode(self, n_steps: int, use_graph: bool = True):
        if not self.prefilled:
            raise hb.DiaHipError("decode() before prefill()")
        self.ensure_noise(self._issued + int(n_steps))
        self._enqueue_steps(int(n_steps), use_graph)
        self._issued += int(n_steps)

    def _enqueue_steps(self, n_steps: int, use_graph: bool):
        hb.check(hb.lib().dia_engine_decode(self._engine, int(n_steps), int(bool(use_graph))), "dia_engine_decode")

    def profile_step(self) -> np.ndarray:
        """per-launch milliseconds of one eager decode step (HIP events on the engine's stream)."""
        n = hb.lib().dia_engine_launches_per_step(self._engine)
        buf = (C.c_float * n)()
        self.ensure_noise(self._issued + 1)
        hb.check(hb.lib().dia_engine_profile_step(self._engine, buf, n), "dia_engine_profile_step")
        self._issued += 1
        return np.array(buf[:], dtype=np.float64)

    def launches_per_step(self) -> int:
        return int(hb.lib().dia_engine_launches_per_step(self._engine))

    def seg_error(self) -> int:
        """0, or the code of a persistent-segment wait that timed out (synchronises the stream)"""
        if not self.seg:
            return 0
        return int(hb.lib().dia_seg_error(hb.ptr(self.seg_ws), C.c_void_p(self.stream.cuda_stream)))

    def time_step(self) -> np.ndarray:
        """kernel durations (milliseconds, launch order) of one eager decode step, each kernel bracketed by its own
        dispatch-level start / stop events — what rocprofv3 --kernel-trace reports per kernel."""
        n = hb.lib().dia_engine_launches_per_step(self._engine)
        buf, ivl = (C.c_float * n)(), (C.c_float * n)()
        self.ensure_noise(self._issued + 1)
        got = hb.lib().dia_engine_time_step(self._engine, buf, ivl, n)
        if got < 0:
            hb.check(got, "dia_engine_time_step")
        self._issued += 1
        self.last_kernel_names = [hb.lib().dia_timed_kernel_name(i).decode() for i in range(got)]
        self.last_intervals_ms = np.array(ivl[:got], dtype=np.float64)      # end of launch i-1 -> end of launch i
        return np.array(buf[:got], dtype=np.float64)

    def sync(self):
        self.stream.synchronize()
        self._pinned.clear()

    def steps_total(self) -> int:
        return self.max_tokens - self.prefill_step

    def run(self, use_graph: bool = True, poll: int = 64):
        """Run until every utterance has finished (EOS countdown or max_tokens); the host looks at
        the device-side `done` flags every `poll` steps only."""
        remaining = self.steps_total()
        first = True
        while remaining > 0:
            n = min(8 if first else poll, remaining)        # a short first chunk: its noise rows are the only ones drawn
            first = False                                   # before anything runs (0.23 ms of host time per row)
            self.decode(n, use_graph)
            remaining -= n
            self.ensure_noise(self._issued + min(poll, remaining))      # next chunk's noise is drawn while this one runs
            self.sync()
            if self.seg and self.seg_error():
                self.results()                               # raises with the give-up code
            if bool((self.fsm[:, 3] != 0).all().item()):
                break

    def logits_host(self) -> np.ndarray:
        """fp32 [B, 2, C, V] logits of the last executed step."""
        self.sync()
        lg = self.logits[: self.R, : self.C * self.V].reshape(self.B, 2, self.C, self.V)
        return lg.cpu().numpy()

    def scores_host(self) -> np.ndarray:
        """fp32 [B, T, C, 3] = (lp_cond, lp_cfg, H_cfg) of every teacher-forced row a step has scored, NaN elsewhere (score=True)"""
        if self.scores is None:
            raise hb.DiaHipError("scores_host(): the session was not built with score=True")
        self.sync()
        return self.scores.cpu().numpy()

    def _raise_if_invalid(self):
        """after a sync: raise when a persistent kernel of the step gave up waiting (results invalid)"""
        if int(self.mlp_barrier[1].item()) != 0:
            raise hb.DiaHipError("fused MLP kernel: a workgroup gave up waiting at the grid barrier; results are invalid")
        code = self.seg_error()
        if code:
            self.seg_ws[: int(hb.lib().dia_seg_workspace_control_bytes())].zero_()       # counters are inconsistent after a give-up
            raise hb.DiaHipError(f"persistent MLP segment: an in-kernel wait timed out (code {code}: 1 x1, 2 hidden, 3 wo partials, "
                                 f"4 x2) — were all 256 workgroups resident?  Results are invalid; set DIA_TUNE=seg=0 to run the launches")

    def results(self) -> List[UtteranceResult]:
        self.sync()
        self._raise_if_invalid()
        tok = self.tokens.cpu().numpy()
        prd = self.pred.cpu().numpy()
        fsm = self.fsm.cpu().numpy()
        cur = self.cur.cpu().numpy()
        out = []
        for b in range(self.B):
            last = int(fsm[b, 4]) if fsm[b, 3] else int(cur[b]) - 1
            out.append(UtteranceResult(tok[b], tok[b, self.first_steps[b]: last + 1].copy(), last, prd[b], self.lens[b]))   # model.py:831
        return out

    # ------------------------------------------------------------------ continuous batching (slots)
    @classmethod
    def open(cls, w: DeviceWeights, slots: int, *, s_cap: Optional[int] = None, kv_dtype: str = "bf16",
             max_tokens: Optional[int] = None, ignore_eos: bool = False, stream: Optional[torch.cuda.Stream] = None,
             cfg_scale: float = 3.0, temperature: float = 1.3, top_p: float = 0.95, top_k: int = 35,
             attention: str = "auto", stream_cap: Optional[int] = None, adapters=None, cross_kv: str = "bf16",
             self_kv: str = "bf16", prompt_prefill: str = "auto") -> "DecodeSession":
        """A session of `slots` PARKED slots for a stream of requests: admit() puts a request into a free slot between two decode
        steps, the step graph (captured once) serves whatever the slots hold, retire() parks a finished one; serve() is the
        driver loop.  Cross caches are sized for texts of `s_cap` bytes (default: the encoder's text_length), the noise buffer for
        `max_tokens` steps per slot (default: audio_length) — a request's own max_tokens may be smaller, not larger.  The sampling
        arguments are what a parked slot holds until its first admission; every request brings its own.
        stream_cap=N adds the buffers of frame streaming (stream_iter): a staging area of N frames per slot on the device, two
        pinned host copies of it, a side stream for the copies.  None: no such buffer exists and nothing new is launched.
        adapters: a lora.AdapterBank; each Request then names its adapter (Request.adapter), and the admission writes the slot's
        entry of adapter_of_slot — the step graph is captured once, with the corrections' launches in it.
        prompt_prefill="batched": an admitted request's audio prompt (more than one frame) is prefilled as one packed batch behind
        dia_slot_admit and the slot starts at step first_step; "auto" / "replay": it replays through first_step - 1 decode steps."""
        if int(slots) < 1:
            raise ValueError("slots must be >= 1")
        if stream_cap is not None and int(stream_cap) < 1:
            raise ValueError("stream_cap must be >= 1")
        if float(temperature) == 0.0:
            temperature = 1.0                      # (the noise buffer is always allocated; requests bring their own temperature)
        cap = w.cfg.data.text_length if s_cap is None else int(s_cap)
        if not (1 <= cap <= w.cfg.data.text_length):
            raise ValueError(f"s_cap must be in [1, {w.cfg.data.text_length}]")
        empty = np.zeros((0,), dtype=np.int32)
        s = cls(w, [empty] * int(slots), kv_dtype=kv_dtype, max_tokens=max_tokens, cfg_scale=cfg_scale, temperature=temperature,
                top_p=top_p, top_k=top_k, ignore_eos=ignore_eos, stream=stream, s_cap=_ceil(cap, 32), attention=attention,
                adapters=adapters, cross_kv=cross_kv, self_kv=self_kv, prompt_prefill=prompt_prefill, _slotted=True)
        s.text_cap = cap                           # (the caches hold whole 32-key blocks; requests are held to what was asked for)
        if stream_cap is not None:
            s._init_stream(int(stream_cap))
        return s

    def _init_slots(self):
        """Per-slot sampling state on the device (dia_sample_args.slot_*), every slot parked, host-side slot table."""
        B, dev, sp = self.B, self.dev, self.sample_params
        self.text_cap = self.S
        self.slot_f32 = [torch.full((B,), float(sp[k]), dtype=torch.float32).to(dev) for k in ("cfg_scale", "temperature", "top_p")]
        self.slot_i32 = [torch.full((B,), int(v), dtype=torch.int32).to(dev) for v in (sp["top_k"], self.max_tokens)]
        fsm = np.zeros((B, 8), dtype=np.int32)
        fsm[:, 1], fsm[:, 2], fsm[:, 3] = -1, self.max_delay, 1             # done: a parked slot samples nothing
        self.fsm = torch.from_numpy(fsm).to(dev)
        self._gens = None                        # (one generator per ADMISSION, below)
        self._live: Dict[int, dict] = {}         # slot -> request, first_step, max_tokens, generator, noise rows resident, _issued at admission
        self._parked = set(range(B))

    def free_slots(self) -> List[int]:
        return [b for b in range(self.B) if b not in self._live]

    def _as_request(self, r) -> Request:
        if not isinstance(r, Request):
            r = Request(np.asarray(r, dtype=np.int32))
        mt = self.max_tokens if r.max_tokens is None else int(r.max_tokens)
        ids = np.asarray(r.text_ids, dtype=np.int32).reshape(-1)
        if len(ids) > self.text_cap:
            raise ValueError(f"request text of {len(ids)} bytes exceeds the session's s_cap = {self.text_cap}")
        if not (2 <= mt <= self.T):
            raise ValueError(f"max_tokens must be in [2, {self.T}]")
        if mt > self.max_tokens:
            raise ValueError(f"max_tokens {mt} exceeds the session's {self.max_tokens} (the noise buffer's steps per slot)")
        pr = r.audio_prompt
        if pr is not None:
            pr = np.asarray(pr)
            if pr.ndim == 3 and pr.shape[0] == 1:
                pr = pr[0]
            if pr.ndim != 2 or pr.shape[1] != self.C:
                raise ValueError(f"Unexpected audio_prompt shape: {pr.shape}. Expected [T, C] or [1, T, C].")   # model.py:316
            if 1 + pr.shape[0] + self.max_delay > self.T:
                raise ValueError(f"audio prompt of {pr.shape[0]} frames does not fit audio_length {self.T}")
        ad = None
        if r.adapter is not None:
            if self.adapters is None:
                raise ValueError("the request names an adapter but the session was opened without adapters=")
            ad = self.adapters.index_of(r.adapter)
            ad = None if ad < 0 else ad
        return Request(ids, r.seed, mt, float(r.cfg_scale), float(r.temperature), float(r.top_p), int(r.top_k or 0), pr, ad)

    def admit(self, requests: Sequence) -> List[int]:
        """Put each request (a Request, or bare text ids with the defaults) into a free slot; returns the slot ids.  Enqueues, on the
        session's stream and without synchronising: the packed encoder pass + cross-K/V of the new texts into their slots' caches,
        dia_slot_admit (token rows, state machine, sampling values), with prompt_prefill="batched" the packed prefill of the admitted
        requests' audio prompts (cur[b] = first_step[b]), and the first input embedding of the admitted slots only.
        The caches of a re-used slot are not cleared (DESIGN.md "Continuous batching")."""
        if not self.slotted:
            raise hb.DiaHipError("admit() needs a session made by DecodeSession.open()")
        reqs = [self._as_request(r) for r in requests]           # every ValueError before anything is enqueued
        free = self.free_slots()
        if len(reqs) > len(free):
            raise hb.DiaHipError(f"admit(): {len(reqs)} requests for {len(free)} free slots")
        pairs = list(zip(free, reqs))
        for i in range(0, len(pairs), hb.SLOTS_PER_CALL):
            self._admit(pairs[i: i + hb.SLOTS_PER_CALL])
        return [b for b, _ in pairs]

    def _admit(self, pairs):
        from .tokens import delayed_prefill
        if not pairs:
            return
        for b, _ in pairs:
            if b in self._live:
                raise hb.DiaHipError(f"slot {b} is admitted twice before it was collected")
        pre = [delayed_prefill(self.cfg, r.audio_prompt) for _, r in pairs]         # (rows [P, C], first sampled step)
        self._enqueue_admit(pairs, pre)
        for (b, r), (_, pstep) in zip(pairs, pre):
            g = None
            if r.temperature != 0.0:             # row 0 of the slot's noise is this request's first draw
                g = torch.Generator()
                g.seed() if r.seed is None else g.manual_seed(int(r.seed))
            # t0: the session's step count at which this slot stood at step 1.  A prefilled slot starts at step first_step, as if
            # first_step - 1 steps had been issued for it already (_steps_left, _ensure_slot_noise: row r stays draw number r)
            skipped = int(pstep) - 1 if self.prompt_prefill == "batched" and int(pstep) > 2 else 0
            self._live[b] = dict(req=r, first_step=int(pstep), gen=g, rows=0, t0=self._issued - skipped, skip=skipped)
            self._parked.discard(b)
            self.lens[b], self.first_steps[b] = len(r.text_ids), int(pstep)

    def _enqueue_admit(self, pairs, pre):
        """the device side of an admission, in stream order: encoder + cross-K/V, dia_slot_admit, first embedding of these slots"""
        L, n = hb.lib(), len(pairs)
        st = C.c_void_p(self.stream.cuda_stream)
        if self.adapters is not None:            # the slots' adapters first: the encoder pass below already reads them
            for b, r in pairs:
                self._adapter_host[b] = -1 if r.adapter is None else int(r.adapter)
            self._push_adapter_slots()
        self._encode([(b, r.text_ids) for b, r in pairs])
        ld = max(p.shape[0] for p, _ in pre)
        n_pre = n * ld * self.C
        host = np.full((_ceil(n_pre, 4) + n,), -1, dtype=np.int32)                  # prefix rows, then the slot list
        for i, (p_, _) in enumerate(pre):
            host[i * ld * self.C: i * ld * self.C + p_.size] = np.asarray(p_, dtype=np.int32).reshape(-1)
        host[_ceil(n_pre, 4):] = [b for b, _ in pairs]
        pin = torch.from_numpy(host).pin_memory()
        self._pinned.append(pin)
        i32 = lambda v: (C.c_int32 * n)(*[int(x) for x in v])
        f32 = lambda v: (C.c_float * n)(*[float(x) for x in v])
        with torch.cuda.stream(self.stream):
            dev_tab = pin.to(self.dev, non_blocking=True)
            a = self._slot_args(n, [b for b, _ in pairs])
            a.text_len, a.first_step = i32(len(r.text_ids) for _, r in pairs), i32(ps for _, ps in pre)
            a.prefix_rows, a.max_tokens = i32(p_.shape[0] for p_, _ in pre), i32(r.max_tokens for _, r in pairs)
            a.cfg_scale, a.temperature, a.top_p = (f32(getattr(r, k) for _, r in pairs) for k in ("cfg_scale", "temperature", "top_p"))
            a.top_k = i32(r.top_k for _, r in pairs)
            a.prefix, a.prefix_ld = dev_tab.data_ptr(), ld
            hb.check(L.dia_slot_admit(C.byref(a), st), "dia_slot_admit")
            if self.prompt_prefill == "batched":     # behind the token rows, ahead of the embedding: cur[b] = first_step[b] of the prefilled slots
                self._prompt_prefill(st, [(b, ps) for (b, _), (_, ps) in zip(pairs, pre)])
            ea = self._embed_args()
            ea.slots, ea.n_slots = dev_tab.data_ptr() + 4 * _ceil(n_pre, 4), n
            hb.check(L.dia_embed_tokens(C.byref(ea), st), "dia_embed_tokens")

    def _slot_args(self, n: int, slots: Sequence[int]) -> hb.SlotAdmitArgs:
        a = hb.SlotAdmitArgs()
        a.B, a.T, a.C, a.S, a.max_delay, a.n = self.B, self.T, self.C, self.S, self.max_delay, n
        a.slot = (C.c_int32 * n)(*[int(b) for b in slots])
        a.tokens, a.pred, a.cur, a.fsm = hb.ptr(self.tokens), hb.ptr(self.pred), hb.ptr(self.cur), hb.ptr(self.fsm)
        a.d_first_step, a.d_text_len = hb.ptr(self.first_step), hb.ptr(self.text_len)
        a.slot_cfg_scale, a.slot_temperature, a.slot_top_p = (hb.ptr(t) for t in self.slot_f32)
        a.slot_top_k, a.slot_max_tokens = (hb.ptr(t) for t in self.slot_i32)
        return a

    def retire(self, slots: Sequence[int]):
        """Park slots (stream order): done, one self-attention key, no cross-attention keys per step until the next admission."""
        slots = [int(b) for b in slots]
        for b in slots:
            if b in self._live:
                raise hb.DiaHipError(f"slot {b} is live: collect() it before retiring it")
        for i in range(0, len(slots), hb.SLOTS_PER_CALL):
            self._enqueue_retire(slots[i: i + hb.SLOTS_PER_CALL])
        for b in slots:
            self._parked.add(b)
            self.lens[b] = 0

    def _enqueue_retire(self, part):
        a = self._slot_args(len(part), part)
        hb.check(hb.lib().dia_slot_retire(C.byref(a), C.c_void_p(self.stream.cuda_stream)), "dia_slot_retire")
        if self.adapters is not None:            # a parked slot runs the base model
            self._adapter_host[list(part)] = -1
            self._push_adapter_slots()

    def _steps_left(self, b: int) -> int:
        """decode steps a live slot can still run: it starts at step 1 and its last step is max_tokens - 1"""
        sl = self._live[b]
        return sl["req"].max_tokens - 1 - (self._issued - sl["t0"])

    def _ensure_slot_noise(self, n_steps: int):
        """Every live slot's Exp(1) rows for its next `n_steps` steps: the slot's own generator, restarted at admission, continues
        where it stopped (row r of a slot = its request's draw number r, read at step first_step + r)."""
        todo = []
        for b, sl in self._live.items():
            if sl["gen"] is None or sl.get("ended"):         # (ended: stream_iter has seen the slot's finished flag)
                continue
            done = self._issued - sl["t0"]
            need = min(done + int(n_steps), sl["req"].max_tokens - 1) - sl.get("skip", 0)      # (prefilled steps drew nothing)
            if need > sl["rows"]:
                todo.append((b, sl, sl["rows"], need))
        if not todo:
            return

        def draw(job):
            _, sl, r0, r1 = job
            t = torch.empty(r1 - r0, self.C, self.V, dtype=torch.float32, pin_memory=self._streaming)
            t.exponential_(1.0, generator=sl["gen"])
            return t

        if len(todo) > 1:
            from concurrent.futures import ThreadPoolExecutor
            with ThreadPoolExecutor(max_workers=min(len(todo), 8)) as pool:       # torch releases the GIL while it draws
                parts = list(pool.map(draw, todo))
        else:
            parts = [draw(todo[0])]
        for (b, sl, r0, r1), t in zip(todo, parts):
            self._upload_noise(b, r0, t)
            sl["rows"] = r1

    def _upload_noise(self, b: int, r0: int, rows: torch.Tensor):
        with torch.cuda.stream(self.stream):
            if self._streaming:                  # drawn into pinned memory: the copy is queued, the host does not wait for the stream
                self._pinned.append(rows)
                self.noise[b, r0: r0 + rows.shape[0]].copy_(rows, non_blocking=True)
                return
            self.noise[b, r0: r0 + rows.shape[0]].copy_(rows, non_blocking=False)

    def _read_state(self):
        """(fsm [B, 8], cur [B]) on the host, after a sync"""
        self.sync()
        self._raise_if_invalid()
        return self.fsm.cpu().numpy(), self.cur.cpu().numpy()

    def _read_slot(self, b: int):
        """(token rows, raw samples) of slot b on the host"""
        return self.tokens[b].cpu().numpy(), self.pred[b].cpu().numpy()

    def finished(self) -> List[int]:
        """live slots whose utterance has ended (synchronises the stream)"""
        fsm, _ = self._read_state()
        return [b for b in sorted(self._live) if fsm[b, 3]]

    def collect(self, b: int) -> UtteranceResult:
        """Result of a finished (or abandoned) live slot — the fields and slicing of results() — and the slot becomes free."""
        sl = self._live[b]
        fsm, cur = self._read_state()
        tok, prd = self._read_slot(b)
        last = int(fsm[b, 4]) if fsm[b, 3] else int(cur[b]) - 1
        del self._live[b]
        return UtteranceResult(tok, tok[sl["first_step"]: last + 1].copy(), last, prd, len(sl["req"].text_ids))   # model.py:831

    def release(self, b: int):
        """A live slot becomes free WITHOUT its result being read (frame streaming took the frames out already; cancel() drops
        them): nothing is downloaded and nothing enqueued.  The driver loop retires or refills the slot at its next iteration."""
        del self._live[b]

    def serve_iter(self, requests: Sequence, poll: int = 64, use_graph: bool = True):
        """The driver loop: fill free slots from the queue, decode up to `poll` steps, collect what finished, retire what stays
        empty — until the queue is empty and every slot is parked.  Yields (request index, UtteranceResult) as utterances end."""
        if not self.slotted:
            raise hb.DiaHipError("serve() needs a session made by DecodeSession.open()")
        reqs = [self._as_request(r) for r in requests]           # every ValueError before anything is enqueued
        nxt, owner = 0, {}
        while nxt < len(reqs) or self._live:
            free = self.free_slots()
            take = min(len(free), len(reqs) - nxt)
            if take:
                pairs = list(zip(free[:take], reqs[nxt: nxt + take]))
                for i in range(0, take, hb.SLOTS_PER_CALL):
                    self._admit(pairs[i: i + hb.SLOTS_PER_CALL])
                for i, (b, _) in enumerate(pairs):
                    owner[b] = nxt + i
                nxt += take
            idle = [b for b in self.free_slots() if b not in self._parked]
            if idle:
                self.retire(idle)
            n = max(1, min(int(poll), max(self._steps_left(b) for b in self._live)))
            self.decode(n, use_graph)
            self.ensure_noise(self._issued + int(poll))          # the next chunk's noise is drawn while this one runs
            for b in self.finished():
                yield owner.pop(b), self.collect(b)
        idle = [b for b in range(self.B) if b not in self._parked]
        if idle:
            self.retire(idle)

    def serve(self, requests: Sequence, poll: int = 64, use_graph: bool = True) -> List[UtteranceResult]:
        """serve_iter() to the end; results in request order."""
        reqs = list(requests)
        out: List[Optional[UtteranceResult]] = [None] * len(reqs)
        for i, r in self.serve_iter(reqs, poll, use_graph):
            out[i] = r
        return out

    # ------------------------------------------------------------------ frame streaming (DESIGN.md "Frame streaming")
    stream_cap: Optional[int] = None             # frames per slot and dia_emit_frames call; None = a session without streaming buffers
    _streaming = False                           # inside stream_iter: noise top-ups are drawn into pinned memory and copied asynchronously

    def _init_stream(self, cap: int):
        """Device staging of dia_emit_frames + what brings it to the host: two pinned copies, a side stream, events."""
        B, dev = self.B, self.dev
        self.stream_cap = cap
        self.emitted = torch.zeros(B, dtype=torch.int32).to(dev)
        self.emit_out = torch.zeros(B, cap, self.C, dtype=torch.int32).to(dev)
        self.emit_state = torch.tensor([[0, 0, -1, 0]] * B, dtype=torch.int32).to(dev)
        self._emit_host = [(torch.zeros(B, cap, self.C, dtype=torch.int32).pin_memory(), torch.zeros(B, 4, dtype=torch.int32).pin_memory())
                           for _ in range(2)]
        self._emit_side = torch.cuda.Stream(device=dev)
        self._emit_ev = torch.cuda.Event()                           # session stream: the emit launch of an iteration is behind us
        self._copy_ev = [torch.cuda.Event(), torch.cuda.Event()]     # side stream: pinned pair i holds that iteration's staging
        self._copy_busy = None                                       # the copy event the next launch that writes the staging waits for
        self._owner: Dict[int, int] = {}                             # slot -> request index of the running stream_iter
        self._queue: List[int] = []                                  # request indices not admitted yet

    def _enqueue_emit(self, slots: Sequence[int], reset: bool = False):
        """dia_emit_frames for these slots on the session's stream (reset: DIA_EMIT_RESET, behind their admission).  The launch
        writes the staging area, so the stream first waits (on the device) for the copy that still reads it."""
        if self._copy_busy is not None:
            self.stream.wait_event(self._copy_busy)
            self._copy_busy = None
        a = hb.EmitArgs()
        a.B, a.T, a.C, a.max_delay, a.codebook_size, a.cap = self.B, self.T, self.C, self.max_delay, CODEBOOK_SIZE, self.stream_cap
        a.flags = hb.EMIT_RESET if reset else 0
        a.tokens, a.cur, a.fsm, a.first_step, a.delay = (hb.ptr(t) for t in (self.tokens, self.cur, self.fsm, self.first_step, self.delay))
        a.emitted, a.out, a.state = hb.ptr(self.emitted), hb.ptr(self.emit_out), hb.ptr(self.emit_state)
        slots = [int(b) for b in slots]
        for i in range(0, len(slots), hb.SLOTS_PER_CALL):
            part = slots[i: i + hb.SLOTS_PER_CALL]
            a.n, a.slot = len(part), (C.c_int32 * len(part))(*part)
            hb.check(hb.lib().dia_emit_frames(C.byref(a), C.c_void_p(self.stream.cuda_stream)), "dia_emit_frames")

    def _enqueue_fetch(self, k: int):
        """staging + records -> pinned pair k % 2, on the side stream behind everything the session's stream holds so far: two
        asynchronous copies of fixed size, then the copy event"""
        out_h, state_h = self._emit_host[k % 2]
        self._emit_ev.record(self.stream)
        self._emit_side.wait_event(self._emit_ev)
        with torch.cuda.stream(self._emit_side):
            out_h.copy_(self.emit_out, non_blocking=True)
            state_h.copy_(self.emit_state, non_blocking=True)
        self._copy_ev[k % 2].record(self._emit_side)
        self._copy_busy = self._copy_ev[k % 2]

    def _wait_fetch(self, k: int):
        """(out [B, cap, C], state [B, 4]) of iteration k on the host: waits for that iteration's copy event, nothing else"""
        self._copy_ev[k % 2].synchronize()
        out_h, state_h = self._emit_host[k % 2]
        return out_h.numpy(), state_h.numpy()

    def cancel(self, request_index: int):
        """Drop a request of the running stream_iter (between two next() calls): no further chunk of it is yielded.  A request
        still queued is never admitted; a running one gives up its slot with release(), and the loop's next iteration retires or
        refills that slot.  Other slots are not touched."""
        ri = int(request_index)
        if ri in self._queue:
            self._queue.remove(ri)
        for b, r in list(self._owner.items()):
            if r == ri:
                del self._owner[b]
                self.release(b)

    def stream_iter(self, requests: Sequence, chunk: int = 16, lag: int = 1, use_graph: bool = True):
        """serve_iter that hands frames out while the utterances run: yields (request index, start frame, codes [1, C, n], final)
        — codes is what codes_for_codec would hold at [:, :, start: start + n] once the utterance has ended.  Every utterance ends
        with exactly one final chunk (empty when its last frames went out earlier or it has no frame at all).

        Iteration k: fill free slots from the queue (DIA_EMIT_RESET behind their admission), retire idle ones, decode up to `chunk`
        steps, dia_emit_frames for the live slots, copy staging and records to pinned pair k % 2 on the side stream.  The host
        then waits for the copy event of iteration k - lag only, never for the session's stream: with lag = 1 the next chunk is
        queued before this one is read.  lag = 0 reads every iteration at once.  A slot is freed (release(): nothing is
        downloaded) when its record says start + n == total; a backlog larger than stream_cap is drained by further calls."""
        if not self.slotted or self.stream_cap is None:
            raise hb.DiaHipError("stream_iter() needs a session made by DecodeSession.open(..., stream_cap=N)")
        if int(lag) not in (0, 1) or int(chunk) < 1:
            raise ValueError("lag must be 0 or 1 (two pinned copies), chunk >= 1")
        if self._live:
            raise hb.DiaHipError("stream_iter() starts on a session without live slots")
        reqs = [self._as_request(r) for r in requests]           # every ValueError before anything is enqueued
        chunk, lag = int(chunk), int(lag)
        owner, queue = self._owner, self._queue
        owner.clear()
        queue[:] = range(len(reqs))
        pending = []            # (k, [(slot, request index)] of its emit call, pinned sources of the copies queued before it)
        k = 0
        self._streaming = True
        try:
            while queue or self._live or pending:
                if queue or self._live:
                    free = self.free_slots()
                    take = min(len(free), len(queue))
                    if take:
                        pairs = [(b, reqs[ri]) for b, ri in zip(free, queue[:take])]
                        for i in range(0, take, hb.SLOTS_PER_CALL):
                            self._admit(pairs[i: i + hb.SLOTS_PER_CALL])
                        self._enqueue_emit(free[:take], reset=True)
                        owner.update(zip(free[:take], queue[:take]))
                        del queue[:take]
                    idle = [b for b in self.free_slots() if b not in self._parked]
                    if idle:
                        self.retire(idle)
                if self._live:
                    n = min(chunk, max([self._steps_left(b) for b, sl in self._live.items() if not sl.get("ended")] + [0]))
                    if n > 0:
                        self.decode(n, use_graph)
                    live = sorted(self._live)
                    self._enqueue_emit(live)
                    self._enqueue_fetch(k)
                    pins, self._pinned = self._pinned, []
                    pending.append((k, [(b, owner[b]) for b in live], pins))
                    k += 1
                    if n > 0:
                        self.ensure_noise(self._issued + chunk)  # the next chunk's noise is drawn while this one runs
                while pending and (len(pending) > lag or not self._live):
                    kk, who, _ = pending.pop(0)
                    out, state = self._wait_fetch(kk)
                    for b, ri in who:
                        if owner.get(b) != ri:                   # released or cancelled since that call was queued
                            continue
                        start, m, total, fin = (int(v) for v in state[b])
                        final = bool(fin) and start + m == total
                        if fin:
                            self._live[b]["ended"] = True        # (no further decode steps on its account)
                        if not (m or final):
                            continue
                        # an own copy: the pinned pair is overwritten two iterations on (a [1, C] window transposed is
                        # contiguous as it stands, so ascontiguousarray would hand out a view of it)
                        codes = np.array(out[b, :m].T, order="C", copy=True)[None]
                        if final:
                            del owner[b]
                            self.release(b)
                        yield ri, start, codes, final
            idle = [b for b in range(self.B) if b not in self._parked and b not in self._live]
            if idle:
                self.retire(idle)
            self.sync()
            self._raise_if_invalid()
        finally:
            self._streaming = False
            for _, _, pins in pending:                           # (an abandoned generator: copies may still be queued)
                self._pinned.extend(pins)

    # ------------------------------------------------------------------ accounting
    @property
    def self_cache_bytes(self) -> int:
        """Bytes of the self K/V caches of all layers and rows as allocated: bf16 / fp32 K and V, or (self_kv="fp8") the e4m3 bytes
        and their scales — (1 + 1/32) / 2 of the bf16 caches at the same R and T."""
        if self.f8_self is not None:
            return self.f8_self.nbytes
        return sum(t.numel() * t.element_size() for t in self.k_self + self.v_self)

    def step_bytes(self, n_keys: Optional[int] = None) -> int:
        """Algorithmic HBM bytes of one decode step at self-KV length `n_keys` (default: current)."""
        d = self.cfg.model.decoder
        kvb = 2 if self.kv_code == hb.KV_BF16 else 4       # fp32, or two bf16 planes
        if n_keys is None:
            n_keys = int(self.cur.max().item())
        kv_self = 2 * d.n_layer * 2 * d.kv_heads * HEAD_DIM * kvb * n_keys      # both rows, K and V
        if self.self_kv == "fp8":                                                # one byte per value, one 4-byte scale per key and head
            kv_self = 2 * d.n_layer * 2 * d.kv_heads * (HEAD_DIM + 4) * n_keys
        kv_cross = d.n_layer * 2 * d.cross_query_heads * HEAD_DIM * kvb          # cond row, per text byte
        return self.w.decode_weight_bytes(self.R) + self.B * kv_self + kv_cross * sum(self.lens)
