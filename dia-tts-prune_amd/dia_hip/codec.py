"""The Descript Audio Codec (44 kHz) on the HIP device (csrc/codec.hip): codes [B, 9, T] -> waveform (DESIGN.md "Codec") and
waveform -> codes (DESIGN.md "Codec: encode side").  The reference goes through the third-party ``dac`` package
(dia/audio.py:166-185: ``quantizer.from_codes`` then ``decode``; model.py:546-575: ``preprocess`` then ``encode``); this module
restates those networks from the state dict and needs no package.

Host side only: configuration, checkpoint loading, weight-norm folding (float64), the HBM weight layouts, windowing and the
streaming state.  All arithmetic on activations happens in the library (dia_codec_embed / dia_codec_conv / dia_codec_convt, and
dia_codec_convs / dia_codec_quantize on the encode side).
"""

from __future__ import annotations

import ctypes as C
import re
from contextlib import contextmanager
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import binding as hb


@dataclass(frozen=True)
class CodecConfig:
    """descript-audio-codec 1.0.0, 44 kHz (d_out = 1)"""
    n_codebooks: int = 9
    codebook_size: int = 1024
    codebook_dim: int = 8
    latent_dim: int = 1024
    decoder_dim: int = 1536
    decoder_rates: Tuple[int, ...] = (8, 8, 4, 2)
    sample_rate: int = 44100
    # the encode side.  A decode-side checkpoint says nothing about these two, so they take no part in equality: the configuration
    # load_codec_state() reads from a decoder's shapes equals the one the checkpoint was made with
    encoder_dim: int = field(default=64, compare=False)
    encoder_rates: Tuple[int, ...] = field(default=(2, 4, 8, 8), compare=False)

    @property
    def hop(self) -> int:
        return int(np.prod(self.decoder_rates))


def mini_config() -> CodecConfig:
    """the real layer sequence and rates at an eighth of the width (tests)"""
    return CodecConfig(latent_dim=64, decoder_dim=192, encoder_dim=8)


# ---------------------------------------------------------------------------------------------- the layer list
def layer_plan(cfg: CodecConfig) -> List[dict]:
    """the decoder as a flat list of convolutions, each with the state-dict prefix of its weights and of the Snake in front of it"""
    plan = [dict(kind="conv", key="decoder.model.0", snake=None, cin=cfg.latent_dim, cout=cfg.decoder_dim, k=7, d=1)]
    c = cfg.decoder_dim
    for i, s in enumerate(cfg.decoder_rates):
        blk = f"decoder.model.{i + 1}.block"
        plan.append(dict(kind="convt", key=f"{blk}.1", snake=f"{blk}.0", cin=c, cout=c // 2, s=int(s)))
        c //= 2
        for u, d in enumerate((1, 3, 9)):
            ru = f"{blk}.{2 + u}.block"
            plan.append(dict(kind="conv", key=f"{ru}.1", snake=f"{ru}.0", cin=c, cout=c, k=7, d=d))
            plan.append(dict(kind="conv", key=f"{ru}.3", snake=f"{ru}.2", cin=c, cout=c, k=1, d=1, res=True))
    n = len(cfg.decoder_rates)
    plan.append(dict(kind="conv", key=f"decoder.model.{n + 2}", snake=f"decoder.model.{n + 1}", cin=c, cout=1, k=7, d=1, tanh=True))
    return plan


def expected_keys(cfg: CodecConfig) -> Dict[str, Tuple[int, ...]]:
    """every decode-side key of the checkpoint with its shape"""
    out: Dict[str, Tuple[int, ...]] = {}
    for i in range(cfg.n_codebooks):
        q = f"quantizer.quantizers.{i}"
        out[f"{q}.codebook.weight"] = (cfg.codebook_size, cfg.codebook_dim)
        out[f"{q}.out_proj.weight_g"] = (cfg.latent_dim, 1, 1)
        out[f"{q}.out_proj.weight_v"] = (cfg.latent_dim, cfg.codebook_dim, 1)
        out[f"{q}.out_proj.bias"] = (cfg.latent_dim,)
    for L in layer_plan(cfg):
        if L["snake"]:
            out[L["snake"] + ".alpha"] = (1, L["cin"], 1)
        if L["kind"] == "conv":
            out[L["key"] + ".weight_g"] = (L["cout"], 1, 1)
            out[L["key"] + ".weight_v"] = (L["cout"], L["cin"], L["k"])
        else:                                                   # transposed: dimension 0 is the INPUT channel
            out[L["key"] + ".weight_g"] = (L["cin"], 1, 1)
            out[L["key"] + ".weight_v"] = (L["cin"], L["cout"], 2 * L["s"])
        out[L["key"] + ".bias"] = (L["cout"],)
    return out


def encoder_plan(cfg: CodecConfig) -> List[dict]:
    """the encoder as a flat list of convolutions, as layer_plan: "conv" is dia_codec_conv (k 7 / 1), "convs" the strided form
    (k = 2 s, padding s / 2) and "conv3" the final k-3 layer, both dia_codec_convs"""
    c = cfg.encoder_dim
    plan = [dict(kind="conv", key="encoder.block.0", snake=None, cin=1, cout=c, k=7, d=1)]
    for i, s in enumerate(cfg.encoder_rates):
        blk = f"encoder.block.{i + 1}.block"
        for u, d in enumerate((1, 3, 9)):
            ru = f"{blk}.{u}.block"
            plan.append(dict(kind="conv", key=f"{ru}.1", snake=f"{ru}.0", cin=c, cout=c, k=7, d=d))
            plan.append(dict(kind="conv", key=f"{ru}.3", snake=f"{ru}.2", cin=c, cout=c, k=1, d=1, res=True))
        plan.append(dict(kind="convs", key=f"{blk}.4", snake=f"{blk}.3", cin=c, cout=2 * c, s=int(s)))
        c *= 2
    n = len(cfg.encoder_rates)
    plan.append(dict(kind="conv3", key=f"encoder.block.{n + 2}", snake=f"encoder.block.{n + 1}", cin=c, cout=cfg.latent_dim, k=3, d=1))
    return plan


def expected_encoder_keys(cfg: CodecConfig) -> Dict[str, Tuple[int, ...]]:
    """every encode-side key of the checkpoint with its shape: the encoder and the quantizers' in_proj"""
    out: Dict[str, Tuple[int, ...]] = {}
    for L in encoder_plan(cfg):
        if L["snake"]:
            out[L["snake"] + ".alpha"] = (1, L["cin"], 1)
        out[L["key"] + ".weight_g"] = (L["cout"], 1, 1)
        out[L["key"] + ".weight_v"] = (L["cout"], L["cin"], 2 * L["s"] if L["kind"] == "convs" else L["k"])
        out[L["key"] + ".bias"] = (L["cout"],)
    for i in range(cfg.n_codebooks):
        q = f"quantizer.quantizers.{i}.in_proj"
        out[f"{q}.weight_g"] = (cfg.codebook_dim, 1, 1)
        out[f"{q}.weight_v"] = (cfg.codebook_dim, cfg.latent_dim, 1)
        out[f"{q}.bias"] = (cfg.codebook_dim,)
    return out


_ENCODE_SIDE = re.compile(r"^(encoder\.|quantizer\.quantizers\.\d+\.in_proj\.)")


def _check_state(want: Dict[str, Tuple[int, ...]], have: Dict[str, torch.Tensor], label: str) -> Dict[str, torch.Tensor]:
    """the tensors of `have` in the order of `want`; a missing or unexpected key, or a wrong shape, is refused by name"""
    missing = [k for k in want if k not in have]
    unexpected = [k for k in have if k not in want]
    if missing:
        raise KeyError(f"{label}: missing keys {missing[:8]}{' ...' if len(missing) > 8 else ''}")
    if unexpected:
        raise KeyError(f"{label}: unexpected keys {unexpected[:8]}{' ...' if len(unexpected) > 8 else ''}")
    for k, shp in want.items():
        if tuple(have[k].shape) != shp:
            raise ValueError(f"{label}: {k} has shape {tuple(have[k].shape)}, expected {shp}")
    return {k: have[k] for k in want}


def check_codec_state(cfg: CodecConfig, sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """the decode-side tensors of `sd`; a missing or unexpected decoder / quantizer key, or a wrong shape, is refused by name.
    Encoder keys and the quantizers' in_proj (the encode side of the same modules) are ignored."""
    return _check_state(expected_keys(cfg), {k: v for k, v in sd.items() if not _ENCODE_SIDE.match(k)}, "codec checkpoint")


def check_codec_encoder_state(cfg: CodecConfig, sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """the encode-side tensors of `sd` (encoder.*, quantizers' in_proj); a missing or unexpected one, or a wrong shape, is refused
    by name.  check_codec_state() is the decode side's and ignores exactly these keys."""
    return _check_state(expected_encoder_keys(cfg), {k: v for k, v in sd.items() if _ENCODE_SIDE.match(k)}, "codec checkpoint (encode side)")


def infer_encoder_config(cfg: CodecConfig, sd: Dict[str, torch.Tensor], kwargs: Optional[dict] = None) -> CodecConfig:
    """`cfg` with encoder_dim / encoder_rates read from the encoder's shapes (metadata fields win where present); shapes that do
    not say are left to check_codec_encoder_state to refuse"""
    kwargs = kwargs or {}
    dim, rates = cfg.encoder_dim, []
    w0 = sd.get("encoder.block.0.weight_v")
    if w0 is not None and w0.dim() == 3:
        dim = int(w0.shape[0])
    while True:
        w = sd.get(f"encoder.block.{len(rates) + 1}.block.4.weight_v")
        if w is None or w.dim() != 3:
            break
        rates.append(int(w.shape[2]) // 2)
    if kwargs.get("encoder_dim") is not None:
        dim = int(kwargs["encoder_dim"])
    if kwargs.get("encoder_rates") is not None:
        rates = [int(r) for r in kwargs["encoder_rates"]]
    return CodecConfig(**{**cfg.__dict__, "encoder_dim": dim, "encoder_rates": tuple(rates) if rates else cfg.encoder_rates})


def infer_config(sd: Dict[str, torch.Tensor], sample_rate: int = 44100) -> CodecConfig:
    """the configuration from tensor shapes alone"""
    def need(k):
        if k not in sd:
            raise KeyError(f"codec checkpoint: missing key {k}")
        return sd[k]
    n_cb = 0
    while f"quantizer.quantizers.{n_cb}.codebook.weight" in sd:
        n_cb += 1
    cb = need("quantizer.quantizers.0.codebook.weight")
    latent = need("quantizer.quantizers.0.out_proj.weight_v").shape[0]
    ddim = need("decoder.model.0.weight_v").shape[0]
    rates = []
    while f"decoder.model.{len(rates) + 1}.block.1.weight_v" in sd:
        rates.append(sd[f"decoder.model.{len(rates) + 1}.block.1.weight_v"].shape[2] // 2)
    return CodecConfig(n_codebooks=n_cb, codebook_size=int(cb.shape[0]), codebook_dim=int(cb.shape[1]), latent_dim=int(latent),
                       decoder_dim=int(ddim), decoder_rates=tuple(int(r) for r in rates), sample_rate=int(sample_rate))


def _open_codec_state(path_or_obj) -> Tuple[CodecConfig, Dict[str, torch.Tensor], dict]:
    """what load_codec_state() accepts -> (configuration of the decode side, the WHOLE state dict unchecked, metadata kwargs)"""
    obj = path_or_obj
    if isinstance(obj, (str, bytes)) or hasattr(obj, "__fspath__"):
        obj = torch.load(obj, map_location="cpu", weights_only=True)
    if isinstance(obj, tuple) and len(obj) == 2 and isinstance(obj[0], CodecConfig):
        return obj[0], obj[1], {"encoder_dim": obj[0].encoder_dim, "encoder_rates": obj[0].encoder_rates}
    if not isinstance(obj, dict):
        raise TypeError(f"codec checkpoint: expected a dict, got {type(obj).__name__}")
    kwargs = {}
    if "state_dict" in obj and isinstance(obj["state_dict"], dict):
        kwargs = dict((obj.get("metadata") or {}).get("kwargs") or {})
        obj = obj["state_dict"]
    cfg = infer_config(obj, int(kwargs.get("sample_rate") or 44100))
    over = {}
    for name in ("n_codebooks", "codebook_size", "codebook_dim", "latent_dim", "decoder_dim"):
        if kwargs.get(name) is not None:
            over[name] = int(kwargs[name])
    if kwargs.get("decoder_rates") is not None:
        over["decoder_rates"] = tuple(int(r) for r in kwargs["decoder_rates"])
    if over:
        cfg = CodecConfig(**{**cfg.__dict__, **over})
    return cfg, obj, kwargs


def load_codec_state(path_or_obj) -> Tuple[CodecConfig, Dict[str, torch.Tensor]]:
    """a DAC ``.pth`` ({"state_dict": ..., "metadata": {"kwargs": {...}}}), a bare state dict, or either as an object already in
    memory -> (configuration, checked decode-side state dict).  Metadata fields win over shapes where they are present."""
    cfg, sd, _ = _open_codec_state(path_or_obj)
    return cfg, check_codec_state(cfg, sd)


def synthetic_state_dict(cfg: CodecConfig, seed: int = 0) -> Dict[str, torch.Tensor]:
    """random decode-side weights in checkpoint form (weight_g / weight_v apart).  The gains keep every layer's output near unit
    scale (fan-in scaling, small residual branches, a final layer that lands in tanh's bend), so that the waveform neither
    vanishes nor saturates: its RMS lies in [0.05, 0.9], which the tests assert."""
    g = torch.Generator().manual_seed(int(seed))

    def rnd(*shape):
        return torch.randn(*shape, generator=g, dtype=torch.float32)

    sd: Dict[str, torch.Tensor] = {}
    for i in range(cfg.n_codebooks):
        q = f"quantizer.quantizers.{i}"
        sd[f"{q}.codebook.weight"] = rnd(cfg.codebook_size, cfg.codebook_dim)
        v = rnd(cfg.latent_dim, cfg.codebook_dim, 1)
        sd[f"{q}.out_proj.weight_v"] = v
        sd[f"{q}.out_proj.weight_g"] = torch.full((cfg.latent_dim, 1, 1), 1.0 / float(np.sqrt(cfg.n_codebooks))) * (1.0 + 0.1 * rnd(cfg.latent_dim, 1, 1))
        sd[f"{q}.out_proj.bias"] = 0.05 * rnd(cfg.latent_dim)
    for L in layer_plan(cfg):
        if L["snake"]:
            sd[L["snake"] + ".alpha"] = 0.5 + torch.rand(1, L["cin"], 1, generator=g, dtype=torch.float32)
        if L["kind"] == "conv":
            v = rnd(L["cout"], L["cin"], L["k"])
            gain = 0.3 if L.get("res") else (0.2 if L.get("tanh") else 1.0)
            # |row of v| ~ sqrt(cin k): weight_g = gain makes the output of unit-scale inputs ~ gain
            sd[L["key"] + ".weight_g"] = gain * (1.0 + 0.1 * rnd(L["cout"], 1, 1))
        else:
            v = rnd(L["cin"], L["cout"], 2 * L["s"])
            # norm over (cout, 2 s) per INPUT channel; an output sums cin x 2 taps
            sd[L["key"] + ".weight_g"] = float(np.sqrt(L["cout"] * 2 * L["s"] / (2.0 * L["cin"]))) * (1.0 + 0.1 * rnd(L["cin"], 1, 1))
        sd[L["key"] + ".weight_v"] = v
        sd[L["key"] + ".bias"] = 0.05 * rnd(L["cout"])
    return sd


def synthetic_encoder_state(cfg: CodecConfig, seed: int = 0) -> Dict[str, torch.Tensor]:
    """random encode-side weights in checkpoint form, from a generator of their own (synthetic_state_dict's draws are untouched).
    Gains as there: fan-in scaling (weight_g = gain makes the output of unit-scale inputs ~ gain), small residual branches; the
    first layer lifts a waveform of RMS ~ 0.2 to unit scale.  The latent's RMS lies in [0.05, 5] on the test inputs."""
    g = torch.Generator().manual_seed(int(seed) + 0x5eed)

    def rnd(*shape):
        return torch.randn(*shape, generator=g, dtype=torch.float32)

    sd: Dict[str, torch.Tensor] = {}
    for L in encoder_plan(cfg):
        if L["snake"]:
            sd[L["snake"] + ".alpha"] = 0.5 + torch.rand(1, L["cin"], 1, generator=g, dtype=torch.float32)
        k = 2 * L["s"] if L["kind"] == "convs" else L["k"]
        gain = 0.3 if L.get("res") else (4.0 if L["cin"] == 1 else 1.0)
        sd[L["key"] + ".weight_g"] = gain * (1.0 + 0.1 * rnd(L["cout"], 1, 1))
        sd[L["key"] + ".weight_v"] = rnd(L["cout"], L["cin"], k)
        sd[L["key"] + ".bias"] = 0.05 * rnd(L["cout"])
    for i in range(cfg.n_codebooks):
        q = f"quantizer.quantizers.{i}.in_proj"
        sd[f"{q}.weight_g"] = 1.0 + 0.1 * rnd(cfg.codebook_dim, 1, 1)
        sd[f"{q}.weight_v"] = rnd(cfg.codebook_dim, cfg.latent_dim, 1)
        sd[f"{q}.bias"] = 0.05 * rnd(cfg.codebook_dim)
    return sd


# ---------------------------------------------------------------------------------------------- folding and layouts
def fold_weight_norm(g: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """w = g v / |v| in float64, the norm over every dimension but 0 (torch.nn.utils.weight_norm, dim = 0).  For a transposed
    convolution dimension 0 is the input channel."""
    v64 = v.detach().to(torch.float64)
    norm = v64.reshape(v64.shape[0], -1).norm(dim=1).reshape(-1, *([1] * (v64.dim() - 1)))
    return g.detach().to(torch.float64) * v64 / norm


def _pad32(n: int) -> int:
    return (n + 31) // 32 * 32


def conv_layout(w: torch.Tensor) -> torch.Tensor:
    """[C_out, C_in, k] -> tap-major fp32 [k][C_in][Cp], Cp = C_out rounded up to 32, zero-filled"""
    co, ci, k = w.shape
    out = torch.zeros(k, ci, _pad32(co), dtype=torch.float32)
    out[:, :, :co] = w.permute(2, 1, 0).to(torch.float32)
    return out.contiguous()


def convt_layout(w: torch.Tensor) -> torch.Tensor:
    """[C_in, C_out, 2 s] -> phase-major fp32 [s][2][C_in][Cp]: phase r, tap 0 = w[:, :, r] (times x[m]), tap 1 = w[:, :, r + s]
    (times x[m - 1])"""
    ci, co, k2 = w.shape
    s = k2 // 2
    out = torch.zeros(s, 2, ci, _pad32(co), dtype=torch.float32)
    out[:, 0, :, :co] = w[:, :, :s].permute(2, 0, 1).to(torch.float32)
    out[:, 1, :, :co] = w[:, :, s:].permute(2, 0, 1).to(torch.float32)
    return out.contiguous()


PRECISIONS = {"fp32": 0, "bf16": 1, "bf16x2": 2}                # DeviceCodec(precision=...) -> bf16 planes of the decoder's MFMA operands


def precision_planes(precision) -> int:
    """0 for "fp32" (the exact kernel), 1 for "bf16", 2 for "bf16x2"; anything else is refused by name"""
    if not isinstance(precision, str) or precision not in PRECISIONS:
        raise ValueError(f"codec precision {precision!r} is not one of 'fp32', 'bf16x2', 'bf16'")
    return PRECISIONS[precision]


def bf16_planes(w: torch.Tensor, planes: int) -> torch.Tensor:
    """fp32 -> [planes, ...] bf16: hi = bf16(w) (round to nearest even) and, for planes = 2, lo = bf16(w - hi), the residual exact
    in fp32: the split k_codec_conv_bf applies to its staged inputs"""
    if planes not in (1, 2):
        raise ValueError(f"planes = {planes} is not 1 or 2")
    w = w.to(torch.float32)
    hi = w.to(torch.bfloat16)
    return torch.stack([hi, (w - hi.to(torch.float32)).to(torch.bfloat16)][:planes])


def _group8(p: torch.Tensor) -> torch.Tensor:
    """[..., C_in, Cp] -> [..., Ci / 8, Cp, 8] with C_in zero-filled to Ci, the next multiple of 16 (the kernel's channel chunk)"""
    ci, cp = p.shape[-2:]
    cpad = (ci + 15) // 16 * 16
    out = torch.zeros(*p.shape[:-2], cpad, cp, dtype=p.dtype)
    out[..., :ci, :] = p
    return out.reshape(*p.shape[:-2], cpad // 8, 8, cp).transpose(-1, -2).contiguous()


def conv_layout_bf16(w: torch.Tensor, planes: int) -> torch.Tensor:
    """[C_out, C_in, k] -> bf16 [planes][k][Ci / 8][Cp][8]: the planes of conv_layout(w) with 8 input channels contiguous per
    (tap, output channel); Ci = C_in rounded up to 16, Cp = C_out rounded up to 32, zero-filled"""
    return _group8(bf16_planes(conv_layout(w), planes))


def convt_layout_bf16(w: torch.Tensor, planes: int) -> torch.Tensor:
    """[C_in, C_out, 2 s] -> bf16 [planes][s][2][Ci / 8][Cp][8]: the planes of convt_layout(w), grouped as conv_layout_bf16"""
    return _group8(bf16_planes(convt_layout(w), planes))


def convs_layout(w: torch.Tensor) -> torch.Tensor:
    """strided convolution [C_out, C_in, 2 s] -> fp32 [2][C_in * s][Cp]: out[t][ci * s + r][co] = w[co][ci][r + t s], the weight of
    x[ci][(o + t) s + r - s / 2] in output o"""
    co, ci, k2 = w.shape
    s = k2 // 2
    out = torch.zeros(2, ci * s, _pad32(co), dtype=torch.float32)
    out[:, :, :co] = w.reshape(co, ci, 2, s).permute(2, 1, 3, 0).reshape(2, ci * s, co).to(torch.float32)
    return out.contiguous()


def quantizer_tables(cfg: CodecConfig, sd: Dict[str, torch.Tensor], enc: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """the search's operands, prepared in float64 and stored fp32: in_proj folded [n][dim][latent] with its bias [n][dim], the
    codebook rows L2-normalised (eps 1e-12) [n][size][dim], the squared norm of each stored row [n][size], and the out_proj bias
    per codebook [n][latent] (the tables themselves are embed_tables')"""
    in_w, in_b, cb, cb2, ob = [], [], [], [], []
    for i in range(cfg.n_codebooks):
        q = f"quantizer.quantizers.{i}"
        in_w.append(fold_weight_norm(enc[f"{q}.in_proj.weight_g"], enc[f"{q}.in_proj.weight_v"])[:, :, 0].to(torch.float32))
        in_b.append(enc[f"{q}.in_proj.bias"].to(torch.float32))
        c = sd[f"{q}.codebook.weight"].to(torch.float64)
        c = (c / c.norm(dim=1, keepdim=True).clamp_min(1e-12)).to(torch.float32)
        cb.append(c)
        cb2.append(c.to(torch.float64).pow(2).sum(dim=1).to(torch.float32))
        ob.append(sd[f"{q}.out_proj.bias"].to(torch.float32))
    return dict(in_w=torch.stack(in_w).contiguous(), in_b=torch.stack(in_b).contiguous(), cb=torch.stack(cb).contiguous(),
                cb2=torch.stack(cb2).contiguous(), bias=torch.stack(ob).contiguous())


def embed_tables(cfg: CodecConfig, sd: Dict[str, torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
    """codebook_i x out_proj_i folded in float64: tables fp32 [n_codebooks][codebook_size][latent_dim] and the summed bias"""
    tabs, bias = [], torch.zeros(cfg.latent_dim, dtype=torch.float64)
    for i in range(cfg.n_codebooks):
        q = f"quantizer.quantizers.{i}"
        w = fold_weight_norm(sd[f"{q}.out_proj.weight_g"], sd[f"{q}.out_proj.weight_v"])[:, :, 0]       # [latent, dim]
        tabs.append(sd[f"{q}.codebook.weight"].to(torch.float64) @ w.T)
        bias += sd[f"{q}.out_proj.bias"].to(torch.float64)
    return torch.stack(tabs).to(torch.float32).contiguous(), bias.to(torch.float32)


# ---------------------------------------------------------------------------------------------- windowing
def context_frames(cfg: CodecConfig) -> int:
    """frames of context a window needs on each side so that its interior equals the whole decode: the dependency cone of one
    output frame walked back through the layers.  A k-7 convolution of dilation d widens an interval [a, b] of positions to
    [a - 3 d, b + 3 d]; a transposed convolution of stride s (kernel 2 s, padding s / 2) reads inputs m - 1 and m with
    m = floor((o + s / 2) / s), so [a, b] becomes [floor((a + s / 2) / s) - 1, floor((b + s / 2) / s)]."""
    a, b = 0, cfg.hop - 1                                       # the samples of frame 0
    for L in reversed(layer_plan(cfg)):
        if L["kind"] == "conv":
            r = (L["k"] // 2) * L["d"]
            a, b = a - r, b + r
        else:
            s = L["s"]
            a, b = (a + s // 2) // s - 1, (b + s // 2) // s
    return max(-a, b)


def encode_context_frames(cfg: CodecConfig) -> int:
    """frames of real samples an encode window needs on each side so that its interior latents equal the whole encode: the
    interval of samples latent frame 0 depends on, walked back through encoder_plan.  k 3 widens [a, b] to [a - 1, b + 1], k 7 of
    dilation d to [a - 3 d, b + 3 d]; a strided convolution (kernel 2 s, padding s / 2) reads [o s - s / 2, o s + 3 s / 2 - 1] for
    output o, so [a, b] becomes [a s - s / 2, b s + 3 s / 2 - 1].  The quantiser is per frame and adds nothing."""
    a, b = 0, 0
    for L in reversed(encoder_plan(cfg)):
        if L["kind"] == "convs":
            s = L["s"]
            a, b = a * s - s // 2, b * s + (3 * s) // 2 - 1
        else:
            r = (L["k"] // 2) * L["d"]
            a, b = a - r, b + r
    hop = int(np.prod(cfg.encoder_rates))
    return max(-(a // hop), b // hop)                           # ceil(-a / hop) frames before, the frame of sample b behind


def encode_windowed(latent_fn: Callable[[np.ndarray], np.ndarray], wave: np.ndarray, window: int, ctx: int, hop: int) -> np.ndarray:
    """samples [L] (L a multiple of hop) through latent_fn (samples of one utterance -> its latents [latent, frames]) window by
    window: every window is encoded with ctx frames of samples on each side as an utterance of its own, the interiors are joined"""
    parts = []
    for lo, f0, f1, hi in window_plan(wave.shape[-1] // hop, window, ctx):
        z = latent_fn(wave[lo * hop:hi * hop])
        parts.append(z[:, f0 - lo:f1 - lo])
    return np.concatenate(parts, axis=1)


def preprocess(wave: np.ndarray, hop: int) -> np.ndarray:
    """DAC's preprocess: zeros on the right up to a multiple of hop"""
    w = np.asarray(wave, dtype=np.float32).reshape(-1)
    pad = -w.shape[0] % hop
    return np.concatenate([w, np.zeros(pad, dtype=np.float32)]) if pad else w


def window_plan(T: int, window: int, ctx: int) -> List[Tuple[int, int, int, int]]:
    """(lo, f0, f1, hi) per window: decode frames [lo, hi) as an utterance of their own, keep those of [f0, f1)"""
    if window < 1:
        raise ValueError("window must be at least 1 frame")
    return [(max(0, f0 - ctx), f0, min(T, f0 + window), min(T, min(T, f0 + window) + ctx)) for f0 in range(0, T, window)]


def decode_windowed(decode_fn: Callable[[np.ndarray], np.ndarray], codes: np.ndarray, window: int, ctx: int, hop: int) -> np.ndarray:
    """codes [n_codebooks, T] through decode_fn (codes of one utterance -> its samples) window by window"""
    parts = []
    for lo, f0, f1, hi in window_plan(codes.shape[-1], window, ctx):
        y = decode_fn(codes[:, lo:hi])
        parts.append(y[(f0 - lo) * hop:(f1 - lo) * hop])
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.float32)


class CodecStream:
    """Streaming decoder state of one utterance: push() takes the code chunks Dia.stream_frames yields and returns the samples
    that have become final.  The last `ctx` frames of a running utterance are held back until more frames arrive or `final` is
    seen; everything goes through the same windows as decode_windowed, so the chunks joined equal the whole decode."""

    def __init__(self, decode_fn: Callable[[np.ndarray], np.ndarray], n_codebooks: int, hop: int, window: int, ctx: int):
        if window < 1:
            raise ValueError("window must be at least 1 frame")
        self.decode_fn, self.hop, self.window, self.ctx = decode_fn, int(hop), int(window), int(ctx)
        self.buf = np.zeros((n_codebooks, 0), dtype=np.int64)   # frames [base, total)
        self.base = 0
        self.total = 0
        self.emitted = 0
        self.final = False

    def push(self, codes: np.ndarray, final: bool = False) -> np.ndarray:
        """codes [n_codebooks, n] or [1, n_codebooks, n] (n may be 0) -> float samples of frames [emitted, emitted'), possibly none"""
        if self.final:
            raise RuntimeError("CodecStream: push() after the final chunk")
        c = np.asarray(codes)
        if c.ndim == 3:
            c = c[0]
        if c.ndim != 2 or c.shape[0] != self.buf.shape[0]:
            raise ValueError(f"CodecStream: codes of shape {np.asarray(codes).shape}, expected [{self.buf.shape[0]}, n]")
        self.buf = np.concatenate([self.buf, c.astype(np.int64)], axis=1)
        self.total += c.shape[1]
        self.final = bool(final)
        ready = self.total if final else max(self.emitted, self.total - self.ctx)
        parts = []
        while self.emitted < ready:
            f0, f1 = self.emitted, min(ready, self.emitted + self.window)
            lo, hi = max(0, f0 - self.ctx), min(self.total, f1 + self.ctx)
            y = self.decode_fn(self.buf[:, lo - self.base:hi - self.base])
            parts.append(y[(f0 - lo) * self.hop:(f1 - lo) * self.hop])
            self.emitted = f1
        keep = max(0, self.emitted - self.ctx)                  # earlier frames are never read again
        if keep > self.base:
            self.buf = self.buf[:, keep - self.base:]
            self.base = keep
        return np.concatenate(parts) if parts else np.zeros(0, dtype=np.float32)


# ---------------------------------------------------------------------------------------------- the ctypes side
class CodecEmbedArgs(C.Structure):
    _fields_ = [
        ("codes", C.c_void_p), ("lens", C.c_void_p), ("B", C.c_int32), ("T", C.c_int32),
        ("n_codebooks", C.c_int32), ("codebook_size", C.c_int32), ("latent_dim", C.c_int32), ("ld_codes", C.c_int32),
        ("tables", C.c_void_p), ("bias", C.c_void_p), ("z", C.c_void_p), ("ldz", C.c_int32), ("_pad0", C.c_int32),
    ]


class CodecConvArgs(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p), ("alpha", C.c_void_p), ("inv", C.c_void_p),
        ("res", C.c_void_p), ("y", C.c_void_p), ("lens", C.c_void_p), ("B", C.c_int32), ("T", C.c_int32),
        ("C_in", C.c_int32), ("C_out", C.c_int32), ("ldx", C.c_int32), ("ldy", C.c_int32),
        ("k", C.c_int32), ("dilation", C.c_int32), ("stride", C.c_int32), ("tanh_out", C.c_int32),
    ]


class CodecQuantizeArgs(C.Structure):
    _fields_ = [
        ("z", C.c_void_p), ("lens", C.c_void_p), ("B", C.c_int32), ("T", C.c_int32),
        ("n_codebooks", C.c_int32), ("codebook_size", C.c_int32), ("codebook_dim", C.c_int32), ("latent_dim", C.c_int32),
        ("ldz", C.c_int32), ("ld_codes", C.c_int32),
        ("in_w", C.c_void_p), ("in_b", C.c_void_p), ("codebook", C.c_void_p), ("codebook_sq", C.c_void_p), ("tables", C.c_void_p),
        ("bias", C.c_void_p), ("codes", C.c_void_p),
    ]


def _fns():
    L = hb.lib()
    L.dia_codec_embed.argtypes = [C.POINTER(CodecEmbedArgs), C.c_void_p]
    L.dia_codec_conv.argtypes = [C.POINTER(CodecConvArgs), C.c_void_p]
    L.dia_codec_convt.argtypes = [C.POINTER(CodecConvArgs), C.c_void_p]
    L.dia_codec_convs.argtypes = [C.POINTER(CodecConvArgs), C.c_void_p]
    L.dia_codec_quantize.argtypes = [C.POINTER(CodecQuantizeArgs), C.c_void_p]
    L.dia_codec_conv_bf16.argtypes = [C.POINTER(CodecConvArgs), C.c_int, C.c_void_p]
    L.dia_codec_convt_bf16.argtypes = [C.POINTER(CodecConvArgs), C.c_int, C.c_void_p]
    return L


def _launch_conv(lib, entry: str, planes: int, a: CodecConvArgs, st) -> None:
    """entry "conv" / "convt" / "convs" with planes 0 (fp32) / 1 / 2 -> dia_codec_<entry> or dia_codec_<entry>_bf16(planes)"""
    name = f"dia_codec_{entry}_bf16" if planes else f"dia_codec_{entry}"
    fn = getattr(lib, name)
    hb.check(fn(C.byref(a), planes, st) if planes else fn(C.byref(a), st), name)


def snake_inverse(alpha: torch.Tensor) -> torch.Tensor:
    """1 / (alpha + 1e-9) per channel, in float64, as fp32"""
    return (1.0 / (alpha.detach().to(torch.float64).reshape(-1) + 1e-9)).to(torch.float32)


def codec_embed(codes: torch.Tensor, tables: torch.Tensor, bias: torch.Tensor, lens: Optional[torch.Tensor] = None,
                T: Optional[int] = None) -> torch.Tensor:
    """dia_codec_embed on device tensors: codes int32 [B, n, ld] -> z fp32 [B, latent, ld] (positions beyond a row's length stay 0)"""
    B, n, ld = codes.shape
    z = torch.zeros(B, tables.shape[2], ld, dtype=torch.float32, device=codes.device)
    a = CodecEmbedArgs(codes=hb.ptr(codes), lens=hb.ptr(lens), B=B, T=ld if T is None else T, n_codebooks=n,
                       codebook_size=tables.shape[1], latent_dim=tables.shape[2], ld_codes=ld, tables=hb.ptr(tables),
                       bias=hb.ptr(bias), z=hb.ptr(z), ldz=ld)
    hb.check(_fns().dia_codec_embed(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "dia_codec_embed")
    return z


def codec_conv(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, *, c_out: int, k: int = 7, dilation: int = 1, stride: int = 0,
               alpha: Optional[torch.Tensor] = None, inv: Optional[torch.Tensor] = None, res: Optional[torch.Tensor] = None,
               tanh: bool = False, lens: Optional[torch.Tensor] = None, precision: str = "fp32") -> torch.Tensor:
    """dia_codec_conv (stride 0) / dia_codec_convt (stride s) on device tensors: x fp32 [B, C_in, T], w in the library's layout ->
    y fp32 [B, c_out, T (* s)]; positions beyond a row's length stay 0.  precision "bf16" / "bf16x2": the _bf16 entry points, w
    from conv_layout_bf16 / convt_layout_bf16 with 1 / 2 planes"""
    planes = precision_planes(precision)
    B, cin, T = x.shape
    To = T * (stride or 1)
    y = torch.zeros(B, c_out, To, dtype=torch.float32, device=x.device)
    a = CodecConvArgs(x=hb.ptr(x), w=hb.ptr(w), bias=hb.ptr(bias), alpha=hb.ptr(alpha), inv=hb.ptr(inv), res=hb.ptr(res), y=hb.ptr(y),
                      lens=hb.ptr(lens), B=B, T=T, C_in=cin, C_out=c_out, ldx=T, ldy=To, k=0 if stride else k,
                      dilation=0 if stride else dilation, stride=stride, tanh_out=int(tanh))
    _launch_conv(_fns(), "convt" if stride else "conv", planes, a, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    return y


def codec_convs(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, *, c_out: int, stride: int = 0, alpha: Optional[torch.Tensor] = None,
                inv: Optional[torch.Tensor] = None, lens: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dia_codec_convs on device tensors: the strided form (stride s, k = 2 s; w from convs_layout) or the k-3 form (stride 0; w
    from conv_layout): x fp32 [B, C_in, T] -> y fp32 [B, c_out, T // s]; `lens` are input lengths; positions beyond stay 0"""
    B, cin, T = x.shape
    To = max(1, T // stride) if stride else T
    y = torch.zeros(B, c_out, To, dtype=torch.float32, device=x.device)
    a = CodecConvArgs(x=hb.ptr(x), w=hb.ptr(w), bias=hb.ptr(bias), alpha=hb.ptr(alpha), inv=hb.ptr(inv), y=hb.ptr(y), lens=hb.ptr(lens),
                      B=B, T=T, C_in=cin, C_out=c_out, ldx=T, ldy=To, k=0 if stride else 3, dilation=1, stride=stride)
    _launch_conv(_fns(), "convs", 0, a, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    return y


def codec_quantize(z: torch.Tensor, q: Dict[str, torch.Tensor], tables: torch.Tensor, lens: Optional[torch.Tensor] = None,
                   T: Optional[int] = None) -> torch.Tensor:
    """dia_codec_quantize on device tensors: z fp32 [B, latent, ld], q = quantizer_tables() on the device, tables = embed_tables()[0]
    -> codes int32 [B, n_codebooks, ld] (frames beyond a row's length stay 0)"""
    B, latent, ld = z.shape
    n, size, dim = q["cb"].shape
    codes = torch.zeros(B, n, ld, dtype=torch.int32, device=z.device)
    a = CodecQuantizeArgs(z=hb.ptr(z), lens=hb.ptr(lens), B=B, T=ld if T is None else T, n_codebooks=n, codebook_size=size,
                          codebook_dim=dim, latent_dim=latent, ldz=ld, ld_codes=ld, in_w=hb.ptr(q["in_w"]), in_b=hb.ptr(q["in_b"]),
                          codebook=hb.ptr(q["cb"]), codebook_sq=hb.ptr(q["cb2"]), tables=hb.ptr(tables), bias=hb.ptr(q["bias"]),
                          codes=hb.ptr(codes))
    hb.check(_fns().dia_codec_quantize(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "dia_codec_quantize")
    return codes


class DeviceCodec:
    """The codec resident on a HIP device: weight norm folded once on the host in float64, weights uploaded in the library's
    tap-major layouts, two ping-pong activation buffers sized by `window` (never by an utterance's length).  The decoder is always
    there; the encoder is prepared when the checkpoint has any ``encoder.`` key, and a checkpoint without one, or with a
    malformed one, still decodes: `encoder_error` keeps what encode() will raise.

    decode() cuts every utterance into windows of at most `window` frames with context_frames(cfg) frames of context on each side,
    runs the windows of all rows as rows of batched launches (each with its own length) and keeps the interiors.

    precision: "fp32" (default) decodes on the exact-fp32 kernel.  "bf16x2" and "bf16" run the DECODER's convolutions on the bf16
    MFMA with two planes / one plane per operand (DESIGN.md "Codec: bf16 modes"): only that mode's bf16 weight image is uploaded
    for the decoder, activations stay fp32.  The encode side (encoder, quantiser) and the embedding stay fp32 in every mode: the
    codes are an arg-min and must not move."""

    def __init__(self, state, device: Optional[torch.device] = None, cfg: Optional[CodecConfig] = None, window: int = 128,
                 workspace_bytes: int = 1 << 30, precision: str = "fp32"):
        self.planes = precision_planes(precision)
        self.precision = precision
        if cfg is not None:
            state = (cfg, state)
        self.cfg, whole, meta = _open_codec_state(state)
        sd = check_codec_state(self.cfg, whole)
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if self.device.type != "cuda":
            raise hb.DiaHipError(f"device {self.device} is not a HIP device; there is no CPU fallback")
        if int(window) < 1:
            raise ValueError("window must be at least 1 frame")
        _fns()
        cfg = self.cfg
        self.window = int(window)
        self.ctx = context_frames(cfg)
        self.wmax = self.window + 2 * self.ctx                  # frames per job
        dev = self.device
        tabs, bias = embed_tables(cfg, sd)
        self.tables, self.embed_bias = tabs.to(dev), bias.to(dev)
        self.layers: List[dict] = []
        rate, per_frame = 1, cfg.latent_dim
        for L in layer_plan(cfg):
            if self.planes:                                     # a reduced mode holds its own image and no fp32 one
                lay = conv_layout_bf16 if L["kind"] == "conv" else convt_layout_bf16
                D = self._upload_layer(L, sd, "w_bf16", lambda w: lay(w, self.planes))
            else:
                D = self._upload_layer(L, sd, "w", conv_layout if L["kind"] == "conv" else convt_layout)
            D["rate_in"] = rate
            if L["kind"] == "convt":
                rate *= L["s"]
            per_frame = max(per_frame, L["cin"] * D["rate_in"], L["cout"] * rate)
            self.layers.append(D)
        self.row_floats = per_frame * self.wmax                 # one job's activations at the widest stage
        self.rows_cap = int(max(1, min(4096, int(workspace_bytes) // (2 * 4 * self.row_floats))))
        self._bufs: Optional[Tuple[torch.Tensor, torch.Tensor]] = None
        self._rows = 0
        self.layer_events: Optional[list] = None                # scratch/codec_speed.py: set to [] to collect (label, start, stop) events per launch
        self.enc_layers: Optional[List[dict]] = None
        self.encoder_error: Optional[Exception] = None
        self._resampler = None                                  # resample.DeviceResampler, made on first use
        self._timescaler = None                                 # timescale.DeviceTimescale, made on first use
        self._loudness = None                                   # loudness.DeviceLoudness, made on first use
        self._spectral = None                                   # spectral.DeviceSpectral, made on first use
        if any(k.startswith("encoder.") for k in whole):
            try:
                self._prepare_encoder(sd, whole, meta, int(workspace_bytes))
            except (KeyError, ValueError) as e:
                self.enc_layers, self.encoder_error = None, e
        else:
            self.encoder_error = KeyError("codec checkpoint: no encode side (missing keys ['encoder.block.0.weight_g', ...]); encode() needs "
                                          "the encoder.* and quantizer.quantizers.N.in_proj.* tensors")

    def _upload_layer(self, L: dict, sd: Dict[str, torch.Tensor], wkey: str, layout: Callable[[torch.Tensor], torch.Tensor]) -> dict:
        """the plan entry L with its device tensors: the folded weight in `layout` under `wkey`, the bias, the Snake's alpha and inverse"""
        D = dict(L)
        D[wkey] = layout(fold_weight_norm(sd[L["key"] + ".weight_g"], sd[L["key"] + ".weight_v"])).to(self.device)
        D["b"] = sd[L["key"] + ".bias"].to(torch.float32).to(self.device)
        if L["snake"]:
            al = sd[L["snake"] + ".alpha"]
            D["alpha"] = al.reshape(-1).to(torch.float32).to(self.device)
            D["inv"] = snake_inverse(al).to(self.device)
        return D

    def _prepare_encoder(self, sd, whole, meta, workspace_bytes: int) -> None:
        self.cfg = cfg = infer_encoder_config(self.cfg, whole, meta)
        if int(np.prod(cfg.encoder_rates)) != cfg.hop:
            raise ValueError(f"codec checkpoint (encode side): encoder_rates {cfg.encoder_rates} do not multiply to the hop {cfg.hop}")
        enc = check_codec_encoder_state(cfg, whole)
        dev = self.device
        layers, div, per_frame = [], 1, cfg.hop
        for L in encoder_plan(cfg):
            D = self._upload_layer(L, enc, "w", convs_layout if L["kind"] == "convs" else conv_layout)
            D["div_in"] = div                                  # samples per position of this layer's input
            if L["kind"] == "convs":
                div *= L["s"]
            per_frame = max(per_frame, L["cin"] * cfg.hop // D["div_in"], L["cout"] * cfg.hop // div)
            layers.append(D)
        self.qtabs = {k: v.to(dev) for k, v in quantizer_tables(cfg, sd, enc).items()}
        self.enc_ctx = encode_context_frames(cfg)
        self.enc_wmax = self.window + 2 * self.enc_ctx
        self.enc_row_floats = per_frame * self.enc_wmax
        self.enc_rows_cap = int(max(1, min(4096, workspace_bytes // (2 * 4 * self.enc_row_floats))))
        self.enc_layers = layers

    @property
    def has_encoder(self) -> bool:
        return self.enc_layers is not None

    # -------------------------------------------------------------------------------------- device side
    def _workspace(self, rows: int) -> Tuple[torch.Tensor, torch.Tensor]:
        if self._bufs is None or rows > self._rows:
            self._bufs = None
            self._bufs = (torch.empty(rows * self.row_floats, dtype=torch.float32, device=self.device),
                          torch.empty(rows * self.row_floats, dtype=torch.float32, device=self.device))
            self._rows = rows
        return self._bufs

    @contextmanager
    def _timed(self, label: str):
        """while layer_events is a list: the launches of the block between a (label, start, stop) event pair appended to it"""
        if self.layer_events is None:
            yield
            return
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self.layer_events.append((label, e0, e1))
        e0.record()
        yield
        e1.record()

    def _window(self, window: Optional[int], why: str = " (the workspace is sized by the codec's window)") -> int:
        """a call's window (None: the codec's) as an int in [1, the codec's]"""
        window = self.window if window is None else int(window)
        if not 1 <= window <= self.window:
            raise ValueError(f"window = {window} outside [1, {self.window}]{why}")
        return window

    def _chain(self, lib, st, layers: List[dict], planes: int, cur: torch.Tensor, oth: torch.Tensor, lens: torch.Tensor, J: int,
               T0: int, W0: int, x0: Optional[torch.Tensor] = None) -> torch.Tensor:
        """`layers` (self.layers or self.enc_layers) as one chain of batched launches over J rows on the ping-pong (cur, oth) -> the
        buffer that holds the last layer's output.  The stream enters in cur, or in x0 for the first layer where given.  A layer
        whose input has "rate_in" r positions (decoder) or 1 / "div_in" d (encoder) per unit of lens runs at T = T0 r / d, leading
        dimension W0 r / d and lengths lens r / d.  A layer that makes a new stream (transposed, strided, k 3, first and last)
        reads cur, writes oth and the two swap; inside a residual unit the k-7 reads cur into oth and the 1x1 reads oth and adds
        onto cur, the unit's input."""
        stage_lens = {(1, 1): lens}
        for i, L in enumerate(layers):
            kind, s = L["kind"], L.get("s", 0)
            with self._timed(f"{kind} {L['cin']}->{L['cout']} k{L.get('k', 2 * s)} d{L.get('d', 1)}"):
                r, d = L.get("rate_in", 1), L.get("div_in", 1)
                if (r, d) not in stage_lens:
                    stage_lens[r, d] = lens * r if d == 1 else lens // d
                ld = W0 * r // d
                a = CodecConvArgs(w=hb.ptr(L["w_bf16" if planes else "w"]), bias=hb.ptr(L["b"]), alpha=hb.ptr(L.get("alpha")),
                                  inv=hb.ptr(L.get("inv")), lens=hb.ptr(stage_lens[r, d]), B=J, T=T0 * r // d, C_in=L["cin"],
                                  C_out=L["cout"], ldx=ld, ldy=ld, tanh_out=int(bool(L.get("tanh"))))
                if L.get("res"):
                    a.x, a.y, a.res, a.k, a.dilation = hb.ptr(oth), hb.ptr(cur), hb.ptr(cur), 1, 1
                else:
                    a.x, a.y = hb.ptr(x0 if i == 0 and x0 is not None else cur), hb.ptr(oth)
                    if kind == "convt":
                        a.ldy, a.stride = ld * s, s
                    elif kind == "convs":
                        a.ldy, a.stride, a.k, a.dilation = ld // s, s, 2 * s, 1
                    else:
                        a.k, a.dilation = L["k"], L["d"]
                    if kind != "conv" or not L["snake"] or L.get("tanh"):
                        cur, oth = oth, cur
                _launch_conv(lib, "convs" if kind == "conv3" else kind, planes, a, st)
        return cur

    def _run(self, jobs: Sequence[np.ndarray]) -> List[np.ndarray]:
        """every job (codes [n_codebooks, n], n <= wmax) decoded as an utterance of its own: rows of one chain of batched launches"""
        cfg, lib = self.cfg, _fns()
        out: List[np.ndarray] = []
        with torch.cuda.device(self.device):
            st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            for g0 in range(0, len(jobs), self.rows_cap):
                grp = jobs[g0:g0 + self.rows_cap]
                J, W = len(grp), self.wmax
                Tg = max(j.shape[1] for j in grp)
                host = np.zeros((J, cfg.n_codebooks, W), dtype=np.int32)
                for r, j in enumerate(grp):
                    host[r, :, :j.shape[1]] = j
                codes = torch.from_numpy(host).to(self.device)
                lens = torch.tensor([j.shape[1] for j in grp], dtype=torch.int32, device=self.device)
                cur, oth = self._workspace(J)
                ea = CodecEmbedArgs(codes=hb.ptr(codes), lens=hb.ptr(lens), B=J, T=Tg, n_codebooks=cfg.n_codebooks,
                                    codebook_size=cfg.codebook_size, latent_dim=cfg.latent_dim, ld_codes=W, tables=hb.ptr(self.tables),
                                    bias=hb.ptr(self.embed_bias), z=hb.ptr(cur), ldz=W)
                hb.check(lib.dia_codec_embed(C.byref(ea), st), "dia_codec_embed")
                cur = self._chain(lib, st, self.layers, self.planes, cur, oth, lens, J, Tg, W)
                wave = cur[:J * W * cfg.hop].view(J, W * cfg.hop).cpu().numpy()
                for r, j in enumerate(grp):
                    out.append(wave[r, :j.shape[1] * cfg.hop].copy())
        return out

    # -------------------------------------------------------------------------------------- public
    def _check_codes(self, codes) -> np.ndarray:
        c = np.asarray(codes.detach().cpu() if isinstance(codes, torch.Tensor) else codes)
        if c.ndim == 3 and c.shape[0] == 1:
            c = c[0]
        if c.ndim != 2 or c.shape[0] != self.cfg.n_codebooks:
            raise ValueError(f"codec: codes of shape {tuple(np.asarray(c).shape)}, expected [{self.cfg.n_codebooks}, T]")
        if c.size and (c.min() < 0 or c.max() >= self.cfg.codebook_size):
            raise ValueError(f"codec: code ids outside [0, {self.cfg.codebook_size})")
        return c.astype(np.int64)

    def decode_batch(self, rows: Sequence, window: Optional[int] = None) -> List[np.ndarray]:
        """one code tensor [n_codebooks, T_b] (or [1, n_codebooks, T_b]) per utterance -> float32 [T_b * hop] per utterance; every
        row comes out as when decoded alone"""
        window = self._window(window)
        rows = [self._check_codes(r) for r in rows]
        jobs, plan = [], []
        for b, c in enumerate(rows):
            for lo, f0, f1, hi in window_plan(c.shape[1], window, self.ctx):
                jobs.append(c[:, lo:hi])
                plan.append((b, (f0 - lo) * self.cfg.hop, (f1 - lo) * self.cfg.hop))
        parts: List[List[np.ndarray]] = [[] for _ in rows]
        for (b, s0, s1), y in zip(plan, self._run(jobs)):
            parts[b].append(y[s0:s1])
        return [np.concatenate(p) if p else np.zeros(0, dtype=np.float32) for p in parts]

    def decode(self, codes, lengths: Optional[Sequence[int]] = None, window: Optional[int] = None):
        """[1, 9, T] or [9, T] -> float32 [T * hop]; [B, 9, T] with per-row `lengths` -> a list of float32 [lengths[b] * hop]"""
        c = np.asarray(codes.detach().cpu() if isinstance(codes, torch.Tensor) else codes)
        if lengths is None and (c.ndim == 2 or (c.ndim == 3 and c.shape[0] == 1)):
            return self.decode_batch([c], window)[0]
        if c.ndim != 3:
            raise ValueError(f"codec: codes of shape {tuple(c.shape)}, expected [B, {self.cfg.n_codebooks}, T]")
        lengths = [c.shape[2]] * c.shape[0] if lengths is None else [int(n) for n in lengths]
        if len(lengths) != c.shape[0] or any(n < 0 or n > c.shape[2] for n in lengths):
            raise ValueError("codec: one length in [0, T] per row")
        return self.decode_batch([c[b, :, :n] for b, n in enumerate(lengths)], window)

    # -------------------------------------------------------------------------------------- encode
    def _run_encode(self, jobs: Sequence[Tuple[np.ndarray, int, int]]) -> List[Tuple[np.ndarray, np.ndarray]]:
        """every job (samples [n hop] with n <= enc_wmax, first kept frame, kept frames) encoded as an utterance of its own: rows of
        one chain of batched launches; the kept latents [latent, kept] alone go to the quantiser -> (codes [n_codebooks, kept], latents)"""
        cfg, lib = self.cfg, _fns()
        hop, out = cfg.hop, []
        with torch.cuda.device(self.device):
            st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            for g0 in range(0, len(jobs), self.enc_rows_cap):
                grp = jobs[g0:g0 + self.enc_rows_cap]
                J, W = len(grp), self.enc_wmax
                Tg = max(j[0].shape[0] for j in grp) // hop
                host = np.zeros((J, W * hop), dtype=np.float32)
                for r, (w, _, _) in enumerate(grp):
                    host[r, :w.shape[0]] = w
                x0 = torch.from_numpy(host).to(self.device)
                lens = torch.tensor([j[0].shape[0] for j in grp], dtype=torch.int32, device=self.device)
                cur, oth = self._workspace(-(-J * self.enc_row_floats // self.row_floats))
                cur = self._chain(lib, st, self.enc_layers, 0, cur, oth, lens, J, Tg * hop, W * hop, x0=x0)
                # the kept frames of every job, gathered to the front of a tensor of their own: the quantiser sees nothing else
                zall = cur[:J * cfg.latent_dim * W].view(J, cfg.latent_dim, W)
                Wq = max(j[2] for j in grp)
                first = torch.tensor([j[1] for j in grp], dtype=torch.int64, device=self.device)
                at = (first[:, None] + torch.arange(Wq, device=self.device)[None, :]).clamp_(max=W - 1)
                z = torch.gather(zall, 2, at[:, None, :].expand(J, cfg.latent_dim, Wq)).contiguous()
                qlens = torch.tensor([j[2] for j in grp], dtype=torch.int32, device=self.device)
                with self._timed(f"quantize {cfg.latent_dim} x {cfg.n_codebooks}"):
                    codes = codec_quantize(z, self.qtabs, self.tables, lens=qlens)
                codes_h, z_h = codes.cpu().numpy(), z.cpu().numpy()
                for r, (_, _, n) in enumerate(grp):
                    out.append((codes_h[r, :, :n].astype(np.int64), z_h[r, :, :n].copy()))
        return out

    def encode_batch(self, rows: Sequence, window: Optional[int] = None, return_latents: bool = False,
                     sample_rates: Optional[Sequence[Optional[int]]] = None):
        """one mono float waveform [L_b] per utterance -> int64 codes [n_codebooks, ceil(L_b / hop)] per utterance (with
        return_latents: also the list of fp32 latents [latent, T_b] the codes were searched from).  Every row is padded with zeros
        on the right to a multiple of hop (DAC's preprocess) and comes out as when encoded alone; long rows run in windows of
        `window` frames with encode_context_frames(cfg) frames of samples on each side.  sample_rates: per row its rate in Hz
        (None = the codec's); rows at another rate are resampled first, those of one rate in one launch (L_b then counts the
        resampled samples)."""
        if self.enc_layers is None:
            raise self.encoder_error
        window = self._window(window)
        if sample_rates is not None and len(sample_rates) != len(rows):
            raise ValueError("codec: one sample rate (or None) per row")
        hop, waves = self.cfg.hop, []
        for r in rows:
            w = np.asarray(r.detach().cpu() if isinstance(r, torch.Tensor) else r)
            if w.ndim == 2 and w.shape[0] == 1:
                w = w[0]
            if w.ndim != 1 or w.dtype.kind != "f":
                raise ValueError(f"codec: a waveform of shape {tuple(w.shape)} and dtype {w.dtype}, expected mono float samples [L]")
            waves.append(w)
        for rate in sorted({int(r) for r in sample_rates or () if r is not None and int(r) != self.cfg.sample_rate}):
            at = [b for b, r in enumerate(sample_rates) if r is not None and int(r) == rate]
            for b, y in zip(at, self.resample([waves[b] for b in at], rate, self.cfg.sample_rate)):
                waves[b] = y
        waves = [preprocess(w, hop) for w in waves]
        jobs, plan = [], []
        for b, w in enumerate(waves):
            for lo, f0, f1, hi in window_plan(w.shape[0] // hop, window, self.enc_ctx):
                jobs.append((w[lo * hop:hi * hop], f0 - lo, f1 - f0))
                plan.append(b)
        codes: List[List[np.ndarray]] = [[] for _ in waves]
        lat: List[List[np.ndarray]] = [[] for _ in waves]
        for b, (c, z) in zip(plan, self._run_encode(jobs)):
            codes[b].append(c)
            lat[b].append(z)
        n, m = self.cfg.n_codebooks, self.cfg.latent_dim
        cs = [np.concatenate(p, axis=1) if p else np.zeros((n, 0), dtype=np.int64) for p in codes]
        if not return_latents:
            return cs
        return cs, [np.concatenate(p, axis=1) if p else np.zeros((m, 0), dtype=np.float32) for p in lat]

    def encode(self, wave, lengths: Optional[Sequence[int]] = None, window: Optional[int] = None) -> np.ndarray:
        """mono float samples [L] or [B, L] (per-row `lengths` in samples, default L) -> int64 codes [B, n_codebooks, T],
        T = ceil(max length / hop); a shorter row's codes end at ceil(lengths[b] / hop) and are 0 behind"""
        w = np.asarray(wave.detach().cpu() if isinstance(wave, torch.Tensor) else wave)
        if w.ndim == 1:
            w = w[None]
        if w.ndim != 2:
            raise ValueError(f"codec: a waveform of shape {tuple(w.shape)}, expected [L] or [B, L]")
        lengths = [w.shape[1]] * w.shape[0] if lengths is None else [int(n) for n in lengths]
        if len(lengths) != w.shape[0] or any(n < 0 or n > w.shape[1] for n in lengths):
            raise ValueError("codec: one length in [0, L] per row")
        rows = self.encode_batch([w[b, :n] for b, n in enumerate(lengths)], window)
        out = np.zeros((len(rows), self.cfg.n_codebooks, max([r.shape[1] for r in rows] + [0])), dtype=np.int64)
        for b, r in enumerate(rows):
            out[b, :, :r.shape[1]] = r
        return out

    # -------------------------------------------------------------------------------------- sample rates
    def _resample(self):
        if self._resampler is None:
            from .resample import DeviceResampler
            self._resampler = DeviceResampler(self.device)
        return self._resampler

    def resample(self, waves, rate_in: int, rate_out: int):
        """mono float samples [L], or a list of them (one launch), at rate_in -> float32 [ceil(L rate_out / rate_in)] at rate_out
        (csrc/resample.hip, DESIGN.md "Resampler"); equal rates return the input"""
        return self._resample().resample(waves, rate_in, rate_out)

    def resample_stream(self, rate_in: int, rate_out: int):
        """a resample.ResampleStream for one signal: push(chunk, final) -> the samples that have become final; joined they equal
        resample() of the whole signal bit for bit"""
        return self._resample().stream(rate_in, rate_out)

    def _timescale(self):
        if self._timescaler is None:
            from .timescale import DeviceTimescale
            self._timescaler = DeviceTimescale(self.device)
        return self._timescaler

    def time_scale(self, waves, speed: float, mode: str = "interp", window: int = 1024, tolerance: int = 512):
        """mono float samples [N], or a list of them, stretched to float32 [int(N / speed)] each on this codec's device
        (csrc/timescale.hip, DESIGN.md "Speed factor"): "interp" is the reference application's speed factor, "wsola" keeps the
        pitch; speed 1 returns the input"""
        return self._timescale().time_scale(waves, speed, mode, window, tolerance)

    def time_scale_stream(self, speed: float, window: int = 1024, tolerance: int = 512, mode: str = "wsola"):
        """a timescale.TimescaleStream for one signal: push(chunk, final) -> the samples that have become final; joined they equal
        time_scale(mode="wsola") of the whole signal bit for bit.  mode "interp" cannot stream: ValueError"""
        return self._timescale().stream(speed, window, tolerance, mode)

    # -------------------------------------------------------------------------------------- loudness
    def _loud(self):
        if self._loudness is None:
            from .loudness import DeviceLoudness
            self._loudness = DeviceLoudness(self.device)
        return self._loudness

    def measure_loudness(self, waves, rate: Optional[int] = None):
        """mono float samples [N], or a list of them, at `rate` Hz (default: the codec's) -> per row {"loudness": LUFS (ITU-R
        BS.1770-4, integrated), "true_peak": dBTP, "sample_peak": dBFS, "steps": ...} (csrc/loudness.hip, DESIGN.md "Loudness")"""
        return self._loud().measure(waves, int(rate) if rate else self.cfg.sample_rate)

    def normalize_loudness(self, waves, rate: Optional[int] = None, target: float = -23.0, peak: float = -1.0, **kw):
        """-> (waves, reports): every row brought to `target` LUFS by one gain, lowered where the true peak would cross `peak` dBTP
        (a pure gain, not a limiter; keywords as loudness.DeviceLoudness.normalize)"""
        return self._loud().normalize(waves, int(rate) if rate else self.cfg.sample_rate, target, peak, **kw)

    # -------------------------------------------------------------------------------------- audio distance
    def audio_distance(self, a, b, rate: Optional[int] = None, **kw):
        """the multi-scale STFT and log-mel distances between waveform a and waveform b (or lists, pair by pair) at `rate` Hz
        (default: the codec's): ``{"stft": x, "mel": y, "per_resolution": {...}}`` per pair (csrc/spectral.hip, DESIGN.md "Audio
        distance"; keywords as spectral.DeviceSpectral.distance)"""
        if self._spectral is None:
            from .spectral import DeviceSpectral
            self._spectral = DeviceSpectral(self.device)
        return self._spectral.distance(a, b, int(rate) if rate else self.cfg.sample_rate, **kw)

    def roundtrip_distance(self, wave, **kw):
        """encode -> decode of mono float samples [L] at the codec's rate (the decoder in this codec's precision), cut to the L
        samples of the input, then audio_distance against the input"""
        w = np.ascontiguousarray(np.asarray(wave.detach().cpu() if isinstance(wave, torch.Tensor) else wave, dtype=np.float32).reshape(-1))
        if w.shape[0] < 1:
            raise ValueError("codec: an empty waveform has no round trip")
        y = self.decode(self.encode(w))                         # [1, n_codebooks, T] -> float32 [T * hop], T * hop >= L
        return self.audio_distance(w, y[:w.shape[0]], **kw)

    def stream(self, window: Optional[int] = None) -> CodecStream:
        """a streaming state for one utterance on this codec"""
        window = self._window(window, why="")
        return CodecStream(lambda c: self._run([self._check_codes(c)])[0], self.cfg.n_codebooks, self.cfg.hop, window, self.ctx)
