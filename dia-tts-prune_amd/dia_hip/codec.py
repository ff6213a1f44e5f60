"""Native decoder of the Descript Audio Codec (44 kHz): codes [B, 9, T] -> waveform on the HIP device (csrc/codec.hip,
DESIGN.md "Codec").  The reference goes through the third-party ``dac`` package (dia/audio.py:166-185:
``quantizer.from_codes`` then ``decode``); this module restates that network from its state dict and needs no package.

Host side only: configuration, checkpoint loading, weight-norm folding (float64), the HBM weight layouts, windowing and the
streaming state.  All arithmetic on activations happens in the library (dia_codec_embed / dia_codec_conv / dia_codec_convt).
"""

from __future__ import annotations

import ctypes as C
import re
from dataclasses import dataclass
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

    @property
    def hop(self) -> int:
        return int(np.prod(self.decoder_rates))


def mini_config() -> CodecConfig:
    """the real layer sequence and rates at an eighth of the width (tests)"""
    return CodecConfig(latent_dim=64, decoder_dim=192)


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


_ENCODE_SIDE = re.compile(r"^(encoder\.|quantizer\.quantizers\.\d+\.in_proj\.)")


def check_codec_state(cfg: CodecConfig, sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """the decode-side tensors of `sd`; a missing or unexpected decoder / quantizer key, or a wrong shape, is refused by name.
    Encoder keys and the quantizers' in_proj (the encode side of the same modules) are ignored."""
    want = expected_keys(cfg)
    have = {k: v for k, v in sd.items() if not _ENCODE_SIDE.match(k)}
    missing = [k for k in want if k not in have]
    unexpected = [k for k in have if k not in want]
    if missing:
        raise KeyError(f"codec checkpoint: missing keys {missing[:8]}{' ...' if len(missing) > 8 else ''}")
    if unexpected:
        raise KeyError(f"codec checkpoint: unexpected keys {unexpected[:8]}{' ...' if len(unexpected) > 8 else ''}")
    for k, shp in want.items():
        if tuple(have[k].shape) != shp:
            raise ValueError(f"codec checkpoint: {k} has shape {tuple(have[k].shape)}, expected {shp}")
    return {k: have[k] for k in want}


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


def load_codec_state(path_or_obj) -> Tuple[CodecConfig, Dict[str, torch.Tensor]]:
    """a DAC ``.pth`` ({"state_dict": ..., "metadata": {"kwargs": {...}}}), a bare state dict, or either as an object already in
    memory -> (configuration, checked decode-side state dict).  Metadata fields win over shapes where they are present."""
    obj = path_or_obj
    if isinstance(obj, (str, bytes)) or hasattr(obj, "__fspath__"):
        obj = torch.load(obj, map_location="cpu", weights_only=True)
    if isinstance(obj, tuple) and len(obj) == 2 and isinstance(obj[0], CodecConfig):
        return obj[0], check_codec_state(obj[0], obj[1])
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
    return cfg, check_codec_state(cfg, obj)


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


def _fns():
    L = hb.lib()
    L.dia_codec_embed.argtypes = [C.POINTER(CodecEmbedArgs), C.c_void_p]
    L.dia_codec_conv.argtypes = [C.POINTER(CodecConvArgs), C.c_void_p]
    L.dia_codec_convt.argtypes = [C.POINTER(CodecConvArgs), C.c_void_p]
    return L


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
               tanh: bool = False, lens: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dia_codec_conv (stride 0) / dia_codec_convt (stride s) on device tensors: x fp32 [B, C_in, T], w in the library's layout ->
    y fp32 [B, c_out, T (* s)]; positions beyond a row's length stay 0"""
    B, cin, T = x.shape
    To = T * (stride or 1)
    y = torch.zeros(B, c_out, To, dtype=torch.float32, device=x.device)
    a = CodecConvArgs(x=hb.ptr(x), w=hb.ptr(w), bias=hb.ptr(bias), alpha=hb.ptr(alpha), inv=hb.ptr(inv), res=hb.ptr(res), y=hb.ptr(y),
                      lens=hb.ptr(lens), B=B, T=T, C_in=cin, C_out=c_out, ldx=T, ldy=To, k=0 if stride else k,
                      dilation=0 if stride else dilation, stride=stride, tanh_out=int(tanh))
    L = _fns()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    hb.check((L.dia_codec_convt if stride else L.dia_codec_conv)(C.byref(a), st), "dia_codec_convt" if stride else "dia_codec_conv")
    return y


class DeviceCodec:
    """The decoder resident on a HIP device: weight norm folded once on the host in float64, weights uploaded in the library's
    tap-major layouts, two ping-pong activation buffers sized by `window` (never by an utterance's length).

    decode() cuts every utterance into windows of at most `window` frames with context_frames(cfg) frames of context on each side,
    runs the windows of all rows as rows of batched launches (each with its own length) and keeps the interiors."""

    def __init__(self, state, device: Optional[torch.device] = None, cfg: Optional[CodecConfig] = None, window: int = 128,
                 workspace_bytes: int = 1 << 30):
        if cfg is not None:
            state = (cfg, state)
        self.cfg, sd = load_codec_state(state)
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
            w = fold_weight_norm(sd[L["key"] + ".weight_g"], sd[L["key"] + ".weight_v"])
            D = dict(L)
            D["w"] = (conv_layout(w) if L["kind"] == "conv" else convt_layout(w)).to(dev)
            D["b"] = sd[L["key"] + ".bias"].to(torch.float32).to(dev)
            if L["snake"]:
                al = sd[L["snake"] + ".alpha"]
                D["alpha"] = al.reshape(-1).to(torch.float32).to(dev)
                D["inv"] = snake_inverse(al).to(dev)
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

    # -------------------------------------------------------------------------------------- device side
    def _workspace(self, rows: int) -> Tuple[torch.Tensor, torch.Tensor]:
        if self._bufs is None or rows > self._rows:
            self._bufs = None
            self._bufs = (torch.empty(rows * self.row_floats, dtype=torch.float32, device=self.device),
                          torch.empty(rows * self.row_floats, dtype=torch.float32, device=self.device))
            self._rows = rows
        return self._bufs

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
                stage_lens = {1: lens}
                for L in self.layers:
                    r = L["rate_in"]
                    if self.layer_events is not None:
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        self.layer_events.append((f"{L['kind']} {L['cin']}->{L['cout']} k{L.get('k', 2 * L.get('s', 0))} d{L.get('d', 1)}", e0, e1))
                        e0.record()
                    if r not in stage_lens:
                        stage_lens[r] = lens * r
                    a = CodecConvArgs(w=hb.ptr(L["w"]), bias=hb.ptr(L["b"]), alpha=hb.ptr(L.get("alpha")), inv=hb.ptr(L.get("inv")),
                                      lens=hb.ptr(stage_lens[r]), B=J, T=Tg * r, C_in=L["cin"], C_out=L["cout"], ldx=W * r,
                                      tanh_out=int(bool(L.get("tanh"))))
                    if L["kind"] == "convt":
                        a.x, a.y, a.ldy, a.stride = hb.ptr(cur), hb.ptr(oth), W * r * L["s"], L["s"]
                        hb.check(lib.dia_codec_convt(C.byref(a), st), "dia_codec_convt")
                        cur, oth = oth, cur
                    elif L.get("res"):                         # the residual unit's 1x1: x is the k-7 output, the sum lands on the unit's input
                        a.x, a.y, a.res, a.ldx, a.ldy, a.k, a.dilation = hb.ptr(oth), hb.ptr(cur), hb.ptr(cur), W * r, W * r, 1, 1
                        hb.check(lib.dia_codec_conv(C.byref(a), st), "dia_codec_conv")
                    else:
                        a.x, a.y, a.ldy, a.k, a.dilation = hb.ptr(cur), hb.ptr(oth), W * r, L["k"], L["d"]
                        hb.check(lib.dia_codec_conv(C.byref(a), st), "dia_codec_conv")
                        if not L["snake"] or L.get("tanh"):    # first and last layer: the result is the new stream
                            cur, oth = oth, cur
                    if self.layer_events is not None:
                        self.layer_events[-1][2].record()
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
        window = self.window if window is None else int(window)
        if not 1 <= window <= self.window:
            raise ValueError(f"window = {window} outside [1, {self.window}] (the workspace is sized by the codec's window)")
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

    def stream(self, window: Optional[int] = None) -> CodecStream:
        """a streaming state for one utterance on this codec"""
        window = self.window if window is None else int(window)
        if not 1 <= window <= self.window:
            raise ValueError(f"window = {window} outside [1, {self.window}]")
        return CodecStream(lambda c: self._run([self._check_codes(c)])[0], self.cfg.n_codebooks, self.cfg.hop, window, self.ctx)
