"""``Dia`` — the drop-in boundary of the decode path (reference dia/model.py:101-846).

Same constructor / ``from_local`` / ``from_pretrained`` / ``generate`` / ``save_audio`` /
``load_audio`` surface and error behaviour as the reference class; underneath, text goes to byte
tokens on the host and everything from the encoder to the sampled token buffer runs in
``libdia_hip.so`` on one MI355X.  Extensions that the reference lacks are additive:
``generate_codes`` (the [1, 9, T'] code tensor the codec would receive — the Descript Audio Codec
itself is a third-party network outside this path), ``generate_batch`` (B utterances per call, the
reference hard-codes B=1, dia/state.py:83-84) and a ``load_dac`` switch for offline use.
"""

from __future__ import annotations

import math
import time
from dataclasses import dataclass
from enum import Enum
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import binding as hb
from .config import DiaConfig
from .engine import DecodeSession, DeviceWeights, Request, UtteranceResult
from .tokens import codes_for_codec, effective_text, encode_text
from . import weights as W

DEFAULT_SAMPLE_RATE = 44100


class ComputeDtype(str, Enum):
    FLOAT32 = "float32"
    FLOAT16 = "float16"
    BFLOAT16 = "bfloat16"

    def to_dtype(self) -> torch.dtype:
        return {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}[self.value]


@dataclass
class GenerationRequest:
    """One utterance of Dia.generate_stream / generate_batch(slots=N): the per-call arguments of generate().  None = the call's
    scalar argument of the same name."""
    text: str
    max_tokens: Optional[int] = None
    cfg_scale: Optional[float] = None
    temperature: Optional[float] = None
    top_p: Optional[float] = None
    cfg_filter_top_k: Optional[int] = None
    seed: Optional[int] = None
    audio_prompt: Optional[np.ndarray] = None
    audio_prompt_text: Optional[str] = None
    adapter: Optional[Union[str, int]] = None       # an adapter of Dia.load_adapters (name or index); None = the call's / the base model


def _nth(arg, i):
    """the i-th of a per-request sequence, or the scalar itself"""
    return arg[i] if isinstance(arg, (list, tuple, np.ndarray)) else arg


def _default_device() -> torch.device:
    if torch.cuda.is_available():
        return torch.device("cuda")
    raise hb.DiaHipError("no HIP device visible: this build of Dia runs on MI355X only (no CPU path)")


class Dia:
    # what compute_dtype="float32" does with a checkpoint that bf16 cannot hold: "exact" = three bf16 planes per weight
    # (the reference's fp32 path, ~3x slower), "bf16x2" = hi + lo bf16 planes (relative error <= 2^-17, 2x the weight
    # traffic, the tuned decode kernels), "round" = one rounded bf16 tile set (fast; the load prints a warning)
    fp32_weights = "exact"
    # "2:4": a 2:4-pruned checkpoint (offline_prune.py --prune-mode 2:4) also carries its decoder matrices and logits head as 2:4
    # sparse streams, which decode steps of batch 1-2 stream instead of the dense tiles (DeviceWeights sparse="2:4"); "off" = dense
    # "unstructured": an unstructured-pruned checkpoint also carries those matrices as lossless lane-local fixed-rate streams (DeviceWeights
    # sparse="unstructured"), streamed at batch 1-2 for the launch classes the knob usparse enables (none by default)
    sparse_weights = "off"
    # "mxfp8": an MXFP8-quantised checkpoint (offline_quantize.py) also carries its decoder matrices and logits head as MXFP8
    # streams, which decode steps of batch 1-8 stream instead of the dense tiles (DeviceWeights quant="mxfp8"); "mxfp4": the same
    # for an MXFP4-quantised checkpoint (offline_quantize.py --format mxfp4, DeviceWeights quant="mxfp4"); "bf16" = dense
    weight_format = "bf16"
    # "fp8": every session of generate* / stream_frames / score* keeps an e4m3 copy of the cross K/V caches with one power-of-two
    # scale per key and head, and its decode steps read that instead of the bf16 caches (DecodeSession cross_kv="fp8"; needs a
    # bf16 compute_dtype).  "bf16" = the caches as they are
    cross_kv = "bf16"
    # "fp8": every such session keeps its SELF K/V caches as e4m3 with one power-of-two scale per key and head — the step's new
    # key is quantised as it is appended, no bf16 self cache exists (0.516 of its bytes) and audio prompts replay through the decode
    # step (DecodeSession self_kv="fp8"; needs a bf16 compute_dtype).  "bf16" = the caches as they are
    self_kv = "bf16"
    # "batched": every such session prefills audio prompts of more than one frame as ONE packed batch wherever it can be asked for —
    # also when a request is admitted into a slot (generate_stream / stream_frames / generate_batch(slots=N)) and onto
    # self_kv="fp8" caches — instead of replaying them through the decode step (DecodeSession prompt_prefill="batched"; a session
    # that cannot serve it — fp32 K/V, adapters, scoring, a compacted or two-plane model — raises ValueError).  "auto" = closed
    # bf16 sessions prefill, everything else replays; "replay" = always replay
    prompt_prefill = "auto"
    # HZ: generate(), generate_audio_batch() and stream_audio() return their samples at this rate, converted from the codec's
    # 44.1 kHz by the native codec's resampler (DeviceCodec.resample / resample_stream); None = the codec's rate, as it comes
    output_sample_rate: Optional[int] = None
    # the reference application's speed factor (clamped to [0.1, 5], below 1 = slower): generate(), generate_audio_batch() and
    # stream_audio() stretch their waveform by it on the device, at the codec's rate and before output_sample_rate's conversion
    # (DeviceCodec.time_scale / time_scale_stream; DESIGN.md "Speed factor").  speed_mode "interp" is the reference's np.interp
    # (the pitch moves with the tempo; cannot stream), "wsola" keeps the pitch.  1.0 = every call launches what it did without it
    speed_factor: float = 1.0
    speed_mode: str = "interp"
    # LUFS: generate(), generate_audio_batch() and generate_long() bring their waveform to this integrated loudness (ITU-R
    # BS.1770-4) by ONE gain per utterance, lowered where the true peak would cross peak_ceiling (dBTP): a pure gain, not a limiter
    # (DeviceCodec.normalize_loudness; DESIGN.md "Loudness").  It is the LAST step, after the speed factor and the resampler, at the
    # delivered rate, so the ceiling holds for the samples the caller gets.  stream_audio() refuses it: the gain depends on the whole
    # utterance.  None = nothing new is constructed or launched
    loudness_target: Optional[float] = None
    peak_ceiling: float = -1.0
    # the native codec's DECODER precision that codec_path= on the loaders asks load_codec() for: "fp32" (the exact kernel), "bf16x2"
    # or "bf16" (bf16 MFMA operands in two planes / one; DESIGN.md "Codec: bf16 modes").  The encode side is fp32 in every mode.
    # load_codec() sets it, on the instance, to the mode it loaded
    codec_precision = "fp32"

    def __init__(self, config: DiaConfig, compute_dtype: Union[str, ComputeDtype] = ComputeDtype.FLOAT32,
                 device: Optional[torch.device] = None):
        """compute_dtype selects the K/V-cache precision: float32 keeps K/V in fp32 (the parity
        configuration against the reference's fp32 CPU path), bfloat16/float16 keep them in bf16
        (the reference's GPU configuration, state.py:142-151).  Weights are streamed as bf16 and all
        accumulation is fp32 in both cases."""
        self.config = config
        self.device = torch.device(device) if device is not None else _default_device()
        if self.device.type != "cuda":
            raise hb.DiaHipError(f"device {self.device} is not a HIP device; there is no CPU fallback")
        if isinstance(compute_dtype, str):
            compute_dtype = ComputeDtype(compute_dtype)
        self.compute_dtype = compute_dtype.to_dtype()
        self.model: Optional[DeviceWeights] = None      # resident weights (reference: DiaModel nn.Module)
        self.dac_model = None
        self.codec = None                               # codec.DeviceCodec of load_codec(): the native DAC codec
        self.last_codes: Optional[np.ndarray] = None
        self.weights_rounded = False
        self.weights_exact_planes = False
        self.adapters = None                            # lora.AdapterBank of load_adapters(): adapters that stay unmerged, per request
        hb.lib()                                        # fail now, not at first generate()

    # ------------------------------------------------------------------ loaders
    def _install(self, sd: Dict[str, torch.Tensor], adapter_path: Optional[str] = None) -> None:
        if any("lora_" in k for k in sd):           # model.py:170-172: adapter keys of a half-merged checkpoint are dropped
            sd = {k: v for k, v in sd.items() if "lora_" not in k}
        if adapter_path:
            from .lora import merge_lora_state_dict
            sd = merge_lora_state_dict(sd, adapter_path)
        missing, unexpected = W.check_state_dict(self.config, sd)
        if unexpected:
            print(f"Warning: Unexpected keys found in checkpoint: {unexpected}")
        if missing:
            # deliberate tightening: the reference loads with strict=False and only warns (model.py:173-177), which
            # leaves the missing tensors at their random initialisation; listed in INTEGRATION.md
            raise RuntimeError(f"Missing keys in checkpoint: {missing}")
        with torch.cuda.device(self.device):
            # sparse_weights="2:4": the checkpoint is taken as the 2:4 one it is said to be and never compacted.  An activation-aware
            # 2:4 pruning (offline_prune.py --act-stats) zeroes a whole input channel wherever that channel is among the two weakest of
            # its group in every column; to the structure detection such rows look like structured pruning
            self.model = DeviceWeights(self.config, sd, self.device, sparse=self.sparse_weights,
                                       compact="off" if self.sparse_weights in ("2:4", "unstructured") else "auto",
                                       quant=self.weight_format if self.weight_format in ("mxfp8", "mxfp4") else "off")
            # DenseGeneral kernels are streamed as ONE bf16 tile set by the fast kernels.  A checkpoint whose values are
            # bf16-representable (bf16-trained weights stored as fp32, the synthetic ones) loses nothing.  A genuine fp32
            # checkpoint would be rounded once at load = the reference's bfloat16 configuration, NOT its float32 path:
            #   compute_dtype="float32": the weights are kept as three bf16 planes (hi + mid + lo == w exactly) and run
            #       through the generic kernel — the reference's fp32 arithmetic for ANY checkpoint, at about a third
            #       of the speed (Dia.fp32_weights = "round" keeps the single rounded tile set and says so);
            #   bfloat16 / float16: rounded once, like the reference's own low-precision modules.
            self.weights_rounded = self.model.max_weight_rounding > 0.0
            self.weights_exact_planes = False
            if self.weights_rounded and self.compute_dtype == torch.float32:
                if self.fp32_weights == "exact":
                    rounding = self.model.max_weight_rounding
                    self.model = DeviceWeights(self.config, sd, self.device, weight_planes=3)
                    self.weights_rounded, self.weights_exact_planes = False, True
                    print(f"Note: checkpoint weights are not bf16-representable (largest relative rounding {rounding:.2e}): "
                          f"compute_dtype='float32' keeps them exact as three bf16 planes (3x the weight traffic, generic kernel).")
                elif self.fp32_weights == "bf16x2":
                    rounding = self.model.max_weight_rounding
                    self.model = DeviceWeights(self.config, sd, self.device, weight_planes=2)
                    self.weights_rounded = False
                    print(f"Note: checkpoint weights are not bf16-representable (largest relative rounding {rounding:.2e}): "
                          f"fp32_weights='bf16x2' keeps them as hi + lo bf16 planes (relative error <= 2^-17, 2x the weight traffic, "
                          f"tuned kernels).")
                else:
                    print(f"Warning: checkpoint weights are not bf16-representable (largest relative rounding "
                          f"{self.model.max_weight_rounding:.2e}); they are streamed as bf16, so compute_dtype='float32' here means "
                          f"fp32 activations / accumulation / K/V over bf16-rounded weights, not the reference's fp32 weights.")

    @classmethod
    def from_state_dict(cls, config: DiaConfig, state_dict: Dict[str, torch.Tensor],
                        compute_dtype: Union[str, ComputeDtype] = ComputeDtype.FLOAT32,
                        device: Optional[torch.device] = None) -> "Dia":
        dia = cls(config, compute_dtype, device)
        dia._install(state_dict)
        return dia

    @classmethod
    def from_local(cls, config_path: str, checkpoint_path: str,
                   compute_dtype: Union[str, ComputeDtype] = ComputeDtype.FLOAT32,
                   device: Optional[torch.device] = None, load_dac: bool = True,
                   adapter_path: Optional[str] = None, codec_path: Optional[str] = None) -> "Dia":
        """reference model.py:139-187: config JSON + pickled/safetensors state_dict (this is the
        loader for ``offline_prune.py`` outputs).  ``adapter_path``: LoRA adapter directory merged into the
        dense weights before they are tiled (reference cli.py:166-174 wraps with PEFT at run time)."""
        config = DiaConfig.load(config_path)
        if config is None:
            raise FileNotFoundError(f"Config file not found at {config_path}")
        dia = cls(config, compute_dtype, device)
        try:
            sd = W.load_state_dict_file(checkpoint_path)
        except FileNotFoundError:
            raise FileNotFoundError(f"Checkpoint file not found at {checkpoint_path}")
        except Exception as e:
            raise RuntimeError(f"Error loading checkpoint from {checkpoint_path}") from e
        dia._install(sd, adapter_path)
        if load_dac:
            dia._load_dac_model()
        if codec_path is not None:
            dia.load_codec(codec_path, precision=dia.codec_precision)
        return dia

    @classmethod
    def from_pretrained(cls, model_name: str = "nari-labs/Dia-1.6B",
                        compute_dtype: Union[str, ComputeDtype] = ComputeDtype.FLOAT32,
                        device: Optional[torch.device] = None, load_dac: bool = True,
                        adapter_path: Optional[str] = None, codec_path: Optional[str] = None, **kwargs) -> "Dia":
        """reference model.py:189-236.  ``model_name`` must be a local directory holding
        ``config.json`` and ``model.safetensors`` / ``pytorch_model.bin`` (hub download needs a network)."""
        p = Path(model_name)
        if not p.is_dir():
            raise FileNotFoundError(
                f"{model_name!r} is not a local model directory; fetching from the Hugging Face Hub is not supported here")
        cfg_path, ckpt = W.find_checkpoint_in_dir(str(p))
        config = W.read_hub_config(cfg_path)
        dia = cls(config, compute_dtype, device)
        dia._install(W.load_state_dict_file(ckpt), adapter_path)
        if load_dac:
            dia._load_dac_model()
        if codec_path is not None:
            dia.load_codec(codec_path, precision=dia.codec_precision)
        return dia

    def load_codec(self, path_or_state, window: int = 128, precision: str = "fp32"):
        """Set the native DAC codec (dia_hip/codec.py, csrc/codec.hip) on this instance: a DAC ``.pth`` / bare state dict, as a
        path or in memory.  generate() then returns waveforms and generate_audio_batch / stream_audio work; the third-party
        ``dac`` package is not needed.  A missing or unexpected decoder / quantizer key is refused by name.  A checkpoint that
        also holds the encoder makes load_audio() / encode_audio() and file prompts work; one without still decodes.
        precision: "fp32", "bf16x2" or "bf16" for the decoder's convolutions; any other value is refused by name.  Voice prompts
        are encoded in fp32 in every mode."""
        from .codec import DeviceCodec, precision_planes
        precision_planes(precision)
        with torch.cuda.device(self.device):
            self.codec = DeviceCodec(path_or_state, self.device, window=window, precision=precision)
        self.codec_precision = precision
        return self.codec

    def _load_dac_model(self):
        """reference model.py:238-252 — raises RuntimeError when the codec cannot be loaded."""
        try:
            import dac  # type: ignore

            print("Loading DAC model...")
            path = dac.utils.download()
            m = dac.DAC.load(path).to(self.device)
            m.eval()
        except Exception as e:
            raise RuntimeError(f"Failed to load DAC model: {e}") from e
        self.dac_model = m

    def load_adapters(self, adapters: Dict[str, str]) -> List[int]:
        """Load LoRA adapter directories {name: dir} into the model's adapter bank, UNMERGED: one base model then serves every one
        of them, per request (``adapter=`` / ``adapters=`` of the generate and score calls; DESIGN.md "Per-request adapters").
        Only q_proj / k_proj / v_proj adapters (the reference's default target set is q_proj v_proj) of rank <= 64; anything else
        raises and can be merged at load instead (``adapter_path=``, one voice per process).  Call it before the first generation
        that uses an adapter: the bank is fixed once a session has been opened with it.  Returns the adapters' indices."""
        from .lora import AdapterBank
        if self.model is None:
            raise RuntimeError("no weights loaded")
        if self.adapters is None:
            self.adapters = AdapterBank(self.config, self.device)
        return [self.adapters.add(name, path) for name, path in adapters.items()]

    def _bank_for(self, wanted: Sequence) -> Optional["object"]:
        """the bank when any of `wanted` names an adapter (sessions without one are the sessions of a model without a bank)"""
        if all(a is None for a in wanted):
            return None
        if self.adapters is None:
            raise ValueError("adapter= given but no adapter is loaded: call Dia.load_adapters({name: dir}) first")
        for a in wanted:
            self.adapters.index_of(a)               # unknown names raise here, before a session exists
        return self.adapters

    # ------------------------------------------------------------------ generation
    def _kv_dtype(self) -> str:
        return "f32" if self.compute_dtype == torch.float32 else "bf16"

    def _run(self, texts: Sequence[str], max_tokens, cfg_scale, temperature, top_p, top_k,
             seeds: Optional[Sequence[Optional[int]]], verbose: bool, ignore_eos: bool = False,
             use_graph: bool = True, audio_prompts: Optional[Sequence[Optional[np.ndarray]]] = None,
             adapters: Optional[Sequence] = None) -> List[UtteranceResult]:
        if self.model is None:
            raise RuntimeError("no weights loaded")
        ids = [encode_text(t, self.config) for t in texts]
        adapters = list(adapters) if adapters is not None else [None] * len(ids)
        bank = self._bank_for(adapters)
        t0 = time.time()
        with torch.cuda.device(self.device):
            s = DecodeSession(self.model, ids, kv_dtype=self._kv_dtype(), cross_kv=self.cross_kv, self_kv=self.self_kv, prompt_prefill=self.prompt_prefill, max_tokens=max_tokens, cfg_scale=cfg_scale,
                              temperature=temperature, top_p=top_p, top_k=top_k, seeds=seeds, ignore_eos=ignore_eos,
                              audio_prompts=audio_prompts, adapters=bank, adapter_ids=adapters if bank is not None else None)
            try:
                s.prefill()
                s.sync()
                t1 = time.time()
                if verbose:
                    print(f"generate: prefill {t1 - t0:.3f}s; prefill audio steps {s.first_steps}; starting generation loop")
                s.run(use_graph=use_graph)
                res = s.results()
                if verbose:
                    dt = time.time() - t1
                    n = sum(r.last_step for r in res)
                    print(f"generate: {n} frames in {dt:.3f}s = {n / max(dt, 1e-9):.1f} frames/s")
            finally:
                s.close()
        return res

    def _requests(self, items, max_tokens, cfg_scale, temperature, top_p, top_k, seeds, audio_prompts, audio_prompt_texts,
                  adapters=None) -> List[Request]:
        """texts or GenerationRequests + scalar-or-per-request arguments -> engine requests"""
        if adapters is not None and len(adapters) != len(items):
            raise ValueError(f"adapters: {len(adapters)} entries for {len(items)} requests (one per request, None = the base model)")
        out = []
        for i, it in enumerate(items):
            g = it if isinstance(it, GenerationRequest) else GenerationRequest(str(it))
            pick = lambda own, arg: own if own is not None else _nth(arg, i)
            prompt = pick(g.audio_prompt, audio_prompts)
            if isinstance(prompt, torch.Tensor):
                prompt = prompt.detach().cpu().numpy()
            ptext = pick(g.audio_prompt_text, audio_prompt_texts)
            if prompt is not None and not ptext:
                raise ValueError("`audio_prompt_text` is required when `audio_prompt` is provided.")
            mt = pick(g.max_tokens, max_tokens)
            out.append(Request(encode_text(effective_text(g.text, ptext), self.config), seed=pick(g.seed, seeds),
                               max_tokens=None if mt is None else int(mt), cfg_scale=float(pick(g.cfg_scale, cfg_scale)),
                               temperature=float(pick(g.temperature, temperature)), top_p=float(pick(g.top_p, top_p)),
                               top_k=int(pick(g.cfg_filter_top_k, top_k) or 0), audio_prompt=prompt,
                               adapter=g.adapter if g.adapter is not None else (None if adapters is None else adapters[i])))
        return out

    # ------------------------------------------------------------------ scoring
    @torch.inference_mode()
    def score_batch(self, texts: Sequence[str], codes_list: Sequence, *, audio_prompts: Optional[Sequence] = None,
                    cfg_scale: float = 3.0, audio_prompt_texts: Optional[Sequence[Optional[str]]] = None,
                    use_graph: bool = True, adapters: Optional[Sequence] = None) -> List["ScoreResult"]:
        """Teacher-forced log-likelihood of known audio codes under the loaded checkpoint, up to 8 utterances of any lengths in
        one decode session — the session generate() would use: this model's K/V dtype, weight format, pruning and compaction.
        codes_list[b]: codec frames [T, C] or a delayed token buffer [rows, C] (score.teacher_rows).  The rows are forced through
        rows - 1 decode steps and every step's logits are reduced on the device (DESIGN.md "Scoring"); with an audio prompt only
        the rows behind it are scored.  Returns one ScoreResult per utterance (nats; no sampling happens).
        adapters: per utterance the name / index of an adapter of load_adapters(), None = the base model."""
        from .score import check_prompt_rows, summarise, teacher_rows, valid_mask

        if self.model is None:
            raise RuntimeError("no weights loaded")
        n = len(texts)
        if not 1 <= n <= 8 or len(codes_list) != n:
            raise ValueError("score_batch: 1..8 texts and as many codes")
        prompts = [None] * n if audio_prompts is None else [None if p is None else (p.detach().cpu().numpy() if isinstance(p, torch.Tensor) else np.asarray(p)) for p in audio_prompts]
        apt = audio_prompt_texts or [None] * n
        rows = [teacher_rows(self.config, c.detach().cpu().numpy() if isinstance(c, torch.Tensor) else c, prompt=p)
                for c, p in zip(codes_list, prompts)]
        first = [1 if p is None else check_prompt_rows(self.config, r, p) for r, p in zip(rows, prompts)]
        mt = max(r.shape[0] for r in rows)
        if mt > self.config.data.audio_length:
            raise ValueError(f"{mt} token rows do not fit audio_length {self.config.data.audio_length}")
        ids = [encode_text(effective_text(t, a), self.config) for t, a in zip(texts, apt)]
        adapters = list(adapters) if adapters is not None else [None] * n
        if len(adapters) != n:
            raise ValueError("score_batch: one adapter entry per text")
        bank = self._bank_for(adapters)
        with torch.cuda.device(self.device):
            s = DecodeSession(self.model, ids, kv_dtype=self._kv_dtype(), cross_kv=self.cross_kv, self_kv=self.self_kv, prompt_prefill=self.prompt_prefill, max_tokens=mt, cfg_scale=cfg_scale, temperature=0.0,
                              teacher_tokens=rows, audio_prompts=prompts, score=True, adapters=bank,
                              adapter_ids=adapters if bank is not None else None)
            try:
                s.prefill()
                s.decode(mt - 1, use_graph=use_graph)
                sc = s.scores_host()
                s._raise_if_invalid()
            finally:
                s.close()
        return [summarise(sc[b, : r.shape[0]], valid_mask(r, f, self.config.data)) for b, (r, f) in enumerate(zip(rows, first))]

    def score(self, text: str, codes, *, audio_prompt=None, cfg_scale: float = 3.0, audio_prompt_text: Optional[str] = None,
              adapter: Optional[Union[str, int]] = None) -> "ScoreResult":
        """score_batch for one utterance"""
        return self.score_batch([text], [codes], audio_prompts=None if audio_prompt is None else [audio_prompt], cfg_scale=cfg_scale,
                                audio_prompt_texts=[audio_prompt_text], adapters=[adapter])[0]

    @torch.inference_mode()
    def calibrate(self, texts: Sequence[str], codes_list: Sequence, *, audio_prompts: Optional[Sequence] = None,
                  cfg_scale: float = 3.0, audio_prompt_texts: Optional[Sequence[Optional[str]]] = None, use_graph: bool = True,
                  batch: int = 8, stats: Optional["ActStats"] = None, gram: bool = False, gram_layers=None,
                  gram_stats: Optional["GramStats"] = None):
        """Activation statistics of the loaded checkpoint over known audio codes (DESIGN.md "Activation statistics"): the texts and
        codes are forced through the model as score_batch forces them (score.teacher_rows), up to ``batch`` (1..8) utterances of equal
        row count per decode session, and every GEMM input's per-channel sum of squares is accumulated on the device.  Returns one ActStats over all of
        them, merged into ``stats`` when given (statistics of earlier calls).  What offline_prune.py --act-stats takes.
        The checkpoint must be loaded uncompacted, without seg="on"; no adapter takes part.
        gram=True (DESIGN.md "Gram matrices and GPTQ"): the sessions run with calibrate="gram" and the call returns
        ``(ActStats, GramStats)``, the Gram matrices of the decode step's GEMM inputs for the layers of ``gram_layers`` (None: all of them
        and the logits head; see DecodeSession), merged into ``gram_stats`` when given.  What offline_quantize.py --gram-stats takes."""
        from .calib import ActStats
        from .score import check_prompt_rows, teacher_rows

        if self.model is None:
            raise RuntimeError("no weights loaded")
        n = len(texts)
        if n < 1 or len(codes_list) != n or not 1 <= batch <= 8:
            raise ValueError("calibrate: at least one text, as many codes, and batch in 1..8")
        prompts = [None] * n if audio_prompts is None else [None if p is None else (p.detach().cpu().numpy() if isinstance(p, torch.Tensor) else np.asarray(p)) for p in audio_prompts]
        apt = audio_prompt_texts or [None] * n
        rows = [teacher_rows(self.config, c.detach().cpu().numpy() if isinstance(c, torch.Tensor) else c, prompt=p)
                for c, p in zip(codes_list, prompts)]
        for r, p in zip(rows, prompts):
            if p is not None:
                check_prompt_rows(self.config, r, p)
            if r.shape[0] > self.config.data.audio_length:
                raise ValueError(f"{r.shape[0]} token rows do not fit audio_length {self.config.data.audio_length}")
        ids = [encode_text(effective_text(t, a), self.config) for t, a in zip(texts, apt)]
        out, gout = stats, gram_stats
        # a teacher-forced utterance runs to the session's max_tokens: a session takes utterances of one row count, so that no step
        # counts rows behind an utterance's codes
        by_len: Dict[int, List[int]] = {}
        for i, r in enumerate(rows):
            by_len.setdefault(r.shape[0], []).append(i)
        chunks = [idx[i: i + batch] for _, idx in sorted(by_len.items()) for i in range(0, len(idx), batch)]
        # the session generate() would use, except that forced rows are replayed (the batched prompt prefill does not serve them)
        caches = dict(cross_kv=self.cross_kv, prompt_prefill="replay" if self.prompt_prefill == "batched" else self.prompt_prefill)
        caches["self_kv"] = self.self_kv
        for sel in chunks:
            mt = rows[sel[0]].shape[0]
            with torch.cuda.device(self.device):
                s = DecodeSession(self.model, [ids[i] for i in sel], kv_dtype=self._kv_dtype(), max_tokens=mt, **caches,
                                  cfg_scale=cfg_scale, temperature=0.0, teacher_tokens=[rows[i] for i in sel],
                                  audio_prompts=[prompts[i] for i in sel], calibrate="gram" if gram else True,
                                  gram_layers=gram_layers if gram else None)
                try:
                    s.prefill()
                    s.decode(mt - 1, use_graph=use_graph)
                    part = s.act_stats()
                    gpart = s.gram_stats() if gram else None
                    s._raise_if_invalid()
                finally:
                    s.close()
            out = part if out is None else out.merge(part)
            if gram:
                gout = gpart if gout is None else gout.merge(gpart)
        return (out, gout) if gram else out

    @torch.inference_mode()
    def generate_stream(self, requests_or_texts: Sequence[Union[str, GenerationRequest]], slots: int = 8,
                        max_tokens=None, cfg_scale=3.0, temperature=1.3, top_p=0.95, cfg_filter_top_k=35,
                        seeds: Optional[Sequence[Optional[int]]] = None, ignore_eos: bool = False,
                        audio_prompts: Optional[Sequence[Optional[np.ndarray]]] = None,
                        audio_prompt_texts: Optional[Sequence[Optional[str]]] = None, poll: int = 64, s_cap: Optional[int] = None,
                        adapters: Optional[Sequence] = None):
        """Continuous batching: any number of utterances through `slots` slots of ONE decode session — a finished utterance's slot
        is refilled from the queue between two decode steps, so the batch stays full while requests last.  Yields
        (request index, codec input [1, C, T']) as utterances finish.  The sampling arguments are defaults: each may be a per-request
        sequence, and a GenerationRequest carries its own.  Every utterance's tokens are those of generating it alone with its
        seed (compute_dtype float32: bit for bit).  adapters: per request the name / index of an adapter of load_adapters()
        (None = the base model); a GenerationRequest's own `adapter` goes first."""
        if self.model is None:
            raise RuntimeError("no weights loaded")
        items = list(requests_or_texts)
        reqs = self._requests(items, max_tokens, cfg_scale, temperature, top_p, cfg_filter_top_k, seeds, audio_prompts, audio_prompt_texts,
                              adapters)
        bank = self._bank_for([r.adapter for r in reqs])
        if not reqs:
            return
        cap = max([r.max_tokens for r in reqs if r.max_tokens is not None] or [self.config.data.audio_length])
        if any(r.max_tokens is None for r in reqs):
            cap = self.config.data.audio_length
        if s_cap is None:
            s_cap = max(32, max(len(r.text_ids) for r in reqs))
        with torch.cuda.device(self.device):
            s = DecodeSession.open(self.model, min(int(slots), len(reqs)), s_cap=min(int(s_cap), self.config.data.text_length),
                                   kv_dtype=self._kv_dtype(), cross_kv=self.cross_kv, self_kv=self.self_kv, prompt_prefill=self.prompt_prefill, max_tokens=cap, ignore_eos=ignore_eos, adapters=bank)
            try:
                for i, res in s.serve_iter(reqs, poll=poll):
                    yield i, codes_for_codec(res.codes, self.config)
            finally:
                s.close()

    @torch.inference_mode()
    def stream_frames(self, requests_or_texts: Sequence[Union[str, GenerationRequest]], slots: int = 8,
                      max_tokens=None, cfg_scale=3.0, temperature=1.3, top_p=0.95, cfg_filter_top_k=35,
                      seeds: Optional[Sequence[Optional[int]]] = None, ignore_eos: bool = False,
                      audio_prompts: Optional[Sequence[Optional[np.ndarray]]] = None,
                      audio_prompt_texts: Optional[Sequence[Optional[str]]] = None, s_cap: Optional[int] = None,
                      chunk: int = 16, stream_cap: Optional[int] = None, lag: int = 1, adapters: Optional[Sequence] = None):
        """generate_stream that hands the codec input out WHILE the utterances run: yields (request index, start frame,
        codes [1, C, n], final) every `chunk` decode steps — frames [start, start + n) of what generate_stream would yield for
        that request at the end, final exactly once per request (possibly with n = 0).  A frame is final max_delay steps after it
        was sampled (DESIGN.md "Frame streaming").  stream_cap: frames per slot one hand-over can carry (default 4 * chunk);
        lag = 1 keeps the next chunk queued on the GPU while this one is read, lag = 0 reads each chunk as soon as it is queued.
        adapters: as generate_stream."""
        if self.model is None:
            raise RuntimeError("no weights loaded")
        items = list(requests_or_texts)
        reqs = self._requests(items, max_tokens, cfg_scale, temperature, top_p, cfg_filter_top_k, seeds, audio_prompts, audio_prompt_texts,
                              adapters)
        bank = self._bank_for([r.adapter for r in reqs])
        if not reqs:
            return
        cap = max([r.max_tokens for r in reqs if r.max_tokens is not None] or [self.config.data.audio_length])
        if any(r.max_tokens is None for r in reqs):
            cap = self.config.data.audio_length
        if s_cap is None:
            s_cap = max(32, max(len(r.text_ids) for r in reqs))
        with torch.cuda.device(self.device):
            s = DecodeSession.open(self.model, min(int(slots), len(reqs)), s_cap=min(int(s_cap), self.config.data.text_length),
                                   kv_dtype=self._kv_dtype(), cross_kv=self.cross_kv, self_kv=self.self_kv, prompt_prefill=self.prompt_prefill, max_tokens=cap, ignore_eos=ignore_eos,
                                   stream_cap=4 * int(chunk) if stream_cap is None else int(stream_cap), adapters=bank)
            try:
                yield from s.stream_iter(reqs, chunk=chunk, lag=lag)
            finally:
                s.close()

    def audio_distance(self, a, b, sample_rate: int = DEFAULT_SAMPLE_RATE, **kw):
        """the multi-scale STFT and log-mel distances between waveform a and waveform b (mono float samples, or lists of them pair by
        pair) at sample_rate Hz, computed on this instance's device (dia_hip/spectral.py, csrc/spectral.hip): per pair
        ``{"stft": x, "mel": y, "per_resolution": {...}}``.  Needs no codec and no weights; keywords as DeviceSpectral.distance."""
        if getattr(self, "_spectral", None) is None:
            from .spectral import DeviceSpectral
            self._spectral = DeviceSpectral(self.device)
        return self._spectral.distance(a, b, int(sample_rate), **kw)

    def codec_roundtrip_distance(self, wave, **kw):
        """what the loaded native codec does to a waveform at its own rate: encode -> decode in the codec's precision, cut to the
        input's length, audio_distance against the input.  Needs load_codec() of a checkpoint that holds the encoder."""
        return self._need_codec().roundtrip_distance(wave, **kw)

    def _need_codec(self):
        if self.codec is None:
            raise RuntimeError("no native codec loaded: call Dia.load_codec(path_or_state) first")
        return self.codec

    @torch.inference_mode()
    def generate_audio_batch(self, texts: Sequence[str], *args, **kw) -> List[np.ndarray]:
        """generate_batch (same arguments), then the native codec over all utterances at once: one float32 waveform
        [T'_b * 512] per utterance, each as when decoded alone.  Needs load_codec()."""
        codec = self._need_codec()
        speed = self._speed(codec)
        rate = self._output_rate(codec)
        target = self._loudness(codec)
        waves = codec.decode_batch(self.generate_batch(texts, *args, **kw))
        if speed is not None:
            waves = codec.time_scale(waves, speed, self.speed_mode)
        if rate:
            waves = codec.resample(waves, codec.cfg.sample_rate, rate)
        if target is not None:
            waves = codec.normalize_loudness(waves, rate or codec.cfg.sample_rate, target, float(self.peak_ceiling))[0]
        return waves

    def _loudness(self, codec) -> Optional[float]:
        """loudness_target where it asks for a normalisation, else None; the normalisation is the native codec's"""
        t = self.loudness_target
        if t is None:
            return None
        for name, v in (("loudness_target", t), ("peak_ceiling", self.peak_ceiling)):
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
                raise ValueError(f"{name} = {v!r} is not a finite number")
        if codec is None or not hasattr(codec, "normalize_loudness"):
            raise RuntimeError(f"loudness_target = {t} needs the native codec's loudness meter: call Dia.load_codec(path_or_state) first")
        return float(t)

    def measure_loudness(self, wave, sample_rate: int = DEFAULT_SAMPLE_RATE):
        """mono float samples [N] (or a list of them) at sample_rate -> {"loudness": LUFS (ITU-R BS.1770-4, integrated),
        "true_peak": dBTP, "sample_peak": dBFS, "steps": ...} per row, on this instance's device (dia_hip/loudness.py,
        csrc/loudness.hip).  Needs no codec and no weights."""
        if getattr(self, "_loudness_meter", None) is None:
            from .loudness import DeviceLoudness
            self._loudness_meter = DeviceLoudness(self.device)
        return self._loudness_meter.measure(wave, int(sample_rate))

    def _speed(self, codec) -> Optional[float]:
        """speed_factor, clamped, where it asks for a time-scaling, else None; the time-scaling is the native codec's"""
        from .timescale import MODES, clamp_speed
        if isinstance(self.speed_factor, bool) or not isinstance(self.speed_factor, (int, float)):
            raise ValueError(f"speed_factor = {self.speed_factor!r} is not a number")
        if self.speed_mode not in MODES:
            raise ValueError(f"speed_mode = {self.speed_mode!r} is not one of {MODES}")
        speed = clamp_speed(self.speed_factor)
        if speed == 1.0:
            return None
        if codec is None or not hasattr(codec, "time_scale"):
            raise RuntimeError(f"speed_factor = {self.speed_factor} needs the native codec's time-scaling: call Dia.load_codec(path_or_state) first")
        return speed

    def time_scale(self, wave, speed: float, mode: Optional[str] = None, window: int = 1024, tolerance: int = 512):
        """mono float samples [N] (or a list of them) stretched to float32 [int(N / speed)] on this instance's device
        (dia_hip/timescale.py, csrc/timescale.hip): mode "interp" (default: speed_mode) is the reference application's speed factor,
        "wsola" keeps the pitch.  Needs no codec and no weights."""
        if getattr(self, "_timescale", None) is None:
            from .timescale import DeviceTimescale
            self._timescale = DeviceTimescale(self.device)
        return self._timescale.time_scale(wave, speed, self.speed_mode if mode is None else mode, window, tolerance)

    def _output_rate(self, codec) -> Optional[int]:
        """output_sample_rate where it asks for another rate than the codec's, else None; the conversion is the native codec's"""
        rate = self.output_sample_rate
        if rate is None or int(rate) == (DEFAULT_SAMPLE_RATE if codec is None else codec.cfg.sample_rate):
            return None
        if int(rate) < 1:
            raise ValueError(f"output_sample_rate = {rate} is not a positive rate in Hz")
        if codec is None or not hasattr(codec, "resample"):
            raise RuntimeError(f"output_sample_rate = {rate} Hz needs the native codec's resampler: call Dia.load_codec(path_or_state) first")
        return int(rate)

    def stream_audio(self, requests_or_texts: Sequence[Union[str, GenerationRequest]], slots: int = 8, **kw):
        """stream_frames (same arguments) with the native codec behind it: yields (request index, start sample, samples, final)
        while the utterances run.  The samples of a request, joined, equal codec.decode() of its whole code tensor; the last
        context_frames frames of a running utterance are held back until more arrive or it ends (DESIGN.md "Codec").  Needs
        load_codec().  With output_sample_rate set the samples are at that rate and equal codec.resample() of the whole waveform.
        With speed_factor other than 1 they are time-scaled first, per request by a WSOLA stream, and joined equal
        codec.time_scale(..., "wsola") of the whole waveform; speed_mode "interp" cannot stream and is refused here, before
        anything runs, and so is a loudness_target: its gain depends on the whole utterance."""
        if self.loudness_target is not None:
            raise ValueError("stream_audio: loudness_target cannot stream (the gain depends on the whole utterance's loudness and "
                             "true peak); set loudness_target = None and normalise the joined samples")
        if self.codec is not None and self._speed(self.codec) is not None and self.speed_mode == "interp":
            raise ValueError("stream_audio: speed_mode 'interp' cannot stream (its positions depend on the utterance's total length); "
                             "set speed_mode = 'wsola'")
        return self._stream_audio(requests_or_texts, slots, **kw)

    @torch.inference_mode()
    def _stream_audio(self, requests_or_texts, slots, **kw):
        codec = self._need_codec()
        rate = self._output_rate(codec)
        speed = self._speed(codec)
        states, starts = {}, {}
        for i, _, codes, final in self.stream_frames(requests_or_texts, slots, **kw):
            st = states.get(i)
            if st is None:
                st = states[i] = (codec.stream(), codec.time_scale_stream(speed) if speed is not None else None,
                                  codec.resample_stream(codec.cfg.sample_rate, rate) if rate else None)
                starts[i] = 0
            y = st[0].push(codes, final)
            for nxt in st[1:]:                                  # one time-scaling and one resampling state per request: start
                if nxt is not None:                             # offsets count delivered samples
                    y = nxt.push(y, final)
            yield i, starts[i], y, final
            starts[i] += y.shape[0]
            if final:
                del states[i]

    @torch.inference_mode()
    def generate_batch(self, texts: Sequence[str], max_tokens: Optional[int] = None, cfg_scale: float = 3.0,
                       temperature: float = 1.3, top_p: float = 0.95, cfg_filter_top_k: int = 35,
                       seeds: Optional[Sequence[Optional[int]]] = None, verbose: bool = False,
                       ignore_eos: bool = False, audio_prompts: Optional[Sequence[Optional[np.ndarray]]] = None,
                       audio_prompt_texts: Optional[Sequence[Optional[str]]] = None, slots: Optional[int] = None,
                       adapters: Optional[Sequence] = None) -> List[np.ndarray]:
        """B utterances in one decode loop; returns the codec inputs [1, C, T'_b] per utterance.
        audio_prompts: per utterance None or codes [Tp, C]; audio_prompt_texts: their transcripts.
        slots=N: the utterances share N slots of a continuously batched session instead (generate_stream); the list returned is
        the same.  adapters: per utterance the name / index of an adapter of load_adapters(), None = the base model."""
        if adapters is not None and len(adapters) != len(texts):
            raise ValueError("generate_batch: one adapter entry per text")
        if slots is not None:
            out: List[Optional[np.ndarray]] = [None] * len(texts)
            for i, codes in self.generate_stream(texts, slots, max_tokens, cfg_scale, temperature, top_p, cfg_filter_top_k, seeds,
                                                 ignore_eos, audio_prompts, audio_prompt_texts, adapters=adapters):
                out[i] = codes
            return out
        apt = audio_prompt_texts or [None] * len(texts)
        eff = [effective_text(t, a) for t, a in zip(texts, apt)]
        res = self._run(eff, max_tokens, cfg_scale, temperature, top_p, cfg_filter_top_k, seeds, verbose, ignore_eos,
                        audio_prompts=audio_prompts, adapters=adapters)
        return [codes_for_codec(r.codes, self.config) for r in res]

    @torch.inference_mode()
    def generate_codes(self, text: str, max_tokens: Optional[int] = None, cfg_scale: float = 3.0,
                       temperature: float = 1.3, top_p: float = 0.95, cfg_filter_top_k: int = 35,
                       seed: Optional[int] = None, verbose: bool = False, adapter: Optional[Union[str, int]] = None) -> Optional[np.ndarray]:
        out = self.generate_batch([text], max_tokens, cfg_scale, temperature, top_p, cfg_filter_top_k,
                                  None if seed is None else [seed], verbose, adapters=[adapter])
        return out[0]

    @torch.inference_mode()
    def generate(self, text: str, max_tokens: Optional[int] = None, cfg_scale: float = 3.0, temperature: float = 1.3,
                 top_p: float = 0.95, use_torch_compile: bool = False, cfg_filter_top_k: int = 35,
                 audio_prompt: Union[str, torch.Tensor, None] = None, audio_prompt_text: Optional[str] = None,
                 seed: Optional[int] = None, verbose: bool = False, adapter: Optional[Union[str, int]] = None) -> Optional[np.ndarray]:
        """reference model.py:631-846.  ``adapter``: an adapter of load_adapters() for this call (None = the base model).  Failures inside generation are printed and turned into
        ``None`` exactly like the reference (model.py:729-733, 817-821, 841-845); ``use_torch_compile``
        is accepted and ignored (there is nothing to compile)."""
        if audio_prompt is not None and not audio_prompt_text:
            raise ValueError("`audio_prompt_text` is required when `audio_prompt` is provided.")
        if seed is not None:
            torch.manual_seed(seed)
            np.random.seed(seed)
        eff = effective_text(text, audio_prompt_text)
        prompt = None
        if audio_prompt is not None:
            # model.py:372-379: a path is encoded by the codec, a tensor is taken as codes [T, C] / [1, T, C].
            # The prompt rows are replayed through the decode step (semantic decision: DESIGN.md, audio prompt).
            try:
                pt = self.load_audio(audio_prompt) if isinstance(audio_prompt, str) else audio_prompt
                prompt = pt.detach().cpu().numpy() if isinstance(pt, torch.Tensor) else np.asarray(pt)
            except Exception as e:
                print(f"Error during preparation: {e}")             # model.py:729-733
                return None
        try:
            res = self._run([eff], max_tokens, cfg_scale, temperature, top_p, cfg_filter_top_k,
                            None if seed is None else [seed], verbose,
                            audio_prompts=None if prompt is None else [prompt], adapters=[adapter])[0]
        except Exception as e:
            print(f"Error during generation loop: {e}")
            import traceback

            traceback.print_exc()
            return None
        if res.codes.shape[0] == 0:
            print("Warning: No new tokens were generated after prefill.")
            return None
        self.last_codes = codes_for_codec(res.codes, self.config)
        try:
            return self._generate_output(self.last_codes)
        except Exception as e:
            print(f"Error during final decoding: {e}")
            return None

    def _generate_output(self, codec_input: np.ndarray, normalize: bool = True) -> Optional[np.ndarray]:
        """codes [1, C, T'] -> waveform: through the native codec when load_codec() set one (at output_sample_rate when that is
        set), else through the third-party codec (model.py:535-544).  normalize=False leaves loudness_target to the caller
        (generate_long normalises the joined waveform once)."""
        rate = self._output_rate(self.codec)
        speed = self._speed(self.codec)
        target = self._loudness(self.codec) if normalize else None
        if self.codec is not None:
            wave = self.codec.decode(codec_input)
            if speed is not None:
                wave = self.codec.time_scale(wave, speed, self.speed_mode)
            if rate:
                wave = self.codec.resample(wave, self.codec.cfg.sample_rate, rate)
            if target is not None:
                wave = self.codec.normalize_loudness(wave, rate or self.codec.cfg.sample_rate, target, float(self.peak_ceiling))[0]
            return wave
        if self.dac_model is None:
            raise RuntimeError("DAC model not loaded. Cannot decode audio.")
        codes = torch.from_numpy(codec_input.astype(np.int64)).to(self.device)
        with torch.inference_mode():
            z = self.dac_model.quantizer.from_codes(codes)
            audio = self.dac_model.decode(z[0])
        return audio.squeeze().cpu().numpy()

    # ------------------------------------------------------------------ audio file IO (host side)
    # With a native codec that has an encode side (load_codec() of a full DAC checkpoint) a file prompt needs no third-party
    # piece: the file is read by torchaudio when that is importable and by the standard library's wave module otherwise, and
    # encoded by DeviceCodec.encode.  Without one the methods keep the reference's names, arguments and failure behaviour
    # (reference model.py:546-595), which need the dac package and torchaudio.
    @torch.inference_mode()
    def encode_audio(self, wave, sample_rate: int = DEFAULT_SAMPLE_RATE, normalize_lufs: Optional[float] = None) -> torch.Tensor:
        """mono float samples [L] (array or tensor) -> codec frames [T, C] (int64), through the native codec: zeros on the right up
        to a multiple of 512 samples (DAC's preprocess), T = ceil(L / 512).  A rate other than the codec's is resampled by the
        codec's own resampler (resample_to).  normalize_lufs: the waveform is brought to that loudness (under peak_ceiling) at the
        codec's rate before it is encoded; None encodes it at the level it has."""
        codec = self._need_codec()
        w = np.asarray(wave.detach().cpu() if isinstance(wave, torch.Tensor) else wave, dtype=np.float32)
        if w.ndim == 2:
            w = w.mean(axis=0)
        w = resample_to(w.reshape(-1), int(sample_rate), codec.cfg.sample_rate, "the waveform", codec)
        if normalize_lufs is not None:
            w = codec.normalize_loudness(w, codec.cfg.sample_rate, float(normalize_lufs), float(self.peak_ceiling))[0]
        return torch.from_numpy(codec.encode(w)[0].T.copy())

    def load_audio(self, audio_path: str, normalize_lufs: Optional[float] = None) -> torch.Tensor:
        """waveform file -> codec frames [T, C] for ``generate(audio_prompt=...)`` (mono; any sample rate with the native codec,
        which resamples to its 44.1 kHz on the device).  normalize_lufs: as encode_audio (native codec only)."""
        if self.codec is not None and self.codec.has_encoder:
            mono, rate = read_audio_mono(audio_path)
            mono = resample_to(mono, rate, self.codec.cfg.sample_rate, audio_path, self.codec)
            return self.encode_audio(mono, self.codec.cfg.sample_rate, normalize_lufs)
        if normalize_lufs is not None:
            raise RuntimeError("normalize_lufs needs the native codec's loudness meter: call Dia.load_codec(path_or_state) first")
        codec = self.dac_model
        if codec is None:
            raise RuntimeError("DAC model not loaded. Cannot encode audio.")
        try:
            import torchaudio  # type: ignore
            wave, rate = torchaudio.load(audio_path)
        except FileNotFoundError:
            raise FileNotFoundError(f"Audio file not found: {audio_path}")
        except Exception as e:
            raise RuntimeError(f"Error loading or encoding audio file {audio_path}: {e}") from e
        try:
            mono = wave if wave.shape[0] == 1 else wave.mean(dim=0, keepdim=True)
            if rate != DEFAULT_SAMPLE_RATE:
                mono = torchaudio.functional.resample(mono, rate, DEFAULT_SAMPLE_RATE)
            with torch.inference_mode():
                prepared = codec.preprocess(mono.to(self.device)[None], DEFAULT_SAMPLE_RATE)
                frames = codec.encode(prepared)[1]              # (z, codes, latents, ...): the codes
            return frames[0].T.contiguous()
        except Exception as e:
            raise RuntimeError(f"Error loading or encoding audio file {audio_path}: {e}") from e

    def save_audio(self, path: str, audio: np.ndarray, sample_rate: int = DEFAULT_SAMPLE_RATE):
        """waveform -> file; failures are printed, not raised, like every failure behind ``generate``."""
        if audio is None:
            print("Warning: Cannot save None audio.")
            return
        try:
            try:
                import soundfile  # type: ignore
            except ImportError:
                if not str(path).lower().endswith(".wav"):
                    raise
                _save_wav_pcm16(path, audio, sample_rate)
                return
            out = Path(path)
            out.parent.mkdir(parents=True, exist_ok=True)
            samples = np.asarray(audio)
            if samples.dtype.kind in "iu":
                samples = samples.astype(np.float32) / float(np.iinfo(samples.dtype).max)
            soundfile.write(str(out), samples.clip(-1.0, 1.0), sample_rate)
        except Exception as e:
            print(f"Error saving audio to {path}: {e}")


def read_audio_mono(path: str) -> Tuple[np.ndarray, int]:
    """audio file -> (mono float32 samples in [-1, 1), sample rate): torchaudio where it is importable, else ``.wav`` through the
    standard library's wave module (8-bit unsigned, 16 / 24 / 32-bit signed PCM); channels are averaged"""
    if not Path(path).is_file():
        raise FileNotFoundError(f"Audio file not found: {path}")
    try:
        import torchaudio  # type: ignore
    except ImportError:
        torchaudio = None
    if torchaudio is not None:
        wav, rate = torchaudio.load(path)
        return wav.mean(dim=0).to(torch.float32).numpy(), int(rate)
    if not str(path).lower().endswith(".wav"):
        raise RuntimeError(f"Error loading audio file {path}: without torchaudio only .wav files can be read")
    import wave

    with wave.open(str(path), "rb") as f:
        ch, width, rate, n = f.getnchannels(), f.getsampwidth(), f.getframerate(), f.getnframes()
        if f.getcomptype() != "NONE":
            raise RuntimeError(f"Error loading audio file {path}: compression {f.getcomptype()} is not PCM")
        raw = f.readframes(n)
    if width == 1:
        x = (np.frombuffer(raw, dtype=np.uint8).astype(np.float64) - 128.0) / 128.0
    elif width == 2:
        x = np.frombuffer(raw, dtype="<i2").astype(np.float64) / 32768.0
    elif width == 3:
        b = np.frombuffer(raw, dtype=np.uint8).reshape(-1, 3).astype(np.int32)
        x = (((b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)) ^ 0x800000) - 0x800000).astype(np.float64) / 8388608.0
    elif width == 4:
        x = np.frombuffer(raw, dtype="<i4").astype(np.float64) / 2147483648.0
    else:
        raise RuntimeError(f"Error loading audio file {path}: {8 * width}-bit samples are not supported")
    return x.reshape(-1, ch).mean(axis=1).astype(np.float32), int(rate)


def resample_to(mono: np.ndarray, rate: int, want: int, what: str, codec=None) -> np.ndarray:
    """`mono` at `want` Hz: unchanged at that rate; through `codec.resample` where the codec object offers one (DeviceCodec: the
    library's own kernel, the same result with or without torchaudio installed); else through torchaudio.functional.resample
    where torchaudio is importable, and refused by rate otherwise"""
    if int(rate) == int(want):
        return mono
    if codec is not None and hasattr(codec, "resample"):
        return codec.resample(np.ascontiguousarray(mono, dtype=np.float32), int(rate), int(want))
    try:
        import torchaudio  # type: ignore
    except ImportError:
        raise RuntimeError(f"{what} has a sample rate of {rate} Hz; the codec takes {want} Hz and resampling needs torchaudio, "
                           f"which is not installed: resample the audio to {want} Hz first") from None
    return torchaudio.functional.resample(torch.from_numpy(np.ascontiguousarray(mono))[None], int(rate), int(want))[0].numpy()


def _save_wav_pcm16(path: str, audio: np.ndarray, sample_rate: int) -> None:
    """save_audio without soundfile: mono 16-bit PCM through the standard library's wave module"""
    import wave

    out = Path(path)
    out.parent.mkdir(parents=True, exist_ok=True)
    samples = np.asarray(audio)
    if samples.dtype.kind in "iu":
        samples = samples.astype(np.float32) / float(np.iinfo(samples.dtype).max)
    pcm = np.round(samples.reshape(-1).astype(np.float64).clip(-1.0, 1.0) * 32767.0).astype("<i2")
    with wave.open(str(out), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(int(sample_rate))
        f.writeframes(pcm.tobytes())
