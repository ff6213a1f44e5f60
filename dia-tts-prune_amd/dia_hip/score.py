"""Host side of teacher-forced scoring (DESIGN.md "Scoring"): which token rows to force, which positions count, and the
reduction of the device's per-position scores to NLL / perplexity.  Pure NumPy: nothing here touches the GPU.

The device writes, per row t and channel c of the token buffer, ``(lp_cond, lp_cfg, H_cfg)`` for the token that row holds
(csrc/score.hip); NaN marks a position no step scored (row 0, audio-prompt rows, rows behind the buffer).
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from .config import DiaConfig
from .tokens import delayed_prefill


def teacher_rows(cfg: DiaConfig, codes, delayed: Optional[bool] = None, prompt=None) -> np.ndarray:
    """The token rows a scoring session forces, int32 [rows, C].

    ``codes`` is either codec frames [T, C] (ids in [0, 1024)): they go through ``tokens.delayed_prefill`` — BOS row, the frames,
    max_delay PAD rows, delay pattern applied, rows = 1 + T + max_delay — behind the frames of the audio ``prompt`` [Tp, C] if
    there is one; or a delayed buffer [rows, C] as a decode leaves it (``UtteranceResult.tokens`` cut to its rows), which is
    taken as is, prompt rows included.  ``delayed=None`` tells them apart by row 0: a delayed buffer starts with a row of BOS,
    which no codec frame contains."""
    da = cfg.data
    a = np.asarray(codes)
    if a.ndim == 3 and a.shape[0] == 1:
        a = a[0]
    if a.ndim != 2 or a.shape[1] != da.channels or a.shape[0] < 1:
        raise ValueError(f"Unexpected codes shape: {np.asarray(codes).shape}. Expected [T, {da.channels}] (T >= 1).")
    if not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"codes must be integers, got {a.dtype}")
    if delayed is None:
        delayed = bool((a[0] == da.audio_bos_value).all())
    if delayed:
        if a.shape[0] < 2:
            raise ValueError("a delayed buffer needs the BOS row and at least one row to score")
        return np.ascontiguousarray(a, dtype=np.int32)
    if prompt is not None:
        a = np.concatenate([np.asarray(prompt).reshape(-1, da.channels).astype(a.dtype), a], axis=0)
    return delayed_prefill(cfg, a)[0]


def valid_mask(tokens, first_step, dims) -> np.ndarray:
    """bool [..., rows, C]: the positions whose score counts — the target is a code in [0, eos), or EOS on channel 0, at a row
    >= first_step.  BOS, PAD, EOS on the delayed channels (the sampler's constraints make them impossible) and the -1 fill
    behind a buffer never count.  ``tokens`` [rows, C] with an int first_step, or [B, rows, C] with one per utterance;
    ``dims`` anything with eos (``oracle.Dims``) or audio_eos_value (``cfg.data``)."""
    tok = np.asarray(tokens)
    eos = int(dims.eos if hasattr(dims, "eos") else dims.audio_eos_value)
    ok = (tok >= 0) & (tok < eos)
    ok[..., 0] |= tok[..., 0] == eos
    rows = np.arange(tok.shape[-2])
    fs = np.asarray(first_step).reshape(tok.shape[:-2] + (1,))
    return ok & (rows >= fs)[..., None]


@dataclass
class ScoreResult:
    """Scores of one utterance, nats.  The arrays are per position [rows, C]; NaN where nothing was scored."""
    lp_cond: np.ndarray            # log p(target) of the conditional row, no guidance, no constraints
    lp_cfg: np.ndarray             # log p(target) under guidance + the sampler's constraints
    entropy_cfg: np.ndarray        # entropy of that guided distribution
    valid: np.ndarray              # bool: the positions the summary below averages over
    n_valid: int
    nll_cond: float                # -mean lp_cond over valid positions
    nll_cfg: float
    mean_entropy_cfg: float
    perplexity_cfg: float          # exp(nll_cfg)
    nll_cond_per_channel: np.ndarray   # [C]; NaN for a channel without a valid position
    nll_cfg_per_channel: np.ndarray

    def summary(self) -> dict:
        """the scalars, JSON-serialisable"""
        return dict(n_valid=self.n_valid, nll_cond=self.nll_cond, nll_cfg=self.nll_cfg, mean_entropy_cfg=self.mean_entropy_cfg,
                    perplexity_cfg=self.perplexity_cfg, nll_cond_per_channel=[float(v) for v in self.nll_cond_per_channel],
                    nll_cfg_per_channel=[float(v) for v in self.nll_cfg_per_channel])


def _masked_mean(x: np.ndarray, m: np.ndarray, axis=None):
    """mean of x where m, in float64; NaN where nothing is selected.  Values at unselected positions (NaN, -inf) never enter;
    a selected -inf or NaN propagates."""
    n = m.sum(axis=axis)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(m, x.astype(np.float64), 0.0).sum(axis=axis) / np.where(n > 0, n, np.nan)


def summarise(scores, valid) -> ScoreResult:
    """``scores`` [rows, C, 3] as the device wrote them, ``valid`` bool [rows, C] (``valid_mask``) -> ScoreResult.
    Invalid positions may hold anything.  A valid position is averaged as it is: a valid target of probability 0 makes the
    NLL +inf, and one that no step scored (NaN) makes it NaN — findings, not something to average away."""
    s = np.asarray(scores)
    m = np.asarray(valid, dtype=bool)
    if s.ndim != 3 or s.shape[-1] != 3 or m.shape != s.shape[:2]:
        raise ValueError(f"summarise: scores {s.shape} must be [rows, C, 3] and valid {m.shape} [rows, C]")
    nll_cond, nll_cfg, ent = (float(v) for v in (-_masked_mean(s[..., 0], m), -_masked_mean(s[..., 1], m), _masked_mean(s[..., 2], m)))
    with np.errstate(over="ignore"):
        ppl = float(np.exp(nll_cfg))
    return ScoreResult(lp_cond=s[..., 0], lp_cfg=s[..., 1], entropy_cfg=s[..., 2], valid=m, n_valid=int(m.sum()),
                       nll_cond=nll_cond, nll_cfg=nll_cfg, mean_entropy_cfg=ent, perplexity_cfg=ppl,
                       nll_cond_per_channel=-_masked_mean(s[..., 0], m, axis=0), nll_cfg_per_channel=-_masked_mean(s[..., 1], m, axis=0))


def check_prompt_rows(cfg: DiaConfig, rows: np.ndarray, prompt) -> int:
    """first_step of a scoring run with an audio prompt [Tp, C]: 1 + Tp, after checking that the forced rows below it are the
    prompt's (those rows depend on the prompt alone: ``out[t, c] = in[t - d_c, c]``)."""
    pre, fs = delayed_prefill(cfg, np.asarray(prompt))
    if fs >= rows.shape[0]:
        raise ValueError(f"audio prompt of {fs - 1} frames leaves nothing to score in {rows.shape[0]} rows")
    if not np.array_equal(rows[:fs], pre[:fs]):
        raise ValueError("the codes do not start with the audio prompt's frames")
    return int(fs)
