"""Host-side callers above ``Dia.generate``: the text chunking of the reference's
Gradio front-end and its chunk chaining, where every batch of chunks is generated with the previous
batch as the audio prompt (reference app.py:79-122 helpers, app.py:200-248 loop).

The reference chains through a WAV file (decode -> write -> ``load_audio`` -> encode).  Here the chain
carries the *codes*: the codec input of batch i, transposed to [T, C], is the prompt of batch i+1 — the
same information without the codec round trip, so it also works offline where no codec exists.  Audio is
produced at the end if (and only if) a codec is loaded.
"""

from __future__ import annotations

from typing import Iterable, Iterator, List, Optional, Sequence

import numpy as np

DEFAULT_SAMPLE_RATE = 44100


def count_effective_length(text: str) -> int:
    """length with ``[S1]`` / ``[S2]`` counted as one character each (app.py:79-81)"""
    return len(text.replace("[S1]", "¤").replace("[S2]", "¤"))


def auto_adjust_chunk_size(text: str, user_chunk_size: int) -> int:
    """a positive user value wins; otherwise 48 / 64 / 96 effective characters by input size (app.py:83-97)"""
    if user_chunk_size > 0:
        return int(user_chunk_size)
    n = count_effective_length(text)
    return 48 if n <= 1024 else (64 if n <= 4096 else 96)


def split_by_words_respecting_special_tokens(text: str, max_effective_chars: int = 64) -> List[str]:
    """greedy word packing up to ``max_effective_chars`` effective characters; a single over-long word
    becomes its own chunk (app.py:100-122)"""
    chunks: List[str] = []
    cur = ""
    for word in text.split():
        cand = f"{cur} {word}".strip() if cur else word
        if count_effective_length(cand) > max_effective_chars:
            if cur:
                chunks.append(cur.strip())
                cur = word
            else:
                chunks.append(word)
                cur = ""
        else:
            cur = cand
    if cur:
        chunks.append(cur.strip())
    return chunks


def batch_chunks(chunks: Sequence[str], batch_size: int) -> Iterator[Sequence[str]]:
    for i in range(0, len(chunks), batch_size):            # app.py:124-127
        yield chunks[i: i + batch_size]


def plan_batches(text: str, chunk_size: int = 0, max_new_tokens: int = 3072, batch_size: int = 4):
    """[(batch text, max_tokens)] exactly as the front-end schedules them (app.py:198-218): chunks joined by
    newlines, token budget scaled by the batch's effective length, never below 256."""
    cs = auto_adjust_chunk_size(text, chunk_size)
    chunks = split_by_words_respecting_special_tokens(text, max_effective_chars=cs)
    plan = []
    for batch in batch_chunks(chunks, batch_size):
        bt = "\n".join(c.strip() for c in batch).strip()
        if not bt:
            raise ValueError("All chunks in this batch were empty after trimming.")
        plan.append((bt, max(256, int(max_new_tokens * (count_effective_length(bt) / cs)))))
    return plan


def generate_long_codes(dia, text: str, *, chunk_size: int = 0, max_new_tokens: int = 3072, cfg_scale: float = 3.0,
                        temperature: float = 1.3, top_p: float = 0.95, cfg_filter_top_k: int = 35,
                        audio_prompt: Optional[np.ndarray] = None, audio_prompt_text: Optional[str] = None,
                        seed: Optional[int] = None, verbose: bool = False) -> List[np.ndarray]:
    """Chunk chaining on codes: one [1, C, T'] codec input per batch of chunks; batch i+1 is prompted with the
    codes and text of batch i (app.py:220-244)."""
    if not text or text.isspace():
        raise ValueError("Text input cannot be empty.")
    if audio_prompt is not None and (not audio_prompt_text or audio_prompt_text.isspace()):
        raise ValueError("Audio Prompt Text input cannot be empty.")
    T_cap = dia.config.data.audio_length
    prompt, ptext = audio_prompt, audio_prompt_text
    out: List[np.ndarray] = []
    for i, (bt, budget) in enumerate(plan_batches(text, chunk_size, max_new_tokens)):
        n_prompt = 0 if prompt is None else int(np.asarray(prompt).reshape(-1, dia.config.data.channels).shape[0])
        # The front-end hands its "max new tokens" budget straight to generate(max_tokens=...), where the
        # prompt rows count too, so a chained batch would be left with budget - prompt frames (none, typically).
        # That loop never ran in the reference (its audio-prompt prefill raises); here the
        # budget means NEW frames, as its name says: rows = BOS + prompt + budget, capped by the buffer.
        mt = min(T_cap, n_prompt + 1 + budget)
        codes = dia.generate_batch([bt], max_tokens=mt, cfg_scale=cfg_scale, temperature=temperature, top_p=top_p,
                                   cfg_filter_top_k=cfg_filter_top_k, seeds=None if seed is None else [seed + i],
                                   verbose=verbose, audio_prompts=[prompt], audio_prompt_texts=[ptext])[0]
        if codes.shape[-1] == 0:
            continue
        out.append(codes)
        prompt, ptext = np.ascontiguousarray(codes[0].T), bt          # next prompt = this batch (codes [T, C])
    return out


def _plan_adapters(adapter, n: int):
    """adapter= of the chunk-plan callers: None, one name for every chunk, or one entry per chunk (None = the base model)"""
    if adapter is None or isinstance(adapter, (str, int)):
        return None if adapter is None else [adapter] * n
    names = list(adapter)
    if len(names) == 1:
        names = names * n
    if len(names) != n:
        raise ValueError(f"{len(names)} adapters for a plan of {n} chunks")
    return names


def generate_chunks_codes(dia, text: str, *, slots: int = 8, chunk_size: int = 0, max_new_tokens: int = 3072, cfg_scale: float = 3.0,
                          temperature: float = 1.3, top_p: float = 0.95, cfg_filter_top_k: int = 35,
                          seed: Optional[int] = None, adapter=None) -> List[np.ndarray]:
    """The same chunk plan WITHOUT the chain: every batch of chunks is an independent utterance (no prompt), so they share
    `slots` slots of one continuously batched session (Dia.generate_batch(slots=N)) instead of running one after the other.
    A chain stays sequential (generate_long_codes): batch i + 1 needs the codes of batch i."""
    if not text or text.isspace():
        raise ValueError("Text input cannot be empty.")
    plan = plan_batches(text, chunk_size, max_new_tokens)
    T_cap = dia.config.data.audio_length
    out = dia.generate_batch([bt for bt, _ in plan], max_tokens=[min(T_cap, 1 + budget) for _, budget in plan], cfg_scale=cfg_scale,
                             temperature=temperature, top_p=top_p, cfg_filter_top_k=cfg_filter_top_k,
                             seeds=None if seed is None else [seed + i for i in range(len(plan))], slots=slots,
                             adapters=_plan_adapters(adapter, len(plan)))
    return [c for c in out if c.shape[-1] > 0]


def stream_chunks_codes(dia, text: str, *, slots: int = 8, chunk: int = 16, chunk_size: int = 0, max_new_tokens: int = 3072,
                        cfg_scale: float = 3.0, temperature: float = 1.3, top_p: float = 0.95, cfg_filter_top_k: int = 35,
                        seed: Optional[int] = None, adapter=None):
    """generate_chunks_codes through Dia.stream_frames: the same plan, seeds and slots, but the frames of every batch of the plan
    arrive while it is generated — yields (plan index, start frame, codes [1, C, n], final).  Joining each batch's chunks and
    dropping the empty batches gives the list generate_chunks_codes returns."""
    if not text or text.isspace():
        raise ValueError("Text input cannot be empty.")
    plan = plan_batches(text, chunk_size, max_new_tokens)
    T_cap = dia.config.data.audio_length
    yield from dia.stream_frames([bt for bt, _ in plan], slots, max_tokens=[min(T_cap, 1 + budget) for _, budget in plan],
                                 cfg_scale=cfg_scale, temperature=temperature, top_p=top_p, cfg_filter_top_k=cfg_filter_top_k,
                                 seeds=None if seed is None else [seed + i for i in range(len(plan))], chunk=chunk,
                                 adapters=_plan_adapters(adapter, len(plan)))


def generate_long(dia, text: str, **kw) -> Optional[np.ndarray]:
    """as the front-end: decode every batch, join with 0.2 s of silence (app.py:238-250).  Needs the codec.  With
    dia.loudness_target set the JOINED waveform is normalised, once: one gain for the whole text, the silence included."""
    segs: List[np.ndarray] = []
    target = dia._loudness(dia.codec) if getattr(dia, "loudness_target", None) is not None else None
    parts = generate_long_codes(dia, text, **kw)
    for i, codes in enumerate(parts):
        segs.append(dia._generate_output(codes) if target is None else dia._generate_output(codes, normalize=False))
        if i + 1 < len(parts):
            segs.append(np.zeros(int(DEFAULT_SAMPLE_RATE * 0.2), dtype=np.float32))
    if not segs:
        return None
    wave = np.concatenate(segs)
    if target is not None:
        rate = dia._output_rate(dia.codec) or dia.codec.cfg.sample_rate
        wave = dia.codec.normalize_loudness(wave, rate, target, float(dia.peak_ceiling))[0]
    return wave
