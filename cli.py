#!/usr/bin/env python3
"""Command-line front-end on the MI355X decode path — same flags as the reference's cli.py (36-98), same
flow (validate -> seed -> load -> optional adapters -> generate -> save, 100-229).

Differences, all forced by the platform: the device is always the HIP device (there is no CPU path);
``--compute-dtype`` selects the K/V cache dtype (weights are bf16 tiles either way; float32 = parity mode);
LoRA adapters are merged into the dense weights at load (``--adapter-path``, dia_hip/lora.py) instead of wrapped by PEFT, or kept
unmerged beside them and chosen per run / per chunk (``--adapter NAME=DIR`` ... ``--use-adapter NAME``);
``--codes-output`` (build-only) saves the codec input ``[1, 9, T]`` as .npy, which is the only possible
output where neither codec is available; ``--no-dac`` skips loading the third-party one.  ``--codec-path FILE`` (build-only) loads
the native DAC decoder (dia_hip/codec.py) from a DAC checkpoint: ``--output`` then needs no ``dac`` package, also with ``--stream-chunk``.
With a checkpoint that holds the encoder too, ``--audio-prompt voice.wav`` is encoded by the same native codec, and
``--encode-audio IN.wav --codes-output out.npy`` (build-only) writes the file's codes ``[T, 9]`` and exits; no model is loaded.
A prompt file at any sample rate is converted to the codec's 44100 Hz by the native resampler, and ``--output-rate HZ`` (build-only)
converts ``--output`` from 44100 Hz to HZ the same way.  ``--codec-precision {fp32,bf16x2,bf16}`` (build-only, with ``--codec-path``)
picks the decoder's arithmetic: the exact fp32 kernel, or bf16 MFMA operands in two planes / one; encoding stays fp32.
``--score-codes FILE.npy`` (build-only) generates nothing: it prints the teacher-forced log-likelihood of the given codes under
the loaded checkpoint (Dia.score) as one JSON line.
``--compare-audio A.wav B.wav`` (build-only) loads no model and no codec: it prints the multi-scale STFT and log-mel distances between
the two files (dia_hip/spectral.py) as one JSON line, B brought to A's sample rate by the native resampler and the longer cut to the
shorter.  ``--codec-roundtrip IN.wav --codec-path FILE`` (build-only) prints the same JSON for the native codec's reconstruction
(encode -> decode, the decoder in ``--codec-precision``) of the file.  Neither needs the text argument.
``--speed-factor X`` (build-only, with ``--output`` and ``--codec-path``) is the reference application's speed slider on the device
(dia_hip/timescale.py): ``--speed-mode interp`` (default) is its np.interp, ``wsola`` keeps the pitch and is the mode ``--stream-chunk``
takes.  ``--time-scale IN.wav --speed-factor X --output OUT.wav`` stretches a file, loads no model and needs no text argument.
``--loudness LUFS [--peak-ceiling DBTP]`` (build-only, with ``--output`` and ``--codec-path``; not with ``--stream-chunk``) brings the
generated waveform to an ITU-R BS.1770-4 integrated loudness under a true-peak ceiling by one gain on the device (dia_hip/loudness.py),
as the last step.  ``--measure-loudness IN.wav`` prints a file's loudness and peaks as one JSON line; it loads no model either.
"""

from __future__ import annotations

import argparse
import math
import os
import random
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "dia-tts-prune_amd"))


def set_seed(seed: int):
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Dia text-to-dialogue on MI355X: text in, audio (or codec codes) out.")
    p.add_argument("text", type=str, nargs="?", default=None, help="text to synthesise ([S1]/[S2] speaker tags); with --audio-prompt give only the new text here, the prompt transcript goes to --audio-prompt-text")
    p.add_argument("--output", type=str, default=None, help="audio file to write (needs a codec: --codec-path FILE, or the dac package)")
    p.add_argument("--codes-output", type=str, default=None, help="(build-only) path for the codec input codes [1, C, T] as .npy")
    g = p.add_argument_group("Model Loading")
    g.add_argument("--model-path", type=str, default="nari-labs/Dia-1.6B", help="model directory holding config.json and the checkpoint (hub ids cannot be fetched offline)")
    g.add_argument("--config", type=str, default=None, help="config.json to use instead of the one in --model-path")
    g.add_argument("--pruned-checkpoint", type=str, default=None, help="checkpoint file to load instead of the one in --model-path, e.g. an offline_prune.py output")
    g.add_argument("--adapter-path", type=str, default=None, help="LoRA adapter directory; folded into the dense weights while loading")
    g.add_argument("--adapter", action="append", default=[], metavar="NAME=DIR", help="(build-only, repeatable) LoRA adapter directory kept "
                   "UNMERGED beside the base weights under NAME (q_proj / k_proj / v_proj adapters, rank <= 64); chosen per run with "
                   "--use-adapter; not with --adapter-path")
    g.add_argument("--use-adapter", type=str, default=None, metavar="NAME", help="(build-only) generate (or score) with this --adapter; with "
                   "--slots N a comma list with one entry per chunk (an empty entry = the base model) or one name for all chunks")
    g.add_argument("--no-dac", action="store_true", help="(build-only) do not load the audio codec; requires --codes-output")
    g.add_argument("--codec-path", type=str, default=None, metavar="FILE", help="(build-only) DAC checkpoint (.pth / state dict) for the "
                   "native codec: --output is decoded on the device by this library, the third-party dac package is not loaded "
                   "(as with --no-dac), and --stream-chunk N may be combined with --output; a checkpoint that holds the encoder "
                   "also encodes an --audio-prompt file and serves --encode-audio")
    g.add_argument("--codec-precision", type=str, default=None, choices=["fp32", "bf16x2", "bf16"], help="(build-only) precision of the "
                   "native codec's decoder convolutions (needs --codec-path): fp32 (default) is the exact kernel; bf16x2 runs them on the "
                   "bf16 MFMA with two planes per operand (errors near the 16-bit PCM step), bf16 with one (lossy, for previews); the "
                   "encode side stays fp32 in every mode")
    g.add_argument("--encode-audio", type=str, default=None, metavar="IN.wav", help="(build-only) encode this audio file with the native "
                   "codec and write its codes [T, 9] to --codes-output as .npy, then exit: needs --codec-path, loads no model, and the "
                   "text argument is ignored (44.1 kHz; another rate needs torchaudio)")
    g = p.add_argument_group("Audio Prompting (Voice Cloning)")
    g.add_argument("--output-rate", type=int, default=None, metavar="HZ", help="(build-only) sample rate of --output: the waveform is converted "
                   "from the codec's 44100 Hz on the device by the native codec's resampler (needs --codec-path); default: 44100 as it comes")
    g.add_argument("--audio-prompt", type=str, default=None, help="voice to clone: an audio file (encoded by the native codec of --codec-path when its checkpoint holds "
                   "the encoder, else by the dac package) or a .npy of codec codes [T, 9]")
    g.add_argument("--audio-prompt-text", type=str, default=None, help="what is said in --audio-prompt (mandatory with it)")
    g = p.add_argument_group("Generation Parameters")
    g.add_argument("--max-tokens", type=int, default=None, help="cap on generated frames incl. the prompt (default: audio_length of the config)")
    g.add_argument("--cfg-scale", type=float, default=3.0, help="classifier-free guidance strength")
    g.add_argument("--temperature", type=float, default=1.3, help="softmax temperature of the sampler; 0 = greedy")
    g.add_argument("--top-p", type=float, default=0.95, help="nucleus (top-p) mass kept by the sampler")
    g.add_argument("--cfg-filter-top-k", type=int, default=35, help="keep only the k best logits after guidance; 0 switches the filter off")
    g.add_argument("--seed", type=int, default=None, help="seed of the sampling noise")
    g.add_argument("--slots", type=int, default=0, help="N > 0: split the text into chunks (the front-end's chunk plan) and generate them as "
                   "independent utterances sharing N slots of one continuously batched session; needs --codes-output (the chunks' "
                   "codes are joined in order); not with --audio-prompt (a prompt chain is sequential)")
    g.add_argument("--stream-chunk", type=int, default=0, help="N > 0: hand the codes out every N decode steps while the utterance is "
                   "generated (Dia.stream_frames; one slot, or the --slots chunk plan); needs --codes-output, whose file is the one "
                   "written without this flag; frames are appended to <codes-output>.frames (raw int32 [n, C]) as they arrive when "
                   "there is one utterance; not with --audio-prompt or --output")
    g = p.add_argument_group("Scoring")
    g.add_argument("--score-codes", type=str, default=None, help="(build-only) .npy of codec frames [T, 9] or of a delayed token buffer "
                   "[rows, 9]: instead of generating, print the teacher-forced NLL / perplexity of these codes for the text under the "
                   "loaded checkpoint (with --weight-format / --sparse-weights / --compute-dtype as given) as one JSON line; "
                   "--audio-prompt (a .npy) is replayed and not scored; needs a local --model-path")
    g.add_argument("--score-output", type=str, default=None, help="with --score-codes: .npz for the per-position arrays "
                   "(lp_cond, lp_cfg, entropy_cfg, valid)")
    g.add_argument("--calibrate-codes", type=str, nargs="+", default=None, metavar="FILE.npy", help="(build-only) one or more .npy of codec "
                   "frames [T, 9] or delayed token buffers: instead of generating, force them through the loaded checkpoint and write the "
                   "per-channel activation statistics of every prunable kernel's input to --stats-output (Dia.calibrate), what "
                   "offline_prune.py --act-stats takes; the text belongs to every file unless --calibrate-texts is given; needs a local "
                   "--model-path, loaded dense and uncompacted")
    g.add_argument("--calibrate-texts", type=str, default=None, metavar="FILE.txt", help="with --calibrate-codes: one transcript per line, in "
                   "the order of the codes files")
    g.add_argument("--stats-output", type=str, default=None, help="with --calibrate-codes: the .npz the statistics go to; an existing file "
                   "of the same model is merged into (sums and row counts add)")
    g.add_argument("--gram-output", type=str, default=None, metavar="FILE.npz", help="with --calibrate-codes: also accumulate the Gram matrix of every "
                   "decode-step GEMM input (Dia.calibrate(gram=True)) and write them here, what offline_quantize.py --gram-stats takes; an "
                   "existing file of the same model is merged into.  T (T + 1) / 2 * 8 KiB of device memory per tap of T = K / 32 k-tiles")
    g.add_argument("--gram-layers", type=str, default=None, metavar="A:B", help="with --gram-output: only decoder layers A .. B - 1 (index n_layer "
                   "is the logits head), to bound memory; runs over disjoint ranges merge into one file")
    g = p.add_argument_group("Audio distance")
    g.add_argument("--compare-audio", type=str, nargs=2, default=None, metavar=("A.wav", "B.wav"), help="(build-only) print the multi-scale "
                   "STFT and log-mel distances between two audio files as one JSON line, then exit: loads no model; B is resampled to A's "
                   "rate on the device when they differ, and the longer file is cut to the shorter")
    g.add_argument("--codec-roundtrip", type=str, default=None, metavar="IN.wav", help="(build-only) print the same distances between this "
                   "file and its reconstruction by the native codec (encode -> decode, the decoder in --codec-precision) as one JSON "
                   "line, then exit: needs --codec-path with a checkpoint that holds the encoder, loads no model")
    g = p.add_argument_group("Speed factor")
    g.add_argument("--speed-factor", type=float, default=None, metavar="X", help="(build-only) stretch the generated waveform on the device, "
                   "clamped to [0.1, 5], below 1 = slower (the reference application's speed slider): needs --output and --codec-path; "
                   "runs at the codec's rate, before --output-rate")
    g.add_argument("--speed-mode", type=str, default=None, choices=["interp", "wsola"], help="(build-only) interp (default) = the reference's "
                   "np.interp, which moves the pitch with the tempo; wsola = waveform-similarity overlap-add, which keeps the pitch and is "
                   "the only mode --stream-chunk takes")
    g.add_argument("--time-scale", type=str, default=None, metavar="IN.wav", help="(build-only) stretch this audio file by --speed-factor in "
                   "--speed-mode on the device and write it to --output, then exit: loads no model and no codec")
    g = p.add_argument_group("Loudness")
    g.add_argument("--loudness", type=float, default=None, metavar="LUFS", help="(build-only) bring the generated waveform to this integrated "
                   "loudness (ITU-R BS.1770-4) by one gain on the device, lowered where the true peak would cross --peak-ceiling (a pure "
                   "gain, not a limiter): needs --output and --codec-path; runs last, after --speed-factor and --output-rate; not with "
                   "--stream-chunk (the gain depends on the whole utterance)")
    g.add_argument("--peak-ceiling", type=float, default=None, metavar="DBTP", help="(build-only) true-peak ceiling of --loudness in dBTP "
                   "(default -1)")
    g.add_argument("--measure-loudness", type=str, default=None, metavar="IN.wav", help="(build-only) print the integrated loudness (LUFS), "
                   "the true peak (dBTP) and the sample peak (dBFS) of this audio file as one JSON line, then exit: loads no model and "
                   "no codec")
    g = p.add_argument_group("Infrastructure")
    g.add_argument("--device", type=str, default=None, help="HIP device such as cuda:0 (default: the current one)")
    g.add_argument("--compute-dtype", type=str, default="bfloat16", choices=["float16", "bfloat16", "float32"], help="K/V cache dtype: bfloat16 (default; float16 is accepted and mapped to it) or float32.")
    g.add_argument("--fp32-weights", type=str, default="exact", choices=["exact", "bf16x2", "round"],
                   help="compute_dtype float32 with a checkpoint bf16 cannot hold: exact = three bf16 planes (generic kernel), "
                        "bf16x2 = hi + lo bf16 planes (relative error <= 2^-17, tuned kernels), round = one rounded bf16 tile set")
    g.add_argument("--sparse-weights", type=str, default="off", choices=["off", "2:4", "unstructured"],
                   help="2:4 = the checkpoint is 2:4-pruned (offline_prune.py --prune-mode 2:4): batch 1-2 decode steps stream its "
                        "decoder matrices in the compressed 2:4 form (sparse MFMA); unstructured = the checkpoint is unstructured-pruned "
                        "(--prune-mode unstructured): it also carries lossless mask + window streams of those matrices, which batch 1-2 "
                        "steps stream for the classes of the knob usparse (DIA_TUNE=usparse=127: all; default none); off = dense tiles only")
    g.add_argument("--weight-format", type=str, default="bf16", choices=["bf16", "mxfp8", "mxfp4"],
                   help="mxfp8 = the checkpoint is MXFP8-quantised (offline_quantize.py): batch 1-8 decode steps stream its decoder "
                        "matrices as e4m3 elements + block scales (half the weight bytes); mxfp4 = the same for an MXFP4-quantised "
                        "checkpoint (--format mxfp4: e2m1 elements, a quarter of the bytes); bf16 = dense tiles only")
    g.add_argument("--cross-kv", type=str, default="bf16", choices=["bf16", "fp8"],
                   help="(build-only) fp8: the decode step reads an e4m3 copy of the cross-attention K/V caches (one power-of-two scale per "
                        "key and head) instead of the bf16 caches; needs a bf16 --compute-dtype")
    g.add_argument("--prompt-prefill", type=str, default="auto", choices=["auto", "replay", "batched"],
                   help="(build-only) batched: audio prompts of more than one frame are prefilled as one packed batch also at slot admission "
                        "(--slots N) and onto --self-kv fp8 caches; auto: closed bf16 sessions prefill, everything else replays the prompt "
                        "through the decode step; replay: always replay")
    g.add_argument("--self-kv", type=str, default="bf16", choices=["bf16", "fp8"],
                   help="(build-only) fp8: the self-attention K/V caches are kept as e4m3 (one power-of-two scale per key and head, the new "
                        "key quantised as it is appended) instead of bf16: 0.516 of the bytes; needs a bf16 --compute-dtype")
    g.add_argument("--verbose", action="store_true", help="report prefill and generation timing")
    return p


def parse_adapter_flags(parser, args):
    """--adapter NAME=DIR ... / --use-adapter: {name: dir} of the unmerged bank; every conflict goes through parser.error"""
    if (args.adapter or args.use_adapter) and args.adapter_path:
        parser.error("--adapter-path merges ONE adapter into the weights at load; it cannot be combined with --adapter / --use-adapter "
                     "(the unmerged, per-request bank).")
    dirs = {}
    for item in args.adapter:
        name, sep, path = item.partition("=")
        if not sep or not name or not path:
            parser.error(f"--adapter takes NAME=DIR, got {item!r}")
        if name in dirs:
            parser.error(f"--adapter {name!r} is given twice")
        dirs[name] = path
    if args.use_adapter is not None:
        names = args.use_adapter.split(",")
        if len(names) > 1 and not args.slots:
            parser.error("--use-adapter takes a comma list only with --slots N (one entry per chunk).")
        for n_ in names:
            if n_ and n_ not in dirs:
                parser.error(f"--use-adapter {n_!r} is not among the --adapter names {sorted(dirs)}")
    return dirs


def used_adapters(args):
    """--use-adapter as the callers take it: None, or the list of names (an empty entry = the base model)"""
    return None if args.use_adapter is None else [n_ or None for n_ in args.use_adapter.split(",")]


def stream_to_file(dia, args, full_text: str) -> int:
    """--stream-chunk: the text (one utterance in one slot, or the --slots chunk plan) through Dia.stream_frames.  With one
    utterance every chunk is appended to <codes-output>.frames the moment it arrives; at the end the chunks are joined into the
    .npy that the run without --stream-chunk writes, and the .frames file is removed."""
    import time

    kw = dict(cfg_scale=args.cfg_scale, temperature=args.temperature, top_p=args.top_p, cfg_filter_top_k=args.cfg_filter_top_k)
    if args.slots:
        from dia_hip.callers import stream_chunks_codes
        it = stream_chunks_codes(dia, full_text, slots=args.slots, chunk=args.stream_chunk, seed=args.seed, adapter=used_adapters(args),
                                 max_new_tokens=args.max_tokens or dia.config.data.audio_length, **kw)
    else:
        it = dia.stream_frames([full_text], 1, max_tokens=args.max_tokens, seeds=None if args.seed is None else [args.seed],
                               chunk=args.stream_chunk, adapters=used_adapters(args), **kw)
    out = Path(args.codes_output)
    out.parent.mkdir(parents=True, exist_ok=True)
    side = None if args.slots else open(str(out) + ".frames", "wb")
    parts, t0, first = {}, time.time(), None
    try:
        for i, start, codes, final in it:
            now = time.time() - t0
            parts.setdefault(i, []).append(codes)
            if codes.shape[-1]:
                first = now if first is None else first
                if side is not None:
                    side.write(np.ascontiguousarray(codes[0].T).tobytes())
                    side.flush()
            if args.verbose:
                print(f"stream: utterance {i} frames [{start}, {start + codes.shape[-1]}){' final' if final else ''} at {now * 1e3:.1f} ms")
    finally:
        if side is not None:
            side.close()
            os.remove(side.name)
    joined = [np.concatenate(parts[i], axis=-1) for i in sorted(parts)]
    joined = [c for c in joined if c.shape[-1] > 0]
    if not joined:
        print("Generation failed to produce codes.")
        return 1
    codes = np.concatenate(joined, axis=-1)
    np.save(args.codes_output, codes)
    if args.verbose and first is not None:
        print(f"stream: first chunk after {first * 1e3:.1f} ms, {codes.shape[-1]} frames in {time.time() - t0:.3f}s")
    print(f"Codes saved to {args.codes_output}: shape {tuple(codes.shape)}")
    return 0


def stream_audio_to_file(dia, args, full_text: str) -> int:
    """--stream-chunk with --output (needs --codec-path): one utterance through Dia.stream_frames, every chunk decoded as it arrives
    by the native codec's streaming state; the file is written from the chunks' samples (and --codes-output from their codes)"""
    state = dia.codec.stream()
    rate = dia.output_sample_rate or dia.codec.cfg.sample_rate
    to_rate = dia.codec.resample_stream(dia.codec.cfg.sample_rate, rate)       # equal rates: chunks pass through
    to_speed = dia.codec.time_scale_stream(dia.speed_factor)                   # speed 1: chunks pass through
    samples, frames = [], []
    for _, start, codes, final in dia.stream_frames([full_text], 1, max_tokens=args.max_tokens, seeds=None if args.seed is None else [args.seed],
                                                    chunk=args.stream_chunk, adapters=used_adapters(args), cfg_scale=args.cfg_scale,
                                                    temperature=args.temperature, top_p=args.top_p, cfg_filter_top_k=args.cfg_filter_top_k):
        y = to_rate.push(to_speed.push(state.push(codes, final), final), final)
        frames.append(codes)
        samples.append(y)
        if args.verbose:
            print(f"stream: frames [{start}, {start + codes.shape[-1]}) -> {y.shape[0]} samples{' final' if final else ''}")
    audio = np.concatenate(samples) if samples else np.zeros(0, dtype=np.float32)
    if audio.shape[0] == 0:
        print("Generation failed to produce audio.")
        return 1
    if args.codes_output:
        Path(args.codes_output).parent.mkdir(parents=True, exist_ok=True)
        np.save(args.codes_output, np.concatenate(frames, axis=-1))
        print(f"Codes saved to {args.codes_output}")
    Path(args.output).parent.mkdir(parents=True, exist_ok=True)
    print(f"Saving audio to {args.output}...")
    dia.save_audio(args.output, audio, rate)
    print(f"Audio successfully saved to {args.output}")
    return 0


def score_to_stdout(dia, args, text: str, prompt) -> int:
    """--score-codes: Dia.score of the file's codes; the summary as one JSON line, the arrays to --score-output"""
    import json

    res = dia.score(text, np.load(args.score_codes), audio_prompt=prompt, cfg_scale=args.cfg_scale,
                    audio_prompt_text=args.audio_prompt_text, adapter=args.use_adapter)
    print(json.dumps(res.summary()))
    if args.score_output:
        Path(args.score_output).parent.mkdir(parents=True, exist_ok=True)
        np.savez(args.score_output, lp_cond=res.lp_cond, lp_cfg=res.lp_cfg, entropy_cfg=res.entropy_cfg, valid=res.valid)
    return 0


def calibrate_to_file(dia, args, text: str) -> int:
    """--calibrate-codes: Dia.calibrate over the files' codes; the statistics to --stats-output, a summary as one JSON line"""
    import json

    from dia_hip.calib import ActStats, GramStats

    codes = [np.load(f) for f in args.calibrate_codes]
    texts = [text] * len(codes)
    if args.calibrate_texts:
        texts = [ln.strip() for ln in Path(args.calibrate_texts).read_text().splitlines() if ln.strip()]
        if len(texts) != len(codes):
            raise ValueError(f"--calibrate-texts holds {len(texts)} lines for {len(codes)} codes files")
    out = Path(args.stats_output)
    prior = ActStats.load(str(out)) if out.is_file() else None
    summary = {}
    if args.gram_output:
        gout = Path(args.gram_output)
        layers = None
        if args.gram_layers:
            first, _, end = args.gram_layers.partition(":")
            layers = (int(first), int(end))
        stats, grams = dia.calibrate(texts, codes, cfg_scale=args.cfg_scale, stats=prior, gram=True, gram_layers=layers,
                                     gram_stats=GramStats.load(str(gout)) if gout.is_file() else None)
        gout.parent.mkdir(parents=True, exist_ok=True)
        grams.save(str(gout))
        summary = dict(gram_taps=len(grams.taps()), gram_rows_min=min(grams.rows.values()), gram_bytes=int(sum(v.nbytes for v in grams.packed.values())))
    else:
        stats = dia.calibrate(texts, codes, cfg_scale=args.cfg_scale, stats=prior)
    out.parent.mkdir(parents=True, exist_ok=True)
    stats.save(str(out))
    print(json.dumps(dict(files=len(codes), kernels=len(stats.names()), rows_min=min(stats.rows.values()), rows_max=max(stats.rows.values()), **summary)))
    return 0


def encode_to_file(args) -> int:
    """--encode-audio: the file through the native codec alone, codes [T, C] to --codes-output"""
    try:
        from dia_hip.codec import DeviceCodec
        from dia_hip.model import read_audio_mono, resample_to

        device = torch.device(args.device) if args.device else None
        codec = DeviceCodec(args.codec_path, device)
        mono, rate = read_audio_mono(args.encode_audio)
        codes = codec.encode(resample_to(mono, rate, codec.cfg.sample_rate, args.encode_audio, codec))[0].T.copy()
        Path(args.codes_output).parent.mkdir(parents=True, exist_ok=True)
        np.save(args.codes_output, codes)
        print(f"Codes saved to {args.codes_output}: shape {tuple(codes.shape)}")
        return 0
    except Exception as e:
        print(f"Error encoding {args.encode_audio}: {e}")
        import traceback
        traceback.print_exc()
        return 1


def distance_json(res: dict, **head) -> str:
    """one JSON line: the metrics, then the terms of every resolution under string keys"""
    import json

    per = {m: {str(w): t for w, t in r.items()} for m, r in res["per_resolution"].items()}
    return json.dumps({**head, **{k: v for k, v in res.items() if k != "per_resolution"}, "per_resolution": per})


def compare_to_stdout(args) -> int:
    """--compare-audio: two files through the device's spectral kernel; no model, no codec"""
    try:
        from dia_hip.model import read_audio_mono
        from dia_hip.resample import DeviceResampler
        from dia_hip.spectral import DeviceSpectral

        device = torch.device(args.device) if args.device else None
        (a, rate), (b, rate_b) = (read_audio_mono(f) for f in args.compare_audio)
        if rate_b != rate:
            b = DeviceResampler(device).resample(np.ascontiguousarray(b, dtype=np.float32), rate_b, rate)
        res = DeviceSpectral(device).distance(a, b, rate, trim=True)
        print(distance_json(res, sample_rate=rate, samples=int(min(a.shape[0], b.shape[0]))))
        return 0
    except Exception as e:
        print(f"Error comparing {args.compare_audio[0]} and {args.compare_audio[1]}: {e}")
        import traceback
        traceback.print_exc()
        return 1


def loudness_to_stdout(args) -> int:
    """--measure-loudness: the file through the device's loudness meter at its own rate; no model, no codec"""
    try:
        import json

        from dia_hip.loudness import DeviceLoudness
        from dia_hip.model import read_audio_mono

        mono, rate = read_audio_mono(args.measure_loudness)
        r = DeviceLoudness(torch.device(args.device) if args.device else None).measure(np.ascontiguousarray(mono, dtype=np.float32), rate)
        print(json.dumps({"loudness_lufs": r["loudness"], "true_peak_dbtp": r["true_peak"], "sample_peak_dbfs": r["sample_peak"],
                          "sample_rate": int(rate), "samples": int(mono.shape[0])}))
        return 0
    except Exception as e:
        print(f"Error measuring {args.measure_loudness}: {e}")
        import traceback
        traceback.print_exc()
        return 1


def time_scale_to_file(args) -> int:
    """--time-scale: the file through the device's time-scaling kernels at its own rate; no model, no codec"""
    try:
        from dia_hip.model import _save_wav_pcm16, read_audio_mono
        from dia_hip.timescale import DeviceTimescale

        mono, rate = read_audio_mono(args.time_scale)
        y = DeviceTimescale(torch.device(args.device) if args.device else None).time_scale(
            np.ascontiguousarray(mono, dtype=np.float32), args.speed_factor, args.speed_mode or "interp")
        _save_wav_pcm16(args.output, y, rate)
        print(f"{args.time_scale}: {mono.shape[0]} samples -> {y.shape[0]} at {rate} Hz ({args.speed_mode or 'interp'}), saved to {args.output}")
        return 0
    except Exception as e:
        print(f"Error time-scaling {args.time_scale}: {e}")
        import traceback
        traceback.print_exc()
        return 1


def roundtrip_to_stdout(args) -> int:
    """--codec-roundtrip: the file against its reconstruction by the native codec alone"""
    try:
        from dia_hip.codec import DeviceCodec
        from dia_hip.model import read_audio_mono, resample_to

        device = torch.device(args.device) if args.device else None
        codec = DeviceCodec(args.codec_path, device, precision=args.codec_precision or "fp32")
        mono, rate = read_audio_mono(args.codec_roundtrip)
        mono = resample_to(mono, rate, codec.cfg.sample_rate, args.codec_roundtrip, codec)
        print(distance_json(codec.roundtrip_distance(mono), sample_rate=codec.cfg.sample_rate, samples=int(mono.shape[0]),
                            codec_precision=codec.precision))
        return 0
    except Exception as e:
        print(f"Error in the codec round trip of {args.codec_roundtrip}: {e}")
        import traceback
        traceback.print_exc()
        return 1


def main(argv=None) -> int:
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.speed_factor is not None and not math.isfinite(args.speed_factor):
        parser.error("--speed-factor X needs a finite number.")
    if args.speed_mode is not None and args.speed_factor is None:
        parser.error("--speed-mode needs --speed-factor X.")
    if args.peak_ceiling is not None and args.loudness is None:
        parser.error("--peak-ceiling needs --loudness LUFS.")
    if args.measure_loudness:
        if (args.loudness is not None or args.time_scale or args.speed_factor is not None or args.output or args.compare_audio
                or args.codec_roundtrip or args.codes_output or args.score_codes or args.slots or args.stream_chunk or args.audio_prompt
                or args.encode_audio or args.codec_path or args.codec_precision or args.output_rate is not None):
            parser.error("--measure-loudness measures one file: none of --loudness, --time-scale, --speed-factor, --output, "
                         "--compare-audio, --codec-roundtrip, --codes-output, --score-codes, --slots, --stream-chunk, --audio-prompt, "
                         "--encode-audio, --codec-path, --codec-precision or --output-rate.")
        return loudness_to_stdout(args)
    if args.loudness is not None:
        if not math.isfinite(args.loudness) or (args.peak_ceiling is not None and not math.isfinite(args.peak_ceiling)):
            parser.error("--loudness LUFS and --peak-ceiling DBTP need finite numbers.")
        if (not args.output or not args.codec_path or args.time_scale or args.score_codes or args.encode_audio or args.compare_audio
                or args.codec_roundtrip):
            parser.error("--loudness LUFS normalises the generated waveform: it needs --output and --codec-path (the native codec "
                         "runs the meter).")
        if args.stream_chunk:
            parser.error("--loudness cannot be combined with --stream-chunk: the gain depends on the whole utterance.")
    if args.time_scale:
        if args.speed_factor is None or not args.output or not args.output.lower().endswith(".wav"):
            parser.error("--time-scale IN.wav needs --speed-factor X and --output OUT.wav.")
        if (args.compare_audio or args.codec_roundtrip or args.codes_output or args.score_codes or args.slots or args.stream_chunk
                or args.audio_prompt or args.encode_audio or args.codec_path or args.codec_precision or args.output_rate is not None):
            parser.error("--time-scale stretches one file: none of --compare-audio, --codec-roundtrip, --codes-output, --score-codes, "
                         "--slots, --stream-chunk, --audio-prompt, --encode-audio, --codec-path, --codec-precision or --output-rate.")
        return time_scale_to_file(args)
    if args.speed_factor is not None:
        if not args.output or not args.codec_path or args.score_codes or args.encode_audio or args.compare_audio or args.codec_roundtrip:
            parser.error("--speed-factor X stretches the generated waveform: it needs --output and --codec-path (the native codec "
                         "runs the time-scaling).")
        if args.stream_chunk and (args.speed_mode or "interp") != "wsola":
            parser.error("--speed-factor with --stream-chunk needs --speed-mode wsola: interp cannot stream (its positions depend "
                         "on the total length).")
    if args.compare_audio or args.codec_roundtrip:
        if args.compare_audio and args.codec_roundtrip:
            parser.error("--compare-audio and --codec-roundtrip are separate runs.")
        if args.output or args.codes_output or args.score_codes or args.slots or args.stream_chunk or args.audio_prompt or args.encode_audio:
            parser.error("--compare-audio / --codec-roundtrip print distances only: none of --output, --codes-output, --score-codes, "
                         "--slots, --stream-chunk, --audio-prompt or --encode-audio.")
        if args.compare_audio:
            if args.codec_path or args.codec_precision:
                parser.error("--compare-audio loads no codec: not with --codec-path / --codec-precision.")
            return compare_to_stdout(args)
        if not args.codec_path or not Path(args.codec_path).is_file():
            parser.error("--codec-roundtrip needs --codec-path FILE: a DAC checkpoint that holds the encoder.")
        return roundtrip_to_stdout(args)
    if args.text is None:
        parser.error("the following arguments are required: text")
    if args.encode_audio:
        if not args.codec_path or not Path(args.codec_path).is_file():
            parser.error("--encode-audio needs --codec-path FILE: a DAC checkpoint that holds the encoder.")
        if not args.codes_output or args.output or args.score_codes or args.slots or args.stream_chunk or args.audio_prompt:
            parser.error("--encode-audio writes codes only: it needs --codes-output and takes none of --output, --score-codes, "
                         "--slots, --stream-chunk or --audio-prompt.")
        return encode_to_file(args)
    if args.score_codes:
        if not Path(args.model_path).is_dir() and not (args.pruned_checkpoint and args.config):
            parser.error("--score-codes needs --model-path: a local model directory holding config.json and the checkpoint "
                         "(or --pruned-checkpoint with --config).")
        if args.output or args.codes_output or args.slots or args.stream_chunk:
            parser.error("--score-codes generates nothing: not with --output, --codes-output, --slots or --stream-chunk.")
        if args.audio_prompt and not args.audio_prompt.endswith(".npy"):
            parser.error("--score-codes takes --audio-prompt as a .npy of codec codes.")
        args.no_dac = True
    elif args.score_output:
        parser.error("--score-output needs --score-codes.")
    if args.calibrate_codes:
        if not args.stats_output:
            parser.error("--calibrate-codes needs --stats-output FILE.npz.")
        if not Path(args.model_path).is_dir() and not (args.pruned_checkpoint and args.config):
            parser.error("--calibrate-codes needs --model-path: a local model directory holding config.json and the checkpoint "
                         "(or --pruned-checkpoint with --config).")
        if args.score_codes or args.output or args.codes_output or args.slots or args.stream_chunk or args.audio_prompt or args.codec_path:
            parser.error("--calibrate-codes generates nothing: not with --score-codes, --output, --codes-output, --slots, --stream-chunk, "
                         "--audio-prompt or --codec-path.")
        args.no_dac = True
    elif args.stats_output or args.calibrate_texts or args.gram_output:
        parser.error("--stats-output / --calibrate-texts / --gram-output need --calibrate-codes.")
    if args.gram_layers and not args.gram_output:
        parser.error("--gram-layers needs --gram-output.")
    if args.gram_layers and (args.gram_layers.count(":") != 1 or not all(v.isdigit() for v in args.gram_layers.split(":"))):
        parser.error("--gram-layers takes A:B, two layer indices.")
    if args.audio_prompt and not args.audio_prompt_text:
        parser.error("--audio-prompt needs its transcript: pass --audio-prompt-text")
    bank_dirs = parse_adapter_flags(parser, args)
    if args.pruned_checkpoint and not args.config and not Path(args.model_path).is_dir():
        parser.error("--pruned-checkpoint needs --config unless --model-path is a local directory with a config.json")
    if not args.output and not args.codes_output and not args.score_codes and not args.calibrate_codes:
        parser.error("one of --output / --codes-output is required.")
    if args.slots < 0 or (args.slots and (args.audio_prompt or not args.codes_output or args.output)):
        parser.error("--slots N needs N > 0, --codes-output, and neither --audio-prompt nor --output.")
    stream_wav = bool(args.stream_chunk and args.codec_path and args.output and not args.slots and not args.audio_prompt)
    if args.stream_chunk < 0 or (args.stream_chunk and not stream_wav and (args.audio_prompt or not args.codes_output or args.output)):
        parser.error("--stream-chunk N needs N > 0, --codes-output, and neither --audio-prompt nor --output "
                     "(--output is allowed with --codec-path).")
    if args.output_rate is not None and (args.output_rate < 1 or not args.codec_path or not args.output):
        parser.error("--output-rate HZ needs HZ > 0, --output and --codec-path (the native codec converts the rate).")
    if args.codec_precision is not None and not args.codec_path:
        parser.error("--codec-precision belongs to the native codec: it needs --codec-path FILE.")
    if args.no_dac and args.output and not args.codec_path:
        parser.error("--output needs the audio codec; use --codes-output with --no-dac.")
    if args.codec_path:
        if args.score_codes:
            parser.error("--codec-path decodes generated codes: not with --score-codes.")
        if not Path(args.codec_path).is_file():
            parser.error(f"--codec-path {args.codec_path!r} is not a file.")
        args.no_dac = True                                     # the native codec replaces the third-party import

    from dia_hip.model import Dia

    Dia.fp32_weights = args.fp32_weights
    Dia.sparse_weights = args.sparse_weights
    Dia.weight_format = args.weight_format
    Dia.cross_kv = args.cross_kv
    Dia.self_kv = args.self_kv
    Dia.prompt_prefill = args.prompt_prefill
    if args.seed is not None:
        set_seed(args.seed)
        print(f"Using seed: {args.seed}")
    device = torch.device(args.device) if args.device else None
    print("Loading model...")
    try:
        load_dac = not args.no_dac
        if args.pruned_checkpoint:
            cfg_path = args.config or str(Path(args.model_path) / "config.json")
            if not Path(cfg_path).exists():
                parser.error(f"Config file not found in {args.model_path} and --config not provided.")
            print(f"Loading specific checkpoint: {args.pruned_checkpoint}\nUsing config: {cfg_path}")
            dia = Dia.from_local(cfg_path, args.pruned_checkpoint, args.compute_dtype, device, load_dac=load_dac,
                                 adapter_path=args.adapter_path)
        else:
            print(f"Loading model from: {args.model_path}")
            dia = Dia.from_pretrained(args.model_path, args.compute_dtype, device, load_dac=load_dac,
                                      adapter_path=args.adapter_path)
        if args.adapter_path:
            print("LoRA adapters merged successfully.")
        if args.codec_path:
            dia.load_codec(args.codec_path, precision=args.codec_precision or "fp32")
            dia.output_sample_rate = args.output_rate
            if args.speed_factor is not None:
                dia.speed_factor, dia.speed_mode = args.speed_factor, args.speed_mode or "interp"
            if args.loudness is not None:
                dia.loudness_target = args.loudness
                dia.peak_ceiling = -1.0 if args.peak_ceiling is None else args.peak_ceiling
            print(f"Native codec loaded from {args.codec_path}" + (f" ({args.codec_precision} decoder)" if args.codec_precision else ""))
        if bank_dirs:
            dia.load_adapters(bank_dirs)
            print(f"LoRA adapters loaded unmerged: {sorted(bank_dirs)}")
        print("Model loaded successfully.")
    except Exception as e:
        print(f"Error loading model: {e}")
        import traceback
        traceback.print_exc()
        return 1

    full_text = (args.audio_prompt_text.strip() + " " + args.text.strip()) if args.audio_prompt else args.text.strip()   # cli.py:186-190
    prompt = args.audio_prompt
    if prompt and prompt.endswith(".npy"):
        prompt = torch.from_numpy(np.load(prompt).astype(np.int64))
    if args.score_codes:
        try:
            return score_to_stdout(dia, args, args.text.strip(), None if prompt is None else prompt.numpy())
        except Exception as e:
            print(f"Error during scoring: {e}")
            import traceback
            traceback.print_exc()
            return 1
    if args.calibrate_codes:
        try:
            return calibrate_to_file(dia, args, args.text.strip())
        except Exception as e:
            print(f"Error during calibration: {e}")
            import traceback
            traceback.print_exc()
            return 1
    print("Generating audio...")
    if args.stream_chunk:
        try:
            if stream_wav:
                return stream_audio_to_file(dia, args, full_text)
            return stream_to_file(dia, args, full_text)
        except Exception as e:
            print(f"Error during audio generation or saving: {e}")
            import traceback
            traceback.print_exc()
            return 1
    if args.slots:
        try:
            from dia_hip.callers import generate_chunks_codes
            parts = generate_chunks_codes(dia, full_text, slots=args.slots, max_new_tokens=args.max_tokens or dia.config.data.audio_length,
                                          cfg_scale=args.cfg_scale, temperature=args.temperature, top_p=args.top_p,
                                          cfg_filter_top_k=args.cfg_filter_top_k, seed=args.seed, adapter=used_adapters(args))
            if not parts:
                print("Generation failed to produce codes.")
                return 1
            codes = np.concatenate(parts, axis=-1)
            Path(args.codes_output).parent.mkdir(parents=True, exist_ok=True)
            np.save(args.codes_output, codes)
            print(f"Codes of {len(parts)} chunks saved to {args.codes_output}: shape {tuple(codes.shape)}")
            return 0
        except Exception as e:
            print(f"Error during audio generation or saving: {e}")
            import traceback
            traceback.print_exc()
            return 1
    try:
        audio = dia.generate(text=full_text, audio_prompt=prompt, audio_prompt_text=args.audio_prompt_text,
                             max_tokens=args.max_tokens, cfg_scale=args.cfg_scale, temperature=args.temperature,
                             top_p=args.top_p, cfg_filter_top_k=args.cfg_filter_top_k, seed=args.seed, verbose=args.verbose,
                             adapter=args.use_adapter)
        if args.codes_output and dia.last_codes is not None:
            Path(args.codes_output).parent.mkdir(parents=True, exist_ok=True)
            np.save(args.codes_output, dia.last_codes)
            print(f"Codes saved to {args.codes_output}: shape {tuple(dia.last_codes.shape)}")
        if args.output:
            if audio is None:
                print("Generation failed to produce audio.")
                return 1
            Path(args.output).parent.mkdir(parents=True, exist_ok=True)
            print(f"Saving audio to {args.output}...")
            dia.save_audio(args.output, audio, args.output_rate or 44100)
            print(f"Audio successfully saved to {args.output}")
        elif dia.last_codes is None:
            print("Generation failed to produce codes.")
            return 1
        print("Audio generation complete.")
    except Exception as e:
        print(f"Error during audio generation or saving: {e}")
        import traceback
        traceback.print_exc()
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
