"""The resampler on the MI355X (csrc/resample.hip: dia_resample; dia_hip/resample.py: DeviceResampler, ResampleStream; DESIGN.md
"Resampler") against the float64 compact form of tests/resample_ref.py.

Bound, derived and not measured: the device evaluates sum_k f32(f[p][k]) * x_k as an fp32 fma chain of nt terms.  Rounding a
coefficient costs at most u |f x| per term (u = 2^-24), the chain at most nt u sum_k |f x| to first order (the standard forward
bound of a recursive dot product), so every output must lie within (nt + 2) u sum_k |f[p][k] x_k| of the float64 result, plus 1e-30
for sums that are exactly zero.  Everything else here is bitwise: masking, batch rows, chunked streams.  Every test prints its
figures before it asserts."""
import os
import sys
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import resample_ref as R
from dia_hip import resample as S

DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def dev():
    return S.DeviceResampler(DEV)


@pytest.mark.parametrize("rate_in,rate_out", R.GPU_PAIRS)
def test_against_float64(dev, rate_in, rate_out):
    plan = S.resample_plan(rate_in, rate_out)
    worst = 0.0
    for L in sorted({1, plan.o - 1, plan.o + 1, 3001}):
        x = R.noise(L, seed=100 + L)
        y = dev.resample(x, rate_in, rate_out)
        ref, scale = R.resample_compact(x, plan.o, plan.n, plan.nt, plan.first, plan.bank)
        assert y.dtype == np.float32 and y.shape == ref.shape == (plan.out_len(L),)
        if L == 0:
            continue
        assert (x == 1.0).any() and (L == 1 or (x == -1.0).any())
        bound = (plan.nt + 2) * 2.0 ** -24 * scale + 1e-30
        err = np.abs(y.astype(np.float64) - ref)
        ratio = float((err / bound).max())
        worst = max(worst, ratio)
        print(f"resample-accuracy {rate_in}->{rate_out} L {L}: {y.shape[0]} outputs, max err {err.max():.3e}, largest err / bound {ratio:.3f}")
        assert np.all(np.isfinite(y)) and np.all(err <= bound), (L, ratio)
    print(f"resample-accuracy {rate_in}->{rate_out}: largest err / bound over the lengths {worst:.3f}")


@pytest.mark.parametrize("rate_in,rate_out", [(48000, 44100), (44100, 16000), (16000, 44100)])
def test_nan_beyond_a_rows_length_is_never_read(dev, rate_in, rate_out):
    plan = S.resample_plan(rate_in, rate_out)
    lengths = [3001, 1, plan.o + 1, 1500, 0]
    clean = np.zeros((len(lengths), 3001 + 64), dtype=np.float32)
    for b, L in enumerate(lengths):
        clean[b, :L] = R.noise(L, seed=7 + b)
    dirty = clean.copy()
    for b, L in enumerate(lengths):
        dirty[b, L:] = np.nan
    a = dev.resample_padded(dirty, lengths, rate_in, rate_out)
    z = dev.resample_padded(clean, lengths, rate_in, rate_out)
    for b, L in enumerate(lengths):
        assert a[b].shape == (plan.out_len(L),) and np.all(np.isfinite(a[b])) and np.array_equal(a[b], z[b]), (b, L)


@pytest.mark.parametrize("rate_in,rate_out", [(48000, 44100), (44100, 16000), (22050, 44100)])
def test_ragged_batch_rows_equal_solo_runs(dev, rate_in, rate_out):
    plan = S.resample_plan(rate_in, rate_out)
    rows = [R.noise(L, seed=40 + L) for L in (3001, plan.o + 1, 1, 2049)]     # more than one tile, and rows that end inside the first
    together = dev.resample(rows, rate_in, rate_out)
    assert isinstance(together, list) and len(together) == 4
    for b, r in enumerate(rows):
        solo = dev.resample(r, rate_in, rate_out)
        assert solo.shape == (plan.out_len(r.shape[0]),) and np.array_equal(together[b], solo), b


@pytest.mark.parametrize("chunks", sorted(R.CHUNKS))
@pytest.mark.parametrize("rate_in,rate_out", [(48000, 44100), (44100, 16000)])
def test_stream_joined_equals_the_whole_signal_bitwise(dev, rate_in, rate_out, chunks):
    plan = S.resample_plan(rate_in, rate_out)
    L = 1300 if chunks == "1" else 3001
    x = R.noise(L, seed=9)
    whole = dev.resample(x, rate_in, rate_out)
    st = dev.stream(rate_in, rate_out)
    size, at, i, parts = R.CHUNKS[chunks], 0, 0, []
    while True:
        c = min(size(i), L - at)
        final = at + c >= L
        parts.append(st.push(x[at:at + c], final))
        at, i = at + c, i + 1
        if final:
            break
    joined = np.concatenate(parts)
    tail = parts[-1].shape[0]
    print(f"resample-stream {rate_in}->{rate_out} chunks {chunks}: {i} pushes, {joined.shape[0]} outputs, {tail} released by the final push")
    assert tail > 0 and joined.dtype == np.float32                             # the tail waits for `final`
    assert joined.shape == whole.shape == (plan.out_len(L),) and np.array_equal(joined, whole)


def test_wrapper_refuses_a_window_that_misses_a_sample(dev):
    plan = S.resample_plan(48000, 44100)
    buf = np.zeros((1, 600), dtype=np.float32)
    with pytest.raises(ValueError, match="read input samples"):
        dev.run_rows(plan, buf, [0], [600], [0], [S.ready_outputs(plan, 600) + 1], [None])


# ---------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def dia():
    from codec_enc_ref import whole_state
    from dia_hip import codec as K
    from dia_hip import config as C
    from dia_hip.model import Dia
    from dia_hip.weights import synthetic_state_dict
    cfg = C.mid_config()
    d = Dia.from_state_dict(cfg, synthetic_state_dict(cfg, seed=1234, std=0.02), "float32", DEV)
    d.load_codec(whole_state(K.mini_config(), 7), window=16)
    return d


def test_load_audio_of_a_22050_hz_file(dia, tmp_path, monkeypatch):
    from codec_enc_ref import make_wave
    monkeypatch.setitem(sys.modules, "torchaudio", None)                       # the wave module reads the file
    assert dia.codec.has_encoder
    pcm = np.round(make_wave(3 * 512 + 200, seed=5).astype(np.float64).clip(-1, 1) * 32767.0).astype("<i2")
    path = tmp_path / "voice.wav"
    with wave.open(str(path), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(22050)
        f.writeframes(pcm.tobytes())
    mono = (pcm.astype(np.float64) / 32768.0).astype(np.float32)
    up = dia.codec.resample(mono, 22050, 44100)
    assert up.shape == (2 * mono.shape[0],)
    want = dia.codec.encode(up)[0].T
    frames = dia.load_audio(str(path))
    assert tuple(frames.shape) == (-(-up.shape[0] // 512), 9) == (7, 9) and np.array_equal(frames.numpy(), want)
    assert np.array_equal(dia.encode_audio(mono, sample_rate=22050).numpy(), want)
    assert np.array_equal(dia.codec.encode_batch([mono, up], sample_rates=[22050, None])[0], want.T)


def test_stream_audio_at_16_khz_equals_the_resampled_whole(dia):
    text = "[S1] Dia is an open weights text to dialogue model."
    try:
        dia.output_sample_rate = None
        wave44 = dia.generate(text, max_tokens=30, seed=3)
        want = dia.codec.resample(wave44, 44100, 16000)
        dia.output_sample_rate = 16000
        chunks = list(dia.stream_audio([text], 1, max_tokens=30, seeds=[3], chunk=4))
        audio = dia.generate(text, max_tokens=30, seed=3)
        batch = dia.generate_audio_batch([text], max_tokens=30, seeds=[3])[0]
    finally:
        dia.output_sample_rate = None
    n = -(-wave44.shape[0] * 160 // 441)
    print(f"resample-end-to-end: {wave44.shape[0]} samples at 44100 Hz -> {n} at 16000 Hz in {len(chunks)} chunks")
    assert wave44.shape[0] > 4 * 512 and want.shape == (n,)
    assert [c[3] for c in chunks] == [False] * (len(chunks) - 1) + [True] and len(chunks) >= 4
    assert [c[1] for c in chunks] == list(np.cumsum([0] + [c[2].shape[0] for c in chunks[:-1]]))      # offsets count 16 kHz samples
    assert np.array_equal(np.concatenate([c[2] for c in chunks]), want)
    assert np.array_equal(audio, want) and np.array_equal(batch, want)
