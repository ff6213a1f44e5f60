"""The speed factor behind the model on the MI355X (Dia.speed_factor / speed_mode, DESIGN.md "Speed factor"): generate(),
generate_audio_batch() and stream_audio() of the synthetic mid-size model with the synthetic codec against DeviceCodec.time_scale
of the decoded waveform.  Everything here is bitwise; the kernels' accuracy is tests/test_gpu_timescale.py's."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
TEXT = "[S1] Dia is an open weights text to dialogue model."
TEXT_B = "[S2] You get full control over scripts and voices."


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


@pytest.fixture(scope="module")
def plain(dia):
    """what the model returns without a speed factor: the waveform of TEXT and the batch of both texts"""
    assert dia.speed_factor == 1.0 and dia.output_sample_rate is None
    wave = dia.generate(TEXT, max_tokens=30, seed=3)
    codes = dia.last_codes.copy()
    batch = dia.generate_audio_batch([TEXT, TEXT_B], max_tokens=30, seeds=[3, 4])
    return wave, codes, batch


def settings(dia, **kw):
    class _Set:
        def __enter__(self):
            for k, v in kw.items():
                setattr(dia, k, v)

        def __exit__(self, *exc):
            for k in kw:
                delattr(dia, k)                                                # back to the class defaults
    return _Set()


def test_speed_one_changes_nothing(dia, plain):
    wave, codes, batch = plain
    with settings(dia, speed_factor=1.0, speed_mode="wsola"):
        again = dia.generate(TEXT, max_tokens=30, seed=3)
        chunks = list(dia.stream_audio([TEXT], 1, max_tokens=30, seeds=[3], chunk=4))
    print(f"speed 1: {wave.shape[0]} samples, {len(chunks)} chunks")
    assert np.array_equal(again, wave) and np.array_equal(wave, dia.codec.decode(codes))
    assert np.array_equal(np.concatenate([c[2] for c in chunks]), wave)
    assert dia.time_scale(wave, 1.0) is wave


@pytest.mark.parametrize("mode", ["interp", "wsola"])
def test_generate_equals_the_time_scaled_decode(dia, plain, mode):
    wave, codes, batch = plain
    want = dia.codec.time_scale(wave, 0.9, mode)
    with settings(dia, speed_factor=0.9, speed_mode=mode):
        got = dia.generate(TEXT, max_tokens=30, seed=3)
        assert np.array_equal(dia.last_codes, codes)
        with settings(dia, output_sample_rate=24000):
            got24 = dia.generate(TEXT, max_tokens=30, seed=3)
        both = dia.generate_audio_batch([TEXT, TEXT_B], max_tokens=30, seeds=[3, 4])
    print(f"generate {mode}: {wave.shape[0]} samples -> {got.shape[0]} at speed 0.9 -> {got24.shape[0]} at 24 kHz")
    assert wave.shape[0] > 4 * 512 and want.shape == (int(wave.shape[0] / 0.9),) and want.dtype == np.float32
    assert np.array_equal(got, want) and not np.array_equal(got[:wave.shape[0]], wave)
    assert np.array_equal(got, dia.codec.time_scale(dia.codec.decode(codes), 0.9, mode))
    assert np.array_equal(got24, dia.codec.resample(want, 44100, 24000))
    assert np.array_equal(dia.time_scale(wave, 0.9, mode), want)              # the model-free entry, same kernels
    assert len(both) == 2 and np.array_equal(both[0], want) and np.array_equal(both[1], dia.codec.time_scale(batch[1], 0.9, mode))


def test_stream_audio_equals_the_batch(dia, plain):
    wave, codes, batch = plain
    with settings(dia, speed_factor=0.9, speed_mode="wsola"):
        want = dia.generate_audio_batch([TEXT], max_tokens=30, seeds=[3])[0]
        chunks = list(dia.stream_audio([TEXT], 1, max_tokens=30, seeds=[3], chunk=4))
        with settings(dia, output_sample_rate=24000):
            want24 = dia.generate_audio_batch([TEXT], max_tokens=30, seeds=[3])[0]
            chunks24 = list(dia.stream_audio([TEXT], 1, max_tokens=30, seeds=[3], chunk=4))
    print(f"stream wsola: {want.shape[0]} samples in {len(chunks)} chunks of {[c[2].shape[0] for c in chunks]}; at 24 kHz {want24.shape[0]}")
    for ch, w in ((chunks, want), (chunks24, want24)):
        assert [c[3] for c in ch] == [False] * (len(ch) - 1) + [True] and len(ch) >= 4
        assert [c[1] for c in ch] == list(np.cumsum([0] + [c[2].shape[0] for c in ch[:-1]]))         # offsets count delivered samples
        assert np.array_equal(np.concatenate([c[2] for c in ch]), w)
    assert np.array_equal(want, dia.codec.time_scale(wave, 0.9, "wsola"))
    with settings(dia, speed_factor=0.9, speed_mode="interp"):
        with pytest.raises(ValueError, match="cannot stream"):
            dia.stream_audio([TEXT], 1, max_tokens=30, seeds=[3], chunk=4)
