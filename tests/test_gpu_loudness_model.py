"""Loudness normalisation behind the model on the MI355X (Dia.loudness_target / peak_ceiling, DESIGN.md "Loudness"): generate() and
generate_audio_batch() of the synthetic mid-size model with the synthetic codec against DeviceCodec.normalize_loudness of what they
return without a target, and the prompt side.  Everything here is bitwise; the kernels' accuracy is tests/test_gpu_loudness.py's."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
TEXT = "[S1] Dia is an open weights text to dialogue model."
TEXT_B = "[S2] You get full control over scripts and voices."
KW = dict(max_tokens=60)                                                       # more than one 400 ms block at either output rate


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


def settings(dia, **kw):
    class _Set:
        def __enter__(self):
            for k, v in kw.items():
                setattr(dia, k, v)

        def __exit__(self, *exc):
            for k in kw:
                delattr(dia, k)                                                # back to the class defaults
    return _Set()


def target_for(dia, wave, rate):
    """a target 6 LU above what the waveform measures: the synthetic codec's level is whatever its random weights give"""
    m = dia.codec.measure_loudness(wave, rate)
    assert math.isfinite(m["loudness"]), (wave.shape, m)
    return m, m["loudness"] + 6.0


@pytest.mark.parametrize("rate,speed", [(None, 1.0), (24000, 0.9)])
def test_generate_equals_normalize_of_the_plain_output(dia, rate, speed):
    assert dia.loudness_target is None and dia.peak_ceiling == -1.0
    with settings(dia, output_sample_rate=rate, speed_factor=speed, speed_mode="wsola"):
        plain = dia.generate(TEXT, seed=3, **KW)
        batch = dia.generate_audio_batch([TEXT, TEXT_B], seeds=[3, 4], **KW)
        at = rate or dia.codec.cfg.sample_rate
        m, target = target_for(dia, plain, at)
        ceiling = m["true_peak"] + 3.0                                         # 6 LU up would cross it: the limited branch
        for tgt, peak, limited in ((target, m["true_peak"] + 60.0, False), (target, ceiling, True)):
            want, rep = dia.codec.normalize_loudness(plain, at, tgt, peak)
            wants = dia.codec.normalize_loudness(batch, at, tgt, peak)[0]
            with settings(dia, loudness_target=tgt, peak_ceiling=peak):
                got = dia.generate(TEXT, seed=3, **KW)
                both = dia.generate_audio_batch([TEXT, TEXT_B], seeds=[3, 4], **KW)
            print(f"rate {at}, speed {speed}: {plain.shape[0]} samples at {m['loudness']:.3f} LUFS, true peak {m['true_peak']:.3f} dBTP -> "
                  f"gain {rep['gain_db']:.3f} dB, limited {rep['limited']}")
            assert rep["limited"] == limited and got.dtype == np.float32
            assert np.array_equal(got, want) and not np.array_equal(got, plain)
            assert len(both) == 2 and all(np.array_equal(a, b) for a, b in zip(both, wants))
            after = dia.measure_loudness(got, at)                              # the model-free entry, same kernels
            if limited:
                assert abs(after["true_peak"] - peak) <= 1e-3
            else:
                assert abs(after["loudness"] - tgt) <= 1e-3


def test_no_target_is_the_parents_path(dia):
    meter, dia.codec._loudness = dia.codec._loudness, None
    try:
        plain = dia.generate(TEXT, seed=3, **KW)
        codes = dia.last_codes.copy()
        assert np.array_equal(plain, dia.codec.decode(codes))
        with settings(dia, loudness_target=None, peak_ceiling=-3.0):
            again = dia.generate(TEXT, seed=3, **KW)
            chunks = list(dia.stream_audio([TEXT], 1, seeds=[3], chunk=4, **KW))
        assert np.array_equal(again, plain) and np.array_equal(np.concatenate([c[2] for c in chunks]), plain)
        assert dia.codec._loudness is None                                     # nothing new was constructed
    finally:
        dia.codec._loudness = meter


def test_stream_audio_refuses_a_target_before_any_session_opens(dia):
    opened = []
    orig = dia.stream_frames
    dia.stream_frames = lambda *a, **k: opened.append(1) or orig(*a, **k)
    try:
        with settings(dia, loudness_target=-23.0):
            with pytest.raises(ValueError, match="loudness_target cannot stream"):
                dia.stream_audio([TEXT], 1, seeds=[3], chunk=4, **KW)
    finally:
        del dia.stream_frames
    assert opened == []


def test_encode_audio_normalises_the_prompt_first(dia):
    if not dia.codec.has_encoder:
        pytest.fail("the synthetic codec state holds the encoder")
    g = np.random.default_rng(9)
    t = np.arange(24000, dtype=np.float64)
    wave = (0.05 * np.sin(2 * np.pi * 220.0 * t / 24000.0) + 0.01 * g.standard_normal(24000)).astype(np.float32)        # 1 s at 24 kHz
    at44 = dia.codec.resample(wave, 24000, 44100)
    norm, rep = dia.codec.normalize_loudness(at44, 44100, -23.0, dia.peak_ceiling)
    assert math.isfinite(rep["loudness"]) and abs(rep["gain_db"]) > 1.0
    got = dia.encode_audio(wave, 24000, normalize_lufs=-23)
    assert torch.equal(got, dia.encode_audio(norm, 44100))
    assert torch.equal(dia.encode_audio(wave, 24000), dia.encode_audio(at44, 44100))                                   # the default: as before
