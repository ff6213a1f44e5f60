"""The audio distance off the GPU (dia_hip/spectral.py, include/dia_hip.h: dia_spectral; DESIGN.md "Audio distance"): the plan's
basis and filterbank against their formulas, the float64 reference of tests/spectral_ref.py against torch.stft and an analytic
case, the C ABI's refusals, and the host's length rules."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import spectral_ref as R
from dia_hip import binding as hb
from dia_hip import spectral as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOWS = (32, 64, 128, 256, 512, 1024, 2048)


@pytest.mark.parametrize("W", WINDOWS)
def test_plan_basis_is_the_windowed_dft_rounded_once(W):
    plan = S.spectral_plan(W)
    assert plan.basis32.dtype == np.float32 and plan.basis32.shape == (W, 2, W // 2 + 1) and plan.n_mels == 0 and plan.fb32 is None
    n, k = np.arange(W)[:, None], np.arange(W // 2 + 1)[None, :]
    want = np.exp(-2j * np.pi * ((n * k) % W) / W) * R.hann(W)[:, None]
    # one rounding to fp32 of a value below 1, and the float64 evaluation of cos / sin and the window (a few 1e-16)
    for plane, ref in ((0, want.real), (1, want.imag)):
        assert np.abs(plan.basis32[:, plane, :].astype(np.float64) - ref).max() <= 2.0 ** -25 + 1e-15
    assert np.all(plan.basis32[0] == 0.0)                                     # the periodic Hann window starts at zero
    assert S.spectral_plan(W) is plan


@pytest.mark.parametrize("W,n_mels", list(zip(R.MEL["windows"], R.MEL["n_mels"])) + [(2048, 80), (512, 1), (32, 20)])
def test_filterbank_shape_and_against_the_reference(W, n_mels):
    rate = 44100
    plan = S.spectral_plan(W, rate, n_mels)
    fb = plan.fb32.astype(np.float64)
    assert plan.fb32.dtype == np.float32 and fb.shape == (n_mels, W // 2 + 1) and np.all(fb >= 0.0)
    ref = R.filterbank(W, rate, n_mels)
    assert np.abs(fb - ref).max() <= 2.0 ** -24 * ref.max() + 1e-18
    centres = []
    for m in range(n_mels):
        lo, hi = (int(v) for v in plan.fb_range[m])
        assert 0 <= lo <= hi <= W // 2 + 1
        assert np.all(fb[m, :lo] == 0.0) and np.all(fb[m, hi:] == 0.0)
        if lo == hi:                                                           # an empty filter: a row of zeros, not an error
            assert np.all(fb[m] == 0.0)
            continue
        row = fb[m, lo:hi]
        assert np.all(row > 0.0)
        top = int(row.argmax())
        assert np.all(np.diff(row[:top + 1]) >= 0.0) and np.all(np.diff(row[top:]) <= 0.0)      # unimodal
        # triangular: both flanks are straight lines (second differences vanish to rounding); the apex lies between two bins, so
        # the largest sample belongs to one flank or to the other
        straight = lambda v: v.shape[0] < 3 or np.abs(np.diff(v, 2)).max() <= 1e-9 * ref[m].max()
        t = lo + top
        assert straight(ref[m, lo:t]) and straight(ref[m, t + 1:hi])
        assert straight(ref[m, lo:t + 1]) or straight(ref[m, t:hi])
        centres.append(float((np.arange(lo, hi) * row).sum() / row.sum()))
    # a filter narrower than two bins has its centroid on a bin, and may share it with its neighbour: never backwards
    assert np.all(np.diff(centres) >= 0.0) and (len(centres) < 2 or centres[-1] > centres[0])
    if (W, n_mels) == (32, 20):
        assert len(centres) < n_mels                                           # filters narrower than the bin spacing can hold no bin
    if (W, n_mels) == (2048, 80):
        assert len(centres) == n_mels


def test_filterbank_refusals():
    for bad in (0, 321):
        with pytest.raises(ValueError, match="n_mels"):
            S.mel_filterbank(512, 44100, bad)
    for bad in (16, 4096, 48, 0):
        with pytest.raises(ValueError, match="power of two"):
            S.spectral_plan(bad)
    with pytest.raises(ValueError, match="sample rate"):
        S.spectral_plan(512, None, 80)


@pytest.mark.parametrize("W", (32, 512, 2048))
def test_frame_count_and_framing_equal_torch_stft(W):
    H = W // 4
    for L in sorted({1, H - 1, H, W // 2, W + 1, 3 * W + 7}):
        x = R.noise(L, seed=L + W).astype(np.float64)
        mag = R.stft_mag(x, W)
        assert mag.shape == (1 + L // H, W // 2 + 1) and S.n_frames(L, W) == 1 + L // H
        t = torch.stft(torch.from_numpy(x), n_fft=W, hop_length=H, win_length=W, window=torch.hann_window(W, periodic=True, dtype=torch.float64),
                       center=True, pad_mode="constant", return_complex=True).abs().numpy().T
        assert t.shape == mag.shape
        assert np.abs(t - mag).max() <= 1e-12 * max(1.0, float(mag.max()))


def test_half_amplitude_sine_gives_twice_log10_two():
    rate, L = 44100, 10007
    a = np.sin(2.0 * np.pi * 1000.0 * np.arange(L) / rate)
    b = 0.5 * a
    for W in R.STFT["windows"]:
        Sa, Sb = R.stft_mag(a, W), R.stft_mag(b, W)
        live = (Sa > R.EPS) & (Sb > R.EPS)
        assert live.sum() >= 100 * Sa.shape[0]                                 # the Hann window's leakage falls below eps far from 1 kHz
        d = np.abs(np.log10(Sa[live] ** 2) - np.log10(Sb[live] ** 2))
        assert np.abs(d - 2.0 * math.log10(2.0)).max() <= 1e-9
        mag, _ = R.terms(Sa, Sb, 2)
        assert abs(mag - 0.5 * Sa.mean()) <= 1e-12 * Sa.mean()


def test_reference_metric_is_a_distance():
    a, b = R.noise(4096, 1), R.noise(4096, 2)
    for spec in (R.STFT, R.MEL):
        assert R.metric(a, a, 44100, spec)[0] == 0.0
        ab, ba = R.metric(a, b, 44100, spec)[0], R.metric(b, a, 44100, spec)[0]
        assert ab == ba and ab > 0.0
    assert S.STFT_DEFAULT["windows"] == R.STFT["windows"] and S.MEL_DEFAULT["windows"] == R.MEL["windows"]
    assert S.MEL_DEFAULT["n_mels"] == R.MEL["n_mels"] and S.EPS == R.EPS
    for k in ("mag_weight", "log_weight", "power"):
        assert S.STFT_DEFAULT[k] == R.STFT[k] and S.MEL_DEFAULT[k] == R.MEL[k]


# ---------------------------------------------------------------------------------------------- the host's rules
class _NoDevice(S.DeviceSpectral):
    def __init__(self):
        self.launches = 0

    def _upload(self, rows):
        raise _Reached([r.shape[0] for r in rows])


class _Reached(Exception):
    pass


def test_distance_raises_on_unequal_lengths_and_trim_cuts():
    d = _NoDevice()
    a, b = R.noise(1000, 1), R.noise(900, 2)
    with pytest.raises(ValueError, match="1000 samples against 900"):
        d.distance(a, b, 44100)
    with pytest.raises(_Reached) as e:                                         # past the length check, at the first upload
        d.distance(a, b, 44100, trim=True)
    assert e.value.args[0] == [900]
    with pytest.raises(_Reached) as e:
        d.distance([a, b], [a, b[:800]], 44100, trim=True)
    assert e.value.args[0] == [1000, 800]
    with pytest.raises(ValueError, match="2 waveforms against 1"):
        d.distance([a, a], [a], 44100)
    with pytest.raises(ValueError, match="unknown metric"):
        d.distance(a, a, 44100, metrics=("snr",))
    with pytest.raises(ValueError, match="mono float"):
        d.distance(np.zeros((2, 8), dtype=np.float32), np.zeros((2, 8), dtype=np.float32), 44100)
    with pytest.raises(ValueError, match="expected 1"):
        d.distance(np.zeros(0, dtype=np.float32), np.zeros(0, dtype=np.float32), 44100)
    ra, rb, single = S.pair_rows(a, b, trim=True)
    assert single and ra[0].shape == rb[0].shape == (900,) and np.array_equal(ra[0], a[:900])


def test_public_surface_exists():
    from dia_hip import codec as K
    from dia_hip import model as M
    import cli
    assert callable(K.DeviceCodec.audio_distance) and callable(M.Dia.audio_distance) and callable(M.Dia.codec_roundtrip_distance)
    p = cli.build_parser()
    assert p.parse_args(["--compare-audio", "a.wav", "b.wav"]).compare_audio == ["a.wav", "b.wav"]
    assert p.parse_args(["--codec-roundtrip", "a.wav", "--codec-path", "c.pth"]).codec_roundtrip == "a.wav"
    with pytest.raises(SystemExit):
        cli.main(["--codec-roundtrip", "a.wav"])                               # no --codec-path
    dia = object.__new__(M.Dia)
    dia.codec = None
    with pytest.raises(RuntimeError, match="codec"):
        dia.codec_roundtrip_distance(np.zeros(1024, dtype=np.float32))


# ---------------------------------------------------------------------------------------------- the C ABI
def test_abi_symbol_struct_and_validation(tmp_path):
    src = open(os.path.join(ROOT, "include", "dia_hip.h")).read()
    assert "int dia_spectral(const dia_spectral_args* a, void* stream);" in src
    assert "dia_spectral" in hb.EXPORTS and hb.ABI_VERSION == 8 and "#define DIA_ABI_VERSION 8" in src
    c = tmp_path / "s.c"
    c.write_text('#include <stdio.h>\n#include "dia_hip.h"\nint main(void){ printf("%zu %d %d %d %d %d %d\\n", sizeof(dia_spectral_args), '
                 'DIA_SPECTRAL_MAX_ROWS, DIA_SPECTRAL_MAX_T, DIA_SPECTRAL_MIN_WINDOW, DIA_SPECTRAL_MAX_WINDOW, DIA_SPECTRAL_MAX_MELS, '
                 'DIA_SPECTRAL_TILE_FRAMES); return 0; }\n')
    exe = tmp_path / "s"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(hb.SpectralArgs), S.MAX_ROWS, S.MAX_T, S.MIN_WINDOW, S.MAX_WINDOW, S.MAX_MELS, S.TILE_FRAMES]
    assert got[1:] == [64, 1 << 24, 32, 2048, 320, 16]
    L = hb.lib()
    assert L.dia_abi_version() == 8
    fn = L.dia_spectral

    def err(a):
        assert fn(ctypes.byref(a), None) == -1                                 # DIA_E_ARG, before any HIP call
        return L.dia_last_error().decode()

    assert fn(None, None) == -1 and "null argument" in L.dia_last_error().decode()
    assert "null pointer" in err(hb.SpectralArgs())                            # the zeroed struct
    i32 = ctypes.c_int32 * 2

    def good(**kw):
        f = dict(a=0x1000, b=0x2000, basis=0x3000, fb=0x4000, fb_range=0x5000, partial=0x6000, out=0, B=2, ld=4096, window=512, n_mels=80,
                 tiles=3, out_frames=0, power=1, eps=1e-5, len=i32(4096, 1))
        f.update(kw)
        return hb.SpectralArgs(**f)

    assert "null pointer" in err(good(a=0)) and "null pointer" in err(good(basis=0)) and "null pointer" in err(good(len=None))
    for w in (0, 16, 48, 500, 4096, -512):
        assert f"window = {w} is not a power of two" in err(good(window=w))
    assert "n_mels = -1" in err(good(n_mels=-1)) and "n_mels = 321" in err(good(n_mels=321))
    assert "needs fb and fb_range" in err(good(fb=0)) and "needs fb and fb_range" in err(good(fb_range=0))
    assert "B = 0" in err(good(B=0)) and "B = 65" in err(good(B=65))
    assert "ld = 0" in err(good(ld=0)) and "ld = 16777217" in err(good(ld=(1 << 24) + 1))
    assert "row 1: len = 0" in err(good(len=i32(4096, 0))) and "row 0: len = 4097" in err(good(len=i32(4097, 1)))
    assert "power = 3" in err(good(power=3)) and "power = 0" in err(good(power=0))
    assert "eps" in err(good(eps=0.0)) and "eps" in err(good(eps=float("nan")))
    # the output of the mode asked for: partials for a distance, out for spectra only
    assert "needs partial" in err(good(partial=0))
    assert "tiles = 2 below the 3 frame tiles" in err(good(tiles=2))           # 1 + 4096 // 128 = 33 frames, 16 to a tile
    assert "needs out" in err(good(b=0, partial=0))
    assert "out_frames = 32 below the 33 frames" in err(good(b=0, out=0x7000, out_frames=32))
