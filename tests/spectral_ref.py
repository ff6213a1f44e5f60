"""Float64 numpy restatement of the audio distance (DESIGN.md "Audio distance"), independent of dia_hip/spectral.py's plan code:
framing by zero padding, np.fft.rfft, a Slaney mel bank written out step by step, and the two L1 terms."""
import functools
import math

import numpy as np

EPS = 1e-5
STFT = dict(windows=(2048, 512), mag_weight=1.0, log_weight=1.0, power=2)
MEL = dict(windows=(32, 64, 128, 256, 512, 1024, 2048), n_mels=(5, 10, 20, 40, 80, 160, 320), mag_weight=0.0, log_weight=1.0, power=1)


def noise(L, seed):
    """uniform in [-1, 1] with both ends present where there is room"""
    x = np.random.default_rng(seed).uniform(-1.0, 1.0, size=L)
    if L >= 1:
        x[L // 2] = 1.0
    if L >= 2:
        x[L // 3] = -1.0
    return x.astype(np.float32)


def hann(W):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(W) / W)


def frames(x, W):
    """float64 [1 + L // H][W]: frame f holds samples f H - W / 2 .. f H + W / 2 - 1, zero outside the signal"""
    x = np.asarray(x, dtype=np.float64)
    H = W // 4
    F = 1 + x.shape[0] // H
    pad = np.concatenate([np.zeros(W // 2), x, np.zeros(W)])
    return np.stack([pad[f * H:f * H + W] for f in range(F)])


def stft_mag(x, W):
    return np.abs(np.fft.rfft(frames(x, W) * hann(W)[None, :], axis=1))


def mag_scale(x, W):
    """sum_n |x_n| |w_n| per frame: the scale of the fp32 dot-product bound"""
    return (np.abs(frames(x, W)) * hann(W)[None, :]).sum(axis=1)


def _hz_to_mel(f):
    if f < 1000.0:
        return f / (200.0 / 3.0)
    return 15.0 + math.log(f / 1000.0) / (math.log(6.4) / 27.0)


def _mel_to_hz(m):
    if m < 15.0:
        return m * (200.0 / 3.0)
    return 1000.0 * math.exp((m - 15.0) * (math.log(6.4) / 27.0))


@functools.lru_cache(maxsize=None)
def filterbank(W, rate, n_mels):
    """float64 [n_mels][W / 2 + 1], cached: treat as read-only"""
    nbin = W // 2 + 1
    top = _hz_to_mel(rate / 2.0)
    pts = [_mel_to_hz(top * i / (n_mels + 1)) for i in range(n_mels + 2)]
    fb = np.zeros((n_mels, nbin))
    for m in range(n_mels):
        lo, mid, hi = pts[m], pts[m + 1], pts[m + 2]
        for k in range(nbin):
            f = k * rate / W
            up, down = (f - lo) / (mid - lo), (hi - f) / (hi - mid)
            fb[m, k] = max(0.0, min(up, down)) * 2.0 / (hi - lo)
    return fb


def mel(x, W, rate, n_mels, fb=None):
    return stft_mag(x, W) @ (filterbank(W, rate, n_mels) if fb is None else fb).T


def terms(Sa, Sb, power, eps=EPS):
    mag = np.abs(Sa - Sb).mean()
    log = np.abs(np.log10(np.maximum(Sa, eps) ** power) - np.log10(np.maximum(Sb, eps) ** power)).mean()
    return float(mag), float(log)


def metric(a, b, rate, spec, spectrum=None):
    """(value, {window: (mag_term, log_term)}) of one metric; `spectrum(x, W, n_mels)` replaces the float64 spectra (the float32
    yardstick of the GPU test does)"""
    total, per = 0.0, {}
    for i, W in enumerate(spec["windows"]):
        nm = spec["n_mels"][i] if "n_mels" in spec else 0
        if spectrum is not None:
            Sa, Sb = spectrum(a, W, nm), spectrum(b, W, nm)
        elif nm:
            fb = filterbank(W, rate, nm)
            Sa, Sb = mel(a, W, rate, nm, fb), mel(b, W, rate, nm, fb)
        else:
            Sa, Sb = stft_mag(a, W), stft_mag(b, W)
        per[W] = terms(Sa, Sb, spec["power"])
        total += spec["mag_weight"] * per[W][0] + spec["log_weight"] * per[W][1]
    return total / len(spec["windows"]), per
