"""Float64 restatement of the resampling filter in its FULL form, written from the formula alone (torchaudio's documented default:
sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99) and independently of dia_hip.resample.resample_plan:

    g = gcd(rate_in, rate_out), o = rate_in / g, n = rate_out / g, base = min(o, n) * 0.99, width = ceil(6 o / base), K = 2 width + o
    tap k of phase p:  t = (-p / n + (k - width) / o) * base,  tc = clamp(t, -6, 6)
    f[p][k] = sinc(pi tc) * cos(pi tc / 12)^2 * base / o
    output q n + p = sum_k f[p][k] * x[q o - width + k]  (x = 0 outside [0, L)),  ceil(n L / o) outputs

plus an evaluator of the COMPACT form (any first[] / bank[][] handed in) in float64 with the forward-error bound of its fp32
evaluation, and the shared cases of the CPU and GPU tests."""
import functools
import math

import numpy as np

PAIRS = ((22050, 44100), (48000, 44100), (16000, 44100), (8000, 44100), (32000, 44100), (44100, 48000), (44100, 24000), (44100, 16000),
         (96000, 44100))
GPU_PAIRS = ((22050, 44100), (48000, 44100), (16000, 44100), (44100, 16000), (44100, 48000))
CHUNKS = {"1": lambda i: 1, "7": lambda i: 7, "512": lambda i: 512, "irregular": lambda i: (3, 0, 250, 1, 1024, 17, 64)[i % 7]}


def reduced(rate_in, rate_out):
    g = math.gcd(rate_in, rate_out)
    return rate_in // g, rate_out // g


@functools.lru_cache(maxsize=None)
def full_bank(rate_in, rate_out):
    """-> (o, n, width, f float64 [n][K])"""
    o, n = reduced(rate_in, rate_out)
    base = min(o, n) * 0.99
    width = math.ceil(6 * o / base)
    f = np.empty((n, 2 * width + o), dtype=np.float64)
    for p in range(n):
        k = np.arange(2 * width + o, dtype=np.float64)
        t = (-p / n + (k - width) / o) * base
        tc = np.minimum(np.maximum(t, -6.0), 6.0)
        a = np.pi * tc
        s = np.ones_like(a)
        nz = a != 0.0
        s[nz] = np.sin(a[nz]) / a[nz]
        f[p] = s * np.cos(np.pi * tc / 12.0) ** 2 * (base / o)
    f.setflags(write=False)
    return o, n, width, f


def out_len(rate_in, rate_out, L):
    o, n = reduced(rate_in, rate_out)
    return -(-n * L // o)


def _full_frames(x, rate_in, rate_out):
    o, n, width, f = full_bank(rate_in, rate_out)
    x = np.asarray(x, dtype=np.float64)
    L, K = x.shape[0], f.shape[1]
    m = -(-n * L // o)
    nq = -(-m // n)
    xp = np.zeros(width + nq * o + K, dtype=np.float64)
    xp[width:width + L] = x
    return np.lib.stride_tricks.sliding_window_view(xp, K)[:nq * o:o], f, m     # frames[q][k] = x[q o - width + k]


def resample_full(x, rate_in, rate_out):
    """the whole signal x through the full bank, float64"""
    frames, f, m = _full_frames(x, rate_in, rate_out)
    return (frames @ f.T).reshape(-1)[:m]


def _compact_products(x, o, n, nt, first, bank):
    x = np.asarray(x, dtype=np.float64)
    bank = np.asarray(bank, dtype=np.float64)
    L = x.shape[0]
    m = np.arange(-(-n * L // o), dtype=np.int64)
    q, p = m // n, m % n
    at = (q * o + np.asarray(first, dtype=np.int64)[p])[:, None] + np.arange(nt, dtype=np.int64)[None, :]
    ok = (at >= 0) & (at < L)
    return bank[p] * np.where(ok, x[np.clip(at, 0, max(L - 1, 0))] if L else 0.0, 0.0)


def resample_compact(x, o, n, nt, first, bank):
    """the compact form in float64: -> (y [ceil(n L / o)], s [same]) with y[m] = sum_k bank[p][k] x[q o + first[p] + k] and
    s[m] = sum_k |bank[p][k] x[...]|, the scale of the fp32 evaluation's forward-error bound"""
    prod = _compact_products(x, o, n, nt, first, bank)
    return prod.sum(axis=1), np.abs(prod).sum(axis=1)


def full_minus_compact(x, rate_in, rate_out, nt, first, bank):
    """full output - compact output per sample, free of summation error: math.fsum (the correctly rounded sum) over the float64
    products of the full form and the negated ones of the compact form together.  Comparing two separately rounded sums would
    not do: terms of 1e-49 decide ties, which sums of a dozen doubles hit often."""
    frames, f, m = _full_frames(x, rate_in, rate_out)
    o, n = reduced(rate_in, rate_out)
    pf = (frames[:, None, :] * f[None, :, :]).reshape(-1, f.shape[1])[:m]
    pc = _compact_products(x, o, n, nt, first, bank)
    return np.array([math.fsum(np.concatenate([a, -b])) for a, b in zip(pf, pc)], dtype=np.float64)



def noise(L, seed):
    """uniform noise in [-1, 1] with exact +1 and -1 samples among it"""
    g = np.random.default_rng(seed)
    x = g.uniform(-1.0, 1.0, size=L).astype(np.float32)
    x[::5][:2] = 1.0
    if L > 1:
        x[1::7][:2] = -1.0
    return x


def lengths_of(o):
    """signal lengths around one input period (o - 1 = 0 for o = 1: the empty signal)"""
    return sorted({1, o - 1, o, o + 1, 1300})
