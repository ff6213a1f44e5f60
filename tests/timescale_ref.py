"""The speed factor in float64 (DESIGN.md "Speed factor"), restated from its formulas for the tests: the interpolating mode, WSOLA's
search and its two-term overlap-add.  Nothing here comes from the kernel or from dia_hip/timescale.py: the window, the centres, the
frame count and the tie rule are written out again.

A signal may be given as a WINDOW (in_start, total) of a longer one, as the library's rows: it reads as zero outside the window and
outside [0, total)."""
import math

import numpy as np

SPEEDS = (0.8, 0.94, 1.25, 2.0)


def clamp(speed):
    return min(max(float(speed), 0.1), 5.0)


def out_len(N, speed):
    return int(N / clamp(speed))


def interp(x, speed):
    """y[j] = (x[i + 1] - x[i]) * (pos_j - i) + x[i], pos_j = j (N - 1) / (M - 1), pos_{M - 1} = N - 1, i = min(floor(pos_j), N - 2)"""
    x = np.asarray(x, dtype=np.float64)
    N, s = x.shape[0], clamp(speed)
    M = out_len(N, s)
    if s == 1.0 or M == N or M <= 0:
        return x
    if N == 1:
        return np.full(M, x[0])
    y = np.empty(M, dtype=np.float64)
    for j in range(M):
        pos = 0.0 if M == 1 else (float(N - 1) if j == M - 1 else float(j * (N - 1)) / float(M - 1))
        i = min(int(math.floor(pos)), N - 2)
        y[j] = (x[i + 1] - x[i]) * (pos - i) + x[i]
    return y


def window(W):
    return np.array([0.5 - 0.5 * math.cos(2.0 * math.pi * n / W) for n in range(W)], dtype=np.float64)


def centre(k, W, speed):
    return int(math.floor(k * (W // 2) * clamp(speed) + 0.5))


def frames(M, W):
    return -(-M // (W // 2)) + 1


class Signal:
    """samples [in_start, in_start + len(x)) of a signal of `total` samples (None: no end yet); zero everywhere else"""

    def __init__(self, x, in_start=0, total=None):
        self.x = np.asarray(x, dtype=np.float64)
        self.lo = int(in_start)
        self.hi = self.lo + self.x.shape[0] if total is None else min(self.lo + self.x.shape[0], int(total))

    def seg(self, start, n):
        out = np.zeros(n, dtype=np.float64)
        a, b = max(start, self.lo), min(start + n, self.hi)
        if a < b:
            out[a - start:b - start] = self.x[a - self.lo:b - self.lo]
        return out


def candidate_order(D):
    """delta in the order of the tie rule: the smallest |delta| first, the negative one before the positive"""
    return np.array([0] + [v for d in range(1, D + 1) for v in (-d, d)], dtype=np.int64)


def correlations(sig, k, delta_prev, W, D, speed):
    """(corr float64 [2 D + 1] of delta = -D .. D, bound [2 D + 1] = sum_n |t_k[n]| |x[...]|) of frame k >= 1"""
    Hs = W // 2
    t = sig.seg(centre(k - 1, W, speed) + delta_prev, W)                      # p_{k-1} + Hs
    span = sig.seg(centre(k, W, speed) - D - Hs, W + 2 * D)
    win = np.lib.stride_tricks.sliding_window_view(span, W)                   # [2 D + 1][W]
    return win @ t, np.abs(win) @ np.abs(t)


def pick(corr, D):
    order = candidate_order(D)
    return int(order[int(np.argmax(corr[order + D]))])


def search(sig, k0, k1, delta_prev, W, D, speed):
    """delta of frames [k0, k1), int64"""
    out = np.zeros(k1 - k0, dtype=np.int64)
    for k in range(k0, k1):
        if k > 0:
            delta_prev = pick(correlations(sig, k, delta_prev, W, D, speed)[0], D)
        else:
            delta_prev = 0
        out[k - k0] = delta_prev
    return out


def synth(sig, out_start, out_count, delta, k_first, W, speed, w=None):
    """outputs [out_start, + out_count) in float64 from delta[k - k_first]: (y, |x_a| + |x_b| per output).  w: the window to use
    (default float64; the device's is rounded to fp32 once)"""
    Hs = W // 2
    w = window(W) if w is None else np.asarray(w, dtype=np.float64)
    m = out_start + np.arange(out_count, dtype=np.int64)
    ka = m // Hs
    nb = m - ka * Hs
    na = nb + Hs
    cs = np.array([centre(k, W, speed) for k in range(k_first, k_first + len(delta))], dtype=np.int64)
    p = cs + np.asarray(delta, dtype=np.int64) - Hs
    ia, ib = p[ka - k_first] + na, p[ka + 1 - k_first] + nb
    lo = int(min(ia.min(), ib.min())) if out_count else 0
    hi = int(max(ia.max(), ib.max())) + 1 if out_count else 0
    s = sig.seg(lo, hi - lo)
    xa, xb = s[ia - lo], s[ib - lo]
    return w[na] * xa + w[nb] * xb, np.abs(xa) + np.abs(xb)


def wsola(x, speed, W=1024, D=512):
    """(y float64 [M], delta int64 [F]) of a whole signal; the input itself when nothing is to do"""
    x = np.asarray(x, dtype=np.float64)
    N, s = x.shape[0], clamp(speed)
    M = out_len(N, s)
    if s == 1.0 or M <= 0:
        return x, np.zeros(0, dtype=np.int64)
    sig = Signal(x, 0, N)
    F = frames(M, W)
    delta = search(sig, 0, F, 0, W, D, s)
    return synth(sig, 0, M, delta, 0, W, s)[0], delta


def stream_run(W, D, speed):
    """the `run` callback of dia_hip.timescale.TimescaleStream on this reference (float64 kept: the joined chunks are compared
    with wsola() exactly)"""
    def run(win, in_start, k0, k1, delta_prev, out_start, out_count, total):
        sig = Signal(win, in_start, total)
        delta = search(sig, k0, k1, delta_prev, W, D, speed)
        both = np.concatenate([[delta_prev], delta]) if k0 > 0 else delta
        y = synth(sig, out_start, out_count, both, max(k0 - 1, 0), W, speed)[0]
        return delta, y
    return run
