"""Float64 restatement of the loudness meter, written from ITU-R BS.1770-4 and the issue's formulas and independently of
dia_hip.loudness: the K-weighting coefficients, the two biquads run SEQUENTIALLY sample by sample, the sums over 100 ms steps, the
gating, the true peak through tests/resample_ref.py's 1 -> 4 conversion, the gain and the trim.  Also: the same recursion with a
float32 state (the yardstick the device's deviation is measured against), an emulation of the device's chunk scheme from a plan's
table, and the shared signals of the CPU and GPU tests.

pyloudnorm and libebur128 are not available offline: the meter is pinned on the standard's 48 kHz table and on the 997 Hz sine of
EBU Tech 3341 only."""
import functools
import math

import numpy as np

import resample_ref as RR

TABLE_48K = {"shelf_b": (1.53512485958697, -2.69169618940638, 1.19839281085285), "shelf_a": (1.0, -1.69065929318241, 0.73248077421585),
             "hp_b": (1.0, -2.0, 1.0), "hp_a": (1.0, -1.99004745483398, 0.99007225036621)}
GPU_RATES = (8000, 11025, 44100, 48000)


def step_of(rate):
    return (int(rate) + 5) // 10


def coefficients(rate):
    """-> (shelf b, shelf a, high-pass b, high-pass a), tuples of 3 floats"""
    fs = float(rate)
    K = math.tan(math.pi * 1681.974450955533 / fs)
    Q = 0.7071752369554196
    Vh = 10.0 ** (3.999843853973347 / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    sb = ((Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0)
    sa = (1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0)
    K = math.tan(math.pi * 38.13547087602444 / fs)
    Q = 0.5003270373238773
    a0 = 1.0 + K / Q + K * K
    return sb, sa, (1.0, -2.0, 1.0), (1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0)


def _f32(v):
    return float(np.float32(v))


def step_sums(x, rate, state32=False):
    """the K-weighted signal's sum of squares over every whole step of x, float64 [len // step]: both biquads in transposed direct
    form II, sample by sample.  state32: the four state variables are rounded to float32 after every sample (the arithmetic and
    the sums stay float64)."""
    sb, sa, hb, ha = coefficients(rate)
    S = step_of(rate)
    xs = [float(v) for v in np.asarray(x, dtype=np.float64)]
    ns = len(xs) // S
    out = np.zeros(ns, dtype=np.float64)
    r = _f32 if state32 else (lambda v: v)
    s1a = s2a = s1b = s2b = 0.0
    for s in range(ns):
        acc = 0.0
        for v in xs[s * S:(s + 1) * S]:
            y1 = sb[0] * v + s1a
            s1a = r(sb[1] * v + s2a - sa[1] * y1)
            s2a = r(sb[2] * v - sa[2] * y1)
            y2 = hb[0] * y1 + s1b
            s1b = r(hb[1] * y1 + s2b - ha[1] * y2)
            s2b = r(hb[2] * y1 - ha[2] * y2)
            acc += y2 * y2
        out[s] = acc
    return out


def block_loudness(z):
    return -0.691 + 10.0 * math.log10(z) if z > 0.0 else -math.inf


def integrated(steps, step):
    """BS.1770-4 gating from the step sums"""
    s = [float(v) for v in steps]
    z = [(s[j] + s[j + 1] + s[j + 2] + s[j + 3]) / (4.0 * step) for j in range(len(s) - 3)]
    g = [v for v in z if block_loudness(v) >= -70.0]
    if not g:
        return -math.inf
    rel = block_loudness(sum(g) / len(g)) - 10.0
    g = [v for v in g if block_loudness(v) > rel]
    if not g:
        return -math.inf
    return block_loudness(sum(g) / len(g))


def loudness(x, rate, state32=False):
    return integrated(step_sums(x, rate, state32), step_of(rate))


def db(v):
    return 20.0 * math.log10(v) if v > 0.0 else -math.inf


def sample_peak(x):
    x = np.asarray(x, dtype=np.float64)
    return float(np.abs(x).max()) if x.shape[0] else 0.0


def true_peak(x):
    """max |.| over x and over x 4 x oversampled by the full float64 bank (linear)"""
    x = np.asarray(x, dtype=np.float64)
    if x.shape[0] == 0:
        return 0.0
    return max(sample_peak(x), float(np.abs(RR.resample_full(x, 1, 4)).max()))


def oversampled(x, nt, first, bank32):
    """the compact fp32 bank evaluated in float64 -> (values [4 len], sum |h_i x_i| [4 len])"""
    return RR.resample_compact(x, 1, 4, nt, first, bank32)


def apply_gain(x, gain, start=0, stop=None):
    x = np.asarray(x, dtype=np.float32)
    return (x[start:stop].astype(np.float64) * float(gain)).astype(np.float32)


def choose_gain(loud, tp_db, target, peak):
    if not math.isfinite(loud):
        return 0.0, False
    g = target - loud
    if tp_db + g > peak:
        return peak - tp_db, True
    return g, False


def trim(steps, step, n, trim_db, pad):
    """[start, stop): leading / trailing whole steps below trim_db go, except `pad` on either side"""
    l = [block_loudness(float(v) / step) for v in steps]
    loud = [i for i, v in enumerate(l) if v >= trim_db]
    if not loud:
        return 0, n
    lead, trail = loud[0], len(l) - 1 - loud[-1]
    start = max(0, lead - pad) * step
    stop = n if trail <= pad else (len(l) - (trail - pad)) * step
    return start, stop


def chunked_step_sums(plan, x):
    """the device's scheme in float64 from a LoudnessPlan's table: zero-state end states per chunk, the carry within a step and over
    the steps, the second run from the true initial states"""
    c = [float(v) for v in plan.table[:10]]
    ML = plan.table[10:26].reshape(4, 4)
    MS = plan.table[26:42].reshape(4, 4)
    P = plan.table[42:].reshape(plan.chunks, 4, 4)
    S, L, C = plan.step, plan.chunk, plan.chunks
    xs = [float(v) for v in np.asarray(x, dtype=np.float64)]

    def run(state, lo, hi, sq=False):
        s1a, s2a, s1b, s2b = state
        acc = 0.0
        for v in xs[lo:hi]:
            y1 = c[0] * v + s1a
            s1a, s2a = c[1] * v + s2a - c[3] * y1, c[2] * v - c[4] * y1
            y2 = c[5] * y1 + s1b
            s1b, s2b = c[6] * y1 + s2b - c[8] * y2, c[7] * y1 - c[9] * y2
            acc += y2 * y2
        return np.array([s1a, s2a, s1b, s2b]), acc

    ns = len(xs) // S
    zs, Es = [], []
    for s in range(ns):
        z = [np.zeros(4)]
        for k in range(C - 1):
            e, _ = run(np.zeros(4), s * S + k * L, s * S + min((k + 1) * L, S))
            z.append(ML @ z[-1] + e)
        zs.append(z)
        Es.append(run(z[-1], s * S + (C - 1) * L, (s + 1) * S)[0])
    init, out = np.zeros(4), np.zeros(ns)
    for s in range(ns):
        out[s] = sum(run(zs[s][k] + P[k] @ init, s * S + k * L, s * S + min((k + 1) * L, S))[1] for k in range(C))
        init = MS @ init + Es[s]
    return out


# ---------------------------------------------------------------------------------------------- shared signals
def sine(rate, freq, seconds, amp=1.0, phase=0.0):
    n = np.arange(int(round(rate * seconds)), dtype=np.float64)
    return (amp * np.sin(2.0 * np.pi * freq * n / rate + phase)).astype(np.float32)


def speechlike(n, seed, level=0.1):
    """noise with a slow envelope and a DC step: exercises both filters"""
    g = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    env = 0.55 + 0.45 * np.sin(2.0 * np.pi * t / 7000.0)
    return (level * env * g.standard_normal(n) + 0.02).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(rate, n, seed):
    """-> (x float32 [n], float64 step sums, float32-state step sums): computed once, shared, read-only"""
    x = speechlike(n, seed)
    a, b = step_sums(x, rate), step_sums(x, rate, state32=True)
    for v in (x, a, b):
        v.setflags(write=False)
    return x, a, b
