"""The speed factor on the MI355X (csrc/timescale.hip: dia_timescale; dia_hip/timescale.py: DeviceTimescale, TimescaleStream;
DESIGN.md "Speed factor") against the float64 restatement of tests/timescale_ref.py.

Bounds, derived and not measured (u = 2^-24):
  interp     the device evaluates (x1 - x0) * frac + x0 in float64 and rounds once: one fp32 ulp of the float64 value covers the
             rounding and whatever an fma contraction moves in float64.
  search     on integer samples in [-8, 8] every fp32 chain is exact (|corr| <= 64 W < 2^24), so delta must equal the restatement's
             at every frame, ties included.  On noise an fp32 fma chain of W terms is off by at most W u sum |t x| (the forward
             bound of a recursive dot product); applied to the winner and to the true maximum, the float64 correlation at the
             device's delta must reach the float64 maximum minus 2 W u max_delta sum |t x|.
  synthesis  a window value rounded once, one product, one fma: 3 u (|x_a| + |x_b|).
Everything else here is bitwise: batch rows, masking, chunked streams, repeated runs.  Every test prints its figures before it
asserts."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import timescale_ref as R
from dia_hip import timescale as S

DEV = torch.device("cuda:0")
U = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    return S.DeviceTimescale(DEV)


def noise(n, seed):
    return np.random.default_rng(seed).standard_normal(n).astype(np.float32)


def integers(n, seed):
    return np.random.default_rng(seed).integers(-8, 9, size=n).astype(np.float32)


# ---------------------------------------------------------------------------------------------- interp
@pytest.mark.parametrize("N", [1, 2, 3001])
def test_interp_within_one_ulp_of_float64(dev, N):
    x = noise(N, 10 + N)
    for speed in (0.1, 0.8, 0.94, 1.25, 5.0, 7.0):
        ref = R.interp(x, speed)
        y = dev.time_scale(x, speed)
        M = R.out_len(N, speed)
        if M <= 0 or M == N:
            print(f"interp N {N} speed {speed}: M {M}, the input comes back")
            assert y is x
            continue
        ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
        err = np.abs(y.astype(np.float64) - ref)
        print(f"interp N {N} speed {speed}: M {M}, worst error {float((err / ulp).max()):.3f} ulp")
        assert y.dtype == np.float32 and y.shape == (M,)
        assert np.all(err <= ulp)
        assert y[0] == x[0]
    assert dev.time_scale(x, 1.0) is x                                         # no launch, the input itself


# ---------------------------------------------------------------------------------------------- search
CASES = [(64, 16, 5000), (1024, 512, 20000),
         (1024, 1024, 12000),                                                  # 2 D + 1 > 1280: a second pass over the offsets
         (4096, 4096, 30000)]                                                  # the limits: more than 64 KiB of LDS


@pytest.mark.parametrize("W,D,N", CASES)
@pytest.mark.parametrize("speed", [0.8, 1.25, 2.0])
def test_search_is_exact_on_integer_samples(dev, W, D, N, speed):
    x = integers(N, W + D)
    _, want = R.wsola(x, speed, W, D)
    y, delta = dev.time_scale(x, speed, "wsola", W, D, return_delta=True)
    ties = sum(int((c == c.max()).sum() > 1) for k in range(1, min(want.shape[0], 12))
               for c in [R.correlations(R.Signal(x, 0, N), k, int(want[k - 1]), W, D, speed)[0]])
    bad = np.flatnonzero(delta != want)
    print(f"search-exact W {W} D {D} N {N} speed {speed}: {want.shape[0]} frames, {bad.shape[0]} differ, |delta| up to {int(np.abs(want).max())}, "
          f"{ties} of the first frames have tied maxima")
    assert delta.dtype == np.int32 and delta.shape == want.shape == (R.frames(R.out_len(N, speed), W),)
    assert bad.shape[0] == 0, (bad[:5], delta[bad[:5]], want[bad[:5]])


@pytest.mark.parametrize("speed", [0.8, 1.25])
def test_search_on_noise_within_the_dot_product_bound(dev, speed):
    W, D, N = 1024, 512, 20000
    x = noise(N, 77)
    sig = R.Signal(x, 0, N)
    _, delta = dev.time_scale(x, speed, "wsola", W, D, return_delta=True)
    worst, agree = -np.inf, 0
    assert delta[0] == 0
    for k in range(1, delta.shape[0]):                                         # the device's own chain: delta_{k-1} is the device's
        corr, mass = R.correlations(sig, k, int(delta[k - 1]), W, D, speed)
        slack = 2 * W * U * float(mass.max())
        short = float(corr.max() - corr[int(delta[k]) + D])
        worst = max(worst, short - slack)
        agree += int(delta[k]) == R.pick(corr, D)
        assert abs(int(delta[k])) <= D and short <= slack, (k, int(delta[k]), short, slack)
    print(f"search-noise speed {speed}: {delta.shape[0]} frames, {agree} pick the float64 maximum itself, worst (shortfall - bound) {worst:.3e}, "
          f"last bound {slack:.3e} against correlations of std {float(corr.std()):.1f}")


# ---------------------------------------------------------------------------------------------- synthesis
@pytest.mark.parametrize("W,D,N", CASES[:2])
@pytest.mark.parametrize("speed", [0.8, 1.25, 2.0])
def test_synthesis_within_three_roundings(dev, W, D, N, speed):
    x = noise(N, 5)
    y, delta = dev.time_scale(x, speed, "wsola", W, D, return_delta=True)
    M = R.out_len(N, speed)
    ref, mass = R.synth(R.Signal(x, 0, N), 0, M, delta, 0, W, speed)
    err = np.abs(y.astype(np.float64) - ref)
    print(f"synthesis W {W} D {D} N {N} speed {speed}: M {M}, worst error {float(err.max()):.3e}, worst error / bound "
          f"{float((err / np.maximum(3 * U * mass, 1e-300)).max()):.3f}")
    assert y.dtype == np.float32 and y.shape == (M,)
    assert np.all(err <= 3 * U * mass)


@pytest.mark.parametrize("speed", [0.8, 1.25])
def test_periodic_signal_comes_back(dev, speed):
    W, D, N, P = 1024, 512, 20000, 128
    per = noise(P, 9)
    x = np.tile(per, N // P + 1)[:N]
    y, delta = dev.time_scale(x, speed, "wsola", W, D, return_delta=True)
    M = R.out_len(N, speed)
    n = M - 3 * W
    want = np.tile(per.astype(np.float64), M // P + 2)[:n]
    err = np.abs(y[:n].astype(np.float64) - want)
    print(f"periodic speed {speed}: M {M}, checked [0, {n}), worst error {float(err.max()):.3e}, worst error / bound "
          f"{float((err / np.maximum(6 * U * np.abs(want), 1e-300)).max()):.3f}")
    assert n > 4 * W and np.all(err <= 3 * U * 2 * np.abs(want))               # x_a = x_b = the continuation's sample


# ---------------------------------------------------------------------------------------------- bitwise
LENGTHS = (20000, 1, 63, 5000, 0)


@pytest.mark.parametrize("mode", ["interp", "wsola"])
def test_ragged_batch_equals_solo_rows_and_ignores_what_lies_behind_them(dev, mode):
    speed = 0.8
    rows = [noise(n, 30 + i) for i, n in enumerate(LENGTHS)]
    batch, bdelta = dev.time_scale(rows, speed, mode, return_delta=True)
    solo = [dev.time_scale(r, speed, mode, return_delta=True) for r in rows]
    again = dev.time_scale(rows, speed, mode)
    print(f"batch {mode}: lengths {LENGTHS} -> {[b.shape[0] for b in batch]}")
    assert [b.shape[0] for b in batch] == [R.out_len(n, speed) if n else 0 for n in LENGTHS]
    for b, d, (y, dd), a in zip(batch, bdelta, solo, again):
        assert np.array_equal(b, y) and np.array_equal(d, dd) and np.array_equal(b, a)
    # NaN behind every row's length in one padded buffer
    plan = S.TimescalePlan(speed, mode)
    at = [i for i, n in enumerate(LENGTHS) if n]
    buf = np.full((len(at), max(LENGTHS) + 5), np.nan, dtype=np.float32)
    for r, i in enumerate(at):
        buf[r, :LENGTHS[i]] = rows[i]
    lens = [LENGTHS[i] for i in at]
    M = [plan.out_len(n) for n in lens]
    zero = [0] * len(at)
    ys, ds = dev.run_rows(plan, buf, zero, lens, zero, [plan.frames(m) for m in M], zero, zero, M, lens)
    for r, i in enumerate(at):
        assert not np.isnan(ys[r]).any() and np.array_equal(ys[r], batch[i])
        assert mode == "interp" or np.array_equal(ds[r], bdelta[i])


@pytest.mark.parametrize("W,D,N,chunks", [(64, 16, 5000, (1, 777)), (1024, 512, 20000, (777, 512 * 5, 20000))])
def test_stream_joined_equals_the_whole_bit_for_bit(dev, W, D, N, chunks):
    for speed in (0.8, 1.25):
        x = noise(N, 3)
        whole, delta = dev.time_scale(x, speed, "wsola", W, D, return_delta=True)
        for step in chunks:
            st = dev.stream(speed, W, D)
            parts, starts = [], []
            for i in range(0, N, step):
                starts.append(st.emitted)
                parts.append(st.push(x[i:i + step], i + step >= N))
            joined = np.concatenate(parts)
            print(f"stream W {W} D {D} speed {speed} chunk {step}: {len(parts)} pushes, {sum(p.shape[0] > 0 for p in parts)} with samples, "
                  f"{joined.shape[0]} of {whole.shape[0]} samples")
            assert starts == [int(v) for v in np.cumsum([0] + [p.shape[0] for p in parts[:-1]])]
            assert joined.dtype == np.float32 and np.array_equal(joined, whole)
            assert st.decided == delta.shape[0] and st.delta_last == int(delta[-1])
    with pytest.raises(ValueError, match="cannot stream"):
        dev.stream(0.8, mode="interp")


def test_wrapper_refuses_a_window_that_misses_a_sample(dev):
    plan = S.TimescalePlan(0.8, "wsola", 64, 16)
    buf = np.zeros((1, 600), dtype=np.float32)
    with pytest.raises(ValueError, match="the window holds"):
        dev.run_rows(plan, buf, [0], [600], [0], [plan.ready_frames(600) + 1], [0], [0], [0], [None])


def test_refusals_through_the_binding():
    from test_timescale_cpu import refusals
    refusals()
