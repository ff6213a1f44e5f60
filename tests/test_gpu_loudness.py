"""dia_loudness on the MI355X (csrc/loudness.hip, DESIGN.md "Loudness") against the float64 restatement of tests/loudness_ref.py:
the step sums and the integrated loudness (the device's deviation from the sequential float64 recursion must be 1000 x smaller than
that of the same recursion with a float32 state, both computed here), the peaks (the sample peak exactly, the true peak within the
fp32 dot-product bound), bitwise reproducibility across batches, the gain, and normalize()."""
import functools
import math

import numpy as np
import pytest
import torch

import loudness_ref as R
from dia_hip import loudness as S

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
U = 2.0 ** -24


def lengths(rate):
    p = S.loudness_plan(rate)
    return [0, 1, p.chunk - 1, p.step, p.block - 1, p.block, p.block + p.step - 1, 7 * p.step + p.chunk + 3]


@functools.lru_cache(maxsize=None)
def cases(rate):
    """the rows of one rate with their references (tests/loudness_ref.case: computed once, read-only)"""
    return [R.case(rate, n, 100 + i) for i, n in enumerate(lengths(rate))]


@pytest.fixture(scope="module")
def meter():
    return S.DeviceLoudness(DEV)


@pytest.fixture(scope="module")
def reports(meter):
    """the ragged batch of every rate, measured once"""
    return {rate: meter.measure([c[0] for c in cases(rate)], rate) for rate in R.GPU_RATES}


def rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("rate", R.GPU_RATES)
def test_step_sums_against_the_sequential_float64_recursion(reports, rate):
    p = S.loudness_plan(rate)
    for (x, seq, seq32), rep in zip(cases(rate), reports[rate]):
        assert rep["steps"].dtype == np.float64 and rep["steps"].shape == (x.shape[0] // p.step,) == seq.shape
        if seq.shape[0] == 0:
            continue
        dev, f32 = rel(rep["steps"], seq), rel(seq32, seq)
        print(f"{rate} Hz, {x.shape[0]} samples ({seq.shape[0]} steps, chunk {p.chunk} x {p.chunks}): device {dev:.2e} relative, "
              f"float32 state {f32:.2e}, ratio {f32 / max(dev, 1e-300):.1e}")
        assert dev * 1000.0 <= f32


@pytest.mark.parametrize("rate", R.GPU_RATES)
def test_integrated_loudness_against_the_reference(reports, rate):
    p = S.loudness_plan(rate)
    seen = 0
    for (x, seq, seq32), rep in zip(cases(rate), reports[rate]):
        want = R.integrated(seq, p.step)
        if x.shape[0] < p.block:
            assert rep["loudness"] == -math.inf and want == -math.inf
            continue
        dev, f32 = abs(rep["loudness"] - want), abs(R.integrated(seq32, p.step) - want)
        print(f"{rate} Hz, {x.shape[0]} samples: {rep['loudness']:.6f} LUFS, device off by {dev:.2e} dB, float32 state by {f32:.2e} dB")
        assert math.isfinite(want) and dev * 1000.0 <= f32
        seen += 1
    assert seen == 3                                                           # a block, a block and most of a step, seven steps


@pytest.mark.parametrize("rate", R.GPU_RATES)
def test_peaks(reports, rate):
    p = S.loudness_plan(rate)
    gamma = p.nt * U / (1.0 - p.nt * U)
    for (x, _, _), rep in zip(cases(rate), reports[rate]):
        if x.shape[0] == 0:
            assert rep["sample_peak"] == -math.inf and rep["true_peak"] == -math.inf
            continue
        sp = float(np.abs(x).max())
        assert rep["sample_peak"] == R.db(sp)                                  # exact
        y, s = R.oversampled(x, p.nt, p.first, p.bank32)
        assert y.shape == (4 * x.shape[0],)
        lo, hi = max(sp, float((np.abs(y) - gamma * s).max())), max(sp, float((np.abs(y) + gamma * s).max()))
        got = 10.0 ** (rep["true_peak"] / 20.0)
        print(f"{rate} Hz, {x.shape[0]} samples: sample peak {rep['sample_peak']:.4f} dBFS, true peak {rep['true_peak']:.4f} dBTP, "
              f"|device - float64| {abs(got - max(sp, float(np.abs(y).max()))):.2e} (bound {gamma * s.max():.2e})")
        assert lo * (1 - 1e-12) <= got <= hi * (1 + 1e-12)
        # the full float64 bank: the compact fp32 bank differs from it by one rounding per tap
        assert abs(got - R.true_peak(x)) <= (gamma + U) * float(s.max()) * (1 + 1e-9)


def test_impulse_and_intersample_crest_separate_the_peaks(meter):
    imp = np.zeros(4800, dtype=np.float32)
    imp[2000] = 0.5
    crest = R.sine(48000, 12000.0, 0.1, 1.0, math.pi / 4)                      # +-0.7071 samples, the crest of 1.0 between them
    a, b = meter.measure([imp, crest], 48000)
    print(f"impulse: sample {a['sample_peak']:.4f}, true {a['true_peak']:.4f}; fs/4 sine at 45 deg: sample {b['sample_peak']:.4f}, "
          f"true {b['true_peak']:.4f}")
    # phase 0 of the bank is 0.99 at its centre: the oversampled impulse peaks BELOW the sample, and the true peak is the larger
    assert a["sample_peak"] == R.db(0.5) and a["true_peak"] == a["sample_peak"]
    assert abs(b["sample_peak"] - (-3.0103)) < 1e-3 and 2.9 < b["true_peak"] - b["sample_peak"] < 3.2
    assert abs(b["true_peak"] - R.db(R.true_peak(crest))) < 1e-4


@pytest.mark.parametrize("rate", [11025, 44100])
def test_every_row_of_a_batch_equals_its_solo_run(meter, reports, rate):
    rows = [c[0] for c in cases(rate)]
    for x, rep in zip(rows, reports[rate]):
        solo = meter.measure(x, rate)
        assert np.array_equal(solo["steps"], rep["steps"]) and solo["true_peak"] == rep["true_peak"]
        assert solo["sample_peak"] == rep["sample_peak"] and (solo["loudness"] == rep["loudness"])
    back = meter.measure(rows[::-1], rate)[::-1]                               # another place in another batch
    for a, b in zip(back, reports[rate]):
        assert np.array_equal(a["steps"], b["steps"]) and a["true_peak"] == b["true_peak"] and a["sample_peak"] == b["sample_peak"]


def test_65_short_rows_take_two_launches(meter):
    rate = 8000
    rows = [R.speechlike(800 + 13 * i, 500 + i) for i in range(65)]
    reps = meter.measure(rows, rate)
    outs = meter.gain(rows, -3.5)
    assert len(reps) == 65 and len(outs) == 65
    g = 10.0 ** (-3.5 / 20.0)
    for i in (0, 31, 63, 64):
        solo = meter.measure(rows[i], rate)
        assert np.array_equal(solo["steps"], reps[i]["steps"]) and solo["true_peak"] == reps[i]["true_peak"]
        assert rel(reps[i]["steps"], R.step_sums(rows[i], rate)) < 1e-12
    for x, y in zip(rows, outs):
        assert np.array_equal(y, R.apply_gain(x, g))
    assert np.array_equal(meter.gain(rows[64], -3.5), outs[64])


def test_apply_is_one_rounding_and_writes_nothing_else(meter):
    n = [5000, 1, 3000, 2049]
    xs = [R.speechlike(v, 900 + i, level=0.3) for i, v in enumerate(n)]
    xs[0][:4] = [1.0, -1.0, 1e-39, 3.4e38]                                     # a subnormal and a product that overflows to inf
    off, cnt, gain = [1000, 0, 0, 2048], [4000, 1, 0, 1], [10.0 ** (7.3 / 20.0), 0.25, 3.0, 1.0 / 3.0]
    x = torch.from_numpy(meter._pack(xs)).to(DEV)
    canary = np.float32(777.0)
    y = torch.full((4, 4100), float(canary), dtype=torch.float32, device=DEV)
    meter.launch_apply(x, y, n, off, cnt, gain)
    yh = y.cpu().numpy()
    for b in range(4):
        with np.errstate(over="ignore"):
            want = (xs[b][off[b]:off[b] + cnt[b]].astype(np.float64) * gain[b]).astype(np.float32)
        assert np.array_equal(yh[b, :cnt[b]], want) and (yh[b, cnt[b]:] == canary).all()
    assert (yh[2] == canary).all()                                             # the row of no outputs
    y0 = torch.full((4, 4100), float(canary), dtype=torch.float32, device=DEV)
    meter.launch_apply(x, y0, n, [0, 0, 0, 0], [4, 0, 0, 0], [2.0, 1.0, 1.0, 1.0])
    with np.errstate(over="ignore"):
        assert np.array_equal(y0.cpu().numpy()[0, :4], (xs[0][:4].astype(np.float64) * 2.0).astype(np.float32))


def test_normalize(meter):
    rate = 44100
    p = S.loudness_plan(rate)
    plain = R.speechlike(rate, 41)                                             # about -21 LUFS, peaks far below the ceiling
    click = R.speechlike(rate, 42, level=0.01)
    click[30000:30004] = [0.9, -0.8, 0.7, -0.6]                                # -41 LUFS with a peak near full scale: limited
    short = R.speechlike(p.block - 1, 43)                                      # no block: -inf
    silent = np.zeros(rate, dtype=np.float32)
    (a, b, c, d), (ra, rb, rc, rd) = meter.normalize([plain, click, short, silent], rate, target=-23.0, peak=-1.0)
    ma, mb = meter.measure([a, b], rate)
    print(f"plain: {ra['loudness']:.4f} LUFS, gain {ra['gain_db']:.4f} dB -> {ma['loudness']:.6f}; click: {rb['loudness']:.4f} LUFS, true peak "
          f"{rb['true_peak']:.4f}, gain {rb['gain_db']:.4f} dB (limited) -> {mb['loudness']:.4f} LUFS, true peak {mb['true_peak']:.6f}")
    assert not ra["limited"] and abs(ma["loudness"] - (-23.0)) <= 1e-3 and ma["true_peak"] <= -1.0
    assert ra["gain_db"] == -23.0 - ra["loudness"] and np.array_equal(a, R.apply_gain(plain, 10.0 ** (ra["gain_db"] / 20.0)))
    assert rb["limited"] and rb["gain_db"] == -1.0 - rb["true_peak"] and rb["gain_db"] < -23.0 - rb["loudness"]
    assert abs(mb["true_peak"] - (-1.0)) <= 1e-3 and mb["loudness"] < -23.0
    assert c is short and rc["loudness"] == -math.inf and rc["gain_db"] == 0.0 and not rc["limited"]
    assert d is silent and rd["loudness"] == -math.inf and rd["gain_db"] == 0.0
    assert abs(ra["loudness"] - R.loudness(plain, rate)) < 1e-9


def test_normalize_trims_in_the_same_launch(meter):
    rate = 8000
    p = S.loudness_plan(rate)
    x = np.concatenate([np.zeros(5 * p.step, dtype=np.float32), R.speechlike(6 * p.step, 44), np.zeros(4 * p.step + 123, dtype=np.float32)])
    y, r = meter.normalize(x, rate, target=-20.0, trim_db=-60.0, trim_pad=1)
    # the bounds from the REFERENCE's step sums.  The step behind the passage is not silent after the K-weighting: the high-pass
    # rings on from the passage's DC offset, so how many trailing steps go is the filter's answer, not 4
    start, stop = R.trim(R.step_sums(x, rate), p.step, x.shape[0], -60.0, 1)
    assert (start, stop) == tuple(r["kept"]) and start == 4 * p.step and 12 * p.step <= stop < x.shape[0] and stop % p.step == 0
    assert abs(r["loudness"] - R.loudness(x, rate)) < 1e-9                     # measured before the trim
    assert np.array_equal(y, R.apply_gain(x, 10.0 ** (r["gain_db"] / 20.0), start, stop))
    y0, r0 = meter.normalize(x, rate, target=-20.0)
    assert y0.shape == x.shape and r0["kept"] == [0, x.shape[0]] and np.array_equal(y0[start:stop], y)


def test_value_errors(meter):
    f = np.zeros(100, dtype=np.float32)
    for bad in (np.zeros((2, 100), dtype=np.float32), np.zeros(100, dtype=np.int16)):
        with pytest.raises(ValueError, match="expected mono float samples"):
            meter.measure(bad, 44100)
    with pytest.raises(ValueError, match="sample rate"):
        meter.measure(f, 10)
    with pytest.raises(ValueError, match="not finite"):
        meter.normalize(f, 44100, target=math.nan)
    with pytest.raises(ValueError, match="trim_pad"):
        meter.normalize(f, 44100, trim_db=-60.0, trim_pad=-1)
    with pytest.raises(ValueError, match="not finite"):
        meter.gain(f, math.inf)
    assert meter.measure([], 44100) == [] and meter.normalize([], 44100) == ([], [])
