"""Host side of the loudness meter (dia_hip/loudness.py, DESIGN.md "Loudness"), no GPU: the float64 restatement of
tests/loudness_ref.py on the standard's table and on the 997 Hz sine of EBU Tech 3341, the gating on hand-made step sums, the plan's
chunk grid and its transition matrices (an emulation of the device's scheme against the sequential recursion), the gain rule, the
trim, the wiring into Dia and cli.py, and the C ABI's struct and validation."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import loudness_ref as R
from dia_hip import binding as hb
from dia_hip import loudness as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES = (8000, 11025, 22050, 44100, 48000)


# ---------------------------------------------------------------------------------------------- coefficients and the sine
def test_coefficients_at_48k_are_the_standards_table():
    sb, sa, hb_, ha = R.coefficients(48000)
    pb, pa, qb, qa = S.k_weighting(48000)
    for got, mine, want in ((sb, pb, "shelf_b"), (sa, pa, "shelf_a"), (hb_, qb, "hp_b"), (ha, qa, "hp_a")):
        for g, m, w in zip(got, mine, R.TABLE_48K[want]):
            assert abs(g - w) <= 1e-12 and abs(m - w) <= 1e-12, (want, g, m, w)


@pytest.mark.parametrize("rate", [48000, 44100])
def test_full_scale_997_hz_sine_reads_minus_3_01(rate):
    x = R.sine(rate, 997.0, 2.0)
    got = R.loudness(x, rate)
    mine = S.integrated(R.step_sums(x, rate), S.loudness_plan(rate).step)
    print(f"997 Hz full scale at {rate} Hz: {got:.4f} LKFS (restatement), {mine:.4f} (dia_hip gating)")
    assert abs(got - (-3.01)) <= 0.1 and abs(mine - got) <= 1e-9           # 0.1 LU: EBU Tech 3341


# ---------------------------------------------------------------------------------------------- gating
def _level(lkfs, step):
    """the sum of squares of one step at that K-weighted level"""
    return 10.0 ** ((lkfs + 0.691) / 10.0) * step


@pytest.mark.parametrize("fn", [R.integrated, S.integrated], ids=["restatement", "dia_hip"])
def test_gating_cases(fn):
    step = 4800
    loud, quiet = _level(-20.0, step), _level(-80.0, step)
    # a loud passage followed by -80 LKFS noise reads the loud passage's level: the noise blocks fall to the absolute gate, the
    # three blocks that straddle the edge (-21.2, -23.0, -26.0 LKFS) stay above the relative gate and pull the mean down a little
    got = fn([loud] * 20 + [quiet] * 20, step)
    z = [loud] * 17 + [(3 * loud + quiet) / 4, (2 * loud + 2 * quiet) / 4, (loud + 3 * quiet) / 4]
    want = -0.691 + 10.0 * math.log10(sum(z) / len(z) / step)
    assert abs(got - want) <= 1e-9 and -20.5 < got < -20.0
    assert abs(fn([loud] * 20, step) - (-20.0)) <= 1e-9
    # a passage 15 LU down falls to the relative gate
    assert abs(fn([loud] * 20 + [_level(-35.0, step)] * 20, step) - fn([loud] * 20 + [quiet] * 20, step)) <= 0.05
    assert abs(fn([loud] * 4, step) - (-20.0)) <= 1e-9                     # one block exactly
    assert fn([loud] * 3, step) == -math.inf                               # one sample short of a block: three whole steps
    assert fn([], step) == -math.inf
    assert fn([_level(-71.0, step)] * 12, step) == -math.inf               # every block below -70


def test_one_sample_short_of_a_block_has_three_steps():
    for rate in RATES:
        p = S.loudness_plan(rate)
        assert p.block == 4 * p.step and (p.block - 1) // p.step == 3 and p.block // p.step == 4
    x = R.sine(8000, 997.0, 0.4)
    assert x.shape[0] == 3200 and math.isfinite(R.loudness(x, 8000)) and R.loudness(x[:-1], 8000) == -math.inf


# ---------------------------------------------------------------------------------------------- the plan
@pytest.mark.parametrize("rate", RATES)
def test_chunk_grid_never_straddles_a_step(rate):
    p = S.LoudnessPlan(rate)
    assert p.step == R.step_of(rate) == (1103 if rate == 11025 else rate // 10)
    assert 1 <= p.chunks <= S.MAX_CHUNKS and p.chunks == -(-p.step // p.chunk)
    assert p.chunk % 2 == 1 or p.chunks == 1                               # odd: a wave's lanes hit 64 LDS banks
    n = 3 * p.step + p.step // 2
    b = p.chunk_bounds(n)
    assert len(b) == 3 * p.chunks and b[0][0] == 0 and b[-1][1] == 3 * p.step
    for (lo, hi), nxt in zip(b, b[1:] + [(3 * p.step, None)]):
        assert lo < hi <= lo + p.chunk and hi == nxt[0] and lo // p.step == (hi - 1) // p.step
    assert p.table.shape == (42 + 16 * p.chunks,) and p.table.dtype == np.float64
    assert np.array_equal(p.table[42:58].reshape(4, 4), np.eye(4))         # A^0


def test_plan_refusals():
    for bad in (0, 70, 192005, 44100.5, True):
        with pytest.raises(ValueError):
            S.LoudnessPlan(bad)
    assert S.LoudnessPlan(192000).chunks == 64 and S.LoudnessPlan(75).step == 8


@pytest.mark.parametrize("rate", [11025, 44100])
def test_chunk_scheme_equals_the_sequential_recursion(rate):
    """the device's scheme, emulated in float64 from the plan's table, against the sample-by-sample recursion, and the same recursion
    with a float32 state for scale"""
    x, seq, seq32 = R.case(rate, rate // 2 + 37, 5)
    got = R.chunked_step_sums(S.loudness_plan(rate), x)
    err, err32 = np.abs(got - seq).max() / seq.max(), np.abs(seq32 - seq).max() / seq.max()
    print(f"{rate} Hz: chunk scheme {err:.2e} relative, float32 state {err32:.2e}")
    assert err <= 1e-12 and err * 1000 <= err32


# ---------------------------------------------------------------------------------------------- gain, trim, inputs
@pytest.mark.parametrize("fn", [R.choose_gain, S.choose_gain], ids=["restatement", "dia_hip"])
def test_gain_rule(fn):
    assert fn(-30.0, -12.0, -23.0, -1.0) == (7.0, False)
    assert fn(-30.0, -8.0, -23.0, -1.0) == (7.0, False)                    # lands exactly on the ceiling: not over it
    g, lim = fn(-30.0, -5.0, -23.0, -1.0)
    assert g == 4.0 and lim
    g, lim = fn(-10.0, 0.5, -23.0, -1.0)                                   # attenuation
    assert g == -13.0 and not lim
    assert fn(-math.inf, -20.0, -23.0, -1.0) == (0.0, False)


@pytest.mark.parametrize("fn", [R.trim, S.trim_bounds], ids=["restatement", "dia_hip"])
def test_trim_arithmetic(fn):
    step = 800
    q, l = _level(-75.0, step), _level(-20.0, step)
    steps = [q] * 5 + [l] * 6 + [q] * 4
    n = 15 * step + 123
    assert fn(steps, step, n, -60.0, 1) == (4 * step, 12 * step)
    assert fn(steps, step, n, -60.0, 0) == (5 * step, 11 * step)
    assert fn(steps, step, n, -60.0, 4) == (1 * step, n)                   # the pad covers the tail: the samples behind it stay
    assert fn(steps, step, n, -60.0, 9) == (0, n)
    assert fn(steps, step, n, -90.0, 1) == (0, n)                          # nothing is that quiet
    assert fn([q] * 6, step, 6 * step, -60.0, 1) == (0, 6 * step)          # everything is: nothing goes
    assert fn([l, q, q, l], step, 4 * step + 5, -60.0, 0) == (0, 4 * step + 5)        # quiet steps inside stay


def test_trim_none_and_bad_pad():
    assert S.trim_bounds([1.0], 800, 900, None) == (0, 900)
    with pytest.raises(ValueError):
        S.trim_bounds([1.0], 800, 900, -60.0, -1)


def test_input_rules():
    f = np.zeros(10, dtype=np.float32)
    single, rows = S.as_rows(f)
    assert single and rows[0][1].shape == (10,)
    assert S.as_rows([f, f[None]])[1][1][1].shape == (10,)
    for bad in (np.zeros((2, 10), dtype=np.float32), np.zeros(10, dtype=np.int16), np.zeros((1, 1, 4), dtype=np.float32), [f, 3]):
        with pytest.raises(ValueError, match="expected mono float samples"):
            S.as_rows(bad)


def test_device_loudness_needs_a_hip_device():
    with pytest.raises(hb.DiaHipError, match="no CPU fallback"):
        S.DeviceLoudness("cpu")


def test_reference_gain_is_one_rounding():
    x = np.array([0.1, -0.3, 1.0, 3e-39], dtype=np.float32)
    g = 10.0 ** (-7.3 / 20.0)
    assert np.array_equal(R.apply_gain(x, g, 1, 3), (x[1:3].astype(np.float64) * g).astype(np.float32))


# ---------------------------------------------------------------------------------------------- Dia and cli.py
class _FakeCodec:
    class cfg:
        sample_rate = 44100

    has_encoder = True

    def __init__(self):
        self.calls = []

    def decode(self, codes):
        return np.full(codes.shape[-1] * 512, 0.5, dtype=np.float32)

    def decode_batch(self, batch):
        return [self.decode(c) for c in batch]

    def time_scale(self, waves, speed, mode="interp", window=1024, tolerance=512):
        self.calls.append(("time_scale", speed, mode))
        return waves

    def resample(self, waves, rate_in, rate_out):
        self.calls.append(("resample", rate_in, rate_out))
        return waves

    def normalize_loudness(self, waves, rate=None, target=-23.0, peak=-1.0, **kw):
        self.calls.append(("normalize", rate, target, peak))
        return waves, None

    def encode(self, w):
        self.calls.append(("encode", w.shape[0]))
        return np.zeros((1, 9, 2), dtype=np.int64)


def test_dia_loudness_wiring():
    from dia_hip import callers
    from dia_hip import model as M
    assert M.Dia.loudness_target is None and M.Dia.peak_ceiling == -1.0
    dia = object.__new__(M.Dia)
    dia.codec, dia.dac_model = _FakeCodec(), None
    codes = np.zeros((1, 9, 4), dtype=np.int64)
    assert dia._generate_output(codes).shape == (2048,) and dia.codec.calls == []          # default: what it was
    dia.loudness_target, dia.speed_factor, dia.output_sample_rate = -16.0, 0.8, 16000
    dia._generate_output(codes)                                                             # last, at the delivered rate
    assert dia.codec.calls == [("time_scale", 0.8, "interp"), ("resample", 44100, 16000), ("normalize", 16000, -16.0, -1.0)]
    dia.codec.calls.clear()
    dia.speed_factor, dia.output_sample_rate, dia.peak_ceiling = 1.0, None, -2.0
    dia.generate_batch = lambda texts, *a, **k: [codes, codes[:, :, :2]]
    assert len(dia.generate_audio_batch(["a", "b"])) == 2 and dia.codec.calls == [("normalize", 44100, -16.0, -2.0)]
    dia.codec.calls.clear()
    dia._generate_output(codes, normalize=False)
    assert dia.codec.calls == []
    with pytest.raises(ValueError, match="loudness_target cannot stream"):                 # up front: nothing is generated
        dia.stream_audio(["a"])
    for bad in ("loud", True, math.nan, math.inf):
        dia.loudness_target = bad
        with pytest.raises(ValueError, match="loudness_target"):
            dia._generate_output(codes)
    dia.loudness_target, dia.peak_ceiling = -16.0, None
    with pytest.raises(ValueError, match="peak_ceiling"):
        dia._generate_output(codes)
    dia.peak_ceiling = -1.0
    # the prompt side: after the conversion to the codec's rate, before the encoder
    dia.encode_audio(np.zeros(600, dtype=np.float32))
    assert dia.codec.calls == [("encode", 600)]
    dia.codec.calls.clear()
    dia.encode_audio(np.zeros(600, dtype=np.float32), normalize_lufs=-23)
    assert dia.codec.calls == [("normalize", 44100, -23.0, -1.0), ("encode", 600)]
    # a codec object without the meter cannot serve the request: said, not ignored
    dia.codec = type("NoMeter", (), {"cfg": dia.codec.cfg, "decode": lambda self, c: np.zeros(4, dtype=np.float32)})()
    with pytest.raises(RuntimeError, match="needs the native codec's loudness meter"):
        dia._generate_output(codes)
    dia.codec, dia.dac_model = None, object()
    with pytest.raises(RuntimeError, match="needs the native codec's loudness meter"):
        dia._generate_output(codes)
    with pytest.raises(RuntimeError, match="normalize_lufs needs the native codec"):
        dia.load_audio("x.wav", normalize_lufs=-23.0)
    # the long-form join: the joined waveform, once
    dia.codec, dia.dac_model = _FakeCodec(), None
    orig = callers.generate_long_codes
    callers.generate_long_codes = lambda d, text, **kw: [codes, codes]
    try:
        y = callers.generate_long(dia, "x")
        assert y.shape == (2 * 2048 + 8820,) and dia.codec.calls == [("normalize", 44100, -16.0, -1.0)]
        dia.loudness_target = None
        dia.codec.calls.clear()
        assert callers.generate_long(dia, "x").shape == y.shape and dia.codec.calls == []
    finally:
        callers.generate_long_codes = orig


def test_cli_loudness_rules(tmp_path, capsys):
    import cli
    p = cli.build_parser()
    a = p.parse_args(["x", "--output", "a.wav", "--loudness", "-16", "--peak-ceiling", "-2"])
    assert a.loudness == -16.0 and a.peak_ceiling == -2.0 and p.parse_args(["x"]).loudness is None
    assert p.parse_args(["--measure-loudness", "a.wav"]).measure_loudness == "a.wav"
    me = __file__
    for argv in (["x", "--output", "a.wav", "--loudness", "-16"],                                              # no --codec-path
                 ["x", "--codes-output", "a.npy", "--loudness", "-16", "--codec-path", me],                    # no --output
                 ["x", "--output", "a.wav", "--peak-ceiling", "-2", "--codec-path", me],                       # a ceiling without a target
                 ["x", "--output", "a.wav", "--loudness", "nan", "--codec-path", me],
                 ["x", "--output", "a.wav", "--loudness", "-16", "--peak-ceiling", "inf", "--codec-path", me],
                 ["x", "--output", "a.wav", "--loudness", "-16", "--stream-chunk", "8", "--codec-path", me],   # cannot stream
                 ["--time-scale", me, "--speed-factor", "0.9", "--output", "a.wav", "--loudness", "-16"],
                 ["--compare-audio", me, me, "--loudness", "-16"],
                 ["--measure-loudness", me, "--loudness", "-16"],
                 ["--measure-loudness", me, "--output", "a.wav"],
                 ["--measure-loudness", me, "--codec-path", me],
                 ["--measure-loudness", me, "--compare-audio", me, me],
                 ["--measure-loudness", me, "--speed-factor", "0.9"],
                 ["--measure-loudness", me, "--output-rate", "16000"]):
        with pytest.raises(SystemExit):
            cli.main(argv)
    # a file that cannot be read: reported, exit code 1
    assert cli.main(["--measure-loudness", str(tmp_path / "missing.wav")]) == 1
    assert "Error measuring" in capsys.readouterr().out


# ---------------------------------------------------------------------------------------------- the C ABI
def refusals():
    """every DIA_E_ARG condition of dia_loudness, through the binding; they are answered before any HIP call"""
    L = hb.lib()
    fn = L.dia_loudness

    def err(a):
        assert fn(ctypes.byref(a), None) == -1                                 # DIA_E_ARG
        return L.dia_last_error().decode()

    assert fn(None, None) == -1 and "null argument" in L.dia_last_error().decode()
    assert "null pointer" in err(hb.LoudnessArgs())                            # the zeroed struct
    i32, f64 = (ctypes.c_int32 * 2), (ctypes.c_double * 2)
    first = (ctypes.c_int32 * 4)(-6, -5, -5, -5)

    def meas(**kw):
        f = dict(x=0x1000, steps=0x2000, peaks=0x3000, ws=0x4000, table=0x5000, bank=0x6000, ws_doubles=S.ws_doubles(2, 3, 42),
                 mode=hb.LOUD_MEASURE, B=2, ldx=14000, ld_steps=3, step=4410, chunk=105, chunks=42, nt=13, first=first,
                 len=i32(14000, 0))
        f.update(kw)
        return hb.LoudnessArgs(**f)

    def app(**kw):
        f = dict(x=0x1000, y=0x2000, mode=hb.LOUD_APPLY, B=2, ldx=5000, ldy=4000, len=i32(5000, 100), in_off=i32(1000, 0),
                 out_count=i32(4000, 100), gain=f64(0.5, 2.0))
        f.update(kw)
        return hb.LoudnessArgs(**f)

    for a in (meas, app):
        assert "x and the host array len" in err(a(x=None)) and "x and the host array len" in err(a(len=None))
        assert "mode = 2" in err(a(mode=2)) and "mode = -1" in err(a(mode=-1))
        assert "B = 0" in err(a(B=0)) and "B = 65" in err(a(B=65))
        assert "ldx = 0" in err(a(ldx=0)) and "ldx = 16777217" in err(a(ldx=(1 << 24) + 1))
        assert "row 1: len = -1" in err(a(len=i32(100, -1))) and "row 0: len = 14001" in err(a(len=i32(14001, 0), ldx=14000))
    for name in ("steps", "peaks", "ws", "table", "bank", "first"):
        assert "DIA_LOUD_MEASURE needs" in err(meas(**{name: None}))
    assert "step = 7" in err(meas(step=7)) and "step = 19201" in err(meas(step=19201))
    assert "chunk = 0" in err(meas(chunk=0)) and "chunk = 4411" in err(meas(chunk=4411))
    assert "chunks = 41 is not ceil" in err(meas(chunks=41)) and "or above 64" in err(meas(chunk=63, chunks=70))
    assert "nt = 0" in err(meas(nt=0)) and "nt = 33" in err(meas(nt=33))
    assert "phase 0 reads" in err(meas(first=(ctypes.c_int32 * 4)(-33, 0, 0, 0))) and "phase 3 reads" in err(meas(first=(ctypes.c_int32 * 4)(0, 0, 0, 21)))
    assert "ld_steps = 0" in err(meas(ld_steps=0))
    assert "row 0: 3 whole steps exceed ld_steps = 2" in err(meas(ld_steps=2))
    assert "ws_doubles" in err(meas(ws_doubles=S.ws_doubles(2, 3, 42) - 1))
    for name in ("y", "in_off", "out_count", "gain"):
        assert "DIA_LOUD_APPLY needs" in err(app(**{name: None}))
    assert "y must not be x" in err(app(y=0x1000))
    assert "ldy = 0" in err(app(ldy=0)) and "ldy = 16777217" in err(app(ldy=(1 << 24) + 1))
    assert "row 1: in_off = -1" in err(app(in_off=i32(0, -1)))
    assert "row 0: out_count = 4001" in err(app(out_count=i32(4001, 0))) and "row 1: out_count = -2" in err(app(out_count=i32(0, -2)))
    assert "row 0: samples [1001, 5001) lie beyond len = 5000" in err(app(in_off=i32(1001, 0)))
    assert "row 1: the gain is not finite" in err(app(gain=f64(1.0, math.inf))) and "row 0: the gain" in err(app(gain=f64(math.nan, 1.0)))
    return L


def test_abi_struct_and_validation(tmp_path):
    src = open(os.path.join(ROOT, "include", "dia_hip.h")).read()
    assert "int dia_loudness(const dia_loudness_args* a, void* stream);" in src
    assert "dia_loudness" in hb.EXPORTS
    c = tmp_path / "s.c"
    c.write_text('#include <stdio.h>\n#include "dia_hip.h"\nint main(void){ printf("%zu %d %d %d %d %d %d %d %d %d %ld\\n", '
                 'sizeof(dia_loudness_args), DIA_LOUD_MEASURE, DIA_LOUD_APPLY, DIA_LOUD_MAX_ROWS, DIA_LOUD_MAX_T, DIA_LOUD_MIN_STEP, '
                 'DIA_LOUD_MAX_STEP, DIA_LOUD_MAX_CHUNKS, DIA_LOUD_MAX_TAPS, DIA_LOUD_TABLE_DOUBLES(42), '
                 '(long)DIA_LOUD_WS_DOUBLES(3, 20, 42)); return 0; }\n')
    exe = tmp_path / "s"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    p = S.loudness_plan(44100)
    assert got == [ctypes.sizeof(hb.LoudnessArgs), hb.LOUD_MEASURE, hb.LOUD_APPLY, S.MAX_ROWS, S.MAX_T, S.MIN_STEP, S.MAX_STEP,
                   S.MAX_CHUNKS, 32, p.table.shape[0], S.ws_doubles(3, 20, 42)]
    L = refusals()
    assert L.dia_abi_version() == hb.ABI_VERSION
