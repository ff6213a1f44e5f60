"""Host side of the speed factor (dia_hip/timescale.py, DESIGN.md "Speed factor"), no GPU: the float64 restatement of
tests/timescale_ref.py against numpy's interp and on WSOLA's own properties, the plan's integer arithmetic, the stream planner
driven by the restatement, the wiring into Dia and cli.py, and the C ABI's struct and validation."""
import ctypes
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import timescale_ref as R
from dia_hip import binding as hb
from dia_hip import timescale as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------- the restatement: interp
@pytest.mark.parametrize("N,speed", [(3001, 0.8), (3001, 0.94), (3001, 1.25), (3001, 5.0), (3001, 7.0), (500, 0.1), (500, 0.05),
                                     (2, 0.8), (1, 0.5), (3, 2.9), (1, 0.1)])
def test_reference_interp_is_numpy_interp_over_linspace(N, speed):
    x = np.random.default_rng(N).standard_normal(N)
    s = min(max(speed, 0.1), 5.0)
    M = int(N / s)
    y = R.interp(x, speed)
    assert R.out_len(N, speed) == M and y.shape == (M,)
    want = np.interp(np.linspace(0, N - 1, M), np.arange(N), x)
    # linspace's j * ((N - 1) / (M - 1)) and the restatement's (j * (N - 1)) / (M - 1) differ by a few ulp of the position
    # (< N * 2^-52), which the steepest slope turns into a value; the interpolation itself adds a few ulp of the largest sample
    bound = 4 * N * 2.0 ** -52 * (np.abs(np.diff(x)).max() if N > 1 else 0.0) + 8 * 2.0 ** -52 * np.abs(x).max()
    err = float(np.abs(y - want).max())
    print(f"ref-interp N {N} speed {speed} -> M {M}: max |diff| {err:.2e} (bound {bound:.2e})")
    assert err <= bound
    # pos_0 = 0 and pos_{M-1} = N - 1 exactly; the last output is (x[N-1] - x[N-2]) * 1 + x[N-2], x[N-1] up to its two roundings
    assert y[0] == x[0] and (M == 1 or N == 1 or abs(y[-1] - x[-1]) <= 2.0 ** -51 * np.abs(x[-2:]).max())


def test_reference_interp_passes_and_clamps():
    x = np.arange(10.0)
    assert R.interp(x, 1.0) is not None and np.array_equal(R.interp(x, 1.0), x)
    assert np.array_equal(R.interp(x[:1], 3.0), x[:1])                         # M = 0: the input
    assert R.interp(x, 100.0).shape == (2,) and R.interp(x, 0.0).shape == (100,)
    assert R.interp(np.ones(1), 0.25).tolist() == [1.0] * 4                    # N = 1


# ---------------------------------------------------------------------------------------------- the restatement: wsola
@pytest.mark.parametrize("W,D,N,speed", [(64, 16, 6000, 0.8), (64, 16, 6000, 0.94), (64, 16, 6000, 1.25), (64, 16, 6000, 2.0),
                                         (1024, 512, 12000, 0.8)])
def test_reference_wsola_reproduces_a_periodic_signal(W, D, N, speed):
    P = 32                                                                     # P | W
    per = np.random.default_rng(3).standard_normal(P)
    x = np.tile(per, N // P + 1)[:N]
    y, delta = R.wsola(x, speed, W, D)
    M = y.shape[0]
    n = M - 3 * W
    err = float(np.abs(y[:n] - np.tile(per, M // P + 2)[:n]).max())
    print(f"ref-wsola periodic W {W} D {D} speed {speed}: M {M}, frames {delta.shape[0]}, max |diff| on [0, {n}) {err:.2e}")
    assert M == int(N / speed) and delta.shape[0] == -(-M // (W // 2)) + 1 and np.abs(delta).max() <= D
    assert err <= 1e-14                                                        # head included


@pytest.mark.parametrize("W,D,f0,speed", [(64, 16, 2205.0, 0.8), (64, 16, 2205.0, 0.94), (64, 16, 2205.0, 1.25),
                                          (1024, 512, 220.0, 0.8), (1024, 512, 220.0, 0.94), (1024, 512, 220.0, 1.25)])
def test_reference_wsola_keeps_a_sine_in_its_bin(W, D, f0, speed):
    """220 Hz at the defaults.  A search of +-16 samples cannot realign a 200-sample period (measured with this restatement: the
    peak moves to 175 / 207 / 275 Hz, with the tempo), so the small window is checked on a period it can hold, 20 samples"""
    rate = 44100
    N = 22050 if W == 64 else 30000
    x = np.sin(2 * np.pi * f0 * np.arange(N) / rate)
    y, _ = R.wsola(x, speed, W, D)
    body = y[2 * W:y.shape[0] - 3 * W]
    L = 1 << int(math.log2(body.shape[0]))
    spec = np.abs(np.fft.rfft(body[:L] * np.hanning(L)))
    peak = int(np.argmax(spec)) * rate / L
    rms = float(np.sqrt(np.mean(body ** 2)))
    print(f"ref-wsola sine W {W} D {D} f0 {f0} speed {speed}: peak {peak:.1f} Hz (bin {rate / L:.1f} Hz), rms {rms:.4f}")
    assert abs(peak - f0) <= rate / L and abs(rms - math.sqrt(0.5)) < 0.005


def test_reference_tie_rule_on_silence():
    y, delta = R.wsola(np.zeros(5000), 0.8, 64, 16)
    assert np.all(delta == 0) and np.all(y == 0.0)
    assert R.candidate_order(2).tolist() == [0, -1, 1, -2, 2]
    c = np.array([1.0, 3.0, 2.0, 3.0, 0.0])                                    # delta -2 .. 2: maxima at -1 and +1
    assert R.pick(c, 2) == -1
    assert R.pick(np.array([5.0, 0.0, 1.0, 0.0, 5.0]), 2) == -2 and R.pick(np.array([5.0, 0.0, 5.0, 0.0, 5.0]), 2) == 0


# ---------------------------------------------------------------------------------------------- the plan
def test_plan_arithmetic():
    for speed in (0.8, 0.94, 1.25, 2.0, 0.1, 5.0, 0.05, 9.0):
        for W, D in ((64, 16), (1024, 512)):
            p = S.TimescalePlan(speed, "wsola", W, D)
            s = min(max(speed, 0.1), 5.0)
            assert p.speed == s and p.hop == W // 2
            for N in (0, 1, 2, 63, 5000, 20000, (1 << 24) - 1):
                M = int(N / s)
                assert p.out_len(N) == M == R.out_len(N, speed)
                assert p.frames(M) == -(-M // (W // 2)) + 1 == R.frames(M, W)
            ks = [0, 1, 2, 3, 7, 100, 12345, 1 << 20]
            for k in ks:                                                       # float64 against exact rational arithmetic on the same double
                assert p.centre(k) == math.floor(Fraction(k * (W // 2)) * Fraction(s) + Fraction(1, 2)) == R.centre(k, W, speed)
            assert p.centres(3, 40).tolist() == [p.centre(k) for k in range(3, 40)]
            # ready_frames never asks for input beyond `got`, and stops only where the next frame would
            for got in (0, 1, W // 2, W + D, 777, 5000, 44100):
                K = p.ready_frames(got)
                assert all(p.need(k) <= got for k in range(K)) and p.need(K) > got
                if K:
                    lo, hi = p.span(0, K)
                    assert hi <= got and lo == -(W // 2) - D
    assert S.TimescalePlan(1.0).identity and S.TimescalePlan(1.0).passes(100)
    assert S.TimescalePlan(0.9999, "interp").passes(100) and not S.TimescalePlan(0.9999, "wsola").passes(100)   # M == N: interp only
    assert S.TimescalePlan(5.0).passes(4) and not S.TimescalePlan(5.0).passes(5)
    w = S.hann(64)
    assert np.array_equal(w, R.window(64)) and np.allclose(w[:32] + w[32:], 1.0, atol=1e-15) and w[0] == 0.0


def test_plan_and_coverage_refusals():
    for kw in (dict(window=96), dict(window=32), dict(window=8192), dict(tolerance=-1), dict(window=64, tolerance=65), dict(mode="fast")):
        with pytest.raises(ValueError):
            S.TimescalePlan(0.8, **{"mode": "wsola", **kw})
    with pytest.raises(ValueError):
        S.TimescalePlan(float("nan"))
    p = S.TimescalePlan(0.8, "wsola", 64, 16)
    S.check_coverage(p, 0, 5000, 0, 10, 0, 9 * 32, 5000)
    with pytest.raises(ValueError, match="outside the range of frames"):
        S.check_coverage(p, 0, 5000, 0, 10, 0, 9 * 32 + 1, 5000)
    with pytest.raises(ValueError, match="outside the range of frames"):
        S.check_coverage(p, 0, 5000, 5, 10, 3 * 32, 10, 5000)                  # frame 3 is not frame k0 - 1
    with pytest.raises(ValueError, match="the window holds"):
        S.check_coverage(p, 0, 200, 0, 10, 0, 0, 5000)
    with pytest.raises(ValueError, match="the window holds"):
        S.check_coverage(p, 300, 4700, 5, 10, 4 * 32, 10, 5000)
    with pytest.raises(ValueError, match="cannot stream"):
        S.TimescaleStream(S.TimescalePlan(0.8, "interp"), None)
    dev = object.__new__(S.DeviceTimescale)                                    # no device: these never reach one
    x = np.ones(7, dtype=np.float32)
    assert dev.time_scale(x, 1.0) is x and dev.time_scale(x, 1.0, "wsola") is x
    assert dev.time_scale(x[:3], 5.0) is not None and dev.time_scale(x[:3], 9.0).shape == (3,)       # M = 0
    assert [w.shape[0] for w in dev.time_scale([x, x[:0]], 1.0)] == [7, 0]
    with pytest.raises(ValueError, match="mono float samples"):
        dev.time_scale(np.ones((2, 5), dtype=np.float32), 0.8)
    with pytest.raises(ValueError, match="cannot stream"):
        dev.stream(0.8, mode="interp")
    st = dev.stream(1.0)
    assert np.array_equal(st.push(x), x) and st.emitted == 7


# ---------------------------------------------------------------------------------------------- the stream planner
@pytest.mark.parametrize("speed", [0.8, 1.25, 0.5, 2.0])
@pytest.mark.parametrize("chunk", [1, 777, 512, None])
def test_stream_joined_equals_the_whole(speed, chunk):
    W, D, N = 64, 16, 5000
    x = np.random.default_rng(5).integers(-8, 9, size=N).astype(np.float64)   # integers: every float64 correlation is exact
    whole, delta = R.wsola(x, speed, W, D)
    calls = []

    def run(win, in_start, k0, k1, delta_prev, out_start, out_count, total):
        assert in_start >= 0 and in_start + win.shape[0] <= (N if total is None else total)
        S.check_coverage(S.TimescalePlan(speed, "wsola", W, D), in_start, win.shape[0], k0, k1, out_start, out_count, total)
        calls.append((k0, k1, out_start, out_count, win.shape[0]))
        return R.stream_run(W, D, speed)(win, in_start, k0, k1, delta_prev, out_start, out_count, total)

    st = S.TimescaleStream(S.TimescalePlan(speed, "wsola", W, D), run)
    step = N if chunk is None else chunk
    parts, starts = [], []
    for i in range(0, N, step):
        starts.append(st.emitted)
        parts.append(st.push(x[i:i + step], i + step >= N))
    joined = np.concatenate(parts)
    assert starts == [int(v) for v in np.cumsum([0] + [p.shape[0] for p in parts[:-1]])]
    assert [c[0] for c in calls] == [0] + [c[1] for c in calls[:-1]] and calls[-1][1] == delta.shape[0]      # every frame once
    assert max(c[4] for c in calls) <= (N if chunk is None else max(step, 1) + 2 * W + 2 * D + int(W * max(speed, 1.0)) + 2)
    assert joined.shape == whole.shape and np.array_equal(joined, whole)
    with pytest.raises(RuntimeError, match="after the final"):
        st.push(x[:1])


def test_stream_of_a_signal_too_short_for_an_output():
    st = S.TimescaleStream(S.TimescalePlan(5.0, "wsola", 64, 16), lambda *a: pytest.fail("no launch"))
    assert st.push(np.ones(2, dtype=np.float32)).shape == (0,)
    assert st.push(np.ones(2, dtype=np.float32), True).tolist() == [1.0] * 4   # M = int(4 / 5) = 0: the input, as time_scale()


# ---------------------------------------------------------------------------------------------- Dia and cli.py
class _FakeCodec:
    class cfg:
        sample_rate = 44100

    def __init__(self):
        self.calls = []

    def decode(self, codes):
        return np.full(codes.shape[-1] * 512, 0.5, dtype=np.float32)

    def decode_batch(self, batch):
        return [self.decode(c) for c in batch]

    def time_scale(self, waves, speed, mode="interp", window=1024, tolerance=512):
        self.calls.append(("time_scale", speed, mode))
        one = lambda w: np.full(int(w.shape[0] / speed), 0.25, dtype=np.float32)
        return [one(w) for w in waves] if isinstance(waves, list) else one(waves)

    def resample(self, waves, rate_in, rate_out):
        self.calls.append(("resample", rate_in, rate_out))
        return waves


def test_dia_speed_factor_wiring():
    from dia_hip import model as M
    assert M.Dia.speed_factor == 1.0 and M.Dia.speed_mode == "interp"
    dia = object.__new__(M.Dia)
    dia.codec, dia.dac_model = _FakeCodec(), None
    codes = np.zeros((1, 9, 4), dtype=np.int64)
    assert dia._generate_output(codes).shape == (2048,) and dia.codec.calls == []          # default: what it was
    dia.speed_factor = 0.8
    assert dia._generate_output(codes).shape == (2560,) and dia.codec.calls == [("time_scale", 0.8, "interp")]
    dia.speed_factor, dia.speed_mode, dia.output_sample_rate = 9.0, "wsola", 16000        # clamped; before the resampler
    dia.codec.calls.clear()
    dia._generate_output(codes)
    assert dia.codec.calls == [("time_scale", 5.0, "wsola"), ("resample", 44100, 16000)]
    dia.generate_batch = lambda texts, *a, **k: [codes, codes[:, :, :2]]
    dia.codec.calls.clear()
    out = dia.generate_audio_batch(["a", "b"])
    assert [w.shape[0] for w in out] == [409, 204] and [c[0] for c in dia.codec.calls] == ["time_scale", "resample"]
    for bad in ("fast", None, True):
        dia.speed_factor = bad
        with pytest.raises(ValueError, match="speed_factor"):
            dia._generate_output(codes)
    dia.speed_factor, dia.speed_mode = 0.9, "psola"
    with pytest.raises(ValueError, match="speed_mode"):
        dia._generate_output(codes)
    dia.speed_mode = "interp"
    with pytest.raises(ValueError, match="cannot stream"):                     # up front: nothing is generated
        dia.stream_audio(["a"])
    # a codec object without the time-scaling cannot serve the request: said, not ignored
    dia.output_sample_rate = None
    dia.codec = type("NoTimescale", (), {"cfg": dia.codec.cfg, "decode": lambda self, c: np.zeros(4, dtype=np.float32)})()
    with pytest.raises(RuntimeError, match="needs the native codec's time-scaling"):
        dia._generate_output(codes)
    dia.codec, dia.dac_model = None, object()
    with pytest.raises(RuntimeError, match="needs the native codec's time-scaling"):
        dia._generate_output(codes)


def test_cli_speed_factor_rules(tmp_path):
    import cli
    p = cli.build_parser()
    a = p.parse_args(["x", "--output", "a.wav", "--speed-factor", "0.9", "--speed-mode", "wsola"])
    assert a.speed_factor == 0.9 and a.speed_mode == "wsola" and p.parse_args(["x"]).speed_factor is None
    me = __file__
    for argv in (["x", "--output", "a.wav", "--speed-factor", "0.9"],                                          # no --codec-path
                 ["x", "--codes-output", "a.npy", "--speed-factor", "0.9", "--codec-path", me],                # no --output
                 ["x", "--output", "a.wav", "--speed-mode", "wsola", "--codec-path", me],                      # a mode without a factor
                 ["x", "--output", "a.wav", "--speed-factor", "nan", "--codec-path", me],
                 ["x", "--output", "a.wav", "--speed-factor", "0.9", "--speed-mode", "fast", "--codec-path", me],
                 ["x", "--output", "a.wav", "--speed-factor", "0.9", "--stream-chunk", "8", "--codec-path", me],                           # interp cannot stream
                 ["x", "--output", "a.wav", "--speed-factor", "0.9", "--speed-mode", "interp", "--stream-chunk", "8", "--codec-path", me],
                 ["--time-scale", me, "--output", "a.wav"],                                                    # no factor
                 ["--time-scale", me, "--speed-factor", "0.9"],                                                # no --output
                 ["--time-scale", me, "--speed-factor", "0.9", "--output", "a.flac"],
                 ["--time-scale", me, "--speed-factor", "0.9", "--output", "a.wav", "--codec-path", me],
                 ["--time-scale", me, "--speed-factor", "0.9", "--output", "a.wav", "--compare-audio", me, me],
                 ["--time-scale", me, "--speed-factor", "0.9", "--output", "a.wav", "--codes-output", "a.npy"],
                 ["--time-scale", me, "--speed-factor", "0.9", "--output", "a.wav", "--output-rate", "16000"],
                 ["--compare-audio", me, me, "--speed-factor", "0.9"]):
        with pytest.raises(SystemExit):
            cli.main(argv)
    # a file that cannot be read: reported, exit code 1, nothing written
    out = tmp_path / "o.wav"
    assert cli.main(["--time-scale", str(tmp_path / "missing.wav"), "--speed-factor", "0.9", "--output", str(out)]) == 1 and not out.exists()


# ---------------------------------------------------------------------------------------------- the C ABI
def refusals():
    """every DIA_E_ARG condition of dia_timescale, through the binding; they are answered before any HIP call"""
    L = hb.lib()
    fn = L.dia_timescale

    def err(a):
        assert fn(ctypes.byref(a), None) == -1                                 # DIA_E_ARG
        return L.dia_last_error().decode()

    assert fn(None, None) == -1 and "null argument" in L.dia_last_error().decode()
    assert "null pointer" in err(hb.TimescaleArgs())                           # the zeroed struct
    i64, i32 = (ctypes.c_int64 * 2), (ctypes.c_int32 * 2)

    def good(**kw):
        f = dict(x=0x1000, y=0x2000, win=0x3000, centre=0x4000, delta=0x5000, mode=hb.TS_WSOLA, B=2, ldx=5000, ldy=6400, ldk=256,
                 window=64, tolerance=16, in_start=i64(0, 0), out_start=i64(0, 32), total=i64(5000, -1), out_total=i64(6250, 6250),
                 k0=i64(0, 2), k1=i64(197, 100), delta_prev=i32(0, 3), in_count=i32(5000, 4000), out_count=i32(6250, 3000))
        f.update(kw)
        return hb.TimescaleArgs(**f)

    assert "x and y are required" in err(good(x=None)) and "x and y are required" in err(good(y=None))
    for name in ("in_start", "out_start", "total", "in_count", "out_count"):
        assert "host arrays" in err(good(**{name: None}))
    for name in ("win", "centre", "delta", "k0", "k1", "delta_prev"):
        assert "DIA_TS_WSOLA needs" in err(good(**{name: None}))
    assert "out_total" in err(good(mode=hb.TS_INTERP, out_total=None))
    assert "mode = 2" in err(good(mode=2)) and "mode = -1" in err(good(mode=-1))
    assert "y must not be x" in err(good(y=0x1000))
    assert "B = 0" in err(good(B=0)) and "B = 65" in err(good(B=65))
    assert "ldx = 0" in err(good(ldx=0)) and "ldy = 16777217" in err(good(ldy=(1 << 24) + 1))
    for w in (0, 32, 96, 8192, 1000):
        assert f"window = {w} is not a power of two" in err(good(window=w))
    assert "tolerance = -1" in err(good(tolerance=-1)) and "tolerance = 65" in err(good(tolerance=65))
    assert "ldk = 0" in err(good(ldk=0))
    assert "row 1: in_start = -1" in err(good(in_start=i64(0, -1))) and "out_start = -5" in err(good(out_start=i64(-5, 0)))
    assert "row 0: total = -7" in err(good(total=i64(-7, -1)))
    assert "row 1: in_count = -1" in err(good(in_count=i32(5000, -1))) and "row 0: in_count = 5001" in err(good(in_count=i32(5001, 0)))
    assert "row 1: out_count = 6401" in err(good(out_count=i32(0, 6401))) and "row 0: out_count = -3" in err(good(out_count=i32(-3, 0)))
    assert "row 1: frames [5, 4) are not a range" in err(good(k1=i64(197, 4), k0=i64(0, 5)))                  # k1 < k0
    assert "row 0: frames [-1, 197)" in err(good(k0=i64(-1, 2)))
    assert "row 0: 257 frames exceed ldk" in err(good(k1=i64(257, 100)))
    assert "row 0: outputs [0, 6250) lie outside" in err(good(k1=i64(196, 100)))                              # beyond frame k1 - 1
    assert "row 1: outputs [0, 3000) lie outside" in err(good(out_start=i64(0, 0)))                           # before frame k0 - 1
    assert "row 1: DIA_TS_INTERP needs a total" in err(good(mode=hb.TS_INTERP))                               # an open total
    assert "row 0: out_total = 0" in err(good(mode=hb.TS_INTERP, total=i64(5000, 5000), out_total=i64(0, 6250)))
    assert "row 0: outputs [0, 6250) lie beyond out_total = 6249" in err(good(mode=hb.TS_INTERP, total=i64(5000, 5000), out_total=i64(6249, 6250)))
    return L


def test_abi_struct_and_validation(tmp_path):
    src = open(os.path.join(ROOT, "include", "dia_hip.h")).read()
    assert "int dia_timescale(const dia_timescale_args* a, void* stream);" in src
    assert "dia_timescale" in hb.EXPORTS and hb.ABI_VERSION == 8 and "#define DIA_ABI_VERSION 8" in src
    c = tmp_path / "s.c"
    c.write_text('#include <stdio.h>\n#include "dia_hip.h"\nint main(void){ printf("%zu %d %d %d %d %d %d %d\\n", sizeof(dia_timescale_args), '
                 'DIA_TS_INTERP, DIA_TS_WSOLA, DIA_TS_MAX_ROWS, DIA_TS_MAX_T, DIA_TS_MIN_WINDOW, DIA_TS_MAX_WINDOW, DIA_TS_OPEN); return 0; }\n')
    exe = tmp_path / "s"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(hb.TimescaleArgs), hb.TS_INTERP, hb.TS_WSOLA, S.MAX_ROWS, S.MAX_T, S.MIN_WINDOW, S.MAX_WINDOW, hb.TS_OPEN]
    assert refusals().dia_abi_version() == 8
