"""Host side of the resampler (dia_hip/resample.py, DESIGN.md "Resampler"), no GPU: the compact filter bank against the full
K-tap restatement of tests/resample_ref.py, the filter's own properties in float64 (they guard the restatement: torchaudio is not
there to compare with), the stream planner on integers, the refusals, the wiring into Dia, and the C ABI's validation."""
import ctypes
import os
import subprocess
import sys
import wave

import numpy as np
import pytest

import resample_ref as R
from dia_hip import binding as hb
from dia_hip import resample as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def scattered(plan, K):
    """the compact plan back in the full layout [n][K], and the mask of the taps it keeps (|t| < 6)"""
    cols = (plan.first.astype(np.int64) + plan.width)[:, None] + np.arange(plan.nt, dtype=np.int64)[None, :]
    out = np.zeros((plan.n, K), dtype=np.float64)
    inside = (cols >= 0) & (cols < K)
    assert np.all(plan.bank[~inside] == 0.0)
    r = np.broadcast_to(np.arange(plan.n)[:, None], cols.shape)
    out[r[inside], cols[inside]] = plan.bank[inside]
    return out, out != 0.0


@pytest.mark.parametrize("rate_in,rate_out", R.PAIRS)
def test_compact_form_equals_the_full_bank(rate_in, rate_out):
    plan = S.resample_plan(rate_in, rate_out)
    o, n, width, f = R.full_bank(rate_in, rate_out)
    assert (plan.o, plan.n, plan.width, plan.K) == (o, n, width, f.shape[1])
    assert plan.first.dtype == np.int32 and plan.first.shape == (n,) and plan.bank.shape == plan.bank32.shape == (n, plan.nt)
    assert plan.bank.dtype == np.float64 and plan.bank32.dtype == np.float32 and np.array_equal(plan.bank32, plan.bank.astype(np.float32))
    sc, kept = scattered(plan, f.shape[1])
    dropped = float(np.abs(f[~kept]).max())
    runs = kept.sum(axis=1)
    print(f"resample-plan {rate_in}->{rate_out}: o {o} n {n} K {f.shape[1]} nt {plan.nt} runs {runs.min()}..{runs.max()} largest dropped tap {dropped:.2e}")
    assert np.array_equal(sc[kept], f[kept])                                   # every kept tap, exactly
    assert dropped < 1e-30
    assert runs.max() == plan.nt and runs.min() >= plan.nt - 1                 # nt is the longest run, nothing longer is stored
    # the kept run of a phase is contiguous: first[p] is its first tap
    for p in (0, n // 2, n - 1):
        at = np.flatnonzero(kept[p])
        assert at[0] == plan.first[p] + width and np.array_equal(at, np.arange(at[0], at[0] + at.shape[0]))
    x = np.random.default_rng(11).uniform(-1.0, 1.0, size=1300)
    d = R.full_minus_compact(x, rate_in, rate_out, plan.nt, plan.first, plan.bank)
    y_full = R.resample_full(x, rate_in, rate_out)
    y_comp, _ = R.resample_compact(x, plan.o, plan.n, plan.nt, plan.first, plan.bank)
    print(f"resample-plan {rate_in}->{rate_out}: full - compact, exact: {np.abs(d).max():.2e}; as two float64 sums: {np.abs(y_full - y_comp).max():.2e}")
    assert np.abs(d).max() <= 1e-25
    assert np.abs(y_full - y_comp).max() <= 1e-13                              # two summation orders in float64, outputs below 2
    assert S.resample_plan(rate_in, rate_out) is plan                          # cached per pair


@pytest.mark.parametrize("rate_in,rate_out", R.PAIRS)
def test_output_lengths(rate_in, rate_out):
    plan = S.resample_plan(rate_in, rate_out)
    for L in R.lengths_of(plan.o):
        want = -(-plan.n * L // plan.o)
        assert plan.out_len(L) == want == R.out_len(rate_in, rate_out, L)
        x = R.noise(L, seed=L)
        assert R.resample_full(x, rate_in, rate_out).shape == (want,)
        assert R.resample_compact(x, plan.o, plan.n, plan.nt, plan.first, plan.bank)[0].shape == (want,)
        # every output's taps are inside what the stream planner calls known once the signal is complete
        if want:
            assert plan.pos(want - 1) < L and plan.pos(0) <= 0


@pytest.mark.parametrize("rate_in,rate_out", R.PAIRS)
def test_filter_properties_in_float64(rate_in, rate_out):
    """a constant stays 1 and a 1 kHz sine stays that sine within 2e-3 away from the ends (2 % of a second on either side): the
    filter's pass-band ripple, not arithmetic (measured on the full formula: <= 8.8e-4 and <= 6.9e-4 over the nine pairs)"""
    plan = S.resample_plan(rate_in, rate_out)
    L = rate_in // 2
    m = np.arange(plan.out_len(L))
    mid = slice(rate_out // 50, m.shape[0] - rate_out // 50)
    sine = np.sin(2 * np.pi * 1000.0 * np.arange(L) / rate_in)
    for name, fn in (("full", lambda x: R.resample_full(x, rate_in, rate_out)),
                     ("compact", lambda x: R.resample_compact(x, plan.o, plan.n, plan.nt, plan.first, plan.bank)[0])):
        dc = float(np.abs(fn(np.ones(L)) - 1.0)[mid].max())
        se = float(np.abs(fn(sine) - np.sin(2 * np.pi * 1000.0 * m / rate_out))[mid].max())
        print(f"resample-filter {rate_in}->{rate_out} {name}: constant {dc:.2e} sine {se:.2e}")
        assert dc <= 2e-3 and se <= 2e-3


class Recorder:
    """stands where the device launch would: checks coverage as the wrapper does and returns the float64 compact result of the
    window it is given, so the join can be compared with the whole-signal result"""

    def __init__(self, plan):
        self.plan, self.calls = plan, []

    def __call__(self, window, in_start, out_start, out_count, total):
        S.check_coverage(self.plan, in_start, window.shape[0], out_start, out_count, total)
        self.calls.append((in_start, window.shape[0], out_start, out_count, total))
        p = self.plan
        m = np.arange(out_start, out_start + out_count, dtype=np.int64)
        at = ((m // p.n) * p.o + p.first[m % p.n].astype(np.int64))[:, None] + np.arange(p.nt)[None, :] - in_start
        ok = (at >= 0) & (at < window.shape[0])
        # an index outside the window must be outside the signal: check_coverage said so; read it as zero
        return (p.bank[m % p.n] * np.where(ok, window.astype(np.float64)[np.clip(at, 0, max(window.shape[0] - 1, 0))] if window.shape[0] else 0.0, 0.0)).sum(axis=1)


@pytest.mark.parametrize("chunks", sorted(R.CHUNKS))
@pytest.mark.parametrize("rate_in,rate_out", [(48000, 44100), (44100, 16000), (22050, 44100), (16000, 44100)])
def test_stream_planner_on_integers(rate_in, rate_out, chunks):
    plan = S.resample_plan(rate_in, rate_out)
    L = 1300 if chunks != "1" else 700
    x = R.noise(L, seed=3)
    rec = Recorder(plan)
    st = S.ResampleStream(plan, rec)
    size, at, i, parts, held = R.CHUNKS[chunks], 0, 0, [], 0
    while True:
        c = min(size(i), L - at)
        final = at + c >= L
        before = st.emitted
        y = st.push(x[at:at + c], final)
        assert st.emitted - before == y.shape[0]
        if not final:                                                          # exactly the outputs whose taps are all known
            assert st.emitted == S.ready_outputs(plan, at + c)
            assert plan.pos(st.emitted - 1) + plan.nt <= at + c if st.emitted else True
            assert plan.pos(st.emitted) + plan.nt > at + c
        held = max(held, st.buf.shape[0])
        parts.append(y)
        at, i = at + c, i + 1
        if final:
            break
    # the launches' output ranges: disjoint, contiguous, and their union is [0, ceil(n L / o))
    nxt = 0
    for in_start, in_count, out_start, out_count, total in rec.calls:
        assert out_start == nxt and out_count > 0
        nxt += out_count
    assert nxt == st.emitted == plan.out_len(L)
    assert all(c[4] is None for c in rec.calls[:-1]) and rec.calls[-1][4] == L
    whole, _ = R.resample_compact(x, plan.o, plan.n, plan.nt, plan.first, plan.bank)
    assert np.array_equal(np.concatenate(parts), whole)                        # same taps, same order: the same float64 sums
    assert held <= max(size(j) for j in range(7)) + plan.nt + plan.o + 1       # only the tail later outputs need is kept
    with pytest.raises(RuntimeError, match="after the final chunk"):
        st.push(x[:1])


def test_coverage_check_refuses_a_missing_sample():
    plan = S.resample_plan(48000, 44100)
    S.check_coverage(plan, 0, 1300, 0, plan.out_len(1300), 1300)
    with pytest.raises(ValueError, match="read input samples"):
        S.check_coverage(plan, 0, 1299, 0, plan.out_len(1300), 1300)           # the last sample of the signal is not there
    with pytest.raises(ValueError, match="read input samples"):
        S.check_coverage(plan, 1, 1299, 0, 10, None)                           # nor the first
    with pytest.raises(ValueError, match="lie beyond"):
        S.check_coverage(plan, 0, 1300, 0, plan.out_len(1300) + 1, 1300)
    m = S.ready_outputs(plan, 600)
    S.check_coverage(plan, 0, 600, 0, m, None)
    with pytest.raises(ValueError, match="read input samples"):
        S.check_coverage(plan, 0, 600, 0, m + 1, None)                         # an open signal: sample 600 is not known yet


def test_refusals_and_equal_rates():
    with pytest.raises(ValueError, match=r"2000003 Hz -> 2000005 Hz.*64 MiB"):
        S.resample_plan(2000003, 2000005)                                      # coprime: 2000005 phases x 13 taps
    assert 2000005 * 12 * 4 > S.MAX_BANK_BYTES == 64 << 20
    with pytest.raises(ValueError, match=r"192000 Hz -> 8000 Hz.*LDS"):
        S.resample_plan(192000, 8000)                                          # 24 inputs per output: the tile of 1024 outputs
    assert S.MAX_TILE_FLOATS * 4 <= 64 * 1024
    with pytest.raises(ValueError, match="positive"):
        S.resample_plan(0, 44100)
    dev = object.__new__(S.DeviceResampler)                                    # no device: equal rates never reach one
    x = np.zeros(5, dtype=np.float32)
    rows = [x, x[:2]]
    assert dev.resample(x, 44100, 44100) is x and dev.resample(rows, 16000, 16000) is rows
    st = dev.stream(8000, 8000)
    assert st.push(x) is not None and np.array_equal(st.push(x[:2], final=True), x[:2]) and st.emitted == 7


# ---------------------------------------------------------------------------------------------- wiring
def _write_wav16(path, x, rate, channels):
    raw = np.round(np.asarray(x) * 32768.0).clip(-32768, 32767).astype("<i2").tobytes()
    with wave.open(str(path), "wb") as f:
        f.setnchannels(channels)
        f.setsampwidth(2)
        f.setframerate(rate)
        f.writeframes(raw)


class _FakeCodec:
    """a codec object that DOES offer resample: records what it is handed"""
    has_encoder = True

    def __init__(self):
        from dia_hip import codec as K
        self.cfg = K.mini_config()
        self.calls = []

    def resample(self, waves, rate_in, rate_out):
        self.calls.append((waves, rate_in, rate_out))
        one = lambda w: np.full(-(-np.asarray(w).shape[0] * rate_out // rate_in), 0.25, dtype=np.float32)
        return [one(w) for w in waves] if isinstance(waves, list) else one(waves)

    def encode(self, w):
        self.seen = np.asarray(w)
        T = -(-self.seen.shape[0] // 512)
        return np.arange(9 * T, dtype=np.int64).reshape(1, 9, T)

    def decode(self, codes):
        return np.full(np.asarray(codes).shape[-1] * 512, 0.5, dtype=np.float32)

    def decode_batch(self, rows):
        return [self.decode(r) for r in rows]


def test_load_audio_resamples_through_the_codec(tmp_path, monkeypatch):
    from dia_hip import model as M
    monkeypatch.setitem(sys.modules, "torchaudio", None)                       # and with it importable the path is the same one
    dia = object.__new__(M.Dia)
    dia.codec, dia.dac_model = _FakeCodec(), None
    g = np.random.default_rng(2)
    st = g.uniform(-0.9, 0.9, size=(700, 2))
    _write_wav16(tmp_path / "half.wav", st, 22050, 2)
    frames = dia.load_audio(str(tmp_path / "half.wav"))
    (given, rate_in, rate_out), = dia.codec.calls
    assert (rate_in, rate_out) == (22050, 44100)
    want = (np.round(st * 32768.0) / 32768.0).mean(axis=1)
    assert given.dtype == np.float32 and given.shape == (700,) and np.abs(given - want).max() <= 2.0 ** -24    # the channel mean
    assert dia.codec.seen.shape == (1400,) and np.all(dia.codec.seen == 0.25)  # what resample returned is what is encoded
    assert tuple(frames.shape) == (3, 9)
    dia.encode_audio(st[:, 0].astype(np.float32), sample_rate=16000)
    assert dia.codec.calls[-1][1:] == (16000, 44100) and dia.codec.seen.shape == (-(-700 * 44100 // 16000),)
    n = len(dia.codec.calls)
    dia.encode_audio(st[:, 0].astype(np.float32), sample_rate=44100)           # the codec's rate: not called
    assert len(dia.codec.calls) == n and dia.codec.seen.shape == (700,)


def test_output_sample_rate_goes_through_the_codec():
    from dia_hip import model as M
    assert M.Dia.output_sample_rate is None
    dia = object.__new__(M.Dia)
    dia.codec, dia.dac_model = _FakeCodec(), None
    codes = np.zeros((1, 9, 4), dtype=np.int64)
    assert dia._generate_output(codes).shape == (2048,) and dia.codec.calls == []          # default: as it comes
    dia.output_sample_rate = 44100
    assert dia._generate_output(codes).shape == (2048,) and dia.codec.calls == []          # the codec's own rate: nothing to do
    dia.output_sample_rate = 16000
    y = dia._generate_output(codes)
    (given, rate_in, rate_out), = dia.codec.calls
    assert (rate_in, rate_out) == (44100, 16000) and given.shape == (2048,) and np.all(given == 0.5)
    assert y.shape == (-(-2048 * 16000 // 44100),) and np.all(y == 0.25)
    dia.generate_batch = lambda texts, *a, **k: [codes, codes[:, :, :2]]
    out = dia.generate_audio_batch(["a", "b"])
    assert [w.shape[0] for w in dia.codec.calls[-1][0]] == [2048, 1024] and dia.codec.calls[-1][1:] == (44100, 16000)
    assert [w.shape[0] for w in out] == [-(-2048 * 16000 // 44100), -(-1024 * 16000 // 44100)]
    # a codec object without a resampler cannot serve the request: said, not ignored
    dia.codec = type("NoResampler", (), {"cfg": dia.codec.cfg, "decode": lambda self, c: np.zeros(4, dtype=np.float32)})()
    with pytest.raises(RuntimeError, match="16000 Hz needs the native codec's resampler"):
        dia._generate_output(codes)


def test_cli_output_rate_rules():
    import cli
    p = cli.build_parser()
    assert p.parse_args(["x", "--output", "a.wav"]).output_rate is None
    assert p.parse_args(["x", "--output", "a.wav", "--output-rate", "16000"]).output_rate == 16000
    for argv in (["x", "--output", "a.wav", "--output-rate", "16000"],                     # no --codec-path
                 ["x", "--codes-output", "a.npy", "--output-rate", "16000", "--codec-path", __file__],
                 ["x", "--output", "a.wav", "--output-rate", "0", "--codec-path", __file__]):
        with pytest.raises(SystemExit):
            cli.main(argv)


# ---------------------------------------------------------------------------------------------- the C ABI
def test_abi_symbol_struct_and_validation(tmp_path):
    src = open(os.path.join(ROOT, "include", "dia_hip.h")).read()
    assert "int dia_resample(const dia_resample_args* a, void* stream);" in src
    assert "dia_resample" in hb.EXPORTS and hb.ABI_VERSION == 8 and "#define DIA_ABI_VERSION 8" in src
    c = tmp_path / "s.c"
    c.write_text('#include <stdio.h>\n#include "dia_hip.h"\nint main(void){ printf("%zu %d %d %d %d %d\\n", sizeof(dia_resample_args), '
                 'DIA_RESAMPLE_MAX_ROWS, DIA_RESAMPLE_MAX_T, DIA_RESAMPLE_TILE, DIA_RESAMPLE_MAX_TILE_FLOATS, DIA_RESAMPLE_OPEN); return 0; }\n')
    exe = tmp_path / "s"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(hb.ResampleArgs), S.MAX_ROWS, S.MAX_T, S.TILE_OUTPUTS, S.MAX_TILE_FLOATS, hb.RESAMPLE_OPEN]
    L = hb.lib()
    assert L.dia_abi_version() == 8
    fn = L.dia_resample

    def err(a):
        assert fn(ctypes.byref(a), None) == -1                                 # DIA_E_ARG, before any launch
        return L.dia_last_error().decode()

    assert fn(None, None) == -1 and "null argument" in L.dia_last_error().decode()
    assert "null pointer" in err(hb.ResampleArgs())                            # the zeroed struct
    i64, i32 = (ctypes.c_int64 * 2), (ctypes.c_int32 * 2)

    def good(**kw):
        f = dict(x=0x1000, y=0x2000, bank=0x3000, first=0x4000, B=2, ldx=64, ldy=64, o=160, n=147, nt=14,
                 in_start=i64(0, 0), out_start=i64(0, 0), total=i64(64, -1), in_count=i32(64, 64), out_count=i32(58, 40))
        f.update(kw)
        return hb.ResampleArgs(**f)

    assert "host arrays" in err(good(total=None))
    assert "y must not be x" in err(good(y=0x1000))
    assert "B = 0" in err(good(B=0)) and "B = 65" in err(good(B=65))
    assert "n = 0" in err(good(n=0)) and "o = -1" in err(good(o=-1))
    assert "nt = 0" in err(good(nt=0)) and "nt = 5000" in err(good(nt=5000))
    assert "ldx = 0" in err(good(ldx=0)) and "ldy = 16777217" in err(good(ldy=(1 << 24) + 1))
    assert "input tile" in err(good(o=24, n=1, nt=293))
    assert "row 1: in_count = -1" in err(good(in_count=i32(64, -1))) and "row 0: in_count = 65" in err(good(in_count=i32(65, 0)))
    assert "row 1: out_count = 65" in err(good(out_count=i32(0, 65))) and "row 0: out_count = -3" in err(good(out_count=i32(-3, 0)))
    assert "is negative" in err(good(in_start=i64(-1, 0))) and "is negative" in err(good(out_start=i64(0, -5)))
    assert "neither a length" in err(good(total=i64(64, -2)))
    assert "too far" in err(good(in_start=i64(0, 1 << 40)))
    assert fn(ctypes.byref(good(out_count=i32(0, 0))), None) == 0              # nothing asked for: no launch, no device needed
