"""The audio distance on the MI355X (csrc/spectral.hip: dia_spectral; dia_hip/spectral.py: DeviceSpectral; DESIGN.md "Audio
distance") against the float64 restatement of tests/spectral_ref.py.

Bound of a magnitude, derived and not measured: each component of X[f][k] is an fp32 dot product of W terms whose coefficients were
rounded once, so it lies within (W + 1) u sum_n |x_n| |w_n| of the float64 value to first order (u = 2^-24; |cos|, |sin| <= 1), the
two components together move |X| by at most sqrt(2) times that, and the square root and the squares add less than 2 u |X| <=
2 u sum_n |x_n| |w_n|: |mag_dev - mag_ref| <= (W + 3) u sqrt(2) sum_n |x_n| |w_n|, plus 1e-30 for sums that are exactly zero.  A mel row
is bounded by the same figure carried through sum_k fb[m][k].  The log term has no useful bound near eps: the distances are
measured against float64 with the float32 CPU path (torch.stft in float32, the same filterbank and terms) as the yardstick, and the
device may err at most 4 times as far.  Everything else is bitwise.  Every test prints its figures before it asserts.

Measured on an MI355X: largest err / bound of the magnitudes 0.019 / 0.0003 / below 0.00005 at W = 32 / 512 / 2048, of the mel rows
0.027 / 0.0029 / 0.0012.  Distances, device error / float32-CPU error: 0.01 to 1.31 over the twelve (pair, length, metric) cases
(DESIGN.md "Audio distance" has the table)."""
import json
import math
import os
import sys
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import spectral_ref as R
from dia_hip import spectral as S

DEV = torch.device("cuda:0")
RATE = 44100
U = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    return S.DeviceSpectral(DEV)


def edge_lengths(W):
    H = W // 4
    return [1, H - 1, H, W // 2, W + 1, 3 * W + 7]


def mag_bound(x, W):
    """[F][1]: the per-bin bound of every frame"""
    return ((W + 3) * U * math.sqrt(2.0) * R.mag_scale(x, W) + 1e-30)[:, None]


@pytest.fixture(scope="module")
def edge_rows():
    """the ragged rows of tests 1 and 2 and their float64 magnitudes, computed once"""
    out = {}
    for W in (32, 512, 2048):
        rows = [R.noise(L, seed=W + L) for L in edge_lengths(W)]
        out[W] = (rows, [R.stft_mag(x, W) for x in rows])
    return out


@pytest.mark.parametrize("W", (32, 512, 2048))
def test_magnitudes_against_float64(dev, edge_rows, W):
    rows, refs = edge_rows[W]
    batch = dev.stft_mag(rows, W)
    worst = 0.0
    for x, ref, got in zip(rows, refs, batch):
        L = x.shape[0]
        assert got.dtype == np.float32 and got.shape == ref.shape == (1 + L // (W // 4), W // 2 + 1)
        solo = dev.stft_mag(x, W)
        assert np.array_equal(solo, got)                                       # batch 1 holds the same bits
        bound = mag_bound(x, W)
        err = np.abs(got.astype(np.float64) - ref)
        ratio = float((err / bound).max())
        edge = float((err[:, [0, W // 2]] / bound).max())                      # k = 0 and the tail bin k = W / 2
        worst = max(worst, ratio)
        print(f"spectral-mag W {W} L {L}: {ref.shape[0]} frames, max err {err.max():.3e}, largest err / bound {ratio:.4f}, at k = 0 and W/2 {edge:.4f}")
        assert np.all(np.isfinite(got)) and np.all(err <= bound), (L, ratio)
        assert np.all(err[:, 0] <= bound[:, 0]) and np.all(err[:, W // 2] <= bound[:, 0])
    print(f"spectral-mag W {W}: largest err / bound over the lengths {worst:.4f}")


@pytest.mark.parametrize("W,n_mels", [(32, 5), (512, 80), (2048, 320)])
def test_mel_rows_against_float64(dev, edge_rows, W, n_mels):
    rows, refs = edge_rows[W]
    fb = R.filterbank(W, RATE, n_mels)
    batch = dev.mel(rows, W, n_mels, RATE)
    worst = 0.0
    for x, mag, got in zip(rows, refs, batch):
        ref = mag @ fb.T
        assert got.dtype == np.float32 and got.shape == ref.shape == (mag.shape[0], n_mels)
        assert np.array_equal(dev.mel(x, W, n_mels, RATE), got)
        bound = mag_bound(x, W) * fb.sum(axis=1)[None, :] + 1e-30              # the per-bin bound through sum_k fb[m][k]
        err = np.abs(got.astype(np.float64) - ref)
        ratio = float((err / bound).max())
        worst = max(worst, ratio)
        print(f"spectral-mel W {W} n_mels {n_mels} L {x.shape[0]}: max err {err.max():.3e}, largest err / bound {ratio:.4f}")
        assert np.all(np.isfinite(got)) and np.all(err <= bound), (x.shape[0], ratio)
        lm = dev.logmel(x, W, n_mels, RATE)
        assert lm.shape == got.shape and np.array_equal(lm, np.log10(np.maximum(got, np.float32(R.EPS))))
    print(f"spectral-mel W {W} n_mels {n_mels}: largest err / bound over the lengths {worst:.4f}")


# ---------------------------------------------------------------------------------------------- distances
def pairs(L):
    n = np.arange(L)
    x = R.noise(L, seed=L)
    sine = np.sin(2.0 * np.pi * 1000.0 * n / RATE).astype(np.float32)
    sig = (0.5 * R.noise(L, seed=L + 1) + 0.4 * np.sin(2.0 * np.pi * 440.0 * n / RATE)).astype(np.float32)
    late = np.concatenate([np.zeros(3, dtype=np.float32), sig[:-3]])
    return {"noise+1e-3": (x, (x + np.float32(1e-3) * R.noise(L, seed=L + 2)).astype(np.float32)),
            "half sine": (sine, (np.float32(0.5) * sine).astype(np.float32)),
            "delay 3": (sig, late)}


def spectrum32(x, W, n_mels):
    """the float32 CPU path: torch.stft in float32, then the filterbank rounded to float32"""
    t = torch.stft(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)), n_fft=W, hop_length=W // 4, win_length=W,
                   window=torch.hann_window(W, periodic=True, dtype=torch.float32), center=True, pad_mode="constant", return_complex=True).abs().T
    if n_mels:
        t = t @ torch.from_numpy(R.filterbank(W, RATE, n_mels).astype(np.float32)).T
    return t


def metric32(a, b, spec):
    total = 0.0
    for i, W in enumerate(spec["windows"]):
        nm = spec["n_mels"][i] if "n_mels" in spec else 0
        Sa, Sb = spectrum32(a, W, nm), spectrum32(b, W, nm)
        eps = torch.tensor(R.EPS, dtype=torch.float32)
        mag = (Sa - Sb).abs().mean()
        log = (torch.log10(torch.maximum(Sa, eps) ** spec["power"]) - torch.log10(torch.maximum(Sb, eps) ** spec["power"])).abs().mean()
        assert mag.dtype == log.dtype == torch.float32
        total += spec["mag_weight"] * float(mag) + spec["log_weight"] * float(log)
    return total / len(spec["windows"])


@pytest.fixture(scope="module")
def distance_refs():
    """float64 and float32-CPU values of both metrics on every pair, computed once"""
    out = {}
    for L in (4096, 10007):
        for name, (a, b) in pairs(L).items():
            out[(L, name)] = {m: (R.metric(a, b, RATE, spec)[0], metric32(a, b, spec)) for m, spec in (("stft", R.STFT), ("mel", R.MEL))}
    return out


@pytest.mark.parametrize("L", (4096, 10007))
def test_distances_against_float64_with_the_float32_cpu_path_as_yardstick(dev, distance_refs, L):
    ps = pairs(L)
    got = dev.distance([p[0] for p in ps.values()], [p[1] for p in ps.values()], RATE)
    fails = []
    for (name, (a, b)), res in zip(ps.items(), got):
        for m in ("stft", "mel"):
            ref, cpu32 = distance_refs[(L, name)][m]
            e_dev, e_cpu = abs(res[m] - ref), abs(cpu32 - ref)
            print(f"spectral-distance L {L} {name} {m}: float64 {ref:.9g}, device {res[m]:.9g} (err {e_dev:.3e}), float32 CPU {cpu32:.9g} (err {e_cpu:.3e}), "
                  f"ratio {e_dev / e_cpu if e_cpu else float('inf'):.3f}")
            assert math.isfinite(res[m]) and res[m] > 0.0
            if not e_dev <= 4.0 * e_cpu:
                fails.append((name, m, e_dev, e_cpu))
        assert set(res["per_resolution"]["stft"]) == set(R.STFT["windows"]) and set(res["per_resolution"]["mel"]) == set(R.MEL["windows"])
    assert not fails, fails


@pytest.mark.parametrize("L", (4096, 10007))
def test_half_amplitude_sine_gives_twice_log10_two(dev, L):
    a, b = pairs(L)["half sine"]
    want = 2.0 * math.log10(2.0)
    for W in R.STFT["windows"]:
        Sa, Sb = dev.stft_mag([a, b], W)
        live = (Sa > R.EPS) & (Sb > R.EPS)
        d = np.abs(np.log10(Sa[live].astype(np.float64) ** 2) - np.log10(Sb[live].astype(np.float64) ** 2))
        print(f"spectral-half-sine L {L} W {W}: {int(live.sum())} of {live.size} bins above eps, largest |dlog - 2 log10 2| {np.abs(d - want).max():.3e}")
        assert live.sum() >= 100 * Sa.shape[0] and np.abs(d - want).max() <= 1e-5
    # and the kernel's own log term, on a pair that lies above eps everywhere: noise, where every bin is far above it
    x = R.noise(L, seed=5)
    res = dev.distance(x, (np.float32(0.5) * x).astype(np.float32), RATE, metrics=("stft",))
    for W, t in res["per_resolution"]["stft"].items():
        print(f"spectral-half-noise L {L} W {W}: log term {t['log']:.9f}")
        assert abs(t["log"] - want) <= 1e-5


# ---------------------------------------------------------------------------------------------- bit for bit
def test_a_row_has_the_same_bits_alone_and_anywhere_in_a_ragged_batch(dev):
    a, b = R.noise(10007, 1), R.noise(10007, 2)
    others = [(R.noise(L, seed=50 + L), R.noise(L, seed=60 + L)) for L in (1, 700, 4096, 12000)]
    solo = dev.distance(a, b, RATE)
    assert solo["stft"] > 0.0 and solo["mel"] > 0.0
    for at in (0, 3):
        rows = others[:at] + [(a, b)] + others[at:]
        got = dev.distance([r[0] for r in rows], [r[1] for r in rows], RATE)
        assert len(got) == 5 and got[at] == solo, at                          # every term of every resolution, exactly
        for W, nm in ((2048, 0), (512, 0), (32, 5), (2048, 320)):
            one = dev.mel(a, W, nm, RATE) if nm else dev.stft_mag(a, W)
            many = dev.mel([r[0] for r in rows], W, nm, RATE) if nm else dev.stft_mag([r[0] for r in rows], W)
            assert np.array_equal(many[at], one), (at, W, nm)
    same = dev.distance(a, a.copy(), RATE)
    assert same["stft"] == 0.0 and same["mel"] == 0.0
    assert all(t["mag"] == 0.0 and t["log"] == 0.0 for m in same["per_resolution"].values() for t in m.values())
    assert dev.distance(b, a, RATE) == solo                                   # symmetric, exactly
    with pytest.raises(ValueError, match="samples against"):
        dev.distance(a, b[:-1], RATE)
    cut = dev.distance(a, b[:-7], RATE, trim=True)
    assert cut == dev.distance(a[:-7], b[:-7], RATE)


def test_more_pairs_than_one_launch_holds(dev):
    rows = [R.noise(300 + 17 * i, seed=i) for i in range(S.MAX_ROWS + 2)]
    other = [R.noise(r.shape[0], seed=1000 + i) for i, r in enumerate(rows)]
    got = dev.distance(rows, other, RATE, metrics=("stft",), stft=dict(windows=(128,)))
    assert len(got) == S.MAX_ROWS + 2
    for i in (0, S.MAX_ROWS - 1, S.MAX_ROWS, S.MAX_ROWS + 1):
        assert got[i] == dev.distance(rows[i], other[i], RATE, metrics=("stft",), stft=dict(windows=(128,)))


# ---------------------------------------------------------------------------------------------- end to end
def write_wav16(path, samples):
    pcm = np.round(np.asarray(samples, dtype=np.float64).clip(-1, 1) * 32767.0).astype("<i2")
    with wave.open(str(path), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(RATE)
        f.writeframes(pcm.tobytes())
    return (pcm.astype(np.float64) / 32768.0).astype(np.float32)


def last_json(text):
    return json.loads([ln for ln in text.splitlines() if ln.startswith("{")][-1])


def test_end_to_end_on_the_synthetic_codec(tmp_path, capsys, monkeypatch):
    from codec_enc_ref import make_wave, whole_state
    from codec_ref import random_codes
    from dia_hip import codec as K
    from dia_hip import config as C
    from dia_hip.model import Dia
    from dia_hip.weights import synthetic_state_dict
    import cli
    monkeypatch.setitem(sys.modules, "torchaudio", None)                       # the wave module reads the files
    ccfg = K.mini_config()
    csd = whole_state(ccfg, 7)
    codes = random_codes(ccfg, 24, seed=24)
    waves = {m: K.DeviceCodec((ccfg, csd), DEV, window=64, precision=m).decode(codes) for m in ("fp32", "bf16x2", "bf16")}
    cfg = C.mid_config()
    dia = Dia.from_state_dict(cfg, synthetic_state_dict(cfg, seed=1234, std=0.02), "float32", DEV)
    assert dia.codec is None                                                   # no codec: the distance needs only the device
    rough = dia.audio_distance(waves["fp32"], waves["bf16"])
    fine = dia.audio_distance(waves["fp32"], waves["bf16x2"])
    same = dia.audio_distance(waves["fp32"], waves["fp32"].copy())
    for m in ("stft", "mel"):
        print(f"spectral-codec {m}: fp32 vs bf16 {rough[m]:.6e}, fp32 vs bf16x2 {fine[m]:.6e}")
        assert rough[m] > fine[m] > 0.0 and same[m] == 0.0
    with pytest.raises(RuntimeError, match="no native codec"):
        dia.codec_roundtrip_distance(waves["fp32"])
    dia.load_codec(csd)
    assert dia.codec.has_encoder
    samples = write_wav16(tmp_path / "in.wav", make_wave(6 * 512 + 200, seed=5))
    other = write_wav16(tmp_path / "other.wav", 0.9 * make_wave(6 * 512 + 100, seed=5))
    trip = dia.codec_roundtrip_distance(samples)
    print(f"spectral-codec round trip: stft {trip['stft']:.6e}, mel {trip['mel']:.6e}")
    assert all(math.isfinite(trip[m]) and trip[m] > 0.0 for m in ("stft", "mel"))
    assert trip == dia.codec.audio_distance(samples, dia.codec.decode(dia.codec.encode(samples))[:samples.shape[0]])
    # the command line prints the same numbers
    capsys.readouterr()
    assert cli.main(["--compare-audio", str(tmp_path / "in.wav"), str(tmp_path / "other.wav")]) == 0
    got = last_json(capsys.readouterr().out)
    want = dia.audio_distance(samples, other, trim=True)
    assert got["stft"] == want["stft"] and got["mel"] == want["mel"] and got["sample_rate"] == RATE and got["samples"] == 6 * 512 + 100
    assert got["per_resolution"]["mel"]["2048"] == want["per_resolution"]["mel"][2048]
    ck = tmp_path / "codec.pth"
    torch.save({"state_dict": csd, "metadata": {"kwargs": {"sample_rate": RATE, "encoder_dim": 8}}}, ck)
    assert cli.main(["--codec-roundtrip", str(tmp_path / "in.wav"), "--codec-path", str(ck)]) == 0
    got = last_json(capsys.readouterr().out)
    assert got["stft"] == trip["stft"] and got["mel"] == trip["mel"] and got["codec_precision"] == "fp32"
    assert cli.main(["--codec-roundtrip", str(tmp_path / "in.wav"), "--codec-path", str(ck), "--codec-precision", "bf16"]) == 0
    lossy = last_json(capsys.readouterr().out)
    assert lossy["codec_precision"] == "bf16" and lossy["stft"] != trip["stft"] and lossy["stft"] > 0.0
