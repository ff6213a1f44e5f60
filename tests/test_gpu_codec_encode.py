"""The codec's encode side on the MI355X (csrc/codec.hip: dia_codec_convs, dia_codec_quantize; dia_hip/codec.py: DeviceCodec.encode;
DESIGN.md "Codec: encode side") against tests/codec_enc_ref.py, the plain-torch restatement run on the CPU in float64.

Tolerance for activations, as on the decode side: with e32 the largest absolute difference between the same restatement run in
float32 on the CPU and the float64 one on the same input, the device must be within 4 * e32 + 1e-6 of float64.

Rule for codes: the device's codes must equal the float64 reference's, except at a (frame, stage) whose reference margin (second
smallest distance minus the smallest) is below tau = 4 * d32 + 1e-6, d32 being the largest |distance in float32 on the CPU -
distance in float64| of that case.  A frame is compared up to its first excused stage and dropped after it (a flip changes every
later residual); an unexcused mismatch fails; excused frames are capped at 2 % of a case's frames and at zero for T <= 17.  The
cases and seeds are codec_enc_ref.QUANT_CASES; tests/test_codec_encode_cpu.py holds the float32 restatement to the same rule on
them (0 excused frames in each).  Every test prints its figures before it asserts."""
import os
import sys
import wave

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from codec_enc_ref import QUANT_CASES, RefEncoder, compare_codes, distance_error, latent_landing_on, make_wave, quant_case, whole_state
from codec_ref import snake
from dia_hip import codec as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")


def within(name, dev, r64, r32):
    e32 = float(np.abs(np.asarray(r32, dtype=np.float64) - r64).max()) if r64.size else 0.0
    err = float(np.abs(np.asarray(dev, dtype=np.float64) - r64).max()) if r64.size else 0.0
    print(f"codec-encode-accuracy {name}: e32 {e32:.3e} device {err:.3e} bound {4 * e32 + 1e-6:.3e} ratio {err / (4 * e32 + 1e-6):.3f}")
    assert np.all(np.isfinite(dev)) and err <= 4 * e32 + 1e-6, (name, err, e32)


def cap_of(T):
    return 0 if T <= 17 else (2 * T) // 100


def layer_ref(x, w, b, alpha, dtype, s):
    x, w, b = x.to(dtype), w.to(dtype), b.to(dtype)
    if alpha is not None:
        x = snake(x, alpha.to(dtype).reshape(1, -1, 1))
    return (F.conv1d(x, w, b, stride=s, padding=s // 2) if s else F.conv1d(x, w, b, padding=1)).numpy()


def dev_convs(x, w, b, alpha, s, lens=None):
    wl = (K.convs_layout(w) if s else K.conv_layout(w)).to(DEV)
    al = None if alpha is None else alpha.to(torch.float32).to(DEV)
    iv = None if alpha is None else K.snake_inverse(alpha).to(DEV)
    y = K.codec_convs(x.to(torch.float32).to(DEV).contiguous(), wl, b.to(torch.float32).to(DEV), c_out=w.shape[0], stride=s, alpha=al, inv=iv,
                      lens=None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV))
    return y.cpu().numpy()


def make_layer(g, cin, cout, k):
    w = torch.randn(cout, cin, k, generator=g, dtype=torch.float64) / np.sqrt(cin * k)
    return w.float().double(), (0.1 * torch.randn(cout, generator=g)).double(), (0.5 + torch.rand(cin, generator=g)).float().double()


CHANNELS = [(12, 24), (20, 40), (80, 96), (1, 8)]               # 80 -> 96: several input chunks at every stride, two blocks of output channels
OUT_LENS = [1, 2, 31, 32, 33, 127, 128, 129, 130]


@pytest.mark.parametrize("s", [2, 4, 8, 0])                      # 0: the k-3 form
@pytest.mark.parametrize("cin,cout", CHANNELS)
def test_strided_and_k3_family(cin, cout, s):
    g = torch.Generator().manual_seed(cin * 100 + cout * 10 + s)
    w, b, alpha = make_layer(g, cin, cout, 2 * s if s else 3)
    for To in OUT_LENS:
        x = torch.randn(1, cin, To * (s or 1), generator=g).double()
        for a_ in (None, alpha):
            r64 = layer_ref(x, w, b, a_, torch.float64, s)
            dev = dev_convs(x, w, b, a_, s)
            assert dev.shape == r64.shape == (1, cout, To)
            within(f"{'strided s' + str(s) if s else 'k3'} {cin}->{cout} To{To} snake{int(a_ is not None)}", dev, r64, layer_ref(x, w, b, a_, torch.float32, s))


@pytest.mark.parametrize("s", [2, 8, 0])
@pytest.mark.parametrize("cin,cout", [(12, 24), (80, 96)])
def test_batch_rows_equal_solo_launches(cin, cout, s):
    g = torch.Generator().manual_seed(7 + s)
    w, b, alpha = make_layer(g, cin, cout, 2 * s if s else 3)
    m = s or 1
    outs = (130, 1, 64)                                          # 130: two tiles of 128 outputs
    x = torch.randn(3, cin, 130 * m, generator=g)
    for bi, n in enumerate(outs):                                # what lies behind a row's end must never be read
        x[bi, :, n * m:] = float("nan")
    both = dev_convs(x, w, b, alpha, s, lens=[n * m for n in outs])
    for bi, n in enumerate(outs):
        solo = dev_convs(x[bi:bi + 1, :, :n * m], w, b, alpha, s)
        assert np.all(np.isfinite(solo)) and np.array_equal(both[bi, :, :n], solo[0]), (bi, n)
        assert not both[bi, :, n:].any()                         # and nothing is written there
    r64 = layer_ref(x[:1].double(), w, b, alpha, torch.float64, s)
    within(f"batch row 0 {cin}->{cout} s{s}", both[:1], r64, layer_ref(x[:1].double(), w, b, alpha, torch.float32, s))


# ---------------------------------------------------------------------------------------------- the quantiser alone
def dev_quantize(cfg, sd, z, lens=None):
    q = {k: v.to(DEV) for k, v in K.quantizer_tables(cfg, sd, K.check_codec_encoder_state(cfg, sd)).items()}
    tabs = K.embed_tables(cfg, sd)[0].to(DEV)
    return K.codec_quantize(z.to(torch.float32).to(DEV).contiguous(), q, tabs,
                            lens=None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)).cpu().numpy()


@pytest.mark.parametrize("latent,T,seed", QUANT_CASES)
def test_quantiser_alone(latent, T, seed):
    cfg, sd, z, (c64, m64, d64), (c32, _, d32) = quant_case(latent, T, seed)
    rms = float(z.double().pow(2).mean().sqrt())
    d = distance_error(d32, c32, d64, c64)
    print(f"codec-encode quantiser latent{latent} T{T}: latent rms {rms:.3f} d32 {d:.3e} smallest margin {m64.min():.3e}")
    assert 0.05 <= rms <= 5.0
    if T == 130:
        distinct = [len(np.unique(c64[i])) for i in range(cfg.n_codebooks)]
        print(f"codec-encode quantiser latent{latent} T{T}: distinct ids per codebook {distinct}")
        assert min(distinct) >= 32
    got = dev_quantize(cfg, sd, z)
    assert got.shape == (1, 9, T) and got.dtype == np.int32 and got.min() >= 0 and got.max() < cfg.codebook_size
    compare_codes(f"quantiser latent{latent} T{T}", got[0], c64, m64, 4 * d + 1e-6, cap_of(T))


def test_quantiser_rows_equal_solo_launches():
    cfg, sd, z, _, _ = quant_case(64, 17, 12)
    lens = (17, 1, 9)
    zb = z.repeat(3, 1, 1).clone()
    zb[1] = zb[1].flip(-1)
    for bi, n in enumerate(lens):
        zb[bi, :, n:] = float("nan")
    both = dev_quantize(cfg, sd, zb, lens=lens)
    for bi, n in enumerate(lens):
        solo = dev_quantize(cfg, sd, zb[bi:bi + 1, :, :n])
        assert np.array_equal(both[bi, :, :n], solo[0]) and not both[bi, :, n:].any(), bi


def test_lowest_index_wins_an_exact_tie():
    cfg = K.mini_config()
    sd = whole_state(cfg, 1)
    sd["quantizer.quantizers.0.codebook.weight"][700] = sd["quantizer.quantizers.0.codebook.weight"][5]
    ref = RefEncoder(cfg, sd)
    z = latent_landing_on(ref, 5)
    c, m, _ = ref.quantize(z)
    assert int(c[0, 0, 0]) == 5 and float(m[0, 0, 0]) == 0.0     # rows 5 and 700 are the two nearest, at the same distance
    got = dev_quantize(cfg, sd, z)
    assert got[0, 0, 0] == 5


# ---------------------------------------------------------------------------------------------- the whole encoder
@pytest.fixture(scope="module")
def mini():
    cfg = K.mini_config()
    sd = whole_state(cfg, 7)
    return cfg, sd, K.DeviceCodec((cfg, sd), DEV, window=64), RefEncoder(cfg, sd, torch.float64), RefEncoder(cfg, sd, torch.float32)


def whole_encode_check(name, dev, r64, r32, wave_):
    c64, z64, m64, d64 = r64.encode(wave_)
    c32, z32, _, d32 = r32.encode(wave_)
    T = -(-wave_.shape[0] // 512)
    rms = float(np.sqrt((z64 ** 2).mean()))
    print(f"codec-encode {name}: latent rms {rms:.3f}")
    assert 0.05 <= rms <= 5.0
    (codes,), (lat,) = dev.encode_batch([wave_], return_latents=True)
    assert codes.dtype == np.int64 and codes.shape == (9, T) and lat.shape == z64.shape
    within(f"{name} latent", lat, z64, z32)
    compare_codes(name, codes, c64, m64, 4 * distance_error(d32, c32, d64, c64) + 1e-6, cap_of(T))
    assert np.array_equal(dev.encode(wave_), codes[None])


@pytest.mark.parametrize("L", [512, 700, 3 * 512, 40 * 512])      # 700 pads to two frames
def test_mini_encoder(mini, L):
    _, _, dev, r64, r32 = mini
    whole_encode_check(f"mini encoder L{L}", dev, r64, r32, make_wave(L, seed=L))


def test_full_size_encoder_touches_every_real_shape():
    cfg = K.CodecConfig()
    sd = whole_state(cfg, 7)
    dev = K.DeviceCodec(sd, DEV, window=8)                        # configuration from the shapes
    assert dev.cfg == cfg and dev.cfg.encoder_dim == 64 and dev.cfg.encoder_rates == (2, 4, 8, 8) and dev.has_encoder
    whole_encode_check("full encoder L1536", dev, RefEncoder(cfg, sd, torch.float64), RefEncoder(cfg, sd, torch.float32), make_wave(3 * 512, seed=3))


def test_windows_equal_the_whole_encode_bitwise(mini):
    _, _, dev, _, _ = mini
    wave_ = make_wave(40 * 512, seed=40)
    (cw,), (zw,) = dev.encode_batch([wave_], return_latents=True)
    (c8,), (z8,) = dev.encode_batch([wave_], window=8, return_latents=True)
    print(f"codec-encode windows: latent max diff {np.abs(zw - z8).max():.3e}, codes differing {int((cw != c8).sum())}")
    assert zw.shape == (64, 40) and np.array_equal(zw, z8) and np.array_equal(cw, c8)
    with pytest.raises(ValueError):
        dev.encode(wave_, window=65)
    # ragged rows in one pass, each as when encoded alone; an empty row has no frame
    rows = [wave_, wave_[:700], wave_[5000:9000], wave_[:0]]
    got = dev.encode_batch(rows, window=8)
    for r, c in zip(rows, got):
        assert c.shape == (9, -(-r.shape[0] // 512)) and np.array_equal(c, dev.encode_batch([r], window=8)[0])
    padded = np.zeros((3, 40 * 512), dtype=np.float32)
    for i, r in enumerate(rows[:3]):
        padded[i, :r.shape[0]] = r
    out = dev.encode(padded, lengths=[40 * 512, 700, 4000], window=8)
    assert out.shape == (3, 9, 40) and all(np.array_equal(out[i, :, :c.shape[1]], c) and not out[i, :, c.shape[1]:].any() for i, c in enumerate(got[:3]))


def test_decoder_only_and_malformed_checkpoints_still_decode(mini):
    cfg, sd, dev, _, _ = mini
    dec_only = K.synthetic_state_dict(cfg, seed=7)
    codes = dev.encode(make_wave(3 * 512, seed=3))
    want = dev.decode(codes)
    a = K.DeviceCodec((cfg, dec_only), DEV, window=64)
    assert not a.has_encoder and np.array_equal(a.decode(codes), want)
    with pytest.raises(KeyError, match=r"encoder\.block\.0\.weight_g"):
        a.encode(np.zeros(512, dtype=np.float32))
    bad = {**sd, "encoder.block.2.block.4.weight_v": torch.zeros(32, 16, 9)}
    b = K.DeviceCodec((cfg, bad), DEV, window=64)
    assert not b.has_encoder and np.array_equal(b.decode(codes), want)
    with pytest.raises(ValueError, match=r"encoder\.block\.2\.block\.4\.weight_v has shape \(32, 16, 9\)"):
        b.encode(np.zeros(512, dtype=np.float32))
    missing = {k: v for k, v in sd.items() if k != "quantizer.quantizers.6.in_proj.weight_g"}
    with pytest.raises(KeyError, match=r"quantizer\.quantizers\.6\.in_proj\.weight_g"):
        K.DeviceCodec((cfg, missing), DEV, window=64).encode(np.zeros(512, dtype=np.float32))
    with pytest.raises(ValueError, match="mono float"):
        dev.encode_batch([np.zeros((2, 512), dtype=np.float32)])


# ---------------------------------------------------------------------------------------------- end to end
def test_file_prompt_round_trip_through_the_model(mini, tmp_path, monkeypatch):
    from dia_hip import config as C
    from dia_hip.model import Dia
    from dia_hip.weights import synthetic_state_dict
    ccfg, csd, _, _, _ = mini
    monkeypatch.setitem(sys.modules, "torchaudio", None)          # the wave module reads the file
    cfg = C.mid_config()
    sd = synthetic_state_dict(cfg, seed=1234, std=0.02)
    dia = Dia.from_state_dict(cfg, sd, "float32", DEV)
    with pytest.raises(RuntimeError, match="DAC model not loaded"):
        dia.load_audio(str(tmp_path / "voice.wav"))               # without a codec: as before
    dia.load_codec(csd, window=16)
    assert dia.codec.has_encoder
    pcm = np.round(make_wave(6 * 512 + 200, seed=5).astype(np.float64).clip(-1, 1) * 32767.0).astype("<i2")
    path = tmp_path / "voice.wav"
    with wave.open(str(path), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(44100)
        f.writeframes(pcm.tobytes())
    samples = (pcm.astype(np.float64) / 32768.0).astype(np.float32)
    codes = dia.codec.encode(samples)                             # [1, 9, 7]
    assert codes.shape == (1, 9, 7)
    frames = dia.load_audio(str(path))
    assert tuple(frames.shape) == (7, 9) and np.array_equal(frames.numpy(), codes[0].T)
    assert np.array_equal(dia.encode_audio(samples).numpy(), codes[0].T)
    text, ptext = "[S2] You get full control.", "[S1] Dia is an open weights model."
    kw = dict(max_tokens=30, seed=3, audio_prompt_text=ptext)
    a_file = dia.generate(text, audio_prompt=str(path), **kw)
    codes_file = dia.last_codes.copy()
    a_codes = dia.generate(text, audio_prompt=torch.from_numpy(codes[0].T.copy()), **kw)
    assert a_file is not None and codes_file.shape[-1] > 2
    assert np.array_equal(codes_file, dia.last_codes) and np.array_equal(a_file, a_codes)     # the token buffers are identical
    # the CLI writes the same codes, with no model
    import cli
    ck = tmp_path / "codec.pth"
    torch.save({"state_dict": csd, "metadata": {"kwargs": {"sample_rate": 44100, "encoder_dim": 8}}}, ck)
    out = tmp_path / "codes.npy"
    assert cli.main(["-", "--encode-audio", str(path), "--codes-output", str(out), "--codec-path", str(ck)]) == 0
    assert np.array_equal(np.load(out), codes[0].T)
