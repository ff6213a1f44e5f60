"""The native codec on the MI355X (csrc/codec.hip, dia_hip/codec.py, DESIGN.md "Codec") against tests/codec_ref.py, the plain-torch
restatement run on the CPU in float64.

Tolerance, everywhere: with e32 the largest absolute difference between the same restatement run in float32 on the CPU and the
float64 one on the same input, the device must be within 4 * e32 + 1e-6 of float64.  Every test prints e32 and the device's error
before it asserts."""
import os
import sys
import wave

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from codec_ref import RefCodec, random_codes, snake
from dia_hip import codec as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")


def within(name, dev, r64, r32):
    e32 = float(np.abs(np.asarray(r32, dtype=np.float64) - r64).max()) if r64.size else 0.0
    err = float(np.abs(np.asarray(dev, dtype=np.float64) - r64).max()) if r64.size else 0.0
    print(f"codec-accuracy {name}: e32 {e32:.3e} device {err:.3e} bound {4 * e32 + 1e-6:.3e}")
    assert np.all(np.isfinite(dev)) and err <= 4 * e32 + 1e-6, (name, err, e32)


def layer_ref(x, w, b, alpha, res, tanh, dtype, **conv):
    x, w, b = x.to(dtype), w.to(dtype), b.to(dtype)
    if alpha is not None:
        x = snake(x, alpha.to(dtype).reshape(1, -1, 1))
    y = (F.conv_transpose1d if "stride" in conv else F.conv1d)(x, w, b, **conv)
    if res is not None:
        y = y + res.to(dtype)
    return (torch.tanh(y) if tanh else y).numpy()


def dev_conv(x, w, b, alpha, res, tanh, lens=None, **kw):
    """x / res as CPU tensors -> the library's result as a numpy array"""
    stride = kw.get("stride", 0)
    wl = (K.convt_layout(w) if stride else K.conv_layout(w)).to(DEV)
    al = None if alpha is None else alpha.to(torch.float32).to(DEV)
    iv = None if alpha is None else K.snake_inverse(alpha).to(DEV)
    y = K.codec_conv(x.to(torch.float32).to(DEV).contiguous(), wl, b.to(torch.float32).to(DEV), c_out=w.shape[1] if stride else w.shape[0],
                     alpha=al, inv=iv, res=None if res is None else res.to(torch.float32).to(DEV).contiguous(), tanh=tanh,
                     lens=None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV), **kw)
    return y.cpu().numpy()


def make_layer(g, cin, cout, k, transposed=False):
    w = torch.randn(*((cin, cout, k) if transposed else (cout, cin, k)), generator=g, dtype=torch.float64)
    w = w / np.sqrt(cin * (2 if transposed else k))
    return w.float().double(), (0.1 * torch.randn(cout, generator=g)).double(), (0.5 + torch.rand(cin, generator=g)).float().double()


CHANNELS = [(12, 12), (24, 12), (20, 1), (96, 1), (80, 80)]     # the last: five input chunks, two blocks of output channels
TAPS = [(1, 1), (7, 1), (7, 3), (7, 9)]
FLAGS = [(False, False, False), (True, False, False), (False, True, False), (True, True, True)]


@pytest.mark.parametrize("k,d", TAPS)
@pytest.mark.parametrize("cin,cout", CHANNELS)
def test_conv_family(cin, cout, k, d):
    g = torch.Generator().manual_seed(cin * 100 + cout * 10 + k + d)
    w, b, alpha = make_layer(g, cin, cout, k)
    for T in (1, 5, 63, 64, 130):
        x = torch.randn(1, cin, T, generator=g).double()
        r = torch.randn(1, cout, T, generator=g).double()
        for use_snake, use_res, use_tanh in FLAGS:
            a_, r_ = (alpha if use_snake else None), (r if use_res else None)
            conv = dict(dilation=d, padding=(k // 2) * d)
            r64 = layer_ref(x, w, b, a_, r_, use_tanh, torch.float64, **conv)
            r32 = layer_ref(x, w, b, a_, r_, use_tanh, torch.float32, **conv)
            dev = dev_conv(x, w, b, a_, r_, use_tanh, k=k, dilation=d)
            within(f"conv {cin}->{cout} k{k} d{d} T{T} snake{int(use_snake)} res{int(use_res)} tanh{int(use_tanh)}", dev, r64, r32)


@pytest.mark.parametrize("k,d", [(1, 1), (7, 9)])
@pytest.mark.parametrize("cin,cout", [(24, 12), (96, 1)])
def test_conv_batch_rows_equal_solo_launches(cin, cout, k, d):
    g = torch.Generator().manual_seed(5)
    w, b, alpha = make_layer(g, cin, cout, k)
    lens = (130, 1, 64)
    x = torch.randn(3, cin, 130, generator=g)
    r = torch.randn(3, cout, 130, generator=g)
    for bi, n in enumerate(lens):                                # what lies behind a row's end must never be read
        x[bi, :, n:] = float("nan")
        r[bi, :, n:] = float("nan")
    both = dev_conv(x, w, b, alpha, r, False, lens=lens, k=k, dilation=d)
    for bi, n in enumerate(lens):
        solo = dev_conv(x[bi:bi + 1, :, :n], w, b, alpha, r[bi:bi + 1, :, :n], False, k=k, dilation=d)
        assert np.all(np.isfinite(solo)) and np.array_equal(both[bi, :, :n], solo[0]), (bi, n)
        assert not both[bi, :, n:].any()                         # and nothing is written there
    r64 = layer_ref(x[:1].double(), w, b, alpha, r[:1].double(), False, torch.float64, dilation=d, padding=(k // 2) * d)
    r32 = layer_ref(x[:1].double(), w, b, alpha, r[:1].double(), False, torch.float32, dilation=d, padding=(k // 2) * d)
    within(f"conv batch row 0 {cin}->{cout} k{k} d{d}", both[:1], r64, r32)


@pytest.mark.parametrize("s", [2, 4, 8])
@pytest.mark.parametrize("cin,cout", [(24, 12), (96, 48)])
def test_transposed_conv(cin, cout, s):
    g = torch.Generator().manual_seed(cin + s)
    w, b, alpha = make_layer(g, cin, cout, 2 * s, transposed=True)
    for T in (1, 2, 33, 129):                                    # 129: T + 1 input positions, two blocks
        x = torch.randn(1, cin, T, generator=g).double()
        for a_ in (None, alpha):
            conv = dict(stride=s, padding=-(-s // 2))
            r64 = layer_ref(x, w, b, a_, None, False, torch.float64, **conv)
            dev = dev_conv(x, w, b, a_, None, False, stride=s)
            assert dev.shape == r64.shape == (1, cout, T * s)
            within(f"convT {cin}->{cout} s{s} T{T} snake{int(a_ is not None)}", dev, r64, layer_ref(x, w, b, a_, None, False, torch.float32, **conv))
    lens = (33, 1, 20)
    x = torch.randn(3, cin, 33, generator=g)
    for bi, n in enumerate(lens):
        x[bi, :, n:] = float("nan")
    both = dev_conv(x, w, b, alpha, None, False, lens=lens, stride=s)
    for bi, n in enumerate(lens):
        solo = dev_conv(x[bi:bi + 1, :, :n], w, b, alpha, None, False, stride=s)
        assert np.all(np.isfinite(solo)) and np.array_equal(both[bi, :, :n * s], solo[0]) and not both[bi, :, n * s:].any(), (s, bi)


@pytest.mark.parametrize("latent", [64, 1024])
def test_embedding(latent):
    cfg = K.CodecConfig(latent_dim=latent, decoder_dim=192)
    sd = K.synthetic_state_dict(cfg, seed=11)
    tabs, bias = K.embed_tables(cfg, sd)
    r64m, r32m = RefCodec(cfg, sd, torch.float64), RefCodec(cfg, sd, torch.float32)
    for T in (1, 17):
        codes = random_codes(cfg, T, seed=T)
        assert codes.min() == 0 and codes.max() == 1023
        z = K.codec_embed(torch.from_numpy(codes[None].astype(np.int32)).to(DEV), tabs.to(DEV), bias.to(DEV)).cpu().numpy()
        c = torch.from_numpy(codes[None])
        within(f"embed latent{latent} T{T}", z, r64m.from_codes(c).numpy(), r32m.from_codes(c).numpy())
    # rows of their own length; an id outside the codebook is refused by decode() on the host and clamped by the kernel
    codes = random_codes(cfg, 17, seed=3, B=2).astype(np.int32)
    lens = torch.tensor([17, 5], dtype=torch.int32, device=DEV)
    z2 = K.codec_embed(torch.from_numpy(codes).to(DEV), tabs.to(DEV), bias.to(DEV), lens=lens).cpu().numpy()
    solo = K.codec_embed(torch.from_numpy(codes[1:, :, :5].copy()).to(DEV), tabs.to(DEV), bias.to(DEV)).cpu().numpy()
    assert np.array_equal(z2[1, :, :5], solo[0]) and not z2[1, :, 5:].any()


# ---------------------------------------------------------------------------------------------- the whole decoder
@pytest.fixture(scope="module")
def mini():
    cfg = K.mini_config()
    sd = K.synthetic_state_dict(cfg, seed=7)
    return cfg, sd, K.DeviceCodec((cfg, sd), DEV, window=64), RefCodec(cfg, sd, torch.float64), RefCodec(cfg, sd, torch.float32)


@pytest.fixture(scope="module")
def mini40(mini):
    cfg, _, _, r64, r32 = mini
    codes = random_codes(cfg, 40, seed=40)
    return codes, r64.decode(codes), r32.decode(codes)


@pytest.mark.parametrize("T", [1, 3])
def test_mini_decoder(mini, T):
    cfg, _, dev, r64, r32 = mini
    codes = random_codes(cfg, T, seed=T)
    y64 = r64.decode(codes)
    assert 0.05 <= float(np.sqrt((y64 ** 2).mean())) <= 0.9
    y = dev.decode(codes[None])
    assert y.dtype == np.float32 and y.shape == (T * 512,)
    within(f"mini decoder T{T}", y, y64, r32.decode(codes))


def test_mini_decoder_t40_whole_and_windowed(mini, mini40):
    cfg, _, dev, _, _ = mini
    codes, y64, y32 = mini40
    assert 0.05 <= float(np.sqrt((y64 ** 2).mean())) <= 0.9
    whole = dev.decode(codes)
    within("mini decoder T40 whole", whole, y64, y32)
    windowed = dev.decode(codes, window=8)
    within("mini decoder T40 window 8", windowed, y64, y32)
    print(f"codec-accuracy windowed vs whole: bitwise {np.array_equal(whole, windowed)}, max diff {np.abs(whole - windowed).max():.3e}")
    with pytest.raises(ValueError):
        dev.decode(codes, window=65)
    bad = codes.copy()
    bad[0, 0] = 1024
    with pytest.raises(ValueError, match="outside"):
        dev.decode(bad)


def test_full_size_decoder_touches_every_real_shape():
    cfg = K.CodecConfig()
    sd = K.synthetic_state_dict(cfg, seed=7)
    codes = random_codes(cfg, 3, seed=3)
    y64 = RefCodec(cfg, sd, torch.float64).decode(codes)
    assert 0.05 <= float(np.sqrt((y64 ** 2).mean())) <= 0.9
    dev = K.DeviceCodec(sd, DEV, window=8)                        # configuration from the shapes
    assert dev.cfg == cfg
    within("full decoder T3", dev.decode(codes), y64, RefCodec(cfg, sd, torch.float32).decode(codes))


def test_ragged_batch_equals_solo_decodes(mini, mini40):
    cfg, _, dev, _, _ = mini
    codes = mini40[0]
    rows = [codes, codes[:, :1], codes[:, 5:22], codes[:, :0]]
    got = dev.decode_batch(rows, window=8)
    for r, y in zip(rows, got):
        assert y.shape == (r.shape[1] * 512,) and np.array_equal(y, dev.decode(r, window=8))
    padded = np.zeros((3, 9, 40), dtype=np.int64)
    for i, r in enumerate(rows[:3]):
        padded[i, :, :r.shape[1]] = r
    for y, want in zip(dev.decode(padded, lengths=[40, 1, 17], window=8), got):
        assert np.array_equal(y, want)


def test_device_stream_state_equals_decode(mini, mini40):
    cfg, _, dev, _, _ = mini
    codes = mini40[0]
    st = dev.stream(window=8)
    out = [st.push(codes[:, a:b], final=b == 40 and a == 40) for a, b in ((0, 7), (7, 7), (7, 30), (30, 40), (40, 40))]
    assert np.array_equal(np.concatenate(out), dev.decode(codes, window=8))


# ---------------------------------------------------------------------------------------------- end to end
def test_dia_generates_streams_and_writes_audio(mini, tmp_path, monkeypatch):
    from dia_hip import config as C
    from dia_hip.model import Dia
    from dia_hip.weights import synthetic_state_dict
    ccfg, csd, _, _, _ = mini
    cfg = C.mid_config()
    sd = synthetic_state_dict(cfg, seed=1234, std=0.02)
    text = "[S1] Dia is an open weights text to dialogue model."
    dia = Dia.from_state_dict(cfg, sd, "float32", DEV)
    assert dia.generate(text, max_tokens=30, seed=3) is None      # without a codec: as before
    dia.load_codec(csd, window=16)
    assert dia.codec.cfg == ccfg
    codes = dia.generate_codes(text, max_tokens=30, seed=3)
    n = codes.shape[-1]
    assert n > 4
    want = dia.codec.decode(codes)
    audio = dia.generate(text, max_tokens=30, seed=3)
    assert audio.shape == (n * 512,) and np.array_equal(audio, want) and np.array_equal(dia.last_codes, codes)
    assert np.array_equal(dia.generate_audio_batch([text], max_tokens=30, seeds=[3])[0], want)
    chunks = list(dia.stream_audio([text], 1, max_tokens=30, seeds=[3], chunk=4))
    assert [c[3] for c in chunks] == [False] * (len(chunks) - 1) + [True] and len(chunks) >= 4
    assert [c[1] for c in chunks] == list(np.cumsum([0] + [c[2].shape[0] for c in chunks[:-1]]))
    assert np.array_equal(np.concatenate([c[2] for c in chunks]), want)
    # the CLI in this process; soundfile out of reach, so the file is the wave module's
    import cli
    monkeypatch.setitem(sys.modules, "soundfile", None)
    mdir = tmp_path / "model"
    mdir.mkdir()
    torch.save(sd, mdir / "pytorch_model.bin")
    cfg.save(mdir / "config.json")
    ck = tmp_path / "codec.pth"
    torch.save({"state_dict": csd, "metadata": {"kwargs": {"sample_rate": 44100}}}, ck)
    base = [text, "--model-path", str(mdir), "--compute-dtype", "float32", "--max-tokens", "30", "--seed", "3", "--codec-path", str(ck)]
    pcm = np.round(want.astype(np.float64).clip(-1, 1) * 32767.0).astype("<i2")
    for name, extra in (("plain.wav", []), ("streamed.wav", ["--stream-chunk", "4"])):
        out = tmp_path / name
        assert cli.main(base + ["--output", str(out)] + extra) == 0
        with wave.open(str(out), "rb") as f:
            assert (f.getnchannels(), f.getsampwidth(), f.getframerate(), f.getnframes()) == (1, 2, 44100, n * 512)
            assert np.array_equal(np.frombuffer(f.readframes(n * 512), dtype="<i2"), pcm), name
