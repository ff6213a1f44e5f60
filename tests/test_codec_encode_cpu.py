"""The codec's encode side without a GPU (dia_hip/codec.py, DESIGN.md "Codec: encode side"): encoder_plan and its keys, the
encode-side loader beside the unchanged decode-side one, the strided-convolution layout, encode_context_frames and the windowing it
feeds, the file reading of Dia.load_audio, the CLI's --encode-audio rules and every DIA_E_ARG path of dia_codec_convs /
dia_codec_quantize (none of which launches).

The reference is tests/codec_enc_ref.py: a plain-torch restatement in float64 on the CPU."""
import ctypes
import hashlib
import os
import sys
import wave

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from codec_enc_ref import QUANT_CASES, RefEncoder, compare_codes, distance_error, latent_landing_on, make_wave, quant_case, whole_state
from dia_hip import binding as hb
from dia_hip import codec as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


@pytest.fixture(scope="module")
def mini():
    cfg = K.mini_config()
    sd = whole_state(cfg, 7)
    return cfg, sd, RefEncoder(cfg, sd, torch.float64)


def test_encoder_plan_and_keys():
    full, mini_ = K.CodecConfig(), K.mini_config()
    assert (full.encoder_dim, full.encoder_rates, mini_.encoder_dim, mini_.encoder_rates) == (64, (2, 4, 8, 8), 8, (2, 4, 8, 8))
    assert K.CodecConfig(latent_dim=64, decoder_dim=192) == mini_          # the encode-side fields take no part in equality
    for cfg in (full, mini_):
        d = cfg.encoder_dim
        plan = K.encoder_plan(cfg)
        assert len(plan) == 1 + 4 * 7 + 1
        assert plan[0] == dict(kind="conv", key="encoder.block.0", snake=None, cin=1, cout=d, k=7, d=1)
        assert [L["s"] for L in plan if L["kind"] == "convs"] == [2, 4, 8, 8]
        assert [(L["cin"], L["cout"]) for L in plan if L["kind"] == "convs"] == [(d, 2 * d), (2 * d, 4 * d), (4 * d, 8 * d), (8 * d, 16 * d)]
        assert [L["key"] for L in plan if L["kind"] == "convs"] == [f"encoder.block.{b}.block.4" for b in (1, 2, 3, 4)]
        assert [L["snake"] for L in plan if L["kind"] == "convs"] == [f"encoder.block.{b}.block.3" for b in (1, 2, 3, 4)]
        unit = [L for L in plan if L["key"].startswith("encoder.block.2.block.1.")]
        assert [(L["key"], L["snake"], L["k"], L["d"], bool(L.get("res"))) for L in unit] == [
            ("encoder.block.2.block.1.block.1", "encoder.block.2.block.1.block.0", 7, 3, False),
            ("encoder.block.2.block.1.block.3", "encoder.block.2.block.1.block.2", 1, 1, True)]
        assert plan[-1] == dict(kind="conv3", key="encoder.block.6", snake="encoder.block.5", cin=16 * d, cout=cfg.latent_dim, k=3, d=1)
        keys = K.expected_encoder_keys(cfg)
        assert keys["encoder.block.0.weight_v"] == (d, 1, 7) and keys["encoder.block.0.weight_g"] == (d, 1, 1)
        assert keys["encoder.block.4.block.4.weight_v"] == (16 * d, 8 * d, 16) and keys["encoder.block.1.block.4.weight_v"] == (2 * d, d, 4)
        assert keys["encoder.block.3.block.3.alpha"] == (1, 4 * d, 1) and keys["encoder.block.5.alpha"] == (1, 16 * d, 1)
        assert keys["encoder.block.6.weight_v"] == (cfg.latent_dim, 16 * d, 3) and keys["encoder.block.6.bias"] == (cfg.latent_dim,)
        for i in (0, 8):
            q = f"quantizer.quantizers.{i}.in_proj"
            assert (keys[f"{q}.weight_g"], keys[f"{q}.weight_v"], keys[f"{q}.bias"]) == ((8, 1, 1), (8, cfg.latent_dim, 1), (8,))
        assert len(keys) == 3 + 4 * (3 * 8 + 1 + 3) + 1 + 3 + 9 * 3
        assert not set(keys) & set(K.expected_keys(cfg))
        assert set(K.synthetic_encoder_state(cfg, 0)) == set(keys)


def _digest(sd):
    m = hashlib.sha256()
    for k in sorted(sd):
        m.update(k.encode())
        m.update(str(tuple(sd[k].shape)).encode())
        m.update(sd[k].contiguous().numpy().tobytes())
    return m.hexdigest()


def test_synthetic_state_dict_is_unchanged():
    # digests of synthetic_state_dict's tensors computed on the commit before the encode side existed
    assert _digest(K.synthetic_state_dict(K.mini_config(), 7)) == "3ed69885a30577ee9447bb626159ef49743565b20490c60dfaa5e9bb87043ec0"
    assert _digest(K.synthetic_state_dict(K.CodecConfig(), 0)) == "a5ea67c60034db6fa230530e32b5277d68781ff9f90c06b47863980d9c4108e9"
    a, b = K.synthetic_encoder_state(K.mini_config(), 7), K.synthetic_encoder_state(K.mini_config(), 7)
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert not torch.equal(a["encoder.block.0.weight_v"], K.synthetic_encoder_state(K.mini_config(), 8)["encoder.block.0.weight_v"])


def test_encode_side_loader(mini):
    cfg, sd, _ = mini
    dec_only = K.synthetic_state_dict(cfg, seed=7)
    # a decoder-only checkpoint: the decode side loads as ever, the encode side is refused by name
    got_cfg, got = K.load_codec_state(dict(dec_only))
    assert got_cfg == cfg and set(got) == set(dec_only)
    with pytest.raises(KeyError, match=r"encoder\.block\.0\.weight_g"):
        K.check_codec_encoder_state(cfg, dec_only)
    # the whole checkpoint: both sides, each with its own keys
    got_cfg, got = K.load_codec_state({"state_dict": dict(sd), "metadata": {"kwargs": {"encoder_dim": 8, "encoder_rates": [2, 4, 8, 8]}}})
    assert got_cfg == cfg and set(got) == set(dec_only)
    enc = K.check_codec_encoder_state(cfg, sd)
    assert set(enc) == set(K.expected_encoder_keys(cfg)) == set(sd) - set(dec_only)
    assert K.infer_encoder_config(K.CodecConfig(latent_dim=64, decoder_dim=192), sd).encoder_dim == 8
    assert K.infer_encoder_config(K.CodecConfig(latent_dim=64, decoder_dim=192), sd, {"encoder_dim": 16}).encoder_dim == 16
    assert K.infer_encoder_config(cfg, {**sd, "encoder.block.1.block.4.weight_v": torch.zeros(16, 8, 8)}).encoder_rates == (4, 4, 8, 8)
    key = "encoder.block.3.block.4.weight_v"
    with pytest.raises(ValueError, match=key.replace(".", r"\.") + r" has shape \(64, 32, 8\)"):
        K.check_codec_encoder_state(cfg, {**sd, key: torch.zeros(64, 32, 8)})
    with pytest.raises(ValueError, match=r"quantizer\.quantizers\.3\.in_proj\.weight_v"):
        K.check_codec_encoder_state(cfg, {**sd, "quantizer.quantizers.3.in_proj.weight_v": torch.zeros(8, 32, 1)})
    with pytest.raises(KeyError, match=r"missing.*encoder\.block\.5\.alpha"):
        K.check_codec_encoder_state(cfg, {k: v for k, v in sd.items() if k != "encoder.block.5.alpha"})
    with pytest.raises(KeyError, match=r"missing.*quantizer\.quantizers\.8\.in_proj\.bias"):
        K.check_codec_encoder_state(cfg, {k: v for k, v in sd.items() if k != "quantizer.quantizers.8.in_proj.bias"})
    with pytest.raises(KeyError, match=r"unexpected.*encoder\.block\.7\.weight_g"):
        K.check_codec_encoder_state(cfg, {**sd, "encoder.block.7.weight_g": torch.zeros(1)})
    # the decode side still ignores whatever the encode side holds
    assert set(K.check_codec_state(cfg, {**sd, "encoder.block.0.weight_v": torch.zeros(2, 2, 2)})) == set(dec_only)


def test_strided_layout_and_folding_against_float64():
    g = torch.Generator().manual_seed(3)
    for s in (2, 4, 8):
        v = torch.randn(24, 12, 2 * s, generator=g)
        gain = torch.rand(24, 1, 1, generator=g) + 0.5
        w = K.fold_weight_norm(gain, v)
        assert w.dtype == torch.float64
        assert torch.allclose(w.reshape(24, -1).norm(dim=1), gain.reshape(-1).double(), rtol=0, atol=1e-12)
        lay = K.convs_layout(w)
        assert tuple(lay.shape) == (2, 12 * s, 32) and lay.dtype == torch.float32 and float(lay[:, :, 24:].abs().max()) == 0.0
        assert lay[1, 5 * s + 1, 7] == w[7, 5, 1 + s].float() and lay[0, 11 * s + s - 1, 23] == w[23, 11, s - 1].float()
        # the kernel's sum, spelt out: y[o] = sum_{t, ci, r} lay[t][ci s + r][co] x[ci][(o + t) s + r - s / 2], zero outside the row
        L = 5 * s
        x = torch.randn(1, 12, L, generator=g, dtype=torch.float64)
        xp = F.pad(x, (s // 2, 2 * s))
        y = torch.zeros(24, L // s, dtype=torch.float64)
        for o in range(L // s):
            for t in range(2):
                seg = xp[0, :, (o + t) * s:(o + t) * s + s]                     # [ci][r] = x[ci][(o + t) s + r - s / 2]
                y[:, o] += lay[t, :, :24].double().T @ seg.reshape(-1)
        ref = F.conv1d(x, w.float().double(), None, stride=s, padding=s // 2)[0]
        assert ref.shape == y.shape and torch.allclose(y, ref, rtol=0, atol=1e-12), s


def test_quantizer_tables_are_the_search_operands(mini):
    cfg, sd, ref = mini
    q = K.quantizer_tables(cfg, sd, K.check_codec_encoder_state(cfg, sd))
    assert tuple(q["in_w"].shape) == (9, 8, 64) and tuple(q["in_b"].shape) == (9, 8) and tuple(q["cb"].shape) == (9, 1024, 8)
    assert tuple(q["cb2"].shape) == (9, 1024) and tuple(q["bias"].shape) == (9, 64)
    assert torch.allclose(q["in_w"][4].double(), ref.w("quantizer.quantizers.4.in_proj")[:, :, 0], rtol=0, atol=1e-7)
    assert torch.allclose(q["cb"][2].double(), F.normalize(sd["quantizer.quantizers.2.codebook.weight"].double()), rtol=0, atol=1e-7)
    assert torch.allclose(q["cb2"], torch.ones(9, 1024), rtol=0, atol=1e-6)
    assert torch.equal(q["bias"][8], sd["quantizer.quantizers.8.out_proj.bias"])


def test_encode_context_frames_is_exact_and_tight(mini):
    cfg, _, ref = mini
    ctx = K.encode_context_frames(cfg)
    assert ctx == K.encode_context_frames(K.CodecConfig()) == 8               # widths do not enter; DESIGN.md derives the 8
    T = 37                                                                     # no multiple of 3 or 16
    wave_ = make_wave(T * 512 - 100, seed=37)                                  # the last frame is padded by preprocess
    padded = K.preprocess(wave_, cfg.hop)
    assert padded.shape == (T * 512,) and not padded[-100:].any() and np.array_equal(padded[:-100], wave_)
    whole = ref.latents(wave_)
    assert whole.shape == (64, T) and 0.05 <= float(np.sqrt((whole ** 2).mean())) <= 5.0
    for window in (1, 3, 16):
        assert np.array_equal(K.encode_windowed(ref.latents, padded, window, ctx, cfg.hop), whole), window
        short = K.encode_windowed(ref.latents, padded, window, ctx - 1, cfg.hop)
        assert short.shape == whole.shape and not np.array_equal(short, whole), window


def test_reference_search_lowest_index_margin_and_seeds():
    """the float32 restatement under the acceptance rule of tests/test_gpu_codec_encode.py, on that file's cases
    (codec_enc_ref.QUANT_CASES): excused frames must stay within the caps 0 (T <= 17) and 2 % (T = 130)"""
    for latent, T, seed in QUANT_CASES:
        cfg, sd, z32, (c64, m64, d64), (c32, _, d32) = quant_case(latent, T, seed)
        tau = 4 * distance_error(d32, c32, d64, c64) + 1e-6
        compare_codes(f"float32 CPU latent{latent} T{T} seed{seed}", c32, c64, m64, tau, 0 if T <= 17 else (2 * T) // 100)
        assert (m64 >= 0).all() and c64.min() >= 0 and c64.max() < 1024
        if T == 130:
            distinct = [len(np.unique(c64[i])) for i in range(9)]
            print("distinct ids per codebook", distinct)
            assert min(distinct) >= 32
    # lowest index: two identical rows
    cfg = K.mini_config()
    sd = whole_state(cfg, 1)
    sd["quantizer.quantizers.0.codebook.weight"][700] = sd["quantizer.quantizers.0.codebook.weight"][5]
    ref = RefEncoder(cfg, sd)
    z = latent_landing_on(ref, 5)
    c, m, _ = ref.quantize(z)
    assert int(c[0, 0, 0]) == 5 and float(m[0, 0, 0]) == 0.0


# ---------------------------------------------------------------------------------------------- files
def _write_wav(path, samples, rate, width, channels=1):
    """samples float [n] or [n, channels] in [-1, 1) -> PCM of `width` bytes"""
    x = np.asarray(samples, dtype=np.float64).reshape(-1, channels)
    if width == 1:
        raw = (np.round(x * 128.0) + 128).clip(0, 255).astype(np.uint8).tobytes()
    elif width == 3:
        v = np.round(x * 8388608.0).clip(-8388608, 8388607).astype(np.int32).reshape(-1)
        raw = np.stack([v & 0xFF, (v >> 8) & 0xFF, (v >> 16) & 0xFF], axis=1).astype(np.uint8).tobytes()
    else:
        full = float(1 << (8 * width - 1))
        raw = np.round(x * full).clip(-full, full - 1).astype({2: "<i2", 4: "<i4"}[width]).tobytes()
    with wave.open(str(path), "wb") as f:
        f.setnchannels(channels)
        f.setsampwidth(width)
        f.setframerate(rate)
        f.writeframes(raw)


class _FakeCodec:
    """stands where DeviceCodec would: records the samples it is given"""
    has_encoder = True
    cfg = K.mini_config()

    def encode(self, w):
        self.seen = np.asarray(w)
        T = -(-self.seen.shape[0] // 512)
        return np.arange(9 * T, dtype=np.int64).reshape(1, 9, T)


def test_load_audio_reads_wav_files_without_torchaudio(tmp_path, monkeypatch):
    from dia_hip import model as M
    monkeypatch.setitem(sys.modules, "torchaudio", None)                       # import torchaudio -> ImportError
    dia = object.__new__(M.Dia)
    dia.codec, dia.dac_model = _FakeCodec(), None
    x = make_wave(1300, seed=1).astype(np.float64).clip(-0.99, 0.99)
    # 16-bit mono
    _write_wav(tmp_path / "m16.wav", x, 44100, 2)
    frames = dia.load_audio(str(tmp_path / "m16.wav"))
    assert isinstance(frames, torch.Tensor) and frames.dtype == torch.int64 and tuple(frames.shape) == (3, 9)
    assert np.array_equal(frames.numpy(), np.arange(27).reshape(9, 3).T)
    assert dia.codec.seen.dtype == np.float32 and dia.codec.seen.shape == (1300,)
    assert np.array_equal(dia.codec.seen, (np.round(x * 32768.0) / 32768.0).astype(np.float32))
    # 24-bit stereo: the channels are averaged
    st = np.stack([x, -0.5 * x[::-1]], axis=1)
    _write_wav(tmp_path / "s24.wav", st, 44100, 3, channels=2)
    dia.load_audio(str(tmp_path / "s24.wav"))
    want = (np.round(st * 8388608.0) / 8388608.0).mean(axis=1)
    assert dia.codec.seen.shape == (1300,) and np.abs(dia.codec.seen - want).max() <= 2.0 ** -24
    # 8-bit unsigned and 32-bit
    _write_wav(tmp_path / "u8.wav", x, 44100, 1)
    assert np.abs(M.read_audio_mono(str(tmp_path / "u8.wav"))[0] - x).max() <= 1.0 / 128.0
    _write_wav(tmp_path / "i32.wav", x, 44100, 4)
    mono, rate = M.read_audio_mono(str(tmp_path / "i32.wav"))
    assert rate == 44100 and np.abs(mono - x).max() <= 2.0 ** -23
    # another rate: refused with the rate in the message; no resampler of our own
    _write_wav(tmp_path / "half.wav", x, 22050, 2)
    with pytest.raises(RuntimeError, match="22050 Hz"):
        dia.load_audio(str(tmp_path / "half.wav"))
    with pytest.raises(RuntimeError, match="16000 Hz"):
        dia.encode_audio(x, sample_rate=16000)
    with pytest.raises(FileNotFoundError):
        dia.load_audio(str(tmp_path / "none.wav"))
    with pytest.raises(RuntimeError, match=r"only \.wav"):
        dia.load_audio(__file__)
    # no encode side: today's branch and its error
    dia.codec = None
    with pytest.raises(RuntimeError, match="DAC model not loaded"):
        dia.load_audio(str(tmp_path / "m16.wav"))
    dia.codec = type("DecodeOnly", (), {"has_encoder": False})()
    with pytest.raises(RuntimeError, match="DAC model not loaded"):
        dia.load_audio(str(tmp_path / "m16.wav"))


def test_cli_encode_audio_rules(tmp_path):
    import cli
    p = cli.build_parser()
    a = p.parse_args(["x", "--encode-audio", "in.wav", "--codes-output", "o.npy", "--codec-path", "c.pth"])
    assert a.encode_audio == "in.wav"
    ck = tmp_path / "c.pth"
    torch.save(K.synthetic_state_dict(K.mini_config(), 7), ck)

    def refused(argv):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        return e.value.code == 2

    assert refused(["x", "--encode-audio", "in.wav", "--codes-output", "o.npy"])                               # no codec
    assert refused(["x", "--encode-audio", "in.wav", "--codes-output", "o.npy", "--codec-path", str(tmp_path / "none.pth")])
    assert refused(["x", "--encode-audio", "in.wav", "--codec-path", str(ck)])                                 # nowhere to write
    assert refused(["x", "--encode-audio", "in.wav", "--codes-output", "o.npy", "--codec-path", str(ck), "--output", "o.wav"])
    assert refused(["x", "--encode-audio", "in.wav", "--codes-output", "o.npy", "--codec-path", str(ck), "--slots", "2"])
    assert refused(["x", "--encode-audio", "in.wav", "--codes-output", "o.npy", "--codec-path", str(ck), "--audio-prompt", "p.npy",
                    "--audio-prompt-text", "t"])


# ---------------------------------------------------------------------------------------------- DIA_E_ARG, no launch
def _conv_args(**over):
    buf = ctypes.create_string_buffer(64)
    base = ctypes.addressof(buf) // 16 * 16 + 16
    a = K.CodecConvArgs(x=base, w=base + 16, bias=base, y=base + 4, B=1, T=8, C_in=4, C_out=4, ldx=8, ldy=8, k=3, dilation=1)
    a._keep = buf
    for k, v in over.items():
        setattr(a, k, v)
    return a


def _refused(fn, a, word):
    rc = fn(ctypes.byref(a), None) if a is not None else fn(None, None)
    msg = hb.lib().dia_last_error().decode()
    return rc == -1 and word in msg and msg.startswith(fn.__name__)


def test_encode_entries_argument_validation_without_gpu():
    L = K._fns()
    convs, quant = L.dia_codec_convs, L.dia_codec_quantize
    assert "dia_codec_convs" in hb.EXPORTS and "dia_codec_quantize" in hb.EXPORTS
    assert _refused(convs, None, "null") and _refused(quant, None, "null")
    strided = dict(stride=4, k=8, ldy=2)
    for name in ("x", "w", "bias", "y"):
        assert _refused(convs, _conv_args(**{name: None}), "null"), name
        assert _refused(convs, _conv_args(**{name: None}, **strided), "null"), name
    a = _conv_args()
    assert _refused(convs, _conv_args(alpha=a.x), "alpha and inv") and _refused(convs, _conv_args(inv=a.x, **strided), "alpha and inv")
    alias = _conv_args()
    alias.y = alias.x
    assert _refused(convs, alias, "y must not be x")
    assert _refused(convs, _conv_args(w=a.w + 4), "aligned")
    for field, bad in (("C_in", 0), ("C_in", 4097), ("C_out", 0), ("C_out", 4097)):
        assert _refused(convs, _conv_args(**{field: bad}), "outside"), (field, bad)
    assert _refused(convs, _conv_args(T=0), "T = 0") and _refused(convs, _conv_args(T=(1 << 24) + 1, ldx=1 << 25, ldy=1 << 25), "T =")
    assert _refused(convs, _conv_args(B=0), "B = 0") and _refused(convs, _conv_args(B=65536), "B = 65536")
    assert _refused(convs, _conv_args(ldx=7), "ldx") and _refused(convs, _conv_args(ldy=7), "ldy")
    assert _refused(convs, _conv_args(stride=4, k=8, ldy=1), "ldy")                                  # 8 / 4 = 2 outputs
    assert _refused(convs, _conv_args(tanh_out=2), "tanh_out")
    for s in (1, 3, 6, 16, -2):
        assert _refused(convs, _conv_args(stride=s, k=2 * s), "stride"), s
    for k in (0, 1, 5, 7):
        assert _refused(convs, _conv_args(k=k), "kernel size"), k                                     # stride 0 is the k-3 form only
    assert _refused(convs, _conv_args(stride=4, k=7, ldy=2), "kernel size")
    assert _refused(convs, _conv_args(dilation=3), "dilation") and _refused(convs, _conv_args(dilation=9, **strided), "dilation")
    assert _refused(convs, _conv_args(res=a.x), "residual") and _refused(convs, _conv_args(res=a.x, **strided), "residual")
    assert _refused(convs, _conv_args(T=10, ldx=10, stride=4, k=8, ldy=8), "multiple")               # a row that stride 4 does not divide
    assert _refused(convs, _conv_args(T=7, ldx=8, stride=2, k=4, ldy=8), "multiple")

    def qa(**over):
        q = K.CodecQuantizeArgs(z=a.x, in_w=a.x, in_b=a.x, codebook=a.x, codebook_sq=a.x, tables=a.x, bias=a.x, codes=a.y, B=1, T=4,
                                n_codebooks=9, codebook_size=1024, codebook_dim=8, latent_dim=64, ldz=4, ld_codes=4)
        for k, v in over.items():
            setattr(q, k, v)
        return q

    for name in ("z", "in_w", "in_b", "codebook", "codebook_sq", "tables", "bias", "codes"):
        assert _refused(quant, qa(**{name: None}), "null"), name
    for field, bad, word in (("n_codebooks", 0, "n_codebooks = 0"), ("n_codebooks", 17, "n_codebooks = 17"),
                             ("codebook_size", 0, "codebook_size = 0"), ("codebook_size", 4097, "codebook_size = 4097"),
                             ("codebook_dim", 0, "codebook_dim = 0"), ("codebook_dim", 33, "codebook_dim = 33"),
                             ("latent_dim", 0, "latent_dim = 0"), ("latent_dim", 4097, "latent_dim = 4097"),
                             ("T", 0, "T = 0"), ("T", (1 << 24) + 1, "T ="), ("B", 0, "B = 0"), ("B", 65536, "B = 65536"),
                             ("ldz", 3, "ldz = 3"), ("ld_codes", 3, "ld_codes = 3")):
        over = {field: bad}
        if field == "T" and bad > 4:
            over.update(ldz=1 << 25, ld_codes=1 << 25)
        assert _refused(quant, qa(**over), word), (field, bad)


def test_struct_size_matches_header(tmp_path):
    import subprocess
    c = tmp_path / "s.c"
    c.write_text('#include <stdio.h>\n#include "dia_hip.h"\nint main(void){ printf("%zu %zu %d\\n", sizeof(dia_codec_quantize_args), '
                 'sizeof(dia_codec_conv_args), DIA_CODEC_MAX_CODEBOOK_SIZE); return 0; }\n')
    exe = tmp_path / "s"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    q, v, size = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert (q, v, size) == (ctypes.sizeof(K.CodecQuantizeArgs), ctypes.sizeof(K.CodecConvArgs), 4096)
