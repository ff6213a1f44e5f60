"""The native codec's host side without a GPU (dia_hip/codec.py, DESIGN.md "Codec"): weight-norm folding, the checkpoint loader,
context_frames and the windowing it feeds, the streaming state, the wave fallback of save_audio, the CLI's --codec-path rules and
every DIA_E_ARG path of dia_codec_embed / dia_codec_conv / dia_codec_convt (none of which launches).

The reference is tests/codec_ref.py: a plain-torch restatement in float64 on the CPU."""
import ctypes
import os
import sys
import wave

import numpy as np
import pytest
import torch

from codec_ref import RefCodec, random_codes
from dia_hip import binding as hb
from dia_hip import codec as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


@pytest.fixture(scope="module")
def mini():
    cfg = K.mini_config()
    sd = K.synthetic_state_dict(cfg, seed=7)
    return cfg, sd, RefCodec(cfg, sd, torch.float64)


@pytest.fixture(scope="module")
def whole37(mini):
    cfg, _, ref = mini
    codes = random_codes(cfg, 37, seed=1)
    return codes, ref.decode(codes)


def test_weight_norm_folding_matches_torch():
    torch.manual_seed(0)
    conv = torch.nn.utils.weight_norm(torch.nn.Conv1d(6, 10, 7).double())
    convt = torch.nn.utils.weight_norm(torch.nn.ConvTranspose1d(6, 10, 8, stride=4).double())
    for m in (conv, convt):
        with torch.no_grad():
            m.weight_g.mul_(torch.rand_like(m.weight_g) + 0.5)
        x = torch.randn(1, 6, 9, dtype=torch.float64)
        m(x)                                                     # the hook recomputes .weight from g and v
        w = K.fold_weight_norm(m.weight_g, m.weight_v)
        assert w.dtype == torch.float64
        assert torch.allclose(w, m.weight.detach(), rtol=0, atol=1e-14)
    # the transposed convolution's norm runs per INPUT channel (dimension 0), not per output channel
    assert tuple(convt.weight_g.shape) == (6, 1, 1)
    wrong = convt.weight_g.detach() * convt.weight_v.detach() / convt.weight_v.detach().pow(2).sum(dim=(0, 2), keepdim=True).sqrt().mean()
    assert not torch.allclose(wrong, convt.weight.detach(), atol=1e-6)


def test_layouts_are_tap_major():
    w = torch.arange(5 * 3 * 7, dtype=torch.float64).reshape(5, 3, 7)
    t = K.conv_layout(w)
    assert tuple(t.shape) == (7, 3, 32) and t.dtype == torch.float32
    assert t[4, 2, 3] == w[3, 2, 4] and float(t[:, :, 5:].abs().max()) == 0.0
    wt = torch.arange(3 * 5 * 8, dtype=torch.float64).reshape(3, 5, 8)
    t = K.convt_layout(wt)
    assert tuple(t.shape) == (4, 2, 3, 32)
    assert t[1, 0, 2, 4] == wt[2, 4, 1] and t[1, 1, 2, 4] == wt[2, 4, 5]


def test_synthetic_waveform_neither_vanishes_nor_saturates(mini, whole37):
    assert 0.05 <= float(np.sqrt((whole37[1] ** 2).mean())) <= 0.9
    cfg = K.CodecConfig()
    y = RefCodec(cfg, K.synthetic_state_dict(cfg, seed=7)).decode(random_codes(cfg, 3, seed=3))
    assert y.shape == (3 * 512,) and 0.05 <= float(np.sqrt((y ** 2).mean())) <= 0.9


def test_loader_round_trip_and_refusals(tmp_path, mini):
    cfg, sd, _ = mini
    meta = {"kwargs": {"n_codebooks": 9, "codebook_size": 1024, "codebook_dim": 8, "latent_dim": 64, "decoder_dim": 192,
                       "decoder_rates": [8, 8, 4, 2], "sample_rate": 44100, "encoder_dim": 64}}
    full = dict(sd)
    full["encoder.block.0.weight_v"] = torch.zeros(2, 2, 2)                    # encode side: ignored
    full["quantizer.quantizers.0.in_proj.weight_v"] = torch.zeros(8, 64, 1)
    p = tmp_path / "weights.pth"
    torch.save({"state_dict": full, "metadata": meta}, p)
    got_cfg, got = K.load_codec_state(str(p))
    assert got_cfg == cfg and set(got) == set(sd)
    assert all(torch.equal(got[k], sd[k]) for k in sd)
    bare_cfg, bare = K.load_codec_state(dict(sd))                              # bare state dict: configuration from shapes
    assert bare_cfg == cfg and set(bare) == set(sd)
    assert K.load_codec_state(K.synthetic_state_dict(K.CodecConfig(), 0))[0] == K.CodecConfig()
    key = "decoder.model.2.block.3.block.1.weight_g"
    with pytest.raises(KeyError, match=key.replace(".", r"\.")):
        K.load_codec_state({k: v for k, v in sd.items() if k != key})
    with pytest.raises(KeyError, match=r"quantizer\.quantizers\.4\.out_proj\.bias"):
        K.load_codec_state({k: v for k, v in sd.items() if k != "quantizer.quantizers.4.out_proj.bias"})
    with pytest.raises(KeyError, match=r"unexpected.*decoder\.model\.9\.alpha"):
        K.load_codec_state({**sd, "decoder.model.9.alpha": torch.zeros(1, 4, 1)})
    with pytest.raises(KeyError, match=r"unexpected.*quantizer\.extra"):
        K.load_codec_state({**sd, "quantizer.extra": torch.zeros(1)})
    with pytest.raises(ValueError, match=r"decoder\.model\.6\.bias"):
        K.load_codec_state({**sd, "decoder.model.6.bias": torch.zeros(2)})


def test_context_frames_is_exact_and_tight(mini, whole37):
    cfg, _, ref = mini
    codes, whole = whole37                                                     # T = 37: no multiple of 3 or 16
    ctx = K.context_frames(cfg)
    assert ctx == K.context_frames(K.CodecConfig())                            # widths do not enter
    assert 6 <= ctx <= 16
    for window in (1, 3, 16):
        assert np.array_equal(K.decode_windowed(ref.decode, codes, window, ctx, cfg.hop), whole), window
        short = K.decode_windowed(ref.decode, codes, window, ctx - 1, cfg.hop)
        assert short.shape == whole.shape and not np.array_equal(short, whole), window
    plan = K.window_plan(37, 16, ctx)
    assert [(f0, f1) for _, f0, f1, _ in plan] == [(0, 16), (16, 32), (32, 37)]
    assert all(hi - lo <= 16 + 2 * ctx for lo, _, _, hi in plan)


def test_stream_state_reproduces_whole_decode(mini, whole37):
    cfg, _, ref = mini
    codes, whole = whole37
    ctx = K.context_frames(cfg)
    rng = np.random.default_rng(5)
    for trial, window in enumerate((4, 16, 64)):
        cuts = sorted(rng.integers(0, 38, size=6).tolist())
        chunks = [codes[:, a:b] for a, b in zip([0] + cuts, cuts + [37])]
        chunks.insert(2, codes[:, :0])                                         # an empty chunk on the way
        last_empty = trial % 2 == 0
        if last_empty:
            chunks.append(codes[:, :0])                                        # the final chunk with n = 0
        st = K.CodecStream(ref.decode, cfg.n_codebooks, cfg.hop, window, ctx)
        out, done = [], 0
        for j, c in enumerate(chunks):
            y = st.push(c[None] if j % 2 else c, final=j == len(chunks) - 1)
            out.append(y)
            done += c.shape[1]
            if j < len(chunks) - 1:
                assert sum(o.shape[0] for o in out) == max(0, done - ctx) * cfg.hop   # the last ctx frames are held back
                assert st.buf.shape[1] <= 2 * ctx + max(c.shape[1] for c in chunks)   # the state does not grow with the utterance
        assert np.array_equal(np.concatenate(out), whole)
        with pytest.raises(RuntimeError):
            st.push(codes[:, :1])
    st = K.CodecStream(ref.decode, cfg.n_codebooks, cfg.hop, 8, ctx)
    assert st.push(codes[:, :0], final=True).shape == (0,)                     # an utterance without a frame


def test_save_audio_wave_fallback(tmp_path, monkeypatch):
    from dia_hip.model import Dia
    monkeypatch.setitem(sys.modules, "soundfile", None)                        # import soundfile -> ImportError
    x = np.concatenate([np.linspace(-1.2, 1.2, 999), [0.0, 1.0, -1.0]]).astype(np.float32)
    p = tmp_path / "sub" / "a.wav"
    Dia.save_audio(None, str(p), x)
    with wave.open(str(p), "rb") as f:
        assert (f.getnchannels(), f.getsampwidth(), f.getframerate(), f.getnframes()) == (1, 2, 44100, 1002)
        back = np.frombuffer(f.readframes(1002), dtype="<i2").astype(np.float64) / 32767.0
    assert np.abs(back - x.clip(-1, 1)).max() <= 1.0 / 32767.0
    q = tmp_path / "a.flac"                                                    # every other case behaves as before: printed, not raised
    Dia.save_audio(None, str(q), x)
    assert not q.exists()


def test_cli_codec_path_rules(tmp_path, mini):
    import cli
    p = cli.build_parser()
    assert p.parse_args(["x", "--output", "o.wav", "--codec-path", "c.pth"]).codec_path == "c.pth"
    ck = tmp_path / "c.pth"
    torch.save(mini[1], ck)

    def refused(argv):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        return e.value.code == 2

    assert refused(["x", "--output", "o.wav", "--codec-path", str(tmp_path / "none.pth")])          # not a file
    assert refused(["x", "--output", "o.wav", "--no-dac"])                                           # as before
    assert refused(["x", "--output", "o.wav", "--stream-chunk", "4"])                                # as before: no native codec
    assert refused(["x", "--output", "o.wav", "--stream-chunk", "4", "--codec-path", str(ck), "--slots", "2"])
    assert refused(["x", "--output", "o.wav", "--stream-chunk", "4", "--codec-path", str(ck), "--audio-prompt", "p.npy",
                    "--audio-prompt-text", "t"])
    assert refused(["x", "--score-codes", "c.npy", "--model-path", str(tmp_path), "--codec-path", str(ck)])
    assert refused(["x", "--codec-path", str(ck)])                                                   # an output is still required
    # accepted flag sets get past the parser: they then fail at the model directory, which is not a flag rule
    for argv in (["x", "--output", "o.wav", "--codec-path", str(ck)],
                 ["x", "--output", "o.wav", "--codec-path", str(ck), "--no-dac"],
                 ["x", "--output", "o.wav", "--codec-path", str(ck), "--stream-chunk", "4"]):
        assert cli.main(argv + ["--model-path", str(tmp_path / "no-model")]) == 1


# ---------------------------------------------------------------------------------------------- DIA_E_ARG, no launch
def _conv_args(**over):
    buf = ctypes.create_string_buffer(64)
    base = ctypes.addressof(buf) // 16 * 16 + 16
    a = K.CodecConvArgs(x=base, w=base + 16, bias=base, y=base + 4, B=1, T=8, C_in=4, C_out=4, ldx=8, ldy=8, k=7, dilation=1)
    a._keep = buf
    for k, v in over.items():
        setattr(a, k, v)
    return a


def _refused(fn, a, word):
    rc = fn(ctypes.byref(a), None) if a is not None else fn(None, None)
    msg = hb.lib().dia_last_error().decode()
    return rc == -1 and word in msg


def test_codec_argument_validation_without_gpu():
    L = K._fns()
    conv, convt, embed = L.dia_codec_conv, L.dia_codec_convt, L.dia_codec_embed
    assert _refused(conv, None, "null") and _refused(convt, None, "null") and _refused(embed, None, "null")
    for name in ("x", "w", "bias", "y"):
        assert _refused(conv, _conv_args(**{name: None}), "null"), name
        assert _refused(convt, _conv_args(**{name: None, "stride": 2, "k": 4, "ldy": 16}), "null"), name
    a = _conv_args()
    assert _refused(conv, _conv_args(alpha=a.x), "alpha and inv") and _refused(conv, _conv_args(inv=a.x), "alpha and inv")
    alias = _conv_args()
    alias.y = alias.x
    assert _refused(conv, alias, "y must not be x")
    assert _refused(conv, _conv_args(w=a.w + 4), "aligned")
    for field, bad in (("C_in", 0), ("C_in", 4097), ("C_out", 0), ("C_out", 4097)):
        assert _refused(conv, _conv_args(**{field: bad}), "outside"), (field, bad)
    assert _refused(conv, _conv_args(T=0), "T = 0") and _refused(conv, _conv_args(T=(1 << 24) + 1, ldx=1 << 25, ldy=1 << 25), "T =")
    assert _refused(conv, _conv_args(B=0), "B = 0") and _refused(conv, _conv_args(B=65536), "B = 65536")
    assert _refused(convt, _conv_args(B=8192, stride=8, k=16, ldy=64), "B = 8192")
    assert _refused(conv, _conv_args(ldx=7), "ldx") and _refused(conv, _conv_args(ldy=7), "ldy")
    assert _refused(convt, _conv_args(stride=4, k=8, ldy=31), "ldy")
    assert _refused(conv, _conv_args(tanh_out=2), "tanh_out")
    for k in (0, 3, 5, 9):
        assert _refused(conv, _conv_args(k=k), "kernel size"), k
    for d in (0, 2, 4, 27):
        assert _refused(conv, _conv_args(dilation=d), "dilation"), d
    assert _refused(conv, _conv_args(k=1, dilation=3), "dilation 1")
    assert _refused(conv, _conv_args(stride=2), "stride")
    for s in (0, 1, 3, 16):
        assert _refused(convt, _conv_args(stride=s, k=2 * s, ldy=128), "stride"), s
    assert _refused(convt, _conv_args(stride=4, k=7, ldy=32), "kernel size")
    assert _refused(convt, _conv_args(stride=4, k=8, dilation=3, ldy=32), "dilation")
    assert _refused(convt, _conv_args(stride=4, k=8, dilation=1, ldy=32, res=a.x), "residual")

    def emb(**over):
        e = K.CodecEmbedArgs(codes=a.x, tables=a.x, bias=a.x, z=a.y, B=1, T=4, n_codebooks=9, codebook_size=1024, latent_dim=64,
                             ld_codes=4, ldz=4)
        for k, v in over.items():
            setattr(e, k, v)
        return e

    for name in ("codes", "tables", "bias", "z"):
        assert _refused(embed, emb(**{name: None}), "null"), name
    for field, bad, word in (("n_codebooks", 0, "n_codebooks"), ("n_codebooks", 17, "n_codebooks"), ("codebook_size", 0, "codebook_size"),
                             ("latent_dim", 0, "latent_dim"), ("latent_dim", 4097, "latent_dim"), ("T", 0, "T = 0"), ("B", 0, "B = 0"),
                             ("B", 65536, "B = 65536"), ("ld_codes", 3, "ld_codes"), ("ldz", 3, "ldz")):
        assert _refused(embed, emb(**{field: bad}), word), (field, bad)


def test_decode_refuses_ids_outside_the_codebook(mini):
    cfg, _, _ = mini
    check = K.DeviceCodec._check_codes
    holder = type("H", (), {"cfg": cfg})()
    good = random_codes(cfg, 4, seed=0)
    assert check(holder, good[None]).shape == (9, 4)
    for bad in (-1, 1024):
        c = good.copy()
        c[3, 2] = bad
        with pytest.raises(ValueError, match="outside"):
            check(holder, c)
    with pytest.raises(ValueError, match="shape"):
        check(holder, good[:8])
