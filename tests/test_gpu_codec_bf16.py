"""The codec's bf16 modes on the MI355X (csrc/codec_bf16.hip, dia_hip/codec.py, DESIGN.md "Codec: bf16 modes") against
tests/codec_bf16_ref.py: float64 over operands split as the device splits them, with the derived bound of the fp32 accumulation
(acc_bound) as the only allowance; bitwise reproducibility within a mode; whole decoders against the exact float64 decode with the
CPU emulation's own error as the yardstick.  Every accuracy test prints its figures before it asserts.

The float64 side of a single launch is products() over the split operands, the emulation of the layer: the three products the
kernel forms for bf16x2, so that the device differs from it by its fp32 accumulation and epilogue alone.  For bf16x2 the full
product of the plane sums is checked as well, with the dropped w_lo v_lo at its worst case of 2^-16 sum |w_j| |v_j| (measured
2^-17.55 of it on 12-term sums, 2^-22.1 on 5376-term ones): the 2^-18 the modes were specified with is below what short sums
reach, so against the full product a 12-term case used 1.098 of a bound built with it.

Measured on the MI355X: DESIGN.md "Codec: bf16 modes" has the table."""
import os
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from codec_bf16_ref import EmuCodec, acc_bound, planes_of, products, settle, snr_db
from codec_ref import RefCodec, random_codes, snake
from dia_hip import codec as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")
MODES = ["bf16x2", "bf16"]
PLANES = {"bf16": 1, "bf16x2": 2}


def dev_conv(mode, x, w, b, alpha, res, tanh, lens=None, **kw):
    """x / res as CPU tensors -> the library's result in `mode` as a numpy array"""
    stride = kw.get("stride", 0)
    wl = (K.convt_layout_bf16 if stride else K.conv_layout_bf16)(w, PLANES[mode]).to(DEV)
    al = None if alpha is None else alpha.to(torch.float32).to(DEV)
    iv = None if alpha is None else K.snake_inverse(alpha).to(DEV)
    y = K.codec_conv(x.to(torch.float32).to(DEV).contiguous(), wl, b.to(torch.float32).to(DEV), c_out=w.shape[1] if stride else w.shape[0],
                     alpha=al, inv=iv, res=None if res is None else res.to(torch.float32).to(DEV).contiguous(), tanh=tanh,
                     lens=None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV), precision=mode, **kw)
    return y.cpu().numpy()


def make_layer(g, cin, cout, k, transposed=False):
    w = torch.randn(*((cin, cout, k) if transposed else (cout, cin, k)), generator=g, dtype=torch.float64)
    w = w / np.sqrt(cin * (2 if transposed else k))
    return w.float().double(), (0.1 * torch.randn(cout, generator=g)).double(), (0.5 + torch.rand(cin, generator=g)).float().double()


def check_layer(name, mode, x, w, b, alpha, res, tanh, share, **kw):
    """one launch against float64 over the split operands (products(): what the emulation forms).  x is what the layer reads;
    with alpha it must have been through settle().  Returns nothing; `share` collects the largest used share of the bound."""
    planes = PLANES[mode]
    stride = kw.get("stride", 0)
    if stride:
        conv = lambda a, ww: F.conv_transpose1d(a, ww, None, stride=stride, padding=-(-stride // 2))
        cin, taps = w.shape[0], 2
    else:
        k, d = kw["k"], kw["dilation"]
        conv = lambda a, ww: F.conv1d(a, ww, None, dilation=d, padding=(k // 2) * d)
        cin, taps = w.shape[1], k
    v = x if alpha is None else snake(x, alpha.reshape(1, -1, 1))
    vp, wp = planes_of(v, planes), planes_of(w, planes)
    vq, wq = sum(vp), sum(wp)
    n = (3 if planes == 2 else 1) * cin * taps
    dev = dev_conv(mode, x, w, b, alpha, res, tanh, **kw)
    # the emulation's three products with the specified bound; for bf16x2 also the full product with the dropped term's worst case
    sides = [("emulation", products(lambda a, ww, _: conv(a, ww), vp, wp), 2.0 ** -18)]
    if planes == 2:
        sides.append(("full product", conv(vq, wq), 2.0 ** -16))
    for side, s, lolo in sides:
        pre = s + b.reshape(1, -1, 1)
        out = pre if res is None else pre + res
        ref = torch.tanh(out) if tanh else out
        bound = acc_bound(w, v, planes, conv, n, pre=pre, out=None if res is None else out, tanh=tanh, lolo=lolo)
        if alpha is not None and planes == 2:                    # one unit of the lo plane per staged value cannot be settled away
            bound = bound + conv(2.0 ** -16 * vq.abs(), wq.abs())
        assert dev.shape == tuple(ref.shape) and np.all(np.isfinite(dev)), name
        err = (torch.from_numpy(dev).double() - ref).abs()
        used = float((err / bound).max())
        if side == "emulation":
            share[0] = max(share[0], used)
        if used > 1:
            print(f"codec-bf16 {mode} {name} vs {side}: error {float(err.max()):.3e}, {used:.3f} of the bound")
        assert used <= 1, (name, mode, side, used)


CHANNELS = [(12, 12), (24, 12), (20, 1), (96, 1), (80, 80), (44, 12)]      # (44, 12): no multiple of 8, more than one chunk
TAPS = [(1, 1), (7, 1), (7, 3), (7, 9)]
FLAGS = [(False, False), (True, False), (False, True), (True, True)]      # (residual, tanh)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k,d", TAPS)
@pytest.mark.parametrize("cin,cout", CHANNELS)
def test_conv_family_strict(cin, cout, k, d, mode):
    g = torch.Generator().manual_seed(cin * 100 + cout * 10 + k + d)
    w, b, _ = make_layer(g, cin, cout, k)
    share = [0.0]
    for T in (1, 5, 63, 64, 130):
        x = torch.randn(1, cin, T, generator=g).double()
        r = torch.randn(1, cout, T, generator=g).double()
        for use_res, use_tanh in FLAGS:
            check_layer(f"conv {cin}->{cout} k{k} d{d} T{T} res{int(use_res)} tanh{int(use_tanh)}", mode, x, w, b, None,
                        r if use_res else None, use_tanh, share, k=k, dilation=d)
    print(f"codec-bf16 {mode} conv {cin}->{cout} k{k} d{d}: largest used share of acc_bound {share[0]:.3f}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("s", [2, 4, 8])
@pytest.mark.parametrize("cin,cout", [(24, 12), (96, 48)])
def test_transposed_conv_strict(cin, cout, s, mode):
    g = torch.Generator().manual_seed(cin + s)
    w, b, _ = make_layer(g, cin, cout, 2 * s, transposed=True)
    share = [0.0]
    for T in (1, 2, 33, 129):                                    # 129: T + 1 input positions, two blocks
        x = torch.randn(1, cin, T, generator=g).double()
        check_layer(f"convT {cin}->{cout} s{s} T{T}", mode, x, w, b, None, None, False, share, stride=s)
    print(f"codec-bf16 {mode} convT {cin}->{cout} s{s}: largest used share of acc_bound {share[0]:.3f}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k,d", TAPS)
@pytest.mark.parametrize("cin,cout", CHANNELS)
def test_conv_family_with_snake(cin, cout, k, d, mode):
    g = torch.Generator().manual_seed(cin * 100 + cout * 10 + k + d + 1)
    w, b, alpha = make_layer(g, cin, cout, k)
    share = [0.0]
    for T in (5, 130):
        x, _ = settle(torch.randn(1, cin, T, generator=g).double(), alpha, g)
        r = torch.randn(1, cout, T, generator=g).double()
        for use_res, use_tanh in FLAGS:
            check_layer(f"snake conv {cin}->{cout} k{k} d{d} T{T} res{int(use_res)} tanh{int(use_tanh)}", mode, x, w, b, alpha,
                        r if use_res else None, use_tanh, share, k=k, dilation=d)
    print(f"codec-bf16 {mode} snake conv {cin}->{cout} k{k} d{d}: largest used share of the bound {share[0]:.3f}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("s", [2, 4, 8])
@pytest.mark.parametrize("cin,cout", [(24, 12), (96, 48)])
def test_transposed_conv_with_snake(cin, cout, s, mode):
    g = torch.Generator().manual_seed(cin + s + 1)
    w, b, alpha = make_layer(g, cin, cout, 2 * s, transposed=True)
    share = [0.0]
    for T in (5, 130):
        x, _ = settle(torch.randn(1, cin, T, generator=g).double(), alpha, g)
        check_layer(f"snake convT {cin}->{cout} s{s} T{T}", mode, x, w, b, alpha, None, False, share, stride=s)
    print(f"codec-bf16 {mode} snake convT {cin}->{cout} s{s}: largest used share of the bound {share[0]:.3f}")


# ---------------------------------------------------------------------------------------------- bitwise, per mode
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cin,cout,k,d", [(24, 12, 1, 1), (24, 12, 7, 9), (96, 1, 7, 9), (80, 80, 7, 3)])
def test_conv_batch_rows_equal_solo_launches(cin, cout, k, d, mode):
    g = torch.Generator().manual_seed(5)
    w, b, alpha = make_layer(g, cin, cout, k)
    lens = (130, 1, 64)
    x = torch.randn(3, cin, 130, generator=g)
    r = torch.randn(3, cout, 130, generator=g)
    for bi, n in enumerate(lens):                                # what lies behind a row's end must never be read
        x[bi, :, n:] = float("nan")
        r[bi, :, n:] = float("nan")
    both = dev_conv(mode, x, w, b, alpha, r, False, lens=lens, k=k, dilation=d)
    for bi, n in enumerate(lens):
        solo = dev_conv(mode, x[bi:bi + 1, :, :n], w, b, alpha, r[bi:bi + 1, :, :n], False, k=k, dilation=d)
        assert np.all(np.isfinite(solo)) and np.array_equal(both[bi, :, :n], solo[0]), (bi, n)
        assert not both[bi, :, n:].any()                         # and nothing is written there


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("s", [2, 8])
def test_transposed_batch_rows_equal_solo_launches(s, mode):
    g = torch.Generator().manual_seed(6)
    w, b, alpha = make_layer(g, 24, 12, 2 * s, transposed=True)
    lens = (33, 1, 20)
    x = torch.randn(3, 24, 33, generator=g)
    for bi, n in enumerate(lens):
        x[bi, :, n:] = float("nan")
    both = dev_conv(mode, x, w, b, alpha, None, False, lens=lens, stride=s)
    for bi, n in enumerate(lens):
        solo = dev_conv(mode, x[bi:bi + 1, :, :n], w, b, alpha, None, False, stride=s)
        assert np.all(np.isfinite(solo)) and np.array_equal(both[bi, :, :n * s], solo[0]) and not both[bi, :, n * s:].any(), (s, bi)


@pytest.fixture(scope="module")
def mini():
    cfg = K.mini_config()
    sd = K.synthetic_state_dict(cfg, seed=7)
    return cfg, sd, RefCodec(cfg, sd, torch.float64)


@pytest.fixture(scope="module")
def devs(mini):
    cfg, sd, _ = mini
    return {m: K.DeviceCodec((cfg, sd), DEV, window=64, precision=m) for m in MODES + ["fp32"]}


@pytest.fixture(scope="module")
def mini40(mini):
    codes = random_codes(mini[0], 40, seed=40)
    return codes, mini[2].decode(codes)


@pytest.mark.parametrize("mode", MODES)
def test_windows_ragged_batches_and_streams_are_bitwise(mini, devs, mini40, mode):
    dev, codes = devs[mode], mini40[0]
    assert dev.precision == mode and all("w" not in L and L["w_bf16"].dtype == torch.bfloat16 for L in dev.layers)
    whole = dev.decode(codes)
    assert np.array_equal(whole, dev.decode(codes, window=8))
    assert not np.array_equal(whole, devs["fp32"].decode(codes))  # and it is another arithmetic than the exact kernel's
    rows = [codes, codes[:, :1], codes[:, 5:22], codes[:, :0]]
    got = dev.decode_batch(rows, window=8)
    for r, y in zip(rows, got):
        assert y.shape == (r.shape[1] * 512,) and np.array_equal(y, dev.decode(r, window=8))
    st = dev.stream(window=8)
    out = [st.push(codes[:, a:b], final=b == 40 and a == 40) for a, b in ((0, 7), (7, 7), (7, 30), (30, 40), (40, 40))]
    assert np.array_equal(np.concatenate(out), whole)


# ---------------------------------------------------------------------------------------------- whole decoders against exact float64
def whole_decoder(name, mode, cfg, sd, dev, codes, exact):
    emu = EmuCodec(cfg, sd, PLANES[mode]).decode(codes)
    y = dev.decode(codes)
    assert y.dtype == np.float32 and y.shape == exact.shape and np.all(np.isfinite(y))
    e_emu, e_dev = float(np.abs(emu - exact).max()), float(np.abs(y - exact).max())
    s_emu, s_dev = snr_db(emu, exact), snr_db(y, exact)
    rms = float(np.sqrt((y.astype(np.float64) ** 2).mean()))
    print(f"codec-bf16 {mode} {name}: e_emu {e_emu:.3e} device {e_dev:.3e} bound {2 * e_emu + 1e-6:.3e}; SNR emulation {s_emu:.2f} dB "
          f"device {s_dev:.2f} dB; max|device - emulation| / e_emu {float(np.abs(y - emu).max()) / e_emu:.3f}; rms {rms:.3f}")
    assert e_dev <= 2 * e_emu + 1e-6, (name, mode, e_dev, e_emu)
    assert s_dev >= s_emu - 1.0, (name, mode, s_dev, s_emu)
    assert 0.2 <= rms <= 0.5, (name, mode, rms)


@pytest.mark.parametrize("mode", MODES)
def test_mini_decoders_against_exact(mini, devs, mini40, mode):
    cfg, sd, r64 = mini
    c3 = random_codes(cfg, 3, seed=3)
    whole_decoder("mini T3", mode, cfg, sd, devs[mode], c3, r64.decode(c3))
    whole_decoder("mini T40", mode, cfg, sd, devs[mode], mini40[0], mini40[1])


@pytest.fixture(scope="module")
def full():
    cfg = K.CodecConfig()
    sd = K.synthetic_state_dict(cfg, seed=7)
    codes = random_codes(cfg, 3, seed=3)
    return cfg, sd, codes, RefCodec(cfg, sd, torch.float64).decode(codes)


@pytest.mark.parametrize("mode", MODES)
def test_full_size_decoder_against_exact(full, mode):
    cfg, sd, codes, exact = full
    whole_decoder("full T3", mode, cfg, sd, K.DeviceCodec(sd, DEV, window=8, precision=mode), codes, exact)


# ---------------------------------------------------------------------------------------------- fp32 untouched
def test_fp32_codec_is_the_chain_of_fp32_launches_and_holds_no_bf16_image(mini, devs, mini40):
    cfg, sd, _ = mini
    dev, codes = devs["fp32"], mini40[0]
    assert dev.precision == "fp32" and dev.planes == 0
    assert all("w_bf16" not in L and L["w"].dtype == torch.float32 for L in dev.layers)
    assert not any(isinstance(v, torch.Tensor) and v.dtype == torch.bfloat16 for L in dev.layers for v in L.values())
    assert np.array_equal(dev.decode(codes), K.DeviceCodec((cfg, sd), DEV, window=64).decode(codes))      # the default is fp32
    # the same layers as single codec_conv launches of the fp32 entry points
    x = K.codec_embed(torch.from_numpy(codes[None].astype(np.int32)).to(DEV), dev.tables, dev.embed_bias)
    for L in dev.layers:
        kw = dict(stride=L["s"]) if L["kind"] == "convt" else dict(k=L["k"], dilation=L["d"])
        if L.get("res"):
            x = K.codec_conv(y, L["w"], L["b"], c_out=L["cout"], alpha=L["alpha"], inv=L["inv"], res=x, **kw)
        else:
            y = K.codec_conv(x, L["w"], L["b"], c_out=L["cout"], alpha=L.get("alpha"), inv=L.get("inv"), tanh=bool(L.get("tanh")), **kw)
            if L["kind"] == "convt" or not L["snake"] or L.get("tanh"):
                x = y
    assert np.array_equal(x[0, 0].cpu().numpy(), dev.decode(codes))


# ---------------------------------------------------------------------------------------------- end to end
def test_dia_generates_streams_and_writes_audio_in_bf16x2(mini, tmp_path):
    from dia_hip import config as C
    from dia_hip.model import Dia
    from dia_hip.weights import synthetic_state_dict
    ccfg, csd, _ = mini
    cfg = C.mid_config()
    sd = synthetic_state_dict(cfg, seed=1234, std=0.02)
    text = "[S1] Dia is an open weights text to dialogue model."
    dia = Dia.from_state_dict(cfg, sd, "float32", DEV)
    assert dia.codec_precision == "fp32"
    dia.load_codec(csd, window=16, precision="bf16x2")
    assert dia.codec.cfg == ccfg and dia.codec.precision == "bf16x2" and dia.codec_precision == "bf16x2"
    codes = dia.generate_codes(text, max_tokens=30, seed=3)
    n = codes.shape[-1]
    assert n > 4
    audio = dia.generate(text, max_tokens=30, seed=3)
    assert audio.shape == (n * 512,) and audio.dtype == np.float32 and np.all(np.isfinite(audio))
    assert np.array_equal(audio, dia.codec.decode(codes))
    chunks = list(dia.stream_audio([text], 1, max_tokens=30, seeds=[3], chunk=4))
    assert np.array_equal(np.concatenate([c[2] for c in chunks]), audio)
    # the CLI in a fresh child process; soundfile or not, the file holds the same 16-bit samples
    mdir = tmp_path / "model"
    mdir.mkdir()
    torch.save(sd, mdir / "pytorch_model.bin")
    cfg.save(mdir / "config.json")
    ck = tmp_path / "codec.pth"
    torch.save({"state_dict": csd, "metadata": {"kwargs": {"sample_rate": 44100}}}, ck)
    out = tmp_path / "bf16x2.wav"
    argv = [sys.executable, os.path.join(ROOT, "cli.py"), text, "--model-path", str(mdir), "--compute-dtype", "float32", "--max-tokens", "30",
            "--seed", "3", "--codec-path", str(ck), "--codec-precision", "bf16x2", "--output", str(out)]
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "dia-tts-prune_amd"), ROOT, os.environ.get("PYTHONPATH", "")]))
    done = subprocess.run(argv, env=env, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0 and "bf16x2 decoder" in done.stdout, done.stdout[-2000:] + done.stderr[-2000:]
    pcm = np.round(audio.astype(np.float64).clip(-1, 1) * 32767.0)
    with wave.open(str(out), "rb") as f:                          # 16-bit PCM from soundfile or from the wave module: scales of 32768 / 32767
        assert (f.getnchannels(), f.getsampwidth(), f.getframerate(), f.getnframes()) == (1, 2, 44100, n * 512)
        data = np.frombuffer(f.readframes(n * 512), dtype="<i2").astype(np.float64)
    assert np.abs(data - pcm).max() <= 1
