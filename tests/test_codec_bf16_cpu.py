"""The codec's bf16 modes without a GPU (dia_hip/codec.py, csrc/codec_bf16.hip, DESIGN.md "Codec: bf16 modes"): the bf16 weight
images, the float64 emulation of tests/codec_bf16_ref.py, how far each mode is from the exact decode, the names `precision` is
refused by, and every DIA_E_ARG path of dia_codec_conv_bf16 / dia_codec_convt_bf16 (none of which launches)."""
import ctypes

import numpy as np
import pytest
import torch

from codec_bf16_ref import EmuCodec, boundary_distance, planes_of, q1, q2, settle, settle_margin, snr_db
from codec_ref import RefCodec, random_codes, snake
from dia_hip import binding as hb
from dia_hip import codec as K


@pytest.fixture(scope="module")
def mini():
    cfg = K.mini_config()
    return cfg, K.synthetic_state_dict(cfg, seed=7)


def ungroup(img):
    """[..., Ci / 8, Cp, 8] -> [..., Ci, Cp]"""
    return img.transpose(-1, -2).reshape(*img.shape[:-3], img.shape[-3] * 8, img.shape[-2])


@pytest.mark.parametrize("planes", [1, 2])
def test_bf16_layouts_hold_the_planes_of_the_fp32_layouts(planes):
    g = torch.Generator().manual_seed(1)
    q = q1 if planes == 1 else q2
    for co, ci, k in ((12, 24, 7), (1, 20, 7), (80, 44, 1), (33, 16, 7)):
        w = torch.randn(co, ci, k, generator=g, dtype=torch.float64)
        img = K.conv_layout_bf16(w, planes)
        cp, cpad = (co + 31) // 32 * 32, (ci + 15) // 16 * 16
        assert img.dtype == torch.bfloat16 and img.is_contiguous() and tuple(img.shape) == (planes, k, cpad // 8, cp, 8)
        flat = ungroup(img.to(torch.float64))                   # [planes][k][Ci][Cp]
        f32 = K.conv_layout(w)
        assert torch.equal(flat.sum(dim=0)[:, :ci, :], q(f32.to(torch.float64)))
        assert not flat[:, :, ci:, :].any() and not flat[:, :, :, co:].any()
        assert torch.equal(flat[0, :, :ci, :co], q1(w.permute(2, 1, 0).float().double()))
    for ci, co, s in ((24, 12, 2), (96, 48, 8), (20, 33, 4)):
        w = torch.randn(ci, co, 2 * s, generator=g, dtype=torch.float64)
        img = K.convt_layout_bf16(w, planes)
        cp, cpad = (co + 31) // 32 * 32, (ci + 15) // 16 * 16
        assert img.dtype == torch.bfloat16 and tuple(img.shape) == (planes, s, 2, cpad // 8, cp, 8)
        flat = ungroup(img.to(torch.float64))
        assert torch.equal(flat.sum(dim=0)[:, :, :ci, :], q(K.convt_layout(w).to(torch.float64)))
        assert not flat[:, :, :, ci:, :].any() and not flat[:, :, :, :, co:].any()
    with pytest.raises(ValueError, match="planes"):
        K.conv_layout_bf16(torch.zeros(4, 4, 7), 3)


def test_plane_split_is_round_to_nearest_even_with_an_exact_residual():
    x = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -3.14159, 0.0, 1e-30], dtype=torch.float64)
    hi, lo = planes_of(x, 2)
    assert hi[:4].tolist() == [1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7]         # ties to even, above a tie up
    v = x.float().double()
    assert ((v - hi - lo).abs() <= 2.0 ** -17 * v.abs()).all() and (lo.abs() <= 2.0 ** -8 * v.abs()).all()
    assert torch.equal(q1(x), hi) and torch.equal(q2(x), hi + lo) and torch.equal(planes_of(x, 0)[0], x)


def test_emulation_with_the_identity_equals_the_reference(mini):
    cfg, sd = mini
    codes = random_codes(cfg, 3, seed=3)
    assert np.array_equal(EmuCodec(cfg, sd, 0).decode(codes), RefCodec(cfg, sd, torch.float64).decode(codes))


def test_two_planes_are_a_hundred_times_closer_than_one(mini):
    cfg, sd = mini
    codes = random_codes(cfg, 3, seed=3)
    exact = RefCodec(cfg, sd, torch.float64).decode(codes)
    e1 = np.abs(EmuCodec(cfg, sd, 1).decode(codes) - exact).max()
    y2 = EmuCodec(cfg, sd, 2).decode(codes)
    e2 = np.abs(y2 - exact).max()
    print(f"codec-bf16 emulation mini T3: bf16 max error {e1:.3e}, bf16x2 {e2:.3e}, bf16x2 SNR {snr_db(y2, exact):.1f} dB")
    assert 0 < e2 < e1 / 100 and e1 < 0.1


def test_settle_leaves_nothing_near_a_boundary():
    g = torch.Generator().manual_seed(2)
    alpha = (0.5 + torch.rand(24, generator=g)).float().double()
    x = torch.randn(2, 24, 700, generator=g, dtype=torch.float32).double()
    y, frac = settle(x, alpha, g)
    print(f"codec-bf16 settle: {100 * frac:.3f} % of N(0, 1) inputs re-drawn")
    al = alpha.reshape(1, -1, 1)
    assert 0 < frac < 0.05 and not torch.equal(x, y) and (boundary_distance(snake(y, al)) >= settle_margin(y, al)).all()
    assert torch.equal(y, y.float().double())
    # the distance itself: a bf16 value is half a unit from both its boundaries, a midpoint is on one
    assert boundary_distance(torch.tensor([1.0, 1.0 + 2.0 ** -8, -(1.5 + 2.0 ** -8)], dtype=torch.float64)).tolist() == [2.0 ** -8, 0.0, 0.0]


def test_precision_is_refused_by_name(mini, tmp_path):
    from dia_hip.model import Dia
    import cli
    cfg, sd = mini
    assert [K.precision_planes(p) for p in ("fp32", "bf16", "bf16x2")] == [0, 1, 2]
    for bad in ("fp16", "BF16", "", None, 2):
        with pytest.raises(ValueError, match="codec precision"):
            K.precision_planes(bad)
        with pytest.raises(ValueError, match="codec precision"):
            K.DeviceCodec((cfg, sd), torch.device("cpu"), precision=bad)
        with pytest.raises(ValueError, match="codec precision"):
            Dia.load_codec(type("H", (), {"device": torch.device("cpu")})(), (cfg, sd), precision=bad)
    assert Dia.codec_precision == "fp32"
    p = cli.build_parser()
    assert p.parse_args(["x", "--codec-path", "c.pth", "--codec-precision", "bf16x2"]).codec_precision == "bf16x2"
    assert p.parse_args(["x", "--codec-path", "c.pth"]).codec_precision is None
    ck = tmp_path / "c.pth"
    torch.save(sd, ck)
    for argv in (["x", "--output", "o.wav", "--codec-precision", "bf16x2"],                          # needs --codec-path
                 ["x", "--codes-output", "o.npy", "--no-dac", "--codec-precision", "bf16"],
                 ["x", "--output", "o.wav", "--codec-path", str(ck), "--codec-precision", "fp16"]):  # not a mode
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code == 2, argv
    # a valid mode gets as far as the model
    assert cli.main(["x", "--output", "o.wav", "--codec-path", str(ck), "--codec-precision", "bf16x2", "--model-path", str(tmp_path / "no-model")]) == 1


# ---------------------------------------------------------------------------------------------- DIA_E_ARG, no launch
def _conv_args(**over):
    buf = ctypes.create_string_buffer(64)
    base = ctypes.addressof(buf) // 16 * 16 + 16
    a = K.CodecConvArgs(x=base, w=base + 16, bias=base, y=base + 4, B=1, T=8, C_in=4, C_out=4, ldx=8, ldy=8, k=7, dilation=1)
    a._keep = buf
    for k, v in over.items():
        setattr(a, k, v)
    return a


def _refused(fn, a, word, planes=2):
    rc = fn(ctypes.byref(a), planes, None) if a is not None else fn(None, planes, None)
    msg = hb.lib().dia_last_error().decode()
    return rc == -1 and word in msg


def _bad_blocks():
    """(transposed?, argument block or None) per refusal the fp32 and the bf16 entry points share: every shared check, then every
    conv and convt form check"""
    a = _conv_args()
    alias = _conv_args()
    alias.y = alias.x
    t = dict(stride=2, k=4, ldy=16)
    rows = [(False, None), (True, None)]
    for name in ("x", "w", "bias", "y"):
        rows += [(False, _conv_args(**{name: None})), (True, _conv_args(**{name: None}, **t))]
    rows += [(False, _conv_args(alpha=a.x)), (False, _conv_args(inv=a.x)), (True, _conv_args(alpha=a.x, **t)), (False, alias),
             (False, _conv_args(w=a.w + 4)), (True, _conv_args(w=a.w + 4, **t))]
    rows += [(False, _conv_args(**{f: bad})) for f, bad in (("C_in", 0), ("C_in", 4097), ("C_out", 0), ("C_out", 4097))]
    rows += [(False, _conv_args(T=0)), (False, _conv_args(T=(1 << 24) + 1, ldx=1 << 25, ldy=1 << 25)), (True, _conv_args(T=0, **t)),
             (False, _conv_args(B=0)), (False, _conv_args(B=65536)), (True, _conv_args(B=8192, stride=8, k=16, ldy=64)),
             (False, _conv_args(ldx=7)), (False, _conv_args(ldy=7)), (True, _conv_args(stride=4, k=8, ldy=31)),
             (False, _conv_args(tanh_out=2)), (True, _conv_args(tanh_out=-1, **t))]
    rows += [(False, _conv_args(k=k)) for k in (0, 3, 5, 9)]
    rows += [(False, _conv_args(dilation=d)) for d in (0, 2, 4, 27)]
    rows += [(False, _conv_args(k=1, dilation=3)), (False, _conv_args(stride=2))]
    rows += [(True, _conv_args(stride=s, k=2 * s, ldy=128)) for s in (0, 1, 3, 16)]
    rows += [(True, _conv_args(stride=4, k=7, ldy=32)), (True, _conv_args(stride=4, k=8, dilation=3, ldy=32)),
             (True, _conv_args(stride=4, k=8, dilation=1, ldy=32, res=a.x))]
    return rows


def test_bf16_entries_refuse_what_the_fp32_entries_refuse_in_the_same_words():
    """one set of checks behind both (csrc/codec_conv.hpp): a bad block is refused by dia_codec_conv / dia_codec_convt and, with
    planes = 2, by dia_codec_conv_bf16 / dia_codec_convt_bf16, and the two texts differ in the entry points' names alone"""
    L = K._fns()
    texts = set()
    for i, (transposed, a) in enumerate(_bad_blocks()):
        f32, bf = (L.dia_codec_convt, L.dia_codec_convt_bf16) if transposed else (L.dia_codec_conv, L.dia_codec_conv_bf16)
        ref = ctypes.byref(a) if a is not None else None
        assert f32(ref, None) == -1, i
        want = hb.lib().dia_last_error().decode()
        assert bf(ref, 2, None) == -1, i
        got = hb.lib().dia_last_error().decode()
        renamed = want.replace("dia_codec_convt", "dia_codec_convt_bf16").replace("dia_codec_conv:", "dia_codec_conv_bf16:")
        assert got == renamed and want.startswith("dia_codec_convt: " if transposed else "dia_codec_conv: "), (i, want, got)
        texts.add(want)
    assert len(texts) >= 40, sorted(texts)                       # the rows reach different refusals, not one many times


def test_bf16_entries_argument_validation_without_gpu():
    L = K._fns()
    conv, convt = L.dia_codec_conv_bf16, L.dia_codec_convt_bf16
    assert "dia_codec_conv_bf16" in hb.EXPORTS and "dia_codec_convt_bf16" in hb.EXPORTS
    assert _refused(conv, None, "null") and _refused(convt, None, "null")
    for planes in (0, 3, -1):
        assert _refused(conv, _conv_args(), "planes", planes) and _refused(convt, _conv_args(stride=2, k=4, ldy=16), "planes", planes)
    for name in ("x", "w", "bias", "y"):
        assert _refused(conv, _conv_args(**{name: None}), "null"), name
        assert _refused(convt, _conv_args(**{name: None, "stride": 2, "k": 4, "ldy": 16}), "null", 1), name
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
