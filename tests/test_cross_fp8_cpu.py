"""FP8 cross K/V, the parts that need no GPU (DESIGN.md "FP8 cross K/V"): the host quantiser dia_hip/quant.py quantize_kv_fp8 /
dequantize_kv_fp8 — the reference dia_kv_quantize_fp8 is pinned to — the argument errors of dia_kv_quantize_fp8 and
dia_attn_cross_fp8 (dummy pointers, never dereferenced), the ctypes mirrors against the header, and the structs that must not
have moved.

Idempotence and the format rule: the scale is the smallest 2^e with amax / 2^e <= 448, so amax / scale lies in (224, 448].  Where
it lies in (224, 232] the key's largest element rounds DOWN to the e4m3 value 224 (232 is the tie of 224 and 240 and goes to the
even code, 224), the dequantised key then has amax == 224 * scale exactly, and the same rule gives it scale / 2 with every element
doubled: the same VALUES, other bytes.  No power-of-two rule can have both properties for such a key, so bytes and scales are
asserted identical for every other key, and for these the halved scale, the doubled elements and identical values."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import torch

from dia_hip import binding as hb
from dia_hip import layout as lay
from dia_hip.quant import dequantize_kv_fp8, quantize_kv_fp8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def keys(seed=0, n=4096):
    """bf16 keys [n, 128] over many magnitudes: randn times 2^(-20..20), a few tiny and large ones"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, 128, generator=g) * torch.exp2(torch.randint(-20, 21, (n, 1), generator=g).float())
    x[0] *= 2.0 ** -100
    x[1] *= 2.0 ** 90
    return x.bfloat16().float()


def test_scale_is_a_power_of_two_and_fills_the_range():
    x = keys()
    q, s = quantize_kv_fp8(x)
    assert q.dtype == torch.uint8 and q.shape == x.shape and s.dtype == torch.float32 and s.shape == x.shape[:-1]
    m, _ = torch.frexp(s)
    assert (m == 0.5).all() and (s > 0).all()                         # 2^e exactly
    r = x.abs().amax(-1) / s
    assert (r > 224).all() and (r <= 448).all(), (float(r.min()), float(r.max()))
    assert not ((q & 0x7F) == 0x7F).any()                            # no NaN pattern
    # the boundaries of the rule: 448 * 2^k stays at scale 2^k, the next bf16 above it moves to 2^(k+1)
    e = torch.zeros(3, 128)
    e[0, 5], e[1, 5], e[2, 5] = 448.0, 450.0, -224.0
    assert quantize_kv_fp8(e)[1].tolist() == [1.0, 2.0, 0.5]
    assert quantize_kv_fp8(e)[0][:, 5].tolist() == [0x7E, 0x76, 0xFE]


def test_round_trip_is_bf16_and_within_half_a_step():
    x = keys(1)
    q, s = quantize_kv_fp8(x)
    d = dequantize_kv_fp8(q, s)
    assert d.dtype == torch.float32 and torch.equal(d.bfloat16().float(), d)
    # e4m3 keeps 3 mantissa bits: half a step is 2^-4 relative for normal elements, 2^-10 * scale in the subnormal range
    assert ((d - x).abs() <= torch.maximum(x.abs() * 2.0 ** -4, s[:, None] * 2.0 ** -10)).all()


def test_idempotence():
    x = keys(2)
    q, s = quantize_kv_fp8(x)
    d = dequantize_kv_fp8(q, s)
    q2, s2 = quantize_kv_fp8(d)
    assert torch.equal(dequantize_kv_fp8(q2, s2), d)                  # the values: always
    top = (q & 0x7F).amax(-1)                                         # e4m3 magnitudes order like their codes
    band = top == 0x76                                                # largest element == 224 (module docstring)
    assert ((top > 0x76) | band).all() and 0 < int(band.sum()) < len(x) // 4
    assert torch.equal(q2[~band], q[~band]) and torch.equal(s2[~band], s[~band])
    assert torch.equal(s2[band], s[band] / 2)
    assert torch.equal(dequantize_kv_fp8(q2[band], torch.ones_like(s2[band])), 2 * dequantize_kv_fp8(q[band], torch.ones_like(s[band])))
    q3, s3 = quantize_kv_fp8(dequantize_kv_fp8(q2, s2))               # and from there on bytes and scales stay
    assert torch.equal(q3, q2) and torch.equal(s3, s2)


def test_zero_key():
    x = keys(3, 8)
    x[2] = 0.0
    q, s = quantize_kv_fp8(x)
    assert (q[2] == 0).all() and float(s[2]) == 1.0
    assert torch.equal(dequantize_kv_fp8(q, s)[2], torch.zeros(128))


def test_blocked_v_round_trip():
    """the V copy is the per-key quantisation in the blocked layout of the bf16 V cache: bytes blocked, scales per key"""
    v = keys(4, 2 * 3 * 64).reshape(2, 3, 64, 128)                    # [B, heads, S, 128]
    q, s = quantize_kv_fp8(v)
    qb = lay.v_to_blocked(q)
    assert qb.shape == (2, 3, 2, 128, 32) and qb.dtype == torch.uint8
    back = dequantize_kv_fp8(lay.v_from_blocked(qb), s)
    assert torch.equal(back, dequantize_kv_fp8(q, s))
    assert torch.equal(lay.v_to_blocked(back.bfloat16()).float(), lay.v_to_blocked(back))   # a bf16 blocked cache holds it exactly


def test_refusals_without_a_device():
    L = hb.lib()
    buf = ctypes.create_string_buffer(256)           # never dereferenced: every case is refused before a launch
    addr = (ctypes.addressof(buf) + 15) & ~15

    def ptrs(**kw):
        p = hb.KvFp8Ptrs(k8=addr, v8=addr, ks=addr, vs=addr)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def attn(**kw):
        a = hb.AttnArgs()
        a.mode, a.kv_dtype, a.n_kv_heads, a.group, a.n_rows, a.kv_cap = hb.ATTN_CROSS, hb.KV_BF16, 2, 1, 3, 320
        a.q = a.kc = a.vc = a.cur = a.len = a.cos_t = a.sin_t = a.P = a.scratch = a.tickets = addr
        a.ldq, a.p_ktiles, a.v_blocked = 256, 8, 1
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    assert L.dia_attn_cross_fp8(None, ctypes.byref(ptrs()), None) == -1 and b"null" in L.dia_last_error()
    assert L.dia_attn_cross_fp8(ctypes.byref(attn()), None, None) == -1 and b"null" in L.dia_last_error()
    for kw, word in ((dict(mode=hb.ATTN_SELF), b"mode"), (dict(mode=hb.ATTN_ENC), b"mode"), (dict(group=4), b"group"),
                     (dict(kv_dtype=hb.KV_F32), b"kv_dtype"), (dict(kv_dtype=hb.KV_BF16X2), b"kv_dtype"), (dict(v_blocked=0), b"v_blocked"),
                     (dict(kv_cap=330), b"multiple of 32"), (dict(kv_cap=0), b"multiple of 32"), (dict(q=None), b"null"), (dict(len=None), b"len"),
                     (dict(scratch=None), b"scratch"), (dict(p_ktiles=7), b"narrow"), (dict(n_rows=0), b"empty")):
        assert L.dia_attn_cross_fp8(ctypes.byref(attn(**kw)), ctypes.byref(ptrs()), None) == -1, kw
        assert word in L.dia_last_error(), (kw, L.dia_last_error())
    for kw in (dict(k8=None), dict(v8=None), dict(ks=None), dict(vs=None)):
        assert L.dia_attn_cross_fp8(ctypes.byref(attn()), ctypes.byref(ptrs(**kw)), None) == -1 and b"null" in L.dia_last_error()
    assert L.dia_attn_cross_fp8(ctypes.byref(attn()), ctypes.byref(ptrs(k8=addr + 4)), None) == -1 and b"aligned" in L.dia_last_error()

    def quant(rows=(0, 2), lens=(33, 300), **kw):
        a = hb.KvFp8Args()
        a.kc = a.vc = addr
        a.out = ptrs()
        a.B, a.heads, a.S, a.n = 3, 2, 320, len(rows)
        a.row, a.len = (ctypes.c_int32 * max(len(rows), 1))(*rows), (ctypes.c_int32 * max(len(lens), 1))(*lens)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    assert L.dia_kv_quantize_fp8(None, None) == -1 and b"null" in L.dia_last_error()
    for a, word in ((quant(rows=(), lens=()), b"empty row list"), (quant(n=65), b"empty row list"), (quant(kc=None), b"null"), (quant(vc=None), b"null"),
                    (quant(out=ptrs(vs=None)), b"null"), (quant(S=330), b"multiple of 32"), (quant(B=0), b"positive"),
                    (quant(rows=(0, 3)), b"row outside"), (quant(rows=(1, 1)), b"twice"), (quant(lens=(33, 321)), b"length"),
                    (quant(lens=(-1, 3)), b"length"), (quant(row=None), b"empty row list"), (quant(kc=addr + 8), b"aligned"),
                    (quant(n_layer=2, kv_layer_stride=8, f8_layer_stride=3 * 2 * 320 * 128), b"layer strides"),
                    (quant(n_layer=2, kv_layer_stride=3 * 2 * 320 * 128, f8_layer_stride=3 * 2 * 320 * 128 + 128), b"layer strides")):
        assert L.dia_kv_quantize_fp8(ctypes.byref(a), None) == -1
        assert word in L.dia_last_error(), L.dia_last_error()
    assert L.dia_kv_quantize_fp8(ctypes.byref(quant(lens=(0, 0))), None) == 0         # empty texts: no granule, no launch
    assert L.dia_engine_set_cross_fp8(None, ctypes.byref(ptrs())) == -1 and L.dia_engine_set_cross_fp8(None, None) == -1


def c_layout(struct, names):
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "dia_hip.h"\nint main(void){ printf("%zu", sizeof(' + struct + "));\n"
    prog += "".join(f'printf(" %zu", offsetof({struct}, {n}));\n' for n in names) + "return 0; }\n"
    with tempfile.TemporaryDirectory() as td:
        c, exe = os.path.join(td, "s.c"), os.path.join(td, "s")
        open(c, "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        return [int(v) for v in subprocess.check_output([exe]).split()]


def test_new_structs_match_the_header_and_the_old_ones_did_not_move():
    for struct, cls in (("dia_kv_fp8_ptrs", hb.KvFp8Ptrs), ("dia_kv_fp8_args", hb.KvFp8Args)):
        names = [f[0] for f in cls._fields_]
        assert c_layout(struct, names) == [ctypes.sizeof(cls)] + [getattr(cls, n).offset for n in names], struct
    assert [f[0] for f in hb.KvFp8Ptrs._fields_] == ["k8", "v8", "ks", "vs"]
    # the ABI of everything older: version, sizes, and the tails of the two structs an FP8 mode could have been tempted to grow
    assert hb.ABI_VERSION == 8 and hb.lib().dia_abi_version() == 8
    assert ctypes.sizeof(hb.AttnArgs) == 168 and ctypes.sizeof(hb.EngineDesc) == 584
    assert c_layout("dia_attn_args", ["kv_plane_stride"]) == [168, 160]
    assert c_layout("dia_engine_desc", ["w_logits_f8"]) == [584, 576]
    for name in ("dia_kv_quantize_fp8", "dia_attn_cross_fp8", "dia_engine_set_cross_fp8"):
        assert name in hb.EXPORTS


def test_session_keyword_is_checked_before_anything_is_allocated():
    import inspect

    from dia_hip.engine import DecodeSession
    from dia_hip.model import Dia
    for fn in (DecodeSession.__init__, DecodeSession.open):
        assert inspect.signature(fn).parameters["cross_kv"].default == "bf16"
    assert Dia.cross_kv == "bf16"
