"""FP8 self K/V, the parts that need no GPU (DESIGN.md "FP8 self K/V"): the two entries in the header and the binding with the ABI
version where it was, the argument errors of dia_attn_self_fp8 (dummy pointers, never dereferenced), the self_kv checks of
DecodeSession (they run before anything touches a device), and tests/self_fp8_ref.py — the float64 statement of one step the GPU
tests compare against — against plain float64 attention over dequantize_kv_fp8 of the updated cache."""
import ctypes
import inspect
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import self_fp8_ref as R
from dia_hip import binding as hb
from dia_hip import config as CF
from dia_hip import layout as lay
from dia_hip.quant import dequantize_kv_fp8, quantize_kv_fp8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_entries_and_the_binding_resolves_them():
    h = open(os.path.join(ROOT, "include", "dia_hip.h")).read()
    assert re.search(r"int dia_attn_self_fp8\(const dia_attn_args\* a, const dia_kv_fp8_ptrs\* p, void\* stream\);", h)
    assert re.search(r"int dia_engine_set_self_fp8\(dia_engine\* e, const dia_kv_fp8_ptrs\* layers", h)
    assert re.search(r"#define DIA_ABI_VERSION 8\b", h)
    L = hb.lib()
    for name in ("dia_attn_self_fp8", "dia_engine_set_self_fp8"):
        assert name in hb.EXPORTS and getattr(L, name) is not None
    assert hb.ABI_VERSION == 8 and L.dia_abi_version() == 8
    # no struct grew: the sizes tests/test_cross_fp8_cpu.py pins
    assert ctypes.sizeof(hb.AttnArgs) == 168 and ctypes.sizeof(hb.EngineDesc) == 584 and ctypes.sizeof(hb.KvFp8Ptrs) == 32


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
        a.mode, a.kv_dtype, a.n_kv_heads, a.group, a.n_rows, a.kv_cap = hb.ATTN_SELF, hb.KV_BF16, 2, 4, 4, 320
        a.q = a.cur = a.cos_t = a.sin_t = a.P = a.scratch = a.tickets = addr          # kc == vc == NULL: accepted
        a.ldq, a.k_off, a.v_off, a.p_ktiles, a.v_blocked = 1536, 1024, 1280, 32, 1
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    assert L.dia_attn_self_fp8(None, ctypes.byref(ptrs()), None) == -1 and b"null" in L.dia_last_error()
    assert L.dia_attn_self_fp8(ctypes.byref(attn()), None, None) == -1 and b"null" in L.dia_last_error()
    for kw, word in ((dict(mode=hb.ATTN_CROSS), b"mode must be DIA_ATTN_SELF"), (dict(mode=hb.ATTN_ENC), b"mode must be DIA_ATTN_SELF"),
                     (dict(kv_dtype=hb.KV_F32), b"kv_dtype"), (dict(kv_dtype=hb.KV_BF16X2), b"kv_dtype"), (dict(v_blocked=0), b"v_blocked"),
                     (dict(kv_cap=330), b"multiple of 32"), (dict(kv_cap=0), b"multiple of 32"), (dict(cur=None), b"cur"), (dict(q=None), b"null"),
                     (dict(scratch=None), b"scratch"), (dict(tickets=None), b"tickets"), (dict(group=3), b"group"), (dict(group=8), b"group"),
                     (dict(p_ktiles=31), b"narrow"), (dict(n_rows=0), b"empty"), (dict(rope_rows=320), b"RoPE")):
        assert L.dia_attn_self_fp8(ctypes.byref(attn(**kw)), ctypes.byref(ptrs()), None) == -1, kw
        assert L.dia_last_error().startswith(b"dia_attn_self_fp8:") and word in L.dia_last_error(), (kw, L.dia_last_error())
    for kw in (dict(k8=None), dict(v8=None), dict(ks=None), dict(vs=None)):
        assert L.dia_attn_self_fp8(ctypes.byref(attn()), ctypes.byref(ptrs(**kw)), None) == -1 and b"null" in L.dia_last_error()
    for kw in (dict(k8=addr + 4), dict(v8=addr + 2), dict(ks=addr + 2), dict(vs=addr + 1)):
        assert L.dia_attn_self_fp8(ctypes.byref(attn()), ctypes.byref(ptrs(**kw)), None) == -1 and b"aligned" in L.dia_last_error(), kw
    assert L.dia_engine_set_self_fp8(None, ctypes.byref(ptrs())) == -1 and L.dia_engine_set_self_fp8(None, None) == -1
    assert b"dia_engine_set_self_fp8" in L.dia_last_error()


def test_session_keyword_defaults_and_refusals_by_name():
    from dia_hip.engine import DecodeSession
    from dia_hip.model import Dia
    for fn in (DecodeSession.__init__, DecodeSession.open):
        assert inspect.signature(fn).parameters["self_kv"].default == "bf16"
    assert Dia.self_kv == "bf16"
    src = open(os.path.join(ROOT, "cli.py")).read()
    assert '"--self-kv"' in src and "Dia.self_kv = args.self_kv" in src
    # the checks run before the session allocates or touches its device: a stand-in for DeviceWeights is enough to reach them
    cfg = CF.mid_config()
    w = SimpleNamespace(cfg=cfg, device=torch.device("cpu"))
    ids = [np.arange(40, 50, dtype=np.int32)]
    for kw, word in ((dict(kv_dtype="f32"), "kv_dtype 'f32'"), (dict(kv_dtype="bf16x2"), "kv_dtype 'bf16x2'"),
                     (dict(kv_dtype="bf16", attention="valu"), "attention='valu'"), (dict(kv_dtype="bf16", self_kv="fp4"), "self_kv must be")):
        with pytest.raises(ValueError, match=re.escape(word)) as ei:
            DecodeSession(w, ids, max_tokens=8, **{"self_kv": "fp8", **kw})
        assert "self_kv" in str(ei.value)
    with pytest.raises(ValueError, match="self_kv='fp8'"):
        DecodeSession.open(w, 2, kv_dtype="f32", self_kv="fp8")
    odd = cfg.model_copy(update=dict(data=cfg.data.model_copy(update=dict(audio_length=cfg.data.audio_length + 8))))      # not a multiple of 32
    with pytest.raises(ValueError, match=re.escape("audio_length % 32")):
        DecodeSession(SimpleNamespace(cfg=odd, device=torch.device("cpu")), ids, kv_dtype="bf16", max_tokens=8, self_kv="fp8")


def test_reference_step_equals_plain_attention_over_the_dequantised_cache():
    """self_fp8_ref.step against softmax attention written out here over dequantize_kv_fp8 of the cache it returns, for G = 4 query
    heads, at a first key, inside a granule and on a granule boundary; the appended slot holds quantize_kv_fp8 of the roped key, and
    nothing else moved"""
    g = torch.Generator().manual_seed(3)
    T = 96
    cos, sin = lay.rope_tables(T + 1, 128, 1, 10000)
    kq, ksc = quantize_kv_fp8(torch.randn(T, 128, generator=g) * 3.0)
    vq, vsc = quantize_kv_fp8(torch.randn(T, 128, generator=g) * 0.25)
    k8, ks, v8, vs = kq.numpy(), ksc.numpy(), vq.numpy(), vsc.numpy()
    for cur in (1, 17, 32, 33, 96):
        q = torch.randn(4, 128, generator=g).double().numpy()
        kn, vn = torch.randn(128, generator=g).double().numpy() * 5.0, torch.randn(128, generator=g).double().numpy()
        out, k8n, ksn, v8n, vsn = R.step(q, kn, vn, cos[cur].numpy(), sin[cur].numpy(), k8, ks, v8, vs, cur)
        c, s = cos[cur].double().numpy(), sin[cur].double().numpy()
        kr = np.concatenate([kn[:64] * c - kn[64:] * s, kn[:64] * s + kn[64:] * c])
        qr = np.concatenate([q[:, :64] * c - q[:, 64:] * s, q[:, :64] * s + q[:, 64:] * c], axis=-1)
        wq, ws = quantize_kv_fp8(torch.from_numpy(kr))
        assert np.array_equal(k8n[cur - 1], wq.numpy()) and float(ksn[cur - 1]) == float(ws)
        wq, ws = quantize_kv_fp8(torch.from_numpy(vn))
        assert np.array_equal(v8n[cur - 1], wq.numpy()) and float(vsn[cur - 1]) == float(ws)
        keep = np.arange(T) != cur - 1
        assert np.array_equal(k8n[keep], k8[keep]) and np.array_equal(vsn[keep], vs[keep]) and np.array_equal(v8n[keep], v8[keep]) and np.array_equal(ksn[keep], ks[keep])
        K = dequantize_kv_fp8(torch.from_numpy(k8n), torch.from_numpy(ksn)).double()[:cur]
        V = dequantize_kv_fp8(torch.from_numpy(v8n), torch.from_numpy(vsn)).double()[:cur]
        ref = torch.softmax(torch.from_numpy(qr) @ K.T / np.sqrt(128.0), dim=-1) @ V
        assert out.shape == (4, 128) and np.abs(out - ref.numpy()).max() <= 1e-13
        # the dequantised new key is within half an e4m3 step of the roped key
        kd = K[cur - 1].numpy()
        assert (np.abs(kd - kr) <= np.maximum(np.abs(kr) * 2.0 ** -4, float(ksn[cur - 1]) * 2.0 ** -10) + 1e-7 * np.abs(kr)).all()
