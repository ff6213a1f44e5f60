"""FP8 cross K/V on the device (DESIGN.md "FP8 cross K/V"): dia_kv_quantize_fp8 against the host quantiser bit for bit,
dia_attn_cross_fp8 against dia_attn over bf16 caches holding the dequantised values bit for bit and against a float64
softmax-attention within the bound of tests/test_gpu_attn_decode.py (the same arithmetic: TOL = 2e-5 for randn q / K / V), stale
NaN patterns behind a text's last granule, and DecodeSession(cross_kv="fp8") against a bf16 session whose cross caches were
overwritten with the dequantised values (logits bit-identical), in slots, and its refusals.

Kernel-level shapes: B = 3 cache rows, 2 heads, capacity 320 keys (10 granules: lengths up to 256 stay in one workgroup, 300 is
split over workgroups and merged through the slabs)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from dia_hip import binding as hb
from dia_hip import config as CF
from dia_hip import layout as lay
from dia_hip.quant import dequantize_kv_fp8, quantize_kv_fp8

B, H, S = 3, 2, 320
TOL = 2e-5                      # tests/test_gpu_attn_decode.py: the one-plane bf16 MFMA kernel against its float64 reference
SENT8, SENTS = 0xA5, -3.0       # what the fp8 buffers hold where nothing may be written
SENTINEL = 5.0


def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def caches():
    """bf16 cross caches of one layer (K rows, V blocked) with randn values, a zero key, a key with negative zeros and keys of
    other magnitudes, and the host quantiser's answer over every key: the reference, computed once"""
    g = torch.Generator().manual_seed(7)
    k, v = torch.randn(B, H, S, 128, generator=g), torch.randn(B, H, S, 128, generator=g)
    k[0, 0, 3], v[0, 1, 5] = 0.0, 0.0
    k[2, 1, 8] = -0.0
    k[2, :, 40:48] *= 2.0 ** -9
    v[2, :, 100:110] *= 2.0 ** 7
    k, v = k.bfloat16(), v.bfloat16()
    (qk, sk), (qv, sv) = quantize_kv_fp8(k), quantize_kv_fp8(v)
    d = dev()
    return dict(kc=k.to(d).contiguous(), vc=lay.v_to_blocked(v).to(d).contiguous(), qk=qk, sk=sk, qv=qv, sv=sv)


def fp8_buffers(fill8=0, fills=0.0):
    d = dev()
    return dict(k8=torch.full((B, H, S, 128), fill8, dtype=torch.uint8, device=d), v8=torch.full((B, H, S // 32, 128, 32), fill8, dtype=torch.uint8, device=d),
                ks=torch.full((B, H, S), fills, device=d), vs=torch.full((B, H, S), fills, device=d))


def quantize(c, f, rows, lens):
    a = hb.KvFp8Args()
    a.kc, a.vc = hb.ptr(c["kc"]), hb.ptr(c["vc"])
    a.out.k8, a.out.v8, a.out.ks, a.out.vs = (hb.ptr(f[n]) for n in ("k8", "v8", "ks", "vs"))
    a.B, a.heads, a.S, a.n = B, H, S, len(rows)
    a.row, a.len = (C.c_int32 * len(rows))(*rows), (C.c_int32 * len(lens))(*lens)
    hb.check(hb.lib().dia_kv_quantize_fp8(C.byref(a), None), "dia_kv_quantize_fp8")
    torch.cuda.synchronize()


def expect(state, c, rows, lens):
    """what a call leaves: whole granules of the listed rows — the host quantiser's bytes and scales below the length, zero bytes
    and scale 1 from there to the end of the last granule — everything else as it was"""
    k8, v8, ks, vs = state
    for r, n in zip(rows, lens):
        end = -(-n // 32) * 32
        for dst8, dsts, q, s in ((k8, ks, c["qk"], c["sk"]), (v8, vs, c["qv"], c["sv"])):
            dst8[r, :, :n], dsts[r, :, :n] = q[r, :, :n], s[r, :, :n]
            dst8[r, :, n:end], dsts[r, :, n:end] = 0, 1.0
    return state


def read(f):
    return f["k8"].cpu(), lay.v_from_blocked(f["v8"]).cpu(), f["ks"].cpu(), f["vs"].cpu()


def test_quantiser_equals_the_host_quantiser(caches):
    f = fp8_buffers(SENT8, SENTS)
    state = tuple(t.clone() for t in read(f))
    for rows, lens in (((0, 2), (33, 300)), ((0, 2), (1, 64)), ((2, 1), (0, 320))):
        quantize(caches, f, rows, lens)
        state = expect(state, caches, rows, lens)
        for got, want, name in zip(read(f), state, ("k8", "v8", "ks", "vs")):
            assert torch.equal(got, want), (name, rows, lens)
    k8, v8, ks, vs = read(f)
    # (spelt out once) keys past the length inside the last granule; the untouched row of the first two calls; past the last granule
    assert (k8[0, :, 1:32] == 0).all() and (v8[0, :, 1:32] == 0).all() and (ks[0, :, 1:32] == 1).all() and (vs[0, :, 1:32] == 1).all()
    assert (k8[0, :, 64:] == SENT8).all() and (v8[0, :, 64:] == SENT8).all() and (ks[0, :, 64:] == SENTS).all() and (vs[0, :, 64:] == SENTS).all()
    # the zero keys of the inputs (and the key of negative zeros: sign bytes, scale 1)
    assert (caches["qk"][0, 0, 3] == 0).all() and float(caches["sk"][0, 0, 3]) == 1.0 and (caches["qv"][0, 1, 5] == 0).all() and float(caches["sv"][0, 1, 5]) == 1.0
    assert (k8[1, 0, 3] != SENT8).any() and (caches["qk"][2, 1, 8] == 0x80).all() and float(caches["sk"][2, 1, 8]) == 1.0


def test_quantiser_over_layers(caches):
    """n_layer = 2 over one allocation per buffer: layer 1 = layer 0's caches with K times 4 and V halved"""
    d = dev()
    kc2 = torch.stack([caches["kc"], (caches["kc"].float() * 4).bfloat16()]).contiguous()
    vc2 = torch.stack([caches["vc"], (caches["vc"].float() * 0.5).bfloat16()]).contiguous()
    f = {n: torch.stack([t, t]).contiguous() for n, t in fp8_buffers(SENT8, SENTS).items()}
    a = hb.KvFp8Args()
    a.kc, a.vc = hb.ptr(kc2), hb.ptr(vc2)
    a.out.k8, a.out.v8, a.out.ks, a.out.vs = (hb.ptr(f[n]) for n in ("k8", "v8", "ks", "vs"))
    a.B, a.heads, a.S, a.n, a.n_layer = B, H, S, 2, 2
    a.row, a.len = (C.c_int32 * 2)(2, 0), (C.c_int32 * 2)(70, 31)
    a.kv_layer_stride = a.f8_layer_stride = B * H * S * 128
    hb.check(hb.lib().dia_kv_quantize_fp8(C.byref(a), None), "dia_kv_quantize_fp8")
    torch.cuda.synchronize()
    for l in range(2):
        (qk, sk), (qv, sv) = quantize_kv_fp8(kc2[l].cpu()), quantize_kv_fp8(lay.v_from_blocked(vc2[l]).cpu())
        if l == 0:
            assert torch.equal(qk, caches["qk"]) and torch.equal(sv, caches["sv"])
        want = expect(tuple(t.clone() for t in read(fp8_buffers(SENT8, SENTS))), dict(qk=qk, sk=sk, qv=qv, sv=sv), (2, 0), (70, 31))
        for got, w_, name in zip(read({n: t[l] for n, t in f.items()}), want, ("k8", "v8", "ks", "vs")):
            assert torch.equal(got, w_), (l, name)


# ---- attention ------------------------------------------------------------------------------------------------------------------
class Launch:
    """one cross-attention problem: q rows, positions, lengths, RoPE tables, scratch; run() through dia_attn_cross_fp8 over fp8
    buffers or through dia_attn over bf16 caches, returning the raw output buffer (tiles or planes)"""

    def __init__(self, lens, seed):
        d = dev()
        self.lens, self.curs = list(lens), [3 + 4 * i for i in range(len(lens))]
        g = torch.Generator().manual_seed(seed)
        self.q = torch.randn(2 * len(lens), H * 128, generator=g).to(d)
        self.cos, self.sin = [t.to(d) for t in lay.rope_tables(64, 128, 1, 10000)]
        self.cur_t = torch.tensor(self.curs, dtype=torch.int32, device=d)
        self.len_t = torch.tensor(self.lens, dtype=torch.int32, device=d)
        self.scr = torch.zeros(hb.lib().dia_attn_scratch_floats(len(lens), H, S), device=d)
        self.tk = torch.zeros(len(lens) * H, dtype=torch.int32, device=d)

    def run(self, kc, vc, act_f32, f8=None):
        d, n = dev(), len(self.lens)
        mt, kt = (2 * n + 15) // 16, H * 4
        if act_f32:
            P = torch.full((mt, kt, 64, 8), SENTINEL, dtype=torch.float32, device=d)
        else:
            P = lay.pack_planes(torch.full((mt * 16, H * 128), SENTINEL, device=d))
        a = hb.AttnArgs()
        a.mode, a.kv_dtype, a.n_kv_heads, a.group, a.n_rows, a.kv_cap = hb.ATTN_CROSS, hb.KV_BF16, H, 1, n, S
        a.q, a.ldq, a.q_off = hb.ptr(self.q), H * 128, 0
        a.kc, a.vc, a.cur, a.len = hb.ptr(kc), hb.ptr(vc), hb.ptr(self.cur_t), hb.ptr(self.len_t)
        a.cos_t, a.sin_t, a.rope_rows = hb.ptr(self.cos), hb.ptr(self.sin), self.cos.shape[0]
        a.P, a.p_plane_stride, a.p_ktiles, a.act_f32 = hb.ptr(P), mt * kt * 512, kt, act_f32
        a.scratch, a.tickets, a.v_blocked = hb.ptr(self.scr), hb.ptr(self.tk), 1
        if f8 is None:
            hb.check(hb.lib().dia_attn(C.byref(a), None), "dia_attn")
        else:
            p = hb.KvFp8Ptrs(k8=hb.ptr(f8["k8"]), v8=hb.ptr(f8["v8"]), ks=hb.ptr(f8["ks"]), vs=hb.ptr(f8["vs"]))
            hb.check(hb.lib().dia_attn_cross_fp8(C.byref(a), C.byref(p), None), "dia_attn_cross_fp8")
        torch.cuda.synchronize()
        assert (self.tk == 0).all(), "tickets not back at 0 after the launch"
        return P

    def rows64(self, P, act_f32):
        n = len(self.lens)
        mt = (2 * n + 15) // 16
        out = lay.unpack_f32_tiles(P, mt * 16, H * 128) if act_f32 else lay.unpack_planes(P, mt * 16, H * 128)
        return out.double().reshape(mt * 16, H, 128)


def rope64(x, cos, sin, pos):
    c, s = cos[pos].double()[:, None, :], sin[pos].double()[:, None, :]
    return torch.cat([x[..., :64] * c - x[..., 64:] * s, x[..., :64] * s + x[..., 64:] * c], dim=-1)


LENS = ((1, 31, 32), (33, 200, 300))        # one key; a granule short of one key, full, one over; two granules per wave; split with slab merge


@pytest.fixture(scope="module")
def quantised(caches):
    """the fp8 copy of all three rows at full length (device quantiser) and the bf16 caches that hold its dequantised values"""
    f = fp8_buffers()
    quantize(caches, f, (0, 1, 2), (S, S, S))
    k8, v8, ks, vs = read(f)                                            # (host copies, V unblocked)
    kd, vd = dequantize_kv_fp8(k8, ks), dequantize_kv_fp8(v8, vs)
    assert torch.equal(kd.bfloat16().float(), kd) and torch.equal(vd.bfloat16().float(), vd)
    d = dev()
    return f, kd.bfloat16().to(d).contiguous(), lay.v_to_blocked(vd.bfloat16()).to(d).contiguous(), kd.double().to(d), vd.double().to(d)


@pytest.mark.parametrize("act_f32", [1, 0])
@pytest.mark.parametrize("lens", LENS)
def test_attention_equals_the_bf16_kernel_bit_for_bit_and_the_float64_reference(caches, quantised, lens, act_f32):
    f, kdq, vdq, k64, v64 = quantised
    case = Launch(lens, seed=sum(lens))
    P8 = case.run(caches["kc"], caches["vc"], act_f32, f8=f)
    Pb = case.run(kdq, vdq, act_f32)
    out = case.rows64(P8, act_f32)
    diff = (out - case.rows64(Pb, act_f32)).abs()
    print(f"lens {lens} act_f32 {act_f32}: fp8 form vs bf16 kernel over the dequantised caches: max abs difference {float(diff.max()):.3e}, "
          f"{int((diff > 0).sum())} of {diff.numel()} values differ")
    assert torch.equal(P8.view(torch.int32 if act_f32 else torch.int16), Pb.view(torch.int32 if act_f32 else torch.int16)), "fp8 form != bf16 kernel over the dequantised caches"
    qr = rope64(case.q.double().reshape(-1, H, 128), case.cos, case.sin, torch.tensor([c for c in case.curs for _ in (0, 1)], device=dev()))
    worst = 0.0
    for b, n in enumerate(lens):
        p = torch.softmax((qr[2 * b + 1][:, None, :] @ k64[b, :, :n].transpose(-1, -2)) / np.sqrt(128.0), dim=-1)
        ref = (p @ v64[b, :, :n])[:, 0]
        worst = max(worst, float((out[2 * b + 1] - ref).abs().max()))
        assert (out[2 * b] == 0).all()                                 # the uncond row: all keys masked -> 0
    print(f"lens {lens} act_f32 {act_f32}: max abs error vs float64 {worst:.3e} (bound {TOL})")
    assert worst <= TOL, worst
    assert (out[2 * len(lens):] == SENTINEL).all()


def test_stale_nan_patterns_stay_invisible(caches):
    """a row whose fp8 buffers hold 0x7F (e4m3 NaN) everywhere, as if left by a longer text: a 40-key text quantised into it gives
    the output of a zero-initialised buffer.  Bytes behind the last granule are never addressed (the clamps of the bf16 kernel)"""
    outs = []
    for fill8, fills in ((0x7F, 32.0), (0, 0.0)):
        f = fp8_buffers(fill8, fills)
        quantize(caches, f, (1,), (40,))
        case = Launch((0, 40), seed=3)
        outs.append(case.rows64(case.run(caches["kc"], caches["vc"], 1, f8=f), 1))
    assert torch.isfinite(outs[0][:4]).all() and torch.equal(outs[0], outs[1])
    assert (outs[0][1] == 0).all() and outs[0][3].abs().max() > 0     # an empty text -> 0; the 40-key one attends


# ---- model ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mid():
    from dia_hip.engine import DeviceWeights
    from dia_hip.weights import synthetic_state_dict
    cfg = CF.mid_config()
    return cfg, DeviceWeights(cfg, synthetic_state_dict(cfg, seed=1234, std=0.02), dev())


def ids_of(n, seed):
    return np.random.RandomState(seed).randint(32, 127, size=(n,)).astype(np.int32)


@pytest.mark.parametrize("graph", [True, False])
def test_model_equals_bf16_session_over_the_dequantised_caches(mid, graph):
    from dia_hip.engine import DecodeSession
    cfg, w = mid
    V, Cn = cfg.model.tgt_vocab_size, cfg.data.channels
    ids = [ids_of(5, 1), ids_of(40, 2)]
    rng = np.random.default_rng(5)
    teacher = [rng.integers(0, V - 4, size=(14, Cn)).astype(np.int32) for _ in ids]
    kw = dict(kv_dtype="bf16", max_tokens=16, seeds=[11, 12], ignore_eos=True, teacher_tokens=teacher)
    f = DecodeSession(w, ids, cross_kv="fp8", **kw)
    b = DecodeSession(w, ids, **kw)
    try:
        f.prefill()
        b.prefill()
        f.sync()
        assert torch.equal(f.k_cross_all, b.k_cross_all) and torch.equal(f.v_cross_all, b.v_cross_all)      # the bf16 caches stay
        # the device copy == the host quantiser over the bf16 caches, whole granules
        for r, n in enumerate(f.lens):
            end = -(-n // 32) * 32
            qk, sk = quantize_kv_fp8(f.k_cross_all[:, r, :, :n].cpu())
            vb = f.v_cross_all[:, r].reshape(f.f8_cross.v8[:, r].shape)           # (the bf16 V cache is allocated [.., S, 128] and holds the blocked order)
            qv, sv = quantize_kv_fp8(lay.v_from_blocked(vb).cpu()[:, :, :n])
            assert torch.equal(f.f8_cross.k8[:, r, :, :n].cpu(), qk) and torch.equal(f.f8_cross.ks[:, r, :, :n].cpu(), sk)
            assert torch.equal(lay.v_from_blocked(f.f8_cross.v8[:, r]).cpu()[:, :, :n], qv) and torch.equal(f.f8_cross.vs[:, r, :, :n].cpu(), sv)
            assert (f.f8_cross.k8[:, r, :, n:] == 0).all() and (f.f8_cross.ks[:, r, :, n:end] == 1).all() and (f.f8_cross.ks[:, r, :, end:] == 0).all()
        kd = dequantize_kv_fp8(f.f8_cross.k8.cpu(), f.f8_cross.ks.cpu())
        vd = dequantize_kv_fp8(lay.v_from_blocked(f.f8_cross.v8).cpu(), f.f8_cross.vs.cpu())
        with torch.cuda.stream(b.stream):
            b.k_cross_all.copy_(kd.bfloat16().to(dev()))
            b.v_cross_all.copy_(lay.v_to_blocked(vd.bfloat16()).reshape(b.v_cross_all.shape).to(dev()))
        b.sync()
        assert f.launches_per_step() == b.launches_per_step()
        for step in range(12):
            f.decode(1, use_graph=graph)
            b.decode(1, use_graph=graph)
            lf, lb = f.logits_host(), b.logits_host()
            assert np.isfinite(lf).all() and np.abs(lf).max() > 0
            assert np.array_equal(lf, lb), (step, float(np.abs(lf - lb).max()))
        for rf, rb in zip(f.results(), b.results()):
            assert np.array_equal(rf.preds, rb.preds) and np.array_equal(rf.tokens, rb.tokens)
        names_f = (f.time_step(), list(f.last_kernel_names))[1]
        names_b = (b.time_step(), list(b.last_kernel_names))[1]
        nl = cfg.model.decoder.n_layer
        assert names_f.count("k_attn_mfma_f8") == nl and names_b.count("k_attn_mfma_f8") == 0
        assert len(names_f) == len(names_b)
        for nf, nb in zip(names_f, names_b):      # launch for launch the same step, but for the cross-attention kernel
            assert nb.startswith("k_attn_mfma<1, 1>") if nf == "k_attn_mfma_f8" else nf == nb, (nf, nb)
    finally:
        f.close()
        b.close()


def test_slots_equal_solo_runs(mid):
    """two slots: a 60-byte request and a 25-byte one, then a 9-byte request into the slot the 60-byte text left (its fp8 granules
    1 and the tail of granule 0 hold the longer text's bytes until the quantiser rewrites granule 0).  Each result == the same
    request alone in a fresh session of the same shape, bitwise"""
    from dia_hip.engine import DecodeSession, Request
    cfg, w = mid
    reqs = [Request(ids_of(60, 3), seed=42, max_tokens=20), Request(ids_of(25, 4), seed=7, max_tokens=14, temperature=0.9, top_k=50),
            Request(ids_of(9, 5), seed=9, max_tokens=16)]

    def session():
        return DecodeSession.open(w, 2, s_cap=64, kv_dtype="bf16", max_tokens=20, cross_kv="fp8")

    s = session()
    try:
        out = s.serve(reqs[:2], poll=4) + s.serve(reqs[2:], poll=4)
        assert (s.f8_cross.k8[:, 0, :, 9:32] == 0).all() and (s.f8_cross.ks[:, 0, :, 9:32] == 1).all()
        assert (s.f8_cross.k8[:, 0, :, 32:60] != 0).any()            # the longer text's second granule is still there, unread
    finally:
        s.close()
    for r, got in zip(reqs, out):
        solo = session()
        try:
            want = solo.serve([r], poll=4)[0]
        finally:
            solo.close()
        assert np.array_equal(got.tokens, want.tokens) and np.array_equal(got.preds, want.preds) and got.last_step == want.last_step
        assert np.array_equal(got.codes, want.codes) and got.codes.size > 0


def test_refusals_and_the_default_session(mid):
    from dia_hip.engine import DecodeSession
    cfg, w = mid
    ids = [ids_of(20, 1)]
    for kw, word in ((dict(kv_dtype="float32"), "kv_dtype"), (dict(kv_dtype="bf16x2"), "kv_dtype"), (dict(kv_dtype="bf16", attention="valu"), "blocked"),
                     (dict(kv_dtype="bf16", cross_kv="fp4"), "cross_kv")):
        with pytest.raises(ValueError, match=word):
            DecodeSession(w, ids, max_tokens=8, **{"cross_kv": "fp8", **kw})
    with pytest.raises(ValueError, match="kv_dtype"):
        DecodeSession.open(w, 2, kv_dtype="f32", cross_kv="fp8")
    # the engine hook on an fp32-K/V engine and on a bf16 one whose V is row-major
    p = (hb.KvFp8Ptrs * cfg.model.decoder.n_layer)()
    buf = torch.zeros(64, device=dev())
    for q in p:
        q.k8 = q.v8 = q.ks = q.vs = hb.ptr(buf)
    for kw in (dict(kv_dtype="f32"), dict(kv_dtype="bf16", attention="valu")):
        s = DecodeSession(w, ids, max_tokens=8, **kw)
        try:
            assert hb.lib().dia_engine_set_cross_fp8(s._engine, p) == -1 and b"bf16 K/V" in hb.lib().dia_last_error()
        finally:
            s.close()
    # the default keyword: no fp8 buffer, the kernels of a session that was never told about the keyword
    s = DecodeSession(w, ids, kv_dtype="bf16", max_tokens=8, seeds=[1])
    try:
        assert s.cross_kv == "bf16" and s.f8_cross is None
        s.prefill()
        s.time_step()
        names = list(s.last_kernel_names)
        assert "k_attn_mfma_f8" not in names and sum(n.startswith("k_attn_mfma<1, 1>") for n in names) == cfg.model.decoder.n_layer
        s.decode(1)
        assert hb.lib().dia_engine_set_cross_fp8(s._engine, None) == -3          # DIA_E_STATE: a step has been issued
    finally:
        s.close()
