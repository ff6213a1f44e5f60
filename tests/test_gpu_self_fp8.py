"""FP8 self K/V on the device, kernel level through the C ABI (DESIGN.md "FP8 self K/V"): dia_attn_self_fp8 — attention over e4m3
self caches with the quantising append of the step's new key — against dia_attn (SELF, bf16, blocked V) over caches holding the
dequantised values bit for bit, against tests/self_fp8_ref.py in float64, on a re-used slot, with a pruned head, and its refusals.

Shapes: R = 4 cache rows (two utterances, cur indexed per pair), 2 kv heads x 4 query heads, capacity 320 keys.  cur in
{1, 32, 33, 256, 257, 320}: the first key, both sides of a granule boundary, one workgroup holding 256 keys (two granules per wave),
the split over three workgroups with the slab merge, and a full cache.  One more case forces a single workgroup (knob attn_nz = 1)
at 257 / 320 keys, so that a wave takes three granules and the branch-free steady state of the prefetch runs too."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import self_fp8_ref as REF
from dia_hip import binding as hb
from dia_hip import layout as lay
from dia_hip.quant import dequantize_kv_fp8, quantize_kv_fp8

R, KVH, G, T = 4, 2, 4, 320
QH = KVH * G
NQ = (QH + 2 * KVH) * 128
K_OFF, V_OFF = QH * 128, (QH + KVH) * 128
TOL = 2e-5                      # tests/test_gpu_kernels.py test_attn_self: the bf16 MFMA kernel against its float64 reference (randn q / K / V)
SENTINEL = 5.0
CURS = ((1, 32), (33, 256), (257, 320))


def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def prefill():
    """the caches before the step: random bf16 K / V of mixed magnitudes through the host quantiser (bytes, scales; V in key order).
    Computed once, never modified: every launch works on device copies"""
    g = torch.Generator().manual_seed(11)
    k = torch.randn(R, KVH, T, 128, generator=g) * torch.exp2(torch.randint(-3, 4, (R, KVH, T, 1), generator=g).float())
    v = torch.randn(R, KVH, T, 128, generator=g) * torch.exp2(torch.randint(-2, 3, (R, KVH, T, 1), generator=g).float())
    k[1, 0, 7], v[2, 1, 40] = 0.0, 0.0
    (k8, ks), (v8, vs) = quantize_kv_fp8(k.bfloat16()), quantize_kv_fp8(v.bfloat16())
    return dict(k8=k8, ks=ks, v8=v8, vs=vs)


def real_tables():
    return lay.rope_tables(T + 1, 128, 1, 10000)


def exact_tables(seed):
    """every entry (cos, sin) is (1, 0) or (0, 1): a rotation by 0 or a quarter turn, exact under any contraction"""
    bit = torch.randint(0, 2, (T + 1, 64), generator=torch.Generator().manual_seed(seed)).float()
    return bit.contiguous(), (1.0 - bit).contiguous()


def grid_rows(g, n, peak_at, e_lo, e_hi):
    """[n, 128] fp32, each row e4m3 grid values times one power of two 2^e, e_lo <= e <= e_hi, its largest magnitude 320 .. 448 times
    that power (amax / scale in (232, 448]): quantize_kv_fp8 returns exactly these values"""
    b = torch.randint(0, 256, (n, 128), generator=g, dtype=torch.int32).to(torch.uint8)
    b[(b & 0x7F) == 0x7F] = 0x35
    x = b.view(torch.float8_e4m3fn).float()
    x[:, peak_at] = 320.0
    x = x * torch.exp2(torch.randint(e_lo, e_hi + 1, (n, 1), generator=g).float())
    q, s = quantize_kv_fp8(x)
    assert torch.equal(dequantize_kv_fp8(q, s), x) and torch.equal(x.bfloat16().float(), x)
    r = x.abs().amax(-1) / s
    assert (r > 232).all() and (r <= 448).all()
    return x


class Step:
    """one self-attention launch: qkv rows [R, NQ] (q heads, then the new k and v of the kv heads), cur per utterance, tables"""

    def __init__(self, qkv, curs, tables, head_map=None):
        d = dev()
        self.qkv, self.curs = qkv.to(d).contiguous(), list(curs)
        self.cos, self.sin = [t.to(d).contiguous() for t in tables]
        self.cur_t = torch.tensor(self.curs, dtype=torch.int32, device=d)
        self.scr = torch.zeros(hb.lib().dia_attn_scratch_floats(R, KVH, T), device=d)
        self.tk = torch.zeros(R * KVH, dtype=torch.int32, device=d)
        self.hmap = None if head_map is None else torch.tensor(head_map, dtype=torch.int32, device=d)

    def args(self, P, act_f32):
        mt, kt = 1, QH * 4
        a = hb.AttnArgs()
        a.mode, a.kv_dtype, a.n_kv_heads, a.group, a.n_rows, a.kv_cap = hb.ATTN_SELF, hb.KV_BF16, KVH, G, R, T
        a.q, a.ldq, a.q_off, a.k_off, a.v_off = hb.ptr(self.qkv), NQ, 0, K_OFF, V_OFF
        a.cur, a.cos_t, a.sin_t, a.rope_rows = hb.ptr(self.cur_t), hb.ptr(self.cos), hb.ptr(self.sin), T + 1
        a.P, a.p_plane_stride, a.p_ktiles, a.act_f32 = hb.ptr(P), mt * kt * 512, kt, act_f32
        a.scratch, a.tickets, a.v_blocked = hb.ptr(self.scr), hb.ptr(self.tk), 1
        a.head_map = hb.ptr(self.hmap)
        return a

    def out_buffer(self, act_f32):
        if act_f32:
            return torch.full((1, QH * 4, 64, 8), SENTINEL, dtype=torch.float32, device=dev())
        return lay.pack_planes(torch.full((16, QH * 128), SENTINEL, device=dev()))

    def run_fp8(self, state, act_f32=1):
        """state: host dict k8 / ks / v8 (key order) / vs -> (P, the state read back)"""
        d = dev()
        f = dict(k8=state["k8"].to(d).contiguous(), v8=lay.v_to_blocked(state["v8"]).to(d).contiguous(),
                 ks=state["ks"].to(d).contiguous(), vs=state["vs"].to(d).contiguous())
        P = self.out_buffer(act_f32)
        a = self.args(P, act_f32)                                   # kc == vc == NULL
        p = hb.KvFp8Ptrs(k8=hb.ptr(f["k8"]), v8=hb.ptr(f["v8"]), ks=hb.ptr(f["ks"]), vs=hb.ptr(f["vs"]))
        hb.check(hb.lib().dia_attn_self_fp8(C.byref(a), C.byref(p), None), "dia_attn_self_fp8")
        torch.cuda.synchronize()
        assert (self.tk == 0).all(), "tickets not back at 0 after the launch"
        return P, dict(k8=f["k8"].cpu(), v8=lay.v_from_blocked(f["v8"]).cpu(), ks=f["ks"].cpu(), vs=f["vs"].cpu())

    def run_bf16(self, state, act_f32=1):
        """dia_attn over bf16 caches holding the dequantised state -> (P, K fp32 [R, KVH, T, 128], V likewise, after the launch)"""
        d = dev()
        kd, vd = dequantize_kv_fp8(state["k8"], state["ks"]), dequantize_kv_fp8(state["v8"], state["vs"])
        assert torch.equal(kd.bfloat16().float(), kd) and torch.equal(vd.bfloat16().float(), vd)
        kc, vc = kd.bfloat16().to(d).contiguous(), lay.v_to_blocked(vd.bfloat16()).to(d).contiguous()
        P = self.out_buffer(act_f32)
        a = self.args(P, act_f32)
        a.kc, a.vc = hb.ptr(kc), hb.ptr(vc)
        hb.check(hb.lib().dia_attn(C.byref(a), None), "dia_attn")
        torch.cuda.synchronize()
        assert (self.tk == 0).all()
        return P, kc.float().cpu(), lay.v_from_blocked(vc).float().cpu()

    def rows64(self, P, act_f32=1):
        out = lay.unpack_f32_tiles(P, 16, QH * 128) if act_f32 else lay.unpack_planes(P, 16, QH * 128)
        return out.double().reshape(16, QH, 128).cpu()


def bits(P, act_f32):
    return P.view(torch.int32 if act_f32 else torch.int16)


def assert_only_the_slot_moved(before, after, curs):
    for r in range(R):
        keep = torch.ones(T, dtype=torch.bool)
        keep[curs[r >> 1] - 1] = False
        for n in ("k8", "v8", "ks", "vs"):
            assert torch.equal(after[n][r][:, keep], before[n][r][:, keep]), (n, r)


def exact_step(seed, curs, tables, k_dims=None):
    """qkv of a step whose new k and v quantise to themselves: q random fp32; k, v grid rows (grid_rows).  k_dims: the dims (of the
    first half; their partners d + 64 too) in which k may be nonzero.
    The powers of two keep the new key at the size of the prefilled ones.  The scales fold in exactly (S * ks == q . (k8 * ks),
    bf16(p * vs) == bf16(p) * vs) as long as p * vs is a normal fp32: a key whose score lies 80 or more below the row maximum has
    p < 2^-115, p * vs can leave the normal range and the two kernels round a contribution of 1e-38 differently (a key of magnitude
    2^14 did that here).  Scores of randn q against keys of magnitude <= 32 stay within 60 of each other."""
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(R, NQ, generator=g)
    k = grid_rows(g, R * KVH, peak_at=40, e_lo=-9, e_hi=-5)          # |k| up to 0.9 .. 14: scores of the size of the prefilled keys
    if k_dims is not None:
        m = torch.zeros(128)
        m[k_dims], m[[d + 64 for d in k_dims]] = 1.0, 1.0
        k = k * m
    qkv[:, K_OFF:V_OFF] = k.reshape(R, KVH * 128)
    qkv[:, V_OFF:] = grid_rows(g, R * KVH, peak_at=3, e_lo=-10, e_hi=-4).reshape(R, KVH * 128)
    return Step(qkv, curs, tables)


@pytest.mark.parametrize("act_f32", [1, 0])
@pytest.mark.parametrize("curs,nz", [(c, 0) for c in CURS] + [((257, 320), 1)])
def test_bitwise_against_the_bf16_kernel(prefill, curs, nz, act_f32, tuning):
    """exact rotations, a new key that quantises to itself: outputs, caches and everything outside the slot"""
    if nz:
        tuning("attn_nz", nz)
    case = exact_step(100 + sum(curs), curs, exact_tables(5))
    P8, after = case.run_fp8(prefill, act_f32)
    Pb, kc, vc = case.run_bf16(prefill, act_f32)
    diff = (case.rows64(P8, act_f32) - case.rows64(Pb, act_f32)).abs()
    print(f"cur {curs} nz {nz} act_f32 {act_f32}: fp8 self kernel vs bf16 kernel over the dequantised caches: max abs difference "
          f"{float(diff.max()):.3e}, {int((diff > 0).sum())} of {diff.numel()} values differ")
    assert torch.equal(bits(P8, act_f32), bits(Pb, act_f32)), "fp8 self kernel != bf16 kernel over the dequantised caches"
    out = case.rows64(P8, act_f32)
    assert torch.isfinite(out[:R]).all() and out[:R].abs().max() > 0 and (out[R:] == SENTINEL).all()
    # the fp8 buffers dequantise to exactly the bf16 caches the second launch left, slot included
    assert torch.equal(dequantize_kv_fp8(after["k8"], after["ks"]), kc) and torch.equal(dequantize_kv_fp8(after["v8"], after["vs"]), vc)
    for r in range(R):                                             # (and the slot is the step's key, not what was there)
        s = curs[r >> 1] - 1
        assert torch.equal(dequantize_kv_fp8(after["v8"][r, :, s], after["vs"][r, :, s]), case.qkv[r, V_OFF:].cpu().reshape(KVH, 128))
    assert_only_the_slot_moved(prefill, after, curs)


@pytest.mark.parametrize("curs", CURS)
def test_bitwise_q_rope_with_the_real_tables(prefill, curs):
    """the real RoPE table in the dims 0..31 (and their partners 64..95), exact rotations in the rest; the new k is nonzero only
    where the rotation is exact, so only q sees real angles: pins which product of q's rotation is the rounded one"""
    cos, sin = real_tables()
    ec, es = exact_tables(6)
    cos, sin = cos.clone(), sin.clone()
    cos[:, 32:], sin[:, 32:] = ec[:, 32:], es[:, 32:]
    case = exact_step(200 + sum(curs), curs, (cos, sin), k_dims=list(range(32, 64)))
    P8, after = case.run_fp8(prefill)
    Pb, kc, vc = case.run_bf16(prefill)
    assert torch.equal(bits(P8, 1), bits(Pb, 1)), "q RoPE differs from k_attn_mfma<4, 1>'s"
    assert torch.equal(dequantize_kv_fp8(after["k8"], after["ks"]), kc) and torch.equal(dequantize_kv_fp8(after["v8"], after["vs"]), vc)


def rule_scale64(amax):
    """the format's rule on a float64 amax: the smallest 2^e (e >= -126) with amax / 2^e <= 448, 1 for zero"""
    if amax == 0:
        return 1.0
    m, ex = np.frexp(amax)
    return float(np.ldexp(1.0, max(int(ex) - 9 + (1 if m > 0.875 else 0), -126)))


@pytest.mark.parametrize("curs", CURS)
def test_real_tables_against_float64(prefill, curs):
    g = torch.Generator().manual_seed(300 + sum(curs))
    qkv = torch.randn(R, NQ, generator=g)
    qkv[:, K_OFF:V_OFF] *= 3.0
    cos, sin = real_tables()
    case = Step(qkv, curs, (cos, sin))
    P8, after = case.run_fp8(prefill)
    assert_only_the_slot_moved(prefill, after, curs)
    out = case.rows64(P8)
    checked, worst, worst_el = 0, 0.0, 0.0
    for r in range(R):
        cur = curs[r >> 1]
        c, s = cos[cur].numpy(), sin[cur].numpy()
        for h in range(KVH):
            x = qkv[r, K_OFF + h * 128: K_OFF + (h + 1) * 128].double().numpy()
            kr = REF.rope(x, c, s)
            vn = qkv[r, V_OFF + h * 128: V_OFF + (h + 1) * 128].double().numpy()
            pair = np.abs(x[:64]) + np.abs(x[64:])
            for name8, names, want, rot in (("k8", "ks", kr, np.concatenate([pair, pair])), ("v8", "vs", vn, np.zeros(128))):
                amax = float(np.abs(want).max())
                m, _ = np.frexp(amax / 448.0)
                assert min(abs(m - 0.5) / 0.5, abs(m - 1.0)) > 1e-6, "seed puts an amax on a scale boundary: choose another"
                scale = float(after[names][r, h, cur - 1])
                assert scale == rule_scale64(amax), (name8, r, h, scale, rule_scale64(amax))
                got = REF.dequantize(after[name8][r, h, cur - 1].numpy(), after[names][r, h, cur - 1].numpy())
                err = np.abs(got - want)
                bound = np.maximum(2.0 ** -4 * np.abs(want), 2.0 ** -10 * scale) + 2.0 ** -21 * rot
                worst_el = max(worst_el, float((err / bound).max()))
                assert (err <= bound).all(), (name8, r, h, float((err / bound).max()))
                checked += 1
            qr = REF.rope(qkv[r, h * G * 128: (h + 1) * G * 128].double().numpy().reshape(G, 128), c, s)
            ref = REF.attend(qr, after["k8"][r, h].numpy(), after["ks"][r, h].numpy(), after["v8"][r, h].numpy(), after["vs"][r, h].numpy(), cur)
            worst = max(worst, float(np.abs(out[r, h * G: (h + 1) * G].numpy() - ref).max()))
    print(f"cur {curs}: appended slot at most {worst_el:.3f} of its bound; output max abs error vs float64 over the read-back cache {worst:.3e} (bound {TOL})")
    assert checked == R * KVH * 2, "a scale check was skipped"
    assert worst <= TOL, worst


def test_a_reused_slot(prefill):
    """rows holding 300 old keys with large values and cur = 5: the output equals that of the same rows with everything beyond
    key 5 zeroed (bytes and scales), bit for bit — a masked key contributes 0 x finite"""
    g = torch.Generator().manual_seed(9)
    big = torch.randn(R, KVH, T, 128, generator=g) * 2.0 ** 12
    (k8, ks), (v8, vs) = quantize_kv_fp8(big.bfloat16()), quantize_kv_fp8(big.flip(-1).bfloat16())
    used = {n: prefill[n].clone() for n in prefill}
    used["k8"][:, :, 5:300], used["ks"][:, :, 5:300], used["v8"][:, :, 5:300], used["vs"][:, :, 5:300] = k8[:, :, 5:300], ks[:, :, 5:300], v8[:, :, 5:300], vs[:, :, 5:300]
    clean = {n: used[n].clone() for n in used}
    for n in clean:
        clean[n][:, :, 5:] = 0
    qkv = torch.randn(R, NQ, generator=g)
    outs = []
    for state in (used, clean):
        P, after = Step(qkv, (5, 5), real_tables()).run_fp8(state)
        assert_only_the_slot_moved(state, after, (5, 5))
        outs.append(P)
    assert torch.equal(bits(outs[0], 1), bits(outs[1], 1))
    o = lay.unpack_f32_tiles(outs[0], 16, QH * 128)[:R]
    assert torch.isfinite(o).all() and o.abs().max() > 0


def test_head_map_with_dead_heads(prefill):
    """one query head of kv head 0 pruned, and every query head of kv head 1: the live heads' outputs are those of the launch
    without a map, nothing is emitted for the dead ones, and both kv heads still append"""
    curs = (33, 257)
    g = torch.Generator().manual_seed(17)
    qkv = torch.randn(R, NQ, generator=g)
    hmap = [0, 1, -1, 3, -1, -1, -1, -1]
    Pm, after_m = Step(qkv, curs, real_tables(), head_map=hmap).run_fp8(prefill)
    Pf, after_f = Step(qkv, curs, real_tables()).run_fp8(prefill)
    om, of = lay.unpack_f32_tiles(Pm, 16, QH * 128).reshape(16, QH, 128), lay.unpack_f32_tiles(Pf, 16, QH * 128).reshape(16, QH, 128)
    for h, pos in enumerate(hmap):
        if pos >= 0:
            assert torch.equal(om[:R, pos].view(torch.int32), of[:R, h].view(torch.int32)), h
        else:
            assert (om[:, h] == SENTINEL).all(), h
    for n in after_m:
        assert torch.equal(after_m[n], after_f[n]), n
    assert_only_the_slot_moved(prefill, after_m, curs)
    for r in range(R):
        s = curs[r >> 1] - 1
        assert not torch.equal(after_m["k8"][r, :, s], prefill["k8"][r, :, s])


def test_refusals(prefill):
    case = Step(torch.zeros(R, NQ), (1, 1), real_tables())
    d = dev()
    f = dict(k8=torch.zeros(R, KVH, T, 128, dtype=torch.uint8, device=d), v8=torch.zeros(R, KVH, T // 32, 128, 32, dtype=torch.uint8, device=d),
             ks=torch.zeros(R, KVH, T, device=d), vs=torch.zeros(R, KVH, T, device=d))
    P = case.out_buffer(1)
    L = hb.lib()

    def call(pk=None, **kw):
        a = case.args(P, 1)
        for k, v in kw.items():
            setattr(a, k, v)
        p = hb.KvFp8Ptrs(k8=hb.ptr(f["k8"]), v8=hb.ptr(f["v8"]), ks=hb.ptr(f["ks"]), vs=hb.ptr(f["vs"]))
        for k, v in (pk or {}).items():
            setattr(p, k, v)
        return L.dia_attn_self_fp8(C.byref(a), C.byref(p), None)

    for kw, pk, word in ((dict(mode=hb.ATTN_CROSS), None, b"mode must be DIA_ATTN_SELF"), (dict(kv_dtype=hb.KV_F32), None, b"kv_dtype"),
                         (dict(kv_dtype=hb.KV_BF16X2), None, b"kv_dtype"), (dict(v_blocked=0), None, b"v_blocked"), (dict(kv_cap=T - 8), None, b"multiple of 32"),
                         (dict(cur=None), None, b"cur"), ({}, dict(k8=hb.ptr(f["k8"]) + 4), b"aligned"), ({}, dict(vs=hb.ptr(f["vs"]) + 2), b"aligned"),
                         (dict(scratch=None), None, b"scratch and tickets"), (dict(tickets=None), None, b"scratch and tickets"), (dict(group=3), None, b"group"),
                         ({}, dict(ks=None), b"null")):
        assert call(pk, **kw) == -1, (kw, pk)                          # DIA_E_ARG
        assert L.dia_last_error().startswith(b"dia_attn_self_fp8:") and word in L.dia_last_error(), (kw, pk, L.dia_last_error())
    torch.cuda.synchronize()
    assert all(int(t.count_nonzero()) == 0 for t in f.values())        # nothing was launched
    assert call() == 0                                                 # the same arguments, unrefused (kc == vc == NULL)
    torch.cuda.synchronize()
    assert float(f["ks"][0, 0, 0]) == 1.0 and float(f["vs"][0, 0, 0]) == 1.0      # a zero key at slot 0: scale 1
