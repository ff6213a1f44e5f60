"""The batched prompt prefill onto FP8 self caches, kernel level through the C ABI (DESIGN.md "Prompt prefill at admission and
onto fp8 caches"): dia_dec_prefill_kv_fp8 — every packed row quantised and appended like the decode step's new key — and
dia_dec_prefill_attn_fp8 — the causal prefill attention over the e4m3 caches — against exact constructions, float64, the decode
step's own append (dia_attn_self_fp8), the bf16 prefill attention over the dequantised caches bit for bit, and their refusals.

Shapes: 2 kv heads x 4 query heads, capacity 160 keys, 14 cache rows of which 7 non-adjacent ones are listed.  Segment lengths
{1, 2, 31, 32, 33, 65, 130}: one key, both sides of a granule boundary, and 130 keys — more than 4 granules, so a wave of the
attention kernel takes a second one.  Blocks of padding rows lie between some segments."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import self_fp8_ref as REF
from dia_hip import binding as hb
from dia_hip import layout as lay
from dia_hip.quant import dequantize_kv_fp8, quantize_kv_fp8

NROWS, KVH, G, T = 14, 2, 4, 160
QH = KVH * G
NQ = (QH + 2 * KVH) * 128
K_OFF, V_OFF = QH * 128, (QH + KVH) * 128
TOL = 2e-5                      # tests/test_gpu_prefill.py: the bf16 prefill attention against its float64 reference
SENTINEL = 9.0
# (cache row, prompt rows, blocks of 32 padding rows behind the segment)
SEGS = [(9, 33, 0), (1, 1, 1), (5, 130, 0), (3, 2, 0), (11, 65, 2), (7, 31, 0), (13, 32, 1)]


def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    return torch.device("cuda:0")


def pack():
    """packing tables on the host: offsets (multiples of 32), rows, row -> segment (-1 in padding rows)"""
    offs, tot = [], 0
    for _, n, gap in SEGS:
        offs.append(tot)
        tot += -(-n // 32) * 32 + 32 * gap
    rs = np.full((tot,), -1, dtype=np.int32)
    for i, (_, n, _) in enumerate(SEGS):
        rs[offs[i]: offs[i] + n] = i
    return offs, tot, rs


OFFS, ROWS, ROW_SEG = pack()


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


def rule_scale64(amax):
    """the format's rule on a float64 amax: the smallest 2^e (e >= -126) with amax / 2^e <= 448, 1 for zero"""
    if amax == 0:
        return 1.0
    m, ex = np.frexp(amax)
    return float(np.ldexp(1.0, max(int(ex) - 9 + (1 if m > 0.875 else 0), -126)))


@pytest.fixture(scope="module")
def stale():
    """what the caches hold before a prefill: fixed random finite bytes and power-of-two scales in every row (V in key order).
    Computed once, never modified: every launch works on device copies"""
    g = torch.Generator().manual_seed(21)
    out = {}
    for n in ("k8", "v8"):
        b = torch.randint(0, 256, (NROWS, KVH, T, 128), generator=g, dtype=torch.int32).to(torch.uint8)
        b[(b & 0x7F) == 0x7F] = 0x35                                # (no NaN pattern: every byte finite)
        out[n] = b
    for n in ("ks", "vs"):
        out[n] = torch.exp2(torch.randint(-6, 4, (NROWS, KVH, T), generator=g).float())
    return out


@pytest.fixture(scope="module")
def filled():
    """caches holding keys of the existing fixture's magnitudes in every slot (the slots past a segment's length are the stale
    keys of a re-used row): randn * 2^[-3..3] through the host quantiser"""
    g = torch.Generator().manual_seed(11)
    k = torch.randn(NROWS, KVH, T, 128, generator=g) * torch.exp2(torch.randint(-3, 4, (NROWS, KVH, T, 1), generator=g).float())
    v = torch.randn(NROWS, KVH, T, 128, generator=g) * torch.exp2(torch.randint(-2, 3, (NROWS, KVH, T, 1), generator=g).float())
    k[5, 0, 7], v[5, 1, 40] = 0.0, 0.0
    (k8, ks), (v8, vs) = quantize_kv_fp8(k.bfloat16()), quantize_kv_fp8(v.bfloat16())
    return dict(k8=k8, ks=ks, v8=v8, vs=vs)


class Prefill:
    """one packed prefill problem on the device: qkv [ROWS, NQ], the packing of SEGS, RoPE tables, fp8 caches from a host state"""

    def __init__(self, qkv, tables, state):
        d = dev()
        self.qkv = qkv.to(d).contiguous()
        self.cos, self.sin = [t.to(d).contiguous() for t in tables]
        i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=d)
        self.row_seg, self.seg_off = torch.from_numpy(ROW_SEG).to(d), i32(OFFS)
        self.seg_len, self.seg_row = i32([n for _, n, _ in SEGS]), i32([r for r, _, _ in SEGS])
        self.f = dict(k8=state["k8"].to(d).contiguous(), v8=lay.v_to_blocked(state["v8"]).to(d).contiguous(),
                      ks=state["ks"].to(d).contiguous(), vs=state["vs"].to(d).contiguous())
        self.P = lay.pack_planes(torch.full((ROWS, QH * 128), SENTINEL, device=d))

    def args(self):
        a = hb.DecPrefillArgs()
        a.row_seg, a.seg_off, a.seg_len, a.seg_row, a.rows = hb.ptr(self.row_seg), hb.ptr(self.seg_off), hb.ptr(self.seg_len), hb.ptr(self.seg_row), ROWS
        a.q, a.ldq, a.q_off, a.k_off, a.v_off = hb.ptr(self.qkv), NQ, 0, K_OFF, V_OFF
        a.q_heads, a.kv_heads, a.kv_cap, a.causal = QH, KVH, T, 1
        a.cos_t, a.sin_t = hb.ptr(self.cos), hb.ptr(self.sin)
        a.P, a.p_plane_stride, a.p_ktiles = hb.ptr(self.P), self.P[0].numel(), QH * 128 // 32
        return a                                                   # kc == vc == NULL

    def ptrs(self):
        f = self.f
        return hb.KvFp8Ptrs(k8=hb.ptr(f["k8"]), v8=hb.ptr(f["v8"]), ks=hb.ptr(f["ks"]), vs=hb.ptr(f["vs"]))

    def kv(self):
        a, p = self.args(), self.ptrs()
        hb.check(hb.lib().dia_dec_prefill_kv_fp8(C.byref(a), C.byref(p), None), "dia_dec_prefill_kv_fp8")
        torch.cuda.synchronize()
        return self.state()

    def attn(self):
        a, p = self.args(), self.ptrs()
        hb.check(hb.lib().dia_dec_prefill_attn_fp8(C.byref(a), C.byref(p), None), "dia_dec_prefill_attn_fp8")
        torch.cuda.synchronize()
        return self.P

    def attn_bf16(self, state):
        """dia_dec_prefill_attn (causal) over bf16 caches holding the dequantised state"""
        d = dev()
        kd, vd = dequantize_kv_fp8(state["k8"], state["ks"]), dequantize_kv_fp8(state["v8"], state["vs"])
        assert torch.equal(kd.bfloat16().float(), kd) and torch.equal(vd.bfloat16().float(), vd)
        kc, vc = kd.bfloat16().to(d).contiguous(), lay.v_to_blocked(vd.bfloat16()).to(d).contiguous()
        P = lay.pack_planes(torch.full((ROWS, QH * 128), SENTINEL, device=d))
        a = self.args()
        a.kc, a.vc, a.P = hb.ptr(kc), hb.ptr(vc), hb.ptr(P)
        hb.check(hb.lib().dia_dec_prefill_attn(C.byref(a), None), "dia_dec_prefill_attn")
        torch.cuda.synchronize()
        return P

    def state(self):
        f = self.f
        return dict(k8=f["k8"].cpu(), v8=lay.v_from_blocked(f["v8"]).cpu(), ks=f["ks"].cpu(), vs=f["vs"].cpu())


def assert_nothing_else_moved(before, after):
    written = torch.zeros(NROWS, KVH, T, dtype=torch.bool)
    for crow, n, _ in SEGS:
        written[crow, :, :n] = True
    for n in ("k8", "v8", "ks", "vs"):
        assert torch.equal(after[n][~written], before[n][~written]), n
    return written


def test_append_exact(stale):
    """exact rotations and rows that quantise to themselves: the dequantised K and V are the inputs bit for bit, the scales the rule's,
    and every byte and scale outside [0, len) of the listed rows and in every unlisted row is unchanged"""
    g = torch.Generator().manual_seed(31)
    qkv = torch.randn(ROWS, NQ, generator=g)
    qkv[:, K_OFF:V_OFF] = grid_rows(g, ROWS * KVH, peak_at=40, e_lo=-9, e_hi=-5).reshape(ROWS, KVH * 128)
    qkv[:, V_OFF:] = grid_rows(g, ROWS * KVH, peak_at=3, e_lo=-10, e_hi=-4).reshape(ROWS, KVH * 128)
    cos, sin = exact_tables(5)
    after = Prefill(qkv, (cos, sin), stale).kv()
    written = assert_nothing_else_moved(stale, after)
    assert int(written.sum()) == sum(n for _, n, _ in SEGS) * KVH
    kd, vd = dequantize_kv_fp8(after["k8"], after["ks"]).double(), dequantize_kv_fp8(after["v8"], after["vs"]).double()
    keys = 0
    for (crow, n, _), o in zip(SEGS, OFFS):
        k = qkv[o: o + n, K_OFF:V_OFF].double().reshape(n, KVH, 128).numpy()
        v = qkv[o: o + n, V_OFF:].double().reshape(n, KVH, 128)
        kr = torch.from_numpy(REF.rope(k, cos[1: n + 1, None, :].numpy(), sin[1: n + 1, None, :].numpy()))       # position r + 1
        assert torch.equal(kd[crow, :, :n].transpose(0, 1), kr), crow
        assert torch.equal(vd[crow, :, :n].transpose(0, 1), v), crow
        for want, names in ((kr, "ks"), (v, "vs")):
            _, s = quantize_kv_fp8(want)
            assert torch.equal(after[names][crow, :, :n].transpose(0, 1), s), (crow, names)
            for r in range(n):
                for h in range(KVH):
                    assert float(s[r, h]) == rule_scale64(float(want[r, h].abs().max()))
        keys += n * KVH
    assert keys == sum(n for _, n, _ in SEGS) * KVH


def test_append_real_tables_against_float64(stale):
    g = torch.Generator().manual_seed(303)
    qkv = torch.randn(ROWS, NQ, generator=g)
    qkv[:, K_OFF:V_OFF] *= 3.0
    cos, sin = real_tables()
    after = Prefill(qkv, (cos, sin), stale).kv()
    assert_nothing_else_moved(stale, after)
    checked, worst = 0, 0.0
    for (crow, n, _), o in zip(SEGS, OFFS):
        for r in range(n):
            c, s = cos[r + 1].numpy(), sin[r + 1].numpy()
            for h in range(KVH):
                x = qkv[o + r, K_OFF + h * 128: K_OFF + (h + 1) * 128].double().numpy()
                kr = REF.rope(x, c, s)
                vn = qkv[o + r, V_OFF + h * 128: V_OFF + (h + 1) * 128].double().numpy()
                pair = np.abs(x[:64]) + np.abs(x[64:])
                for name8, names, want, rot in (("k8", "ks", kr, np.concatenate([pair, pair])), ("v8", "vs", vn, np.zeros(128))):
                    amax = float(np.abs(want).max())
                    m, _ = np.frexp(amax / 448.0)
                    assert min(abs(m - 0.5) / 0.5, abs(m - 1.0)) > 1e-6, "seed puts an amax on a scale boundary: choose another"
                    scale = float(after[names][crow, h, r])
                    assert scale == rule_scale64(amax), (name8, crow, r, h, scale, rule_scale64(amax))
                    got = REF.dequantize(after[name8][crow, h, r].numpy(), after[names][crow, h, r].numpy())
                    err = np.abs(got - want)
                    bound = np.maximum(2.0 ** -4 * np.abs(want), 2.0 ** -10 * scale) + 2.0 ** -21 * rot
                    worst = max(worst, float((err / bound).max()))
                    assert (err <= bound).all(), (name8, crow, r, h, float((err / bound).max()))
                    checked += 1
    print(f"prefill append, real tables: an element is at most {worst:.3f} of its bound; {checked} keys checked")
    assert checked == sum(n for _, n, _ in SEGS) * KVH * 2, "a key was skipped"


def step_append(qkv_row, cur, tables, state_rows):
    """dia_attn_self_fp8 at `cur` on a two-row cache (one utterance, both CFG rows = the same qkv row): the state read back"""
    d = dev()
    qkv = torch.stack([qkv_row, qkv_row]).to(d).contiguous()
    cos, sin = [t.to(d).contiguous() for t in tables]
    f = dict(k8=state_rows["k8"].to(d).contiguous(), v8=lay.v_to_blocked(state_rows["v8"]).to(d).contiguous(),
             ks=state_rows["ks"].to(d).contiguous(), vs=state_rows["vs"].to(d).contiguous())
    cur_t = torch.tensor([cur], dtype=torch.int32, device=d)
    scr = torch.zeros(max(1, hb.lib().dia_attn_scratch_floats(2, KVH, T)), device=d)
    tk = torch.zeros(2 * KVH, dtype=torch.int32, device=d)
    kt = QH * 4
    P = torch.full((1, kt, 64, 8), SENTINEL, dtype=torch.float32, device=d)
    a = hb.AttnArgs()
    a.mode, a.kv_dtype, a.n_kv_heads, a.group, a.n_rows, a.kv_cap = hb.ATTN_SELF, hb.KV_BF16, KVH, G, 2, T
    a.q, a.ldq, a.q_off, a.k_off, a.v_off = hb.ptr(qkv), NQ, 0, K_OFF, V_OFF
    a.cur, a.cos_t, a.sin_t, a.rope_rows = hb.ptr(cur_t), hb.ptr(cos), hb.ptr(sin), T + 1
    a.P, a.p_plane_stride, a.p_ktiles, a.act_f32 = hb.ptr(P), kt * 512, kt, 1
    a.scratch, a.tickets, a.v_blocked = hb.ptr(scr), hb.ptr(tk), 1
    p = hb.KvFp8Ptrs(k8=hb.ptr(f["k8"]), v8=hb.ptr(f["v8"]), ks=hb.ptr(f["ks"]), vs=hb.ptr(f["vs"]))
    hb.check(hb.lib().dia_attn_self_fp8(C.byref(a), C.byref(p), None), "dia_attn_self_fp8")
    torch.cuda.synchronize()
    out = lay.unpack_f32_tiles(P, 16, QH * 128).double().reshape(16, QH, 128).cpu()
    return out, dict(k8=f["k8"].cpu(), v8=lay.v_from_blocked(f["v8"]).cpu(), ks=f["ks"].cpu(), vs=f["vs"].cpu())


def test_append_equals_the_steps_append(stale):
    """prompt rows 0, 31 and 32 of the 130-row segment: the bytes and scales of the prefill are those the decode step writes at
    cur = r + 1 for the same qkv row with the real tables, bit for bit"""
    g = torch.Generator().manual_seed(77)
    qkv = torch.randn(ROWS, NQ, generator=g)
    qkv[:, K_OFF:V_OFF] *= 3.0
    tables = real_tables()
    after = Prefill(qkv, tables, stale).kv()
    si = [n for _, n, _ in SEGS].index(130)
    crow, o = SEGS[si][0], OFFS[si]
    two = {n: stale[n][:2] for n in stale}
    for r in (0, 31, 32):
        _, st = step_append(qkv[o + r], r + 1, tables, two)
        for row in (0, 1):
            for n in ("k8", "v8", "ks", "vs"):
                assert torch.equal(st[n][row][:, r], after[n][crow][:, r]), (r, row, n)
                assert not torch.equal(st[n][row][:, r], two[n][row][:, r]) or n in ("ks", "vs"), (r, row, n)      # (the step did write)


def rope_t(x, c, s):
    x1, x2 = x[..., :64], x[..., 64:]
    return torch.cat([x1 * c - x2 * s, x1 * s + x2 * c], dim=-1)


def attn_masked(q, K, V, lim):
    """q [L, Hq, 128], K / V [n, Hkv, 128] float64, lim [L]: query row i sees keys 0 .. lim[i]-1"""
    g = q.shape[1] // K.shape[1]
    Ke, Ve = K.repeat_interleave(g, dim=1), V.repeat_interleave(g, dim=1)
    s = torch.einsum("qhd,khd->hqk", q, Ke) / math.sqrt(128.0)
    keys = torch.arange(K.shape[0])
    vis = (keys[None, :] < lim[:, None])[None]
    span = (s.masked_fill(~vis, -math.inf).amax(-1) - s.masked_fill(~vis, math.inf).amin(-1)).max()
    p = torch.softmax(s.masked_fill(~vis, -math.inf), dim=-1)
    return torch.einsum("hqk,khd->qhd", p, Ve), float(span)


def test_attention_bitwise_against_the_bf16_kernel(filled):
    """dia_dec_prefill_attn_fp8 == dia_dec_prefill_attn (causal) over bf16 caches holding the dequantised values: the three output
    planes as integers, sentinel padding rows untouched; and against float64 over the dequantised cache"""
    g = torch.Generator().manual_seed(43)
    qkv = torch.randn(ROWS, NQ, generator=g)
    cos, sin = real_tables()
    case = Prefill(qkv, (cos, sin), filled)
    P8 = case.attn()
    Pb = case.attn_bf16(filled)
    assert torch.equal(P8.view(torch.int16), Pb.view(torch.int16)), "fp8 prefill attention != bf16 prefill attention over the dequantised caches"
    out = lay.unpack_planes(P8, ROWS, QH * 128).double().reshape(ROWS, QH, 128).cpu()
    pad = torch.from_numpy(ROW_SEG < 0)
    assert (out[pad] == SENTINEL).all() and int(pad.sum()) > 4 * 32
    after = case.state()
    for n in filled:
        assert torch.equal(after[n], filled[n]), n                      # the attention writes no cache
    kd, vd = dequantize_kv_fp8(filled["k8"], filled["ks"]).double(), dequantize_kv_fp8(filled["v8"], filled["vs"]).double()
    worst, span = 0.0, 0.0
    for (crow, n, _), o in zip(SEGS, OFFS):
        q = rope_t(qkv[o: o + n, :K_OFF].double().reshape(n, QH, 128), cos[1: n + 1, None, :].double(), sin[1: n + 1, None, :].double())
        ref, sp = attn_masked(q, kd[crow, :, :n].transpose(0, 1), vd[crow, :, :n].transpose(0, 1), torch.arange(n) + 1)
        span = max(span, sp)
        assert torch.isfinite(out[o: o + n]).all()
        worst = max(worst, float((out[o: o + n] - ref).abs().max()))
    print(f"fp8 prefill attention: bitwise the bf16 kernel's; max abs error vs float64 {worst:.3e} (bound {TOL}); visible scores span {span:.1f} (< 80)")
    assert span < 80.0, "a query row's visible scores span 80 or more: p * vs may leave the normal range — pick another seed"
    assert worst <= TOL, worst


def test_prefill_then_one_decode_step(stale):
    """the decode step reads what the prefill wrote: after the prefill of n rows (33 and 130), dia_attn_self_fp8 at cur = n + 1
    agrees with the float64 reference over the cache it leaves"""
    g = torch.Generator().manual_seed(91)
    qkv = torch.randn(ROWS, NQ, generator=g)
    qkv[:, K_OFF:V_OFF] *= 2.0
    tables = real_tables()
    cos, sin = tables
    after = Prefill(qkv, tables, stale).kv()
    for n in (33, 130):
        si = [m for _, m, _ in SEGS].index(n)
        crow = SEGS[si][0]
        row = torch.randn(NQ, generator=g)
        rows2 = {k: torch.stack([after[k][crow], after[k][crow]]) for k in after}
        out, st = step_append(row, n + 1, tables, rows2)
        worst = 0.0
        for h in range(KVH):
            qr = REF.rope(row[h * G * 128: (h + 1) * G * 128].double().numpy().reshape(G, 128), cos[n + 1].numpy(), sin[n + 1].numpy())
            ref = REF.attend(qr, st["k8"][0, h].numpy(), st["ks"][0, h].numpy(), st["v8"][0, h].numpy(), st["vs"][0, h].numpy(), n + 1)
            worst = max(worst, float(np.abs(out[0, h * G: (h + 1) * G].numpy() - ref).max()))
            assert torch.equal(st["k8"][0, h, :n], after["k8"][crow, h, :n])        # (the step appended slot n, nothing before it)
        print(f"prefill of {n} rows, then a step at cur {n + 1}: max abs error vs float64 {worst:.3e} (bound {TOL})")
        assert worst <= TOL, (n, worst)


def test_refusals(stale):
    zero = {n: torch.zeros_like(stale[n]) for n in stale}
    case = Prefill(torch.zeros(ROWS, NQ), real_tables(), zero)
    L = hb.lib()
    other = torch.zeros(64, dtype=torch.uint8, device=dev())
    for fn, name in ((L.dia_dec_prefill_kv_fp8, b"dia_dec_prefill_kv_fp8"), (L.dia_dec_prefill_attn_fp8, b"dia_dec_prefill_attn_fp8")):
        def call(pk=None, **kw):
            a, p = case.args(), case.ptrs()
            for k, v in kw.items():
                setattr(a, k, v)
            for k, v in (pk or {}).items():
                setattr(p, k, v)
            return fn(C.byref(a), C.byref(p), None)

        for kw, pk, word in ((dict(kc=hb.ptr(other)), None, b"kc / vc must be NULL"), (dict(vc=hb.ptr(other)), None, b"kc / vc must be NULL"),
                             (dict(causal=0), None, b"causal"), (dict(kv_cap=T - 8), None, b"multiple of 32"), (dict(rows=ROWS - 16), None, b"rows"),
                             (dict(row_seg=None), None, b"packing"), (dict(q=None), None, b"bad argument"), (dict(cos_t=None), None, b"bad argument"),
                             ({}, dict(k8=None), b"null"), ({}, dict(vs=None), b"null"), ({}, dict(v8=hb.ptr(case.f["v8"]) + 8), b"aligned")):
            assert call(pk, **kw) == -1, (name, kw, pk)                                # DIA_E_ARG
            assert word in L.dia_last_error(), (name, kw, pk, L.dia_last_error())
        assert fn(None, C.byref(case.ptrs()), None) == -1 and fn(C.byref(case.args()), None, None) == -1
        assert L.dia_last_error().startswith(name + b":")
    torch.cuda.synchronize()
    assert all(int(t.count_nonzero()) == 0 for t in case.f.values())                   # nothing was launched
    assert (lay.unpack_planes(case.P, ROWS, QH * 128) == SENTINEL).all()
    case.kv()                                                                          # the same arguments, unrefused
    assert float(case.f["ks"][1, 0, 0]) == 1.0 and float(case.f["vs"][1, 0, 0]) == 1.0 # a zero key at slot 0 of a listed row: scale 1
    assert float(case.f["ks"][0, 0, 0]) == 0.0                                         # an unlisted row: untouched
