"""dia_lora_apply / dia_lora_crosskv (csrc/lora.hip) through ctypes against float64: the low-rank correction a slot's adapter adds
to a projection's output rows, and to the cross K/V caches in every cache format.  Bound: the GEMM tests' 2e-5 of the output scale
(tests/test_gpu_kernels.py); bf16 caches: one unit in the last place of bf16(base + delta), the format's own condition."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from dia_hip import binding as hb
from dia_hip import layout as lay

DEV = "cuda:0"
EPS = 1e-5
REL = 2e-5


class Bank:
    """device tables of a few adapters for a list of modules (name -> fan-out); ranks[a][name] = 0 leaves the module alone"""

    def __init__(self, D, widths, ranks, seed=0):
        g = torch.Generator().manual_seed(seed)
        self.D, self.widths, self.n = D, widths, len(ranks)
        self.A, self.B, self.rank, self.scale, self.keep, self.tab = {}, {}, {}, {}, [], {}
        for name, n_out in widths.items():
            pa, pb, rk, sc = [], [], [], []
            for a, rr in enumerate(ranks):
                r = rr.get(name, 0)
                A = (torch.randn(max(r, 1), D, generator=g) / D ** 0.5).to(DEV)
                B = torch.randn(max(r, 1), n_out, generator=g).to(DEV)
                self.A[(name, a)], self.B[(name, a)] = A, B
                pa.append(A.data_ptr() if r else 0); pb.append(B.data_ptr() if r else 0)
                rk.append(r); sc.append(0.5 + 0.25 * a)
            self.rank[name], self.scale[name] = rk, sc
            self.tab[name] = (torch.tensor(pa, dtype=torch.int64).to(DEV), torch.tensor(pb, dtype=torch.int64).to(DEV),
                              torch.tensor(rk, dtype=torch.int32).to(DEV), torch.tensor(sc, dtype=torch.float32).to(DEV))

    def seg(self, name, col_off, max_rank=None):
        s = hb.LoraSeg()
        pa, pb, rk, sc = self.tab[name]
        s.col_off, s.n_cols, s.A, s.B, s.rank, s.scale = col_off, self.widths[name], pa.data_ptr(), pb.data_ptr(), rk.data_ptr(), sc.data_ptr()
        s.max_rank = max(self.rank[name]) if max_rank is None else max_rank
        return s

    def delta(self, name, a, xn):
        """float64 [rows, fan-out] correction of adapter a for normed rows xn"""
        r = self.rank[name][a]
        if a < 0 or r == 0:
            return torch.zeros(xn.shape[0], self.widths[name], dtype=torch.float64)
        A, B = self.A[(name, a)][:r].double().cpu(), self.B[(name, a)][:r].double().cpu()
        return self.scale[name][a] * (xn @ A.t()) @ B


def normed(x, g):
    x, g = x.double().cpu(), g.double().cpu()
    return x * g * torch.rsqrt((x * x).mean(dim=1, keepdim=True) + EPS)


def apply_args(bank, x, g, out, segs, adapter_of_slot, row_slot=None, rows_per_slot=2):
    a = hb.LoraArgs()
    a.x, a.ldx, a.D, a.gain, a.eps, a.M = x.data_ptr(), x.shape[1], bank.D, g.data_ptr(), EPS, x.shape[0]
    a.row_slot, a.rows_per_slot = hb.ptr(row_slot), rows_per_slot
    a.adapter_of_slot, a.n_slots, a.n_adapters = adapter_of_slot.data_ptr(), adapter_of_slot.numel(), bank.n
    a.n_segs = len(segs)
    for i, s in enumerate(segs):
        a.seg[i] = s
    a.out, a.ldo = out.data_ptr(), out.shape[1]
    return a


RANKS = [dict(q=8, k=8, v=8), dict(q=1, v=64), dict(q=64, k=3, v=8)]       # per adapter: ranks differ, adapter 1 has no k


@pytest.mark.parametrize("D", [512, 2048])
@pytest.mark.parametrize("M", [1, 2, 5, 16, 17])
def test_lora_apply(D, M):
    """q wider than k = v (GQA), column ranges that do not start at 0, a row_slot map with rows without an adapter and two rows
    sharing one; rows without an adapter are bitwise untouched, the others within 2e-5 of the output scale of float64 base + delta"""
    torch.manual_seed(D + M)
    widths = dict(q=1024, k=256, v=256)
    bank = Bank(D, widths, RANKS, seed=D)
    off = dict(q=128, k=128 + 1024, v=128 + 1024 + 256 + 64)                # gaps: columns between the segments belong to nobody
    ldo = off["v"] + 256 + 32
    x = (torch.randn(M, D) * 3.0).to(DEV)
    g = (1.0 + 0.1 * torch.randn(D)).to(DEV)
    base = torch.randn(M, ldo).to(DEV)
    out = base.clone()
    n_slots = 6
    slot_adapter = torch.tensor([0, -1, 1, 2, -1, 0], dtype=torch.int32)
    rs = torch.tensor([(5 * m + 3) % n_slots if m % 7 != 4 else -1 for m in range(M)], dtype=torch.int32)      # slots 3, 2, 1, 0, -, 4, ...
    if M >= 2:
        rs[1] = rs[0]                                                       # two rows of one slot
    a = apply_args(bank, x, g, out, [bank.seg(n, off[n]) for n in "qkv"], slot_adapter.to(DEV), row_slot=rs.to(DEV))
    hb.check(hb.lib().dia_lora_apply(C.byref(a), None), "dia_lora_apply")
    torch.cuda.synchronize()
    got, ref = out.cpu(), base.double().cpu()
    xn = normed(x, g)
    adapted = torch.zeros(M, dtype=torch.bool)
    for m in range(M):
        ad = int(slot_adapter[rs[m]]) if rs[m] >= 0 else -1
        if ad < 0:
            continue
        adapted[m] = True
        for n in "qkv":
            ref[m, off[n]: off[n] + widths[n]] += bank.delta(n, ad, xn[m: m + 1])[0]
    assert torch.equal(got[~adapted], base.cpu()[~adapted])                 # bitwise
    mask = torch.ones(ldo, dtype=torch.bool)
    for n in "qkv":
        mask[off[n]: off[n] + widths[n]] = False
    assert torch.equal(got[:, mask], base.cpu()[:, mask])                   # columns outside the segments
    assert adapted[0] and (M < 3 or not adapted[2])                         # (the map holds both kinds of row)
    err = (got.double() - ref)[adapted].abs().max().item()
    scale = ref[adapted].abs().max().item()
    print(f"dia_lora_apply D={D} M={M}: max err {err:.3e} = {err / scale:.2e} of the output scale {scale:.2f}")
    assert err <= REL * max(1.0, scale)
    assert (ref - base.double().cpu())[adapted].abs().max().item() > 1e-2 * scale     # the correction is far above the bound


@pytest.mark.parametrize("D", [512, 1024])
def test_lora_apply_rows_per_slot(D):
    """the decode step's row order: rows 2b, 2b + 1 belong to slot b; one segment, rank 8.  D = 1024: the encoder width of Dia-1.6B
    (the middle instantiation of the kernel)"""
    M = 6
    bank = Bank(D, dict(q=512), [dict(q=8), dict(q=8)], seed=3)
    x, g = torch.randn(M, D).to(DEV), torch.ones(D).to(DEV)
    base = torch.randn(M, 512).to(DEV)
    out = base.clone()
    aos = torch.tensor([1, -1, 0], dtype=torch.int32).to(DEV)
    a = apply_args(bank, x, g, out, [bank.seg("q", 0)], aos)
    hb.check(hb.lib().dia_lora_apply(C.byref(a), None), "dia_lora_apply")
    torch.cuda.synchronize()
    xn = normed(x, g)
    ref = base.double().cpu()
    ref[0:2] += bank.delta("q", 1, xn[0:2])
    ref[4:6] += bank.delta("q", 0, xn[4:6])
    assert torch.equal(out[2:4].cpu(), base[2:4].cpu())
    assert (out.double().cpu() - ref).abs().max().item() <= REL * max(1.0, ref.abs().max().item())


def test_lora_apply_refusals():
    D, M = 512, 2
    bank = Bank(D, dict(q=512, k=256), [dict(q=8, k=8)])
    x, g, out = torch.randn(M, D).to(DEV), torch.ones(D).to(DEV), torch.zeros(M, 1024).to(DEV)
    aos = torch.zeros(1, dtype=torch.int32).to(DEV)
    L = hb.lib()

    def refused(mut, word):
        a = apply_args(bank, x, g, out, [bank.seg("q", 0), bank.seg("k", 512)], aos)
        mut(a)
        assert L.dia_lora_apply(C.byref(a), None) == -1
        assert word in L.dia_last_error().decode(), L.dia_last_error()

    refused(lambda a: setattr(a, "x", None), "null")
    refused(lambda a: setattr(a, "out", None), "null")
    refused(lambda a: setattr(a, "adapter_of_slot", None), "null")
    refused(lambda a: setattr(a, "D", 500), "multiple of 256")
    refused(lambda a: setattr(a, "D", 4096), "multiple of 256")
    refused(lambda a: setattr(a, "ldx", 256), "ldx")
    refused(lambda a: setattr(a, "rows_per_slot", 0), "rows_per_slot")
    refused(lambda a: setattr(a, "n_segs", 4), "segments")
    refused(lambda a: setattr(a, "n_segs", 0), "segments")
    refused(lambda a: setattr(a, "ldo", 600), "beyond ldo")
    refused(lambda a: setattr(a.seg[0], "max_rank", 65), "rank above 64")
    refused(lambda a: setattr(a.seg[1], "col_off", 256), "overlap")
    refused(lambda a: setattr(a.seg[1], "n_cols", 6), "multiples of 4")
    refused(lambda a: setattr(a.seg[0], "rank", None), "tables")
    assert torch.count_nonzero(out).item() == 0


# ------------------------------------------------------------------------------------------------ cross K/V caches
H, CAP, E = 2, 64, 512


def cache_tensors(kv, seed):
    """(kc, vc, plane stride): random caches of B = 2 utterances in the format's own value set"""
    g = torch.Generator().manual_seed(seed)
    k32, v32 = torch.randn(2, H, CAP, 128, generator=g), torch.randn(2, H, CAP, 128, generator=g)
    if kv == "f32":
        return k32.to(DEV), v32.to(DEV), 0, k32.double(), v32.double()
    if kv == "bf16":
        kb, vb = k32.bfloat16(), v32.bfloat16()
        return kb.to(DEV), vb.to(DEV), 0, kb.double(), vb.double()
    hi_k, hi_v = k32.bfloat16(), v32.bfloat16()
    lo_k, lo_v = (k32 - hi_k.float()).bfloat16(), (v32 - hi_v.float()).bfloat16()
    return (torch.stack([hi_k, lo_k]).to(DEV), torch.stack([hi_v, lo_v]).to(DEV), k32.numel(),
            hi_k.double() + lo_k.double(), hi_v.double() + lo_v.double())


def read_cache(t, kv):
    t = t.cpu()
    return (t[0].double() + t[1].double()) if kv == "bf16x2" else t.double()


def bf16_ulp(v):
    """one unit in the last place of the bf16 value nearest to v (float64 tensor)"""
    b = v.float().bfloat16().float().abs().clamp(min=2.0 ** -126)
    return (2.0 ** (torch.floor(torch.log2(b)) - 7)).double()


@pytest.mark.parametrize("kv,blocked,E", [("f32", 0, 512), ("bf16", 0, 512), ("bf16", 1, 512), ("bf16x2", 0, 512), ("bf16x2", 1, 512),
                                          ("f32", 0, 1024), ("bf16", 1, 1024), ("bf16x2", 1, 2048)])
def test_lora_crosskv(kv, blocked, E):
    """two packed utterances of 19 and 40 rows (row_b / seg_off), only the second has an adapter: its K rows receive RoPE(dK), its
    V rows dV, in the cache's format and V layout; the other utterance and every row beyond a length stay bitwise.  E = 512, 1024
    (the encoder width of Dia-1.6B) and 2048: one case at least for each instantiation of the kernel"""
    torch.manual_seed(7)
    lens, offs, Mp = [19, 40], [0, 32], 96
    bank = Bank(E, dict(k=H * 128, v=H * 128), [dict(k=8, v=8), dict(k=5, v=16)], seed=11)
    kc, vc, plane, k_ref, v_ref = cache_tensors(kv, 5)
    if blocked:                                    # the V cache in the blocked layout; the reference stays [key][128]
        src = vc if kv == "bf16x2" else vc[None]
        vcb = torch.stack([lay.v_to_blocked(p_.cpu()).reshape(p_.shape) for p_ in src]).to(DEV)
        vc = vcb if kv == "bf16x2" else vcb[0]
    k0, v0 = kc.clone(), vc.clone()
    row_b = torch.full((Mp,), -1, dtype=torch.int32)
    for b in range(2):
        row_b[offs[b]: offs[b] + lens[b]] = b
    x = (torch.randn(Mp, E) * 2.0).to(DEV)
    g = (1.0 + 0.1 * torch.randn(E)).to(DEV)
    cos, sin = lay.rope_tables(CAP + 1, 128, 1, 10000)
    cos, sin = cos.to(DEV), sin.to(DEV)
    aos = torch.tensor([-1, 1], dtype=torch.int32).to(DEV)
    a = hb.LoraCrossKvArgs()
    a.x, a.ldx, a.D, a.gain, a.eps, a.M = x.data_ptr(), E, E, g.data_ptr(), EPS, Mp
    rb_d, so_d = row_b.to(DEV), torch.tensor(offs, dtype=torch.int32).to(DEV)
    a.row_b, a.seg_off, a.adapter_of_slot, a.n_slots, a.n_adapters = rb_d.data_ptr(), so_d.data_ptr(), aos.data_ptr(), 2, 2
    a.k, a.v = bank.seg("k", 0), bank.seg("v", 0)
    a.kc, a.vc, a.kv_dtype, a.kv_heads, a.kv_cap = kc.data_ptr(), vc.data_ptr(), {"f32": 0, "bf16": 1, "bf16x2": 2}[kv], H, CAP
    a.kv_vblocked, a.rope_rows, a.kv_plane_stride, a.cos_t, a.sin_t = blocked, CAP + 1, plane, cos.data_ptr(), sin.data_ptr()
    hb.check(hb.lib().dia_lora_crosskv(C.byref(a), None), "dia_lora_crosskv")
    torch.cuda.synchronize()

    def unblock(t):
        if not blocked:
            return t
        src = t if kv == "bf16x2" else t[None]
        u = torch.stack([lay.v_from_blocked(p_.cpu().reshape(2, H, CAP // 32, 128, 32)) for p_ in src])
        return u if kv == "bf16x2" else u[0]

    k_got, v_got = read_cache(kc, kv), read_cache(unblock(vc), kv)
    # utterance 0 (no adapter) and the rows beyond utterance 1's length: bitwise, in the cache's own bytes
    assert torch.equal(kc.cpu().reshape(-1, 2, H, CAP, 128)[:, 0], k0.cpu().reshape(-1, 2, H, CAP, 128)[:, 0])
    assert torch.equal(unblock(vc).reshape(-1, 2, H, CAP, 128)[:, 0], unblock(v0).reshape(-1, 2, H, CAP, 128)[:, 0])
    assert torch.equal(kc.cpu().reshape(-1, 2, H, CAP, 128)[:, 1, :, lens[1]:], k0.cpu().reshape(-1, 2, H, CAP, 128)[:, 1, :, lens[1]:])
    assert torch.equal(unblock(vc).reshape(-1, 2, H, CAP, 128)[:, 1, :, lens[1]:], unblock(v0).reshape(-1, 2, H, CAP, 128)[:, 1, :, lens[1]:])
    # utterance 1: float64 base + RoPE(dK), base + dV
    xn = normed(x, g)[offs[1]: offs[1] + lens[1]]
    dk = bank.delta("k", 1, xn).reshape(lens[1], H, 128)
    dv = bank.delta("v", 1, xn).reshape(lens[1], H, 128)
    c, s = cos[: lens[1]].double().cpu()[:, None, :], sin[: lens[1]].double().cpu()[:, None, :]
    rk = torch.cat([dk[..., :64] * c - dk[..., 64:] * s, dk[..., :64] * s + dk[..., 64:] * c], dim=-1)
    want_k = k_ref[1, :, : lens[1]] + rk.permute(1, 0, 2)
    want_v = v_ref[1, :, : lens[1]] + dv.permute(1, 0, 2)
    for name, got, want, before in (("K", k_got[1, :, : lens[1]], want_k, k_ref[1, :, : lens[1]]), ("V", v_got[1, :, : lens[1]], want_v, v_ref[1, :, : lens[1]])):
        err = (got - want).abs()
        assert (want - before).abs().max().item() > 0.05 * want.abs().max().item()
        if kv == "bf16":
            want_bf16 = want.float().bfloat16().double()                    # bf16(base + delta), the sum in float64
            worst = ((got - want_bf16).abs() / bf16_ulp(want)).max().item()
            print(f"dia_lora_crosskv {kv} blocked={blocked} {name}: worst error {worst:.3f} bf16 ulp")
            assert worst <= 1.0
        else:
            print(f"dia_lora_crosskv {kv} blocked={blocked} {name}: max err {err.max().item():.3e} of scale {want.abs().max().item():.2f}")
            assert err.max().item() <= REL * max(1.0, want.abs().max().item())


def test_lora_crosskv_refusals():
    bank = Bank(E, dict(k=H * 128, v=H * 128), [dict(k=8, v=8)])
    kc, vc = torch.zeros(2, H, CAP, 128).to(DEV), torch.zeros(2, H, CAP, 128).to(DEV)
    x, g = torch.randn(32, E).to(DEV), torch.ones(E).to(DEV)
    cos, sin = (t.to(DEV) for t in lay.rope_tables(CAP + 1, 128, 1, 10000))
    aos = torch.zeros(2, dtype=torch.int32).to(DEV)
    rb, so = torch.zeros(32, dtype=torch.int32).to(DEV), torch.zeros(2, dtype=torch.int32).to(DEV)
    L = hb.lib()

    def refused(mut, word):
        a = hb.LoraCrossKvArgs()
        a.x, a.ldx, a.D, a.gain, a.eps, a.M = x.data_ptr(), E, E, g.data_ptr(), EPS, 32
        a.row_b, a.seg_off, a.adapter_of_slot, a.n_slots, a.n_adapters = rb.data_ptr(), so.data_ptr(), aos.data_ptr(), 2, 1
        a.k, a.v = bank.seg("k", 0), bank.seg("v", 0)
        a.kc, a.vc, a.kv_dtype, a.kv_heads, a.kv_cap, a.rope_rows = kc.data_ptr(), vc.data_ptr(), 0, H, CAP, CAP + 1
        a.cos_t, a.sin_t = cos.data_ptr(), sin.data_ptr()
        mut(a)
        assert L.dia_lora_crosskv(C.byref(a), None) == -1
        assert word in L.dia_last_error().decode(), L.dia_last_error()

    refused(lambda a: setattr(a, "kc", None), "null")
    refused(lambda a: setattr(a, "cos_t", None), "null")
    refused(lambda a: setattr(a, "seg_off", None), "go together")
    refused(lambda a: setattr(a, "kv_dtype", 3), "kv_dtype")
    refused(lambda a: setattr(a, "kv_dtype", 2), "kv_plane_stride")
    refused(lambda a: setattr(a, "kv_vblocked", 1), "blocked V")
    refused(lambda a: setattr(a, "rope_rows", 0), "rope_rows")
    refused(lambda a: setattr(a, "rope_rows", CAP - 1), "rope_rows >= kv_cap")
    refused(lambda a: setattr(a, "kv_heads", 3), "kv_heads * 128")
    refused(lambda a: setattr(a.k, "max_rank", 100), "rank above 64")
    refused(lambda a: setattr(a, "D", 300), "multiple of 256")
    assert torch.count_nonzero(kc).item() == 0 and torch.count_nonzero(vc).item() == 0
