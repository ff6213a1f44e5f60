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
    """device tables of a few adapters for a list of modules (name -> fan-out); ranks[a][name] = 0 leaves the module alone.
    guard: every A and B gets one more row, of NaN, behind its last rank row: a kernel that reads one rank too many returns NaN"""

    def __init__(self, D, widths, ranks, seed=0, guard=False):
        g = torch.Generator().manual_seed(seed)
        self.D, self.widths, self.n = D, widths, len(ranks)
        self.A, self.B, self.rank, self.scale, self.keep, self.tab = {}, {}, {}, {}, [], {}
        for name, n_out in widths.items():
            pa, pb, rk, sc = [], [], [], []
            for a, rr in enumerate(ranks):
                r = rr.get(name, 0)
                A = torch.randn(max(r, 1), D, generator=g) / D ** 0.5
                B = torch.randn(max(r, 1), n_out, generator=g)
                if guard:
                    A, B = torch.cat([A, torch.full((1, D), float("nan"))]), torch.cat([B, torch.full((1, n_out), float("nan"))])
                A, B = A.to(DEV), B.to(DEV)
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


def cache_tensors(kv, seed, shape=(2, H, CAP, 128)):
    """(kc, vc, plane stride, float64 K, V): random caches [utterances, heads, cap, 128] in the format's own value set"""
    g = torch.Generator().manual_seed(seed)
    k32, v32 = torch.randn(*shape, generator=g), torch.randn(*shape, generator=g)
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


# ------------------------------------------------------------------------------------------------ the branches of lora.hip the cases above do not reach
def launch_apply(a):
    hb.check(hb.lib().dia_lora_apply(C.byref(a), None), "dia_lora_apply")
    torch.cuda.synchronize()


def misaligned_copy(bank, t):
    """the values of t at an address 4 bytes behind a 16-byte boundary (a view buf[1:]); the bank keeps it alive"""
    buf = torch.zeros(t.numel() + 4, dtype=torch.float32, device=DEV)
    view = buf[1: 1 + t.numel()]
    view.copy_(t.reshape(-1))
    assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4
    bank.keep.append(buf)
    return view


@pytest.mark.parametrize("D", [512, 2048])
def test_lora_apply_wide_columns(D):
    """k_lora's column loop behind the first round (`for (c = c0 + LORA_NT; c < nc4; c += LORA_NT)`): a block covers 1024 columns per
    round.  q = 2048: two full rounds; k = 1028: nc4 = 257, one thread alone takes a second round; v = 512: threads without a column.
    Rows of a rank-8 adapter, of no adapter and of a rank-64 adapter; the correction in the columns >= 1024 is far above the bound"""
    torch.manual_seed(D)
    M = 3
    widths = dict(q=2048, k=1028, v=512)
    bank = Bank(D, widths, [dict(q=8, k=8, v=8), dict(q=64, k=64, v=64)], seed=D + 1)
    off = dict(q=128, k=128 + 2048, v=128 + 2048 + 1028 + 64)               # gaps, as in test_lora_apply
    ldo = off["v"] + 512 + 32
    x = (torch.randn(M, D) * 3.0).to(DEV)
    g = (1.0 + 0.1 * torch.randn(D)).to(DEV)
    base = torch.randn(M, ldo).to(DEV)
    out = base.clone()
    slot_adapter = torch.tensor([1, -1, 0], dtype=torch.int32)
    rs = torch.tensor([2, 1, 0], dtype=torch.int32)                         # rank 8, nothing, rank 64
    launch_apply(apply_args(bank, x, g, out, [bank.seg(n, off[n]) for n in "qkv"], slot_adapter.to(DEV), row_slot=rs.to(DEV)))
    got, ref = out.cpu(), base.double().cpu()
    xn = normed(x, g)
    for m, ad in ((0, 0), (2, 1)):
        for n in "qkv":
            ref[m, off[n]: off[n] + widths[n]] += bank.delta(n, ad, xn[m: m + 1])[0]
    adapted = torch.tensor([True, False, True])
    mask = torch.ones(ldo, dtype=torch.bool)
    for n in "qkv":
        mask[off[n]: off[n] + widths[n]] = False
    corr = (ref - base.double().cpu()).abs()
    scale = ref[adapted].abs().max().item()
    for m in (0, 2):
        err = (got[m].double() - ref[m]).abs()
        tail_q, tail_k = slice(off["q"] + 1024, off["q"] + 2048), slice(off["k"] + 1024, off["k"] + 1028)
        print(f"dia_lora_apply wide D={D} row {m} (rank {8 if m == 0 else 64}): max err {err.max().item():.3e}, in q[1024:] {err[tail_q].max().item():.3e}, "
              f"in k[1024:] {err[tail_k].max().item():.3e}; bound {REL * max(1.0, scale):.3e} (scale {scale:.2f}); "
              f"correction in q[1024:] {corr[m, tail_q].max().item():.3f}, in k[1024:] {corr[m, tail_k].max().item():.3f}")
    assert torch.equal(got[~adapted], base.cpu()[~adapted])                 # bitwise
    assert torch.equal(got[:, mask], base.cpu()[:, mask])                   # columns outside the segments
    assert (got.double() - ref)[adapted].abs().max().item() <= REL * max(1.0, scale)
    for m in (0, 2):                                                        # a tail that did nothing would miss the bound by far
        assert corr[m, off["q"] + 1024: off["q"] + 2048].max().item() > 1e-2 * scale
        assert corr[m, off["k"] + 1024: off["k"] + 1028].max().item() > 1e-2 * scale


@pytest.mark.parametrize("D", [256, 768, 1280, 1536, 1792])
def test_lora_apply_in_between_D(D):
    """D / 256 below the instantiation's NX (2, 4 or 8): lora_down's `min(i, nx - 1)` load clamp and its `if (i < nx)` guards, at
    ranks 8 (the prefetched rows alone) and 9 (one round of the loop above them).  x has 64 padding columns of NaN behind D: a sum
    that took anything from behind D is not finite"""
    torch.manual_seed(D)
    M = 2
    bank = Bank(D, dict(q=512), [dict(q=8), dict(q=9)], seed=D + 2, guard=True)
    x = torch.full((M, D + 64), float("nan"))
    x[:, :D] = torch.randn(M, D) * 3.0
    x = x.to(DEV)
    g = (1.0 + 0.1 * torch.randn(D)).to(DEV)
    base = torch.randn(M, 512).to(DEV)
    out = base.clone()
    aos = torch.tensor([0, 1], dtype=torch.int32).to(DEV)
    a = apply_args(bank, x, g, out, [bank.seg("q", 0)], aos, rows_per_slot=1)
    assert a.ldx == D + 64 and a.D == D
    launch_apply(a)
    xn = normed(x[:, :D], g)
    ref = base.double().cpu()
    for m in range(M):
        ref[m] += bank.delta("q", m, xn[m: m + 1])[0]
    got = out.cpu()
    err, scale = (got.double() - ref).abs().max(dim=1).values, ref.abs().max().item()
    print(f"dia_lora_apply D={D} (nx = {D // 256}): max err rank 8 {err[0].item():.3e}, rank 9 {err[1].item():.3e}; bound {REL * max(1.0, scale):.3e} (scale {scale:.2f})")
    assert torch.isfinite(got).all()
    assert err.max().item() <= REL * max(1.0, scale)
    assert (ref - base.double().cpu()).abs().max(dim=1).values.min().item() > 1e-2 * scale


BOUNDARY_RANKS = [1, 4, 5, 7, 8, 9, 12, 63, 64]


def test_lora_rank_boundaries():
    """the last rank inside and the first outside each window: lora_down hands wave w the ranks w and w + 4 from rows requested ahead
    and loops from rank 8; k_lora holds LORA_BPRE = 8 rows of B ahead and loops from 8.  One adapter per rank, selected in turn; row
    r + 1 of every A and B is NaN, so one rank too many is NaN, and one too few misses the bound: each rank's own term is far above it"""
    torch.manual_seed(5)
    D, N = 512, 256
    bank = Bank(D, dict(q=N), [dict(q=r) for r in BOUNDARY_RANKS], seed=9, guard=True)
    x, g = (torch.randn(1, D) * 3.0).to(DEV), (1.0 + 0.1 * torch.randn(D)).to(DEV)
    base = torch.randn(1, N).to(DEV)
    xn = normed(x, g)
    bad = []
    for ad, r in enumerate(BOUNDARY_RANKS):
        out = base.clone()
        aos = torch.tensor([ad], dtype=torch.int32).to(DEV)
        launch_apply(apply_args(bank, x, g, out, [bank.seg("q", 0)], aos, rows_per_slot=1))
        ref = base.double().cpu() + bank.delta("q", ad, xn)
        A, B = bank.A[("q", ad)].double().cpu(), bank.B[("q", ad)].double().cpu()
        assert torch.isnan(A[r]).all() and torch.isnan(B[r]).all() and A.shape[0] == r + 1          # (the sentinel rows)
        last = (bank.scale["q"][ad] * (xn @ A[r - 1: r].t()) @ B[r - 1: r]).abs().max().item()     # what rank r - 1 alone adds
        got = out.cpu()
        err, scale = (got.double() - ref).abs().max().item(), ref.abs().max().item()
        print(f"dia_lora_apply rank {r}: max err {err:.3e}, bound {REL * max(1.0, scale):.3e} (scale {scale:.2f}), the last rank's term {last:.3f}")
        if not (torch.isfinite(got).all() and err <= REL * max(1.0, scale) and last > 1e-2 * scale):
            bad.append(r)
    assert not bad, f"ranks {bad}"


def test_lora_apply_device_side_exits():
    """rows k_lora must leave alone for a reason only the device sees: a slot >= n_slots, a negative slot, an adapter id == n_adapters
    (lora_adapter), a device rank of 65 under max_rank = 64 (`r > LORA_RMAX`), an A at 4 bytes behind a 16-byte boundary
    (lora_tables_ok); bitwise.  The healthy row between them meets the bound.  Behind every refused index lies a healthy adapter with
    tables of its own (one more slot, one more adapter, 65 rank rows, a full misaligned A), and in front of adapter_of_slot one more
    entry: a kernel without one of the checks changes the row, within memory of this test"""
    torch.manual_seed(13)
    D, M, N = 512, 6, 512
    bank = Bank(D, dict(q=N), [dict(q=8), dict(q=65), dict(q=8), dict(q=8)], seed=17)
    n_slots, n_adapters = 5, 3                                              # declared; one more of each exists
    bank.tab["q"][0][2] = misaligned_copy(bank, bank.A[("q", 2)]).data_ptr()
    aos_buf = torch.tensor([0, 0, 3, 1, 2, -1, 0], dtype=torch.int32).to(DEV)       # [-1] and [n_slots] name the healthy adapter
    aos = aos_buf[1:]
    rs = torch.tensor([n_slots, -1, 1, 2, 3, 0], dtype=torch.int32)         # beyond, negative, id == n_adapters, rank 65, misaligned A, healthy
    x, g = (torch.randn(M, D) * 3.0).to(DEV), (1.0 + 0.1 * torch.randn(D)).to(DEV)
    base = torch.randn(M, N).to(DEV)
    out = base.clone()
    a = apply_args(bank, x, g, out, [bank.seg("q", 0, max_rank=64)], aos, row_slot=rs.to(DEV))
    a.n_slots, a.n_adapters = n_slots, n_adapters
    launch_apply(a)
    got = out.cpu()
    ref = base.double().cpu()[5] + bank.delta("q", 0, normed(x, g)[5:6])[0]
    err, scale = (got[5].double() - ref).abs().max().item(), ref.abs().max().item()
    changed = [m for m in range(5) if not torch.equal(got[m], base.cpu()[m])]
    print(f"dia_lora_apply exits: rows changed {changed} of 0..4; healthy row max err {err:.3e}, bound {REL * max(1.0, scale):.3e} (scale {scale:.2f})")
    assert torch.equal(got[:5], base.cpu()[:5])                             # bitwise
    assert err <= REL * max(1.0, scale)
    assert (ref - base.double().cpu()[5]).abs().max().item() > 1e-2 * scale


# the cross K/V caches again
KV_DTYPE = {"f32": 0, "bf16": 1, "bf16x2": 2}


def v_blocked(vc, kv):
    """a V cache [(2 planes,) utterances, heads, cap, 128] re-laid as [cap / 32][128][32] per head, in the same shape"""
    src = vc if kv == "bf16x2" else vc[None]
    out = torch.stack([lay.v_to_blocked(p_.cpu()).reshape(p_.shape) for p_ in src]).to(DEV)
    return out if kv == "bf16x2" else out[0]


def v_unblocked(t, kv):
    src = t if kv == "bf16x2" else t[None]
    u = torch.stack([lay.v_from_blocked(p_.cpu().reshape(*p_.shape[:-2], p_.shape[-2] // 32, 128, 32)) for p_ in src])
    return u if kv == "bf16x2" else u[0]


class CrossKv:
    """caches of `shape` = (utterances, heads, cap, 128) in one format, the RoPE tables, and dia_lora_crosskv on them"""

    def __init__(self, kv, blocked, shape, seed, rope_rows=None):
        self.kv, self.blocked, self.shape = kv, blocked, shape
        self.kc, self.vc, self.plane, self.k_ref, self.v_ref = cache_tensors(kv, seed, shape)
        if blocked:
            self.vc = v_blocked(self.vc, kv)
        self.k0, self.v0 = self.kc.clone(), self.vc.clone()
        self.rope_rows = rope_rows or shape[2] + 1
        self.cos, self.sin = (t.to(DEV) for t in lay.rope_tables(self.rope_rows, 128, 1, 10000))

    def args(self, bank, x, g, aos, n_slots, n_adapters, M, row_b=None, seg_off=None, kv_batch_index=0, max_rank=None):
        a = hb.LoraCrossKvArgs()
        a.x, a.ldx, a.D, a.gain, a.eps, a.M = x.data_ptr(), x.shape[1], bank.D, g.data_ptr(), EPS, M
        a.row_b, a.seg_off, a.adapter_of_slot, a.n_slots, a.n_adapters = hb.ptr(row_b), hb.ptr(seg_off), aos.data_ptr(), n_slots, n_adapters
        a.k, a.v = bank.seg("k", 0, max_rank), bank.seg("v", 0, max_rank)
        a.kc, a.vc, a.kv_dtype, a.kv_heads, a.kv_cap = self.kc.data_ptr(), self.vc.data_ptr(), KV_DTYPE[self.kv], self.shape[1], self.shape[2]
        a.kv_batch_index, a.kv_vblocked, a.rope_rows, a.kv_plane_stride = kv_batch_index, self.blocked, self.rope_rows, self.plane
        a.cos_t, a.sin_t = self.cos.data_ptr(), self.sin.data_ptr()
        return a

    def raw(self):
        """(K, V now, K, V before) as stored, [planes, utterances, heads, cap, 128] on the host, V out of the blocked layout (a permutation)"""
        v, v0 = (v_unblocked(self.vc, self.kv), v_unblocked(self.v0, self.kv)) if self.blocked else (self.vc.cpu(), self.v0.cpu())
        return tuple(t.reshape(-1, *self.shape) for t in (self.kc.cpu(), v, self.k0.cpu(), v0))

    def values(self):
        """(K, V now) in float64 [utterances, heads, cap, 128]"""
        return read_cache(self.kc, self.kv), read_cache(v_unblocked(self.vc, self.kv) if self.blocked else self.vc, self.kv)

    def delta(self, bank, ad, xn, pos):
        """float64 (RoPE(dK), dV) [heads, rows, 128] of adapter ad for the normed rows xn at the cache positions pos"""
        heads = self.shape[1]
        dk, dv = bank.delta("k", ad, xn).reshape(-1, heads, 128), bank.delta("v", ad, xn).reshape(-1, heads, 128)
        c, s = self.cos.double().cpu()[pos][:, None, :], self.sin.double().cpu()[pos][:, None, :]
        rk = torch.cat([dk[..., :64] * c - dk[..., 64:] * s, dk[..., :64] * s + dk[..., 64:] * c], dim=-1)
        return rk.permute(1, 0, 2), dv.permute(1, 0, 2)

    def close_enough(self, tag, got, want, before):
        """prints the figures of one updated block of K or V (float64) and returns whether it meets the format's bound and moved"""
        moved = (want - before).abs().max().item() > 0.05 * want.abs().max().item()
        if self.kv == "bf16":
            worst = ((got - want.float().bfloat16().double()).abs() / bf16_ulp(want)).max().item()      # bf16(base + delta), the sum in float64
            print(f"dia_lora_crosskv {self.kv} blocked={self.blocked} {tag}: worst error {worst:.3f} bf16 ulp")
            return moved and worst <= 1.0
        err, scale = (got - want).abs().max().item(), want.abs().max().item()
        print(f"dia_lora_crosskv {self.kv} blocked={self.blocked} {tag}: max err {err:.3e}, bound {REL * max(1.0, scale):.3e} (scale {scale:.2f})")
        return moved and err <= REL * max(1.0, scale)


def same_outside(now, before, b, rows):
    """bitwise equality of a whole cache allocation [planes, utterances, heads, cap, 128] outside keys `rows` of utterance b"""
    now, before = now.clone(), before.clone()
    now[:, b, :, rows], before[:, b, :, rows] = 0, 0
    return torch.equal(now, before)


@pytest.mark.parametrize("kvb", [0, 2])
@pytest.mark.parametrize("M", [1, 33, CAP])
@pytest.mark.parametrize("kv,blocked", [("f32", 0), ("bf16", 1), ("bf16x2", 1)])
def test_lora_crosskv_single_utterance(kv, blocked, M, kvb):
    """row_b = seg_off = NULL: the M rows are positions 0 .. M - 1 of utterance kv_batch_index (`b = p.kv_batch_index, pos = m`), whose
    slot names the adapter.  M = 33: one key in the second V block; M = CAP: the last position of the last block.  The other two
    utterances and the keys >= M stay bitwise"""
    torch.manual_seed(M + kvb)
    bank = Bank(E, dict(k=H * 128, v=H * 128), [dict(k=8, v=8), dict(k=5, v=16)], seed=11)
    ck = CrossKv(kv, blocked, (3, H, CAP, 128), seed=21)
    x, g = (torch.randn(M, E) * 2.0).to(DEV), (1.0 + 0.1 * torch.randn(E)).to(DEV)
    slot_adapter = [1, -1, 0]
    aos = torch.tensor(slot_adapter, dtype=torch.int32).to(DEV)
    a = ck.args(bank, x, g, aos, 3, 2, M, kv_batch_index=kvb)
    hb.check(hb.lib().dia_lora_crosskv(C.byref(a), None), "dia_lora_crosskv")
    torch.cuda.synchronize()
    (k_got, v_got), (k_raw, v_raw, k_raw0, v_raw0) = ck.values(), ck.raw()
    dk, dv = ck.delta(bank, slot_adapter[kvb], normed(x, g), torch.arange(M))
    ok = [ck.close_enough(f"one utterance b={kvb} M={M} {n}", got[kvb, :, :M], ref[kvb, :, :M] + d, ref[kvb, :, :M])
          for n, got, ref, d in (("K", k_got, ck.k_ref, dk), ("V", v_got, ck.v_ref, dv))]
    assert same_outside(k_raw, k_raw0, kvb, slice(0, M)) and same_outside(v_raw, v_raw0, kvb, slice(0, M))
    assert all(ok)


def test_lora_crosskv_single_utterance_refusals():
    """the host check of the one-utterance form: kv_batch_index outside the slots, more rows than the cache holds; nothing written"""
    bank = Bank(E, dict(k=H * 128, v=H * 128), [dict(k=8, v=8)])
    ck = CrossKv("f32", 0, (3, H, CAP, 128), seed=22)
    x, g = torch.randn(CAP + 1, E).to(DEV), torch.ones(E).to(DEV)
    aos = torch.zeros(3, dtype=torch.int32).to(DEV)
    L = hb.lib()
    for M, kvb in ((4, -1), (4, 3), (CAP + 1, 0)):
        a = ck.args(bank, x, g, aos, 3, 1, M, kv_batch_index=kvb)
        rc, msg = L.dia_lora_crosskv(C.byref(a), None), L.dia_last_error().decode()
        print(f"dia_lora_crosskv one utterance M={M} kv_batch_index={kvb}: {rc} {msg!r}")
        assert rc == -1
        assert "kv_batch_index outside the slots or more rows than kv_cap" in msg
    torch.cuda.synchronize()
    assert torch.equal(ck.kc, ck.k0) and torch.equal(ck.vc, ck.v0)


@pytest.mark.parametrize("heads", [16, 20])
@pytest.mark.parametrize("kv,blocked", [("bf16", 1), ("f32", 0)])
def test_lora_crosskv_many_heads(kv, blocked, heads):
    """k_lora_crosskv's item loop (`for (it = threadIdx.x; it < kv_heads * 16; it += LORA_NT)`): 16 heads (Dia-1.6B) are exactly one
    round of the 256 threads, 20 heads give 64 threads a second one.  One packed utterance of 5 rows, the second of two in the caches;
    each head is held to the bound by itself"""
    torch.manual_seed(heads)
    cap, n, off, Mp = 32, 5, 3, 12
    bank = Bank(E, dict(k=heads * 128, v=heads * 128), [dict(k=8, v=5)], seed=heads)
    ck = CrossKv(kv, blocked, (2, heads, cap, 128), seed=23)
    x, g = (torch.randn(Mp, E) * 2.0).to(DEV), (1.0 + 0.1 * torch.randn(E)).to(DEV)
    row_b = torch.full((Mp,), -1, dtype=torch.int32)
    row_b[off: off + n] = 1
    rb_d, so_d = row_b.to(DEV), torch.tensor([0, off], dtype=torch.int32).to(DEV)
    aos = torch.tensor([-1, 0], dtype=torch.int32).to(DEV)
    a = ck.args(bank, x, g, aos, 2, 1, Mp, row_b=rb_d, seg_off=so_d)
    hb.check(hb.lib().dia_lora_crosskv(C.byref(a), None), "dia_lora_crosskv")
    torch.cuda.synchronize()
    (k_got, v_got), (k_raw, v_raw, k_raw0, v_raw0) = ck.values(), ck.raw()
    dk, dv = ck.delta(bank, 0, normed(x, g)[off: off + n], torch.arange(n))
    bad = [(name, h) for name, got, ref, d in (("K", k_got, ck.k_ref, dk), ("V", v_got, ck.v_ref, dv)) for h in range(heads)
           if not ck.close_enough(f"{heads} heads, {name} head {h}", got[1, h, :n], ref[1, h, :n] + d[h], ref[1, h, :n])]
    assert same_outside(k_raw, k_raw0, 1, slice(0, n)) and same_outside(v_raw, v_raw0, 1, slice(0, n))
    assert not bad, bad


@pytest.mark.parametrize("kv,blocked", [("f32", 0), ("bf16", 1)])
def test_lora_crosskv_device_side_exits(kv, blocked):
    """packed rows k_lora_crosskv must drop: positions >= kv_cap of an utterance packed 40 rows long (CAP = 32; the RoPE tables cover
    them, so `pos >= p.kv_cap` alone stands in the way), a row_b entry == n_slots (checked before seg_off[b] is read), an adapter
    with a device rank of 65 under max_rank = 64, an adapter whose B lies 4 bytes behind a 16-byte boundary.  The first 32 rows of the
    long utterance meet the bound; everything else in the K and V allocations is bitwise what it was.  The allocations hold one more
    utterance, slot and seg_off entry than declared, and the refused adapters full tables: a kernel without one of the checks
    writes inside them, where the comparison sees it"""
    torch.manual_seed(29)
    cap, n_slots, Mp = 32, 3, 64
    bank = Bank(E, dict(k=H * 128, v=H * 128), [dict(k=8, v=5), dict(k=65, v=65), dict(k=8, v=8)], seed=31)
    for n in "kv":
        bank.tab[n][1][2] = misaligned_copy(bank, bank.B[(n, 2)]).data_ptr()
    ck = CrossKv(kv, blocked, (n_slots + 1, H, cap, 128), seed=24, rope_rows=64)
    lens, offs = [40, 5, 6, 1], [0, 40, 48, 56]                            # utterance 3 does not exist: n_slots = 3
    row_b = torch.full((Mp,), -1, dtype=torch.int32)
    for b in range(4):
        row_b[offs[b]: offs[b] + lens[b]] = b
    x, g = (torch.randn(Mp, E) * 2.0).to(DEV), (1.0 + 0.1 * torch.randn(E)).to(DEV)
    rb_d, so_d = row_b.to(DEV), torch.tensor(offs, dtype=torch.int32).to(DEV)      # n_slots + 1 entries
    aos = torch.tensor([0, 1, 2, 0], dtype=torch.int32).to(DEV)             # healthy, rank 65, misaligned B; [n_slots]: healthy
    a = ck.args(bank, x, g, aos, n_slots, 3, Mp, row_b=rb_d, seg_off=so_d, max_rank=64)
    hb.check(hb.lib().dia_lora_crosskv(C.byref(a), None), "dia_lora_crosskv")
    torch.cuda.synchronize()
    (k_got, v_got), (k_raw, v_raw, k_raw0, v_raw0) = ck.values(), ck.raw()
    for name, now, before in (("K", k_raw, k_raw0), ("V", v_raw, v_raw0)):
        diff = (now != before).any(dim=4).any(dim=0)                        # [utterance, head, key]
        print(f"dia_lora_crosskv exits {kv} {name}: keys changed per utterance {[sorted(set(diff[b].nonzero()[:, 1].tolist())) for b in range(4)]}")
    dk, dv = ck.delta(bank, 0, normed(x, g)[:cap], torch.arange(cap))
    ok = [ck.close_enough(f"exits {n}", got[0], ref[0] + d, ref[0]) for n, got, ref, d in (("K", k_got, ck.k_ref, dk), ("V", v_got, ck.v_ref, dv))]
    assert same_outside(k_raw, k_raw0, 0, slice(0, cap)) and same_outside(v_raw, v_raw0, 0, slice(0, cap))
    assert all(ok)
