"""dia_attn where the decode engine really launches it: the full 3072-key capacity (13-24 key splits, the second merge
round of attn_finish), ragged lengths within one launch, consecutive steps on the same caches, GQA groups 1 and 2,
cross-attention over texts longer than one workgroup takes, and the attn_gpw / attn_gpw_cross knobs.

Every launch goes through one harness (`Attn`, `run_attn`) and is compared with one float64 restatement: RoPE on q and
on the new k, then softmax(q.K^T / sqrt(128)).V over the values the cache actually holds (bf16: the rounded values,
bf16x2: hi + lo), so only the kernel's arithmetic is under test.  Bound: max abs error <= 2e-5 for randn q/K/V, the
figure of every attention test in test_gpu_kernels.py; cache appends keep the bounds of test_attn_self.

Beyond every row's length the caches hold +-1e4 (finite: the kernel's contract), so a masking slip or a stale load of
the slot written this step shows as a gross error.  The scratch slabs are pre-filled with a marker and the number of
slabs each (row, kv head) pair published is compared with `slabs()`, the Python restatement of dia_attn's split rule:
a heuristic change cannot silently turn a 24-slab case into a one-round case, and a split that is numerically harmless
(a text of 256 bytes handed off through slabs, attn_gpw ignored) is still seen.  cur[] is allocated with one entry per
ROW (the entries past the batch repeat it), so a row-indexing slip reads a valid length instead of foreign memory."""
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from dia_hip import binding as hb
from dia_hip import layout as lay

KVDS = ("f32", "bf16", "bf16x2")
KVD_CODE = {"f32": hb.KV_F32, "bf16": hb.KV_BF16, "bf16x2": hb.KV_BF16X2}
BIG = 1.0e4                     # what the caches hold beyond a row's length
SENTINEL = 5.0                  # what the output buffer holds before a launch (exact in one bf16 plane)
MARK = -7777.0                  # what the scratch slabs hold before a launch
SLAB = 2 * 8 + 4 * 128          # floats per (pair, split): attn.hip
TOL = 2e-5
SCALE = 1.0 / math.sqrt(128.0)


def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    return torch.device("cuda:0")


# ---- dia_attn's split rule, restated ------------------------------------------------------------------------------
def launch_nz(n_rows, kvh, kv_cap, attn_nz=0):
    """grid z of a launch: ~512 workgroups, or the attn_nz knob; at most one split per 128 keys of capacity"""
    nz = attn_nz if attn_nz > 0 else -(-512 // (n_rows * kvh))
    return max(1, min(nz, -(-kv_cap // 128)))


def slabs(kvd, nkeys, nz, gpw=1):
    """workgroups that take keys of one (row, kv head) pair; they hand off through slabs when there are 2 or more"""
    if kvd == "f32":                                   # k_attn: 64-key units
        return min(nz, max(1, -(-nkeys // 64)))
    ngran = -(-nkeys // 32)                            # k_attn_mfma: 32-key granules, 4 waves x gpw per workgroup
    if ngran <= 8:
        gpw = max(gpw, 2)                              # up to 256 keys stay in one workgroup
    return min(nz, max(1, -(-ngran // (4 * gpw))))


# ---- harness ------------------------------------------------------------------------------------------------------
class Attn:
    """caches of one attention layer and everything a launch needs.  `valid[r]` keys of kv row r hold data (randn, or
    the given K / V), the rest +-BIG.  SELF: kv rows = query rows; CROSS: kv rows = utterances."""

    def __init__(self, mode, kvd, G, KVH, kv_cap, valid, *, seed, K=None, V=None):
        d = dev()
        self.mode, self.kvd, self.G, self.KVH, self.T, self.n = mode, kvd, G, KVH, kv_cap, len(valid)
        self.QH = G * KVH
        self.two, self.blocked = kvd == "bf16x2", kvd != "f32"
        gen = torch.Generator().manual_seed(seed)
        self.gen = gen
        shape = (self.n, KVH, kv_cap, 128)
        kf = K.clone().float() if K is not None else torch.randn(shape, generator=gen)
        vf = V.clone().float() if V is not None else torch.randn(shape, generator=gen)
        for t in (kf, vf):
            sign = torch.randint(0, 2, shape, generator=gen).float() * 2 - 1
            for r, n_valid in enumerate(valid):
                t[r, :, n_valid:] = BIG * sign[r, :, n_valid:]
        kf, vf = kf.to(d), vf.to(d)
        if self.two:                                    # every value as hi + lo bf16 in two planes
            khi, vhi = kf.bfloat16(), vf.bfloat16()
            klo, vlo = (kf - khi.float()).bfloat16(), (vf - vhi.float()).bfloat16()
            self.kc = torch.stack([khi, klo]).contiguous()
            self.vc = torch.stack([lay.v_to_blocked(vhi), lay.v_to_blocked(vlo)]).contiguous()
        elif self.blocked:
            self.kc, self.vc = kf.bfloat16().contiguous(), lay.v_to_blocked(vf.bfloat16())
        else:
            self.kc, self.vc = kf.contiguous(), vf.contiguous()
        self.cos, self.sin = [t.to(d) for t in lay.rope_tables(kv_cap + 1, 128, 1, 10000)]
        self.scr = torch.empty(hb.lib().dia_attn_scratch_floats(self.n, KVH, kv_cap), device=d)
        self.tk = torch.zeros(self.n * KVH, dtype=torch.int32, device=d)
        self.max_chunks = -(-kv_cap // 128)
        assert self.scr.numel() == self.n * KVH * self.max_chunks * SLAB

    def randn(self, *shape):
        return torch.randn(*shape, generator=self.gen).to(dev())

    def draw_qkv(self, curs):
        """fresh fused q|k|v rows for a SELF launch at these lengths (bf16 caches: see rounding_ties)"""
        pos = torch.tensor([c for c in curs for _ in (0, 1)], device=dev())
        for _ in range(100):
            qkv = self.randn(2 * len(curs), (self.QH + 2 * self.KVH) * 128)
            k = qkv.double().reshape(len(pos), -1, 128)[:, self.QH: self.QH + self.KVH]
            if self.kvd != "bf16" or rounding_ties(k, self.cos, self.sin, pos) == 0:
                return qkv
        raise AssertionError("no tie-free draw")

    def planes(self):
        """copies of the caches as stored, V unblocked: K, V [planes, kv row, kv head, key, 128]"""
        if self.two:
            return self.kc.clone(), torch.stack([lay.v_from_blocked(self.vc[0]), lay.v_from_blocked(self.vc[1])])
        v = lay.v_from_blocked(self.vc) if self.blocked else self.vc.clone()
        return self.kc.clone()[None], v[None]

    @staticmethod
    def held(planes):
        """the value a cache holds: the sum of its planes, float64"""
        return planes.double().sum(dim=0)

    def launch(self, q, *, curs, lens=None, n_rows=None, head_map=None, act_f32=0, rope_rows=None):
        """one dia_attn call.  SELF: q = fused q|k|v rows, curs per utterance (2 rows each).  CROSS: q rows of 2 per
        utterance, curs = decoder positions, lens = text lengths.  Returns the output [16 * mtiles, QH, 128] float64
        (rows / head positions the launch did not write keep SENTINEL) and the slabs published per pair."""
        d = dev()
        cross = self.mode == hb.ATTN_CROSS
        n_rows = n_rows if n_rows is not None else self.n
        out_rows = 2 * n_rows if cross else n_rows
        assert q.shape[0] == out_rows and n_rows <= self.n and q.is_contiguous()
        assert all(0 <= c <= self.T for c in curs) and (lens is None or all(0 <= n <= self.T for n in lens))
        assert len(curs) == (n_rows if cross else n_rows // 2) and (not cross or len(lens) == n_rows)
        assert cross or min(curs) >= 1
        cur_t = torch.tensor(list(curs) * 2, dtype=torch.int32, device=d)          # one entry per row (module docstring)
        len_t = torch.tensor(list(lens), dtype=torch.int32, device=d) if cross else None
        mt, kt = (out_rows + 15) // 16, self.QH * 4
        if act_f32:
            P = torch.full((mt, kt, 64, 8), SENTINEL, dtype=torch.float32, device=d)
        else:
            P = lay.pack_planes(torch.full((mt * 16, self.QH * 128), SENTINEL, device=d))
        hm = None if head_map is None else torch.tensor(head_map, dtype=torch.int32, device=d)
        self.scr.fill_(MARK)
        self.raw_before = (self.kc.clone(), self.vc.clone())
        a = hb.AttnArgs()
        a.mode, a.kv_dtype, a.n_kv_heads, a.group, a.n_rows, a.kv_cap = self.mode, KVD_CODE[self.kvd], self.KVH, self.G, n_rows, self.T
        if cross:
            a.q, a.ldq, a.q_off = hb.ptr(q), self.QH * 128, 0
            assert q.shape[1] == self.QH * 128
        else:
            a.q, a.ldq, a.q_off, a.k_off, a.v_off = hb.ptr(q), (self.QH + 2 * self.KVH) * 128, 0, self.QH * 128, (self.QH + self.KVH) * 128
            assert q.shape[1] == (self.QH + 2 * self.KVH) * 128
        a.kc, a.vc, a.cur, a.len = hb.ptr(self.kc), hb.ptr(self.vc), hb.ptr(cur_t), hb.ptr(len_t)
        a.cos_t, a.sin_t = hb.ptr(self.cos), hb.ptr(self.sin)
        a.rope_rows = rope_rows if rope_rows is not None else self.cos.shape[0]        # the host check is live
        a.P, a.p_plane_stride, a.p_ktiles, a.act_f32 = hb.ptr(P), mt * kt * 512, kt, act_f32
        a.scratch, a.tickets, a.head_map = hb.ptr(self.scr), hb.ptr(self.tk), hb.ptr(hm)
        a.v_blocked = int(self.blocked)
        a.kv_plane_stride = self.kc[0].numel() if self.two else 0
        hb.check(hb.lib().dia_attn(C.byref(a), None), "dia_attn")
        torch.cuda.synchronize()
        assert (self.tk == 0).all(), "tickets not back at 0 after the launch"
        if act_f32:
            out = lay.unpack_f32_tiles(P, mt * 16, self.QH * 128)
        else:
            out = lay.unpack_planes(P, mt * 16, self.QH * 128)
        ml = self.scr.reshape(self.n * self.KVH, self.max_chunks, SLAB)[:, :, :2]
        written = (ml != MARK).any(dim=-1)                             # (max, sum) of query head 0 of the pair
        nslab = written.sum(dim=1)
        assert (written == (torch.arange(self.max_chunks, device=d)[None] < nslab[:, None])).all(), "slabs not published in split order"
        return out.double().reshape(mt * 16, self.QH, 128), nslab.reshape(self.n, self.KVH).cpu()


def run_attn(mode, kvd, G, KVH, curs, kv_cap, *, lens=None, head_map=None, act_f32=0, rope_rows=None, seed=0, K=None, V=None, q=None):
    """build the caches for one launch (SELF: cur - 1 keys of data per row, CROSS: len keys), launch, return
    (case, q, output, slabs per pair, cache planes before the launch)"""
    cross = mode == hb.ATTN_CROSS
    valid = list(lens) if cross else [c - 1 for c in curs for _ in (0, 1)]
    case = Attn(mode, kvd, G, KVH, kv_cap, valid, seed=seed, K=K, V=V)
    if q is None:
        q = case.randn(2 * len(curs), G * KVH * 128) if cross else case.draw_qkv(curs)
    before = case.planes()
    out, nslab = case.launch(q, curs=curs, lens=lens, head_map=head_map, act_f32=act_f32, rope_rows=rope_rows)
    return case, q, out, nslab, before


# ---- float64 reference --------------------------------------------------------------------------------------------
def rope64(x, cos, sin, pos):
    """x [rows, heads, 128] float64, pos [rows]"""
    c, s = cos[pos].double()[:, None, :], sin[pos].double()[:, None, :]
    return torch.cat([x[..., :64] * c - x[..., 64:] * s, x[..., :64] * s + x[..., 64:] * c], dim=-1)


def rounding_ties(x, cos, sin, pos):
    """how many of the k rows x [rows, heads, 128] (float64, before RoPE) land, after RoPE at pos, on a bf16 rounding
    tie within fp32 error.  A statement about INPUTS: a bf16 cache's appended k is compared bit-exactly with
    bf16(float64 RoPE), but the kernel rounds its fp32 RoPE, whose two products and one sum are each off by up to 2^-24
    relative, 2^-23 * (|x1 c| + |x2 s|) in all.  Where the exact value lies that close to the midpoint of two bf16
    numbers, the two roundings may differ by one bf16 step without either being wrong (about 5 in 10^5 values).  The
    harness draws bf16 cases' rows again until there is no such value (`Attn.draw_qkv`), so that the exact comparison
    means what it says."""
    c, s = cos[pos].double().abs()[:, None, :], sin[pos].double().abs()[:, None, :]
    x1, x2 = x[..., :64].abs(), x[..., 64:].abs()
    margin = 1.01 * 2.0 ** -23 * torch.cat([x1 * c + x2 * s, x1 * s + x2 * c], dim=-1)
    v = rope64(x, cos, sin, pos).abs().clamp_min(1e-30)
    step = 2.0 ** (torch.floor(torch.log2(v)) - 7)               # spacing of bf16 numbers around v
    dist = ((v / step) % 1.0 - 0.5).abs() * step
    return int((dist <= margin).sum())


def attn64(qh, K, V):
    """qh [KVH, G, 128], K / V [KVH, keys, 128] float64 -> [KVH * G, 128]"""
    p = torch.softmax(qh @ K.transpose(-1, -2) * SCALE, dim=-1)
    return (p @ V).reshape(-1, 128)


def check_self(case, qkv, curs, out, nslab, before, *, nz, gpw=1, head_map=None):
    """one SELF launch: slot cur - 1 of every launched row holds RoPE(k), v; every other cache element is bit-identical;
    the output is attention over keys 0..cur-1 of what the cache holds; the pairs were split as the rule says.
    Returns the worst output error."""
    d = dev()
    R, G, KVH, QH, T = 2 * len(curs), case.G, case.KVH, case.QH, case.T
    pos = torch.tensor([c for c in curs for _ in (0, 1)], device=d)
    rows = torch.arange(R, device=d)
    k_after, v_after = case.planes()
    # -- untouched: everything but (row, slot), plane by plane, bit by bit
    touched = torch.zeros(case.n, T, dtype=torch.bool, device=d)
    touched[rows, pos - 1] = True
    bits = torch.int32 if case.kvd == "f32" else torch.int16
    for new, old in ((k_after, before[0]), (v_after, before[1])):
        changed = (new.view(bits) != old.view(bits)).any(dim=-1).any(dim=0).any(dim=1)          # [kv row, key]
        assert not (changed & ~touched).any(), "a cache element other than the new slot changed"
    # -- appended slot (state.py:99-103), the bounds of test_attn_self
    Kh, Vh = case.held(k_after), case.held(v_after)
    x = qkv.double().reshape(R, QH + 2 * KVH, 128)
    knew, vnew = rope64(x[:, QH: QH + KVH], case.cos, case.sin, pos), x[:, QH + KVH:]
    if case.kvd == "bf16":
        assert rounding_ties(x[:, QH: QH + KVH], case.cos, case.sin, pos) == 0, "inputs: a roped k on a bf16 rounding tie"
        knew, vnew = knew.float().bfloat16().double(), vnew.float().bfloat16().double()
    tol_new = 6e-5 if case.two else 1e-6               # hi + lo keeps 16 significand bits of values up to ~8
    ek = (Kh[rows, :, pos - 1] - knew).abs().max().item()
    ev = (Vh[rows, :, pos - 1] - vnew).abs().max().item()
    assert ek <= (1e-6 if case.kvd == "f32" else 0.0) + tol_new, ek
    assert ev <= tol_new, ev
    # -- output
    q = rope64(x[:, :QH], case.cos, case.sin, pos)
    live = [h for h in range(QH) if head_map is None or head_map[h] >= 0]
    where = live if head_map is None else [head_map[h] for h in live]
    worst = torch.zeros((), dtype=torch.float64, device=d)
    for r in range(R):
        n = curs[r // 2]
        ref = attn64(q[r].reshape(KVH, G, 128), Kh[r, :, :n], Vh[r, :, :n])
        worst = torch.maximum(worst, (out[r, where] - ref[live]).abs().max())
    worst, nlive = worst.item(), len(live)
    assert (out[R:] == SENTINEL).all() and (out[:, nlive:] == SENTINEL).all(), "rows / head positions outside the launch were written"
    # -- split rule
    for r in range(R):
        want = slabs(case.kvd, curs[r // 2], nz, gpw)
        assert (nslab[r] == (want if want > 1 else 0)).all(), (r, curs[r // 2], nslab[r].tolist(), want)
    assert (nslab[R:] == 0).all()
    return worst


def check_cross(case, q, curs, lens, out, nslab, before, *, nz, gpw=1, head_map=None):
    """one CROSS launch: caches untouched, conditional rows = attention over the first len keys (0 for an empty text),
    unconditional rows exactly 0 and written, split as the rule says.  Returns the worst output error."""
    d = dev()
    B, H = len(lens), case.QH
    k_after, v_after = case.planes()
    assert torch.equal(k_after, before[0]) and torch.equal(v_after, before[1])
    Kh, Vh = case.held(k_after), case.held(v_after)
    qc = rope64(q.double().reshape(2 * B, H, 128)[1::2], case.cos, case.sin, torch.tensor(list(curs), device=d))
    live = [h for h in range(H) if head_map is None or head_map[h] >= 0]
    where = live if head_map is None else [head_map[h] for h in live]
    worst = torch.zeros((), dtype=torch.float64, device=d)
    for b in range(B):
        ref = attn64(qc[b].reshape(H, 1, 128), Kh[b, :, :lens[b]], Vh[b, :, :lens[b]]) if lens[b] else torch.zeros(H, 128, dtype=torch.float64, device=d)
        worst = torch.maximum(worst, (out[2 * b + 1, where] - ref[live]).abs().max())
        assert (out[2 * b, where] == 0).all(), f"unconditional row of utterance {b} (len {lens[b]}): not exactly 0"
        if lens[b] == 0:
            assert (out[2 * b + 1, where] == 0).all()
        want = slabs(case.kvd, lens[b], nz, gpw)
        for h in range(H):
            assert nslab[b, h] == (want if want > 1 and h in live else 0), (b, h, lens[b], nslab[b].tolist(), want)
    assert (out[2 * B:] == SENTINEL).all() and (out[:, len(live):] == SENTINEL).all()
    return worst.item()


def report(name, worst):
    print(f"[attn-decode] {name}: worst abs error {worst:.3e} (bound {TOL:.0e})")
    assert worst <= TOL, worst


# ---- A. product capacity ------------------------------------------------------------------------------------------
CAP = 3072                       # Dia-1.6B audio_length
A_MERGES = {("f32", 769): 13, ("f32", 1537): 24, ("f32", 1600): 24, ("f32", 3071): 24, ("f32", 3072): 24,
            ("bf16", 1537): 13, ("bf16", 3072): 24, ("bf16x2", 1537): 13, ("bf16x2", 3072): 24}


def self_twice(kvd, G, KVH, curs, kv_cap, *, nz, gpw=1, seed, K=None, V=None, q=None):
    """case A's protocol: launch, check, restore the caches, launch again (tickets and slabs of the first launch
    behind it), check again; the two outputs are the same bits"""
    case, q, out, nslab, before = run_attn(hb.ATTN_SELF, kvd, G, KVH, curs, kv_cap, seed=seed, K=K, V=V, q=q)
    worst = check_self(case, q, curs, out, nslab, before, nz=nz, gpw=gpw)
    kc1, vc1 = case.kc.clone(), case.vc.clone()
    case.kc.copy_(case.raw_before[0]); case.vc.copy_(case.raw_before[1])
    out2, nslab2 = case.launch(q, curs=curs)
    worst = max(worst, check_self(case, q, curs, out2, nslab2, before, nz=nz, gpw=gpw))
    assert torch.equal(out, out2) and torch.equal(case.kc, kc1) and torch.equal(case.vc, vc1), "second launch differs from the first"
    return worst


@pytest.mark.parametrize("kvd", KVDS)
@pytest.mark.parametrize("cur", [769, 1537, 1600, 3071, 3072])
def test_self_product_capacity(kvd, cur):
    """A: batch 1 of Dia-1.6B (2 rows, 4 kv heads x group 4) at capacity 3072 with the default heuristics: up to 24
    slabs per pair, merged in two rounds of 12."""
    nz = launch_nz(2, 4, CAP)
    assert nz == 24
    if (kvd, cur) in A_MERGES:                        # the second merge round must be what runs here
        assert slabs(kvd, cur, nz) == A_MERGES[(kvd, cur)] >= 13
    report(f"A {kvd} cur={cur} slabs={slabs(kvd, cur, nz)}", self_twice(kvd, 4, 4, [cur], CAP, nz=nz, seed=cur))


@pytest.mark.parametrize("kvd", KVDS)
@pytest.mark.parametrize("attn_nz", [24, 13])
def test_self_product_capacity_forced_splits(kvd, attn_nz, tuning):
    """A: the same at cur = 3072 with attn_nz stated: 24, and 13 = one slab in the second merge round"""
    tuning("attn_nz", attn_nz)
    nz = launch_nz(2, 4, CAP, attn_nz)
    assert nz == attn_nz and slabs(kvd, CAP, nz) == attn_nz >= 13
    report(f"A {kvd} cur={CAP} attn_nz={attn_nz}", self_twice(kvd, 4, 4, [CAP], CAP, nz=nz, seed=attn_nz))


@pytest.mark.parametrize("kvd", ["bf16", "bf16x2"])
@pytest.mark.parametrize("gpw", [2, 3])
def test_self_product_capacity_gpw(kvd, gpw, tuning):
    """A with attn_gpw: every wave takes 2 or 3 granules per round, so 96 granules go to 12 or 8 workgroups"""
    tuning("attn_gpw", gpw)
    nz = launch_nz(2, 4, CAP)
    assert slabs(kvd, CAP, nz, gpw) == {2: 12, 3: 8}[gpw]
    report(f"A {kvd} cur={CAP} attn_gpw={gpw}", self_twice(kvd, 4, 4, [CAP], CAP, nz=nz, gpw=gpw, seed=gpw))


# ---- A'. drifting scores ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kvd", ["f32", "bf16"])
@pytest.mark.parametrize("direction", [1, -1], ids=["ascending", "descending"])
def test_self_drifting_scores(kvd, direction):
    """A': K is built from the roped q (reference side) so that every query head's score moves by 16 from key 0 to key
    3071, plus N(0, 0.25^2).  Ascending: every slab raises the running maximum, the second merge round rescales the
    first by fr ~ e^-8; descending: the first round dominates and the second adds ~e^-8 of it.  A span of 16 keeps the
    fast exponent's argument error (2^-24 * 16 relative) far below the bound.
    bf16x2 is left out: the two-plane kernel drops the q_mid.K_lo and q_lo.K products by design, an error of
    sum|q_i||k_i| * 2^-16 * scale per score: up to |q||k| * 2^-16 * scale ~ 3e-4 for this K (|q| ~ 11, |k| ~ 16, k
    along q) against ~1e-4 for randn keys (sum|q_i||k_i| ~ 82).  That is a statement about the format, not about the
    merge, and the merge is the same code for all three cache types."""
    cur, G, KVH, R = CAP, 4, 4, 2
    gen = torch.Generator().manual_seed(77 + direction)
    qkv = torch.randn(R, (G + 2) * KVH * 128, generator=gen)
    cos, sin = lay.rope_tables(CAP + 1, 128, 1, 10000)
    pos = torch.full((R,), cur)
    q = rope64(qkv.double().reshape(R, -1, 128)[:, : G * KVH], cos, sin, pos).reshape(R, KVH, G, 128)
    drift = direction * 16.0 * (torch.arange(CAP, dtype=torch.float64) / (CAP - 1) - 0.5)                 # [keys]
    pinv = q.transpose(-1, -2) @ torch.linalg.inv(q @ q.transpose(-1, -2))                                # [R, KVH, 128, G]
    K = 0.25 * torch.randn(R, KVH, CAP, 128, generator=gen).double()
    K = K + (drift / SCALE)[None, None, :, None] * pinv.sum(dim=-1)[:, :, None, :]
    s = (q @ K.transpose(-1, -2)) * SCALE                                                                 # [R, KVH, G, keys]
    span = direction * (s[..., -1] - s[..., 0])
    assert span.min().item() > 13.0 and span.max().item() < 19.0, (span.min().item(), span.max().item())
    # the key appended by the launch continues the drift: its pre-RoPE row is the inverse rotation of K[cur - 1]
    c, sn = cos[cur].double(), sin[cur].double()
    kl = K[:, :, cur - 1]
    kraw = torch.cat([kl[..., :64] * c + kl[..., 64:] * sn, -kl[..., :64] * sn + kl[..., 64:] * c], dim=-1)
    qkv = qkv.reshape(R, -1, 128)
    qkv[:, G * KVH: (G + 1) * KVH] = kraw.float()
    qkv = qkv.reshape(R, -1).contiguous().to(dev())
    nz = launch_nz(R, KVH, CAP)
    assert slabs(kvd, cur, nz) == 24
    name = "ascending" if direction > 0 else "descending"
    report(f"A' {kvd} {name}", self_twice(kvd, G, KVH, [cur], CAP, nz=nz, seed=5, K=K.float(), q=qkv))


# ---- B. ragged rows, consecutive steps ----------------------------------------------------------------------------
@pytest.mark.parametrize("kvd", KVDS)
@pytest.mark.parametrize("attn_nz", [0, 3])
def test_self_ragged_consecutive_steps(kvd, attn_nz, tuning):
    """B: four utterances at cur = 1, 64, 299, 1279 decode three steps on the same caches, no restore: each launch reads
    back what the launches before it appended.  Step 2 is 2, 65, 300, 1280 (65: the new slot is key 0 of a fresh
    unit / granule); the full utterance is dropped from step 3 (6 rows)."""
    if attn_nz:
        tuning("attn_nz", attn_nz)
    G, KVH, T = 4, 4, 1280
    curs = [1, 64, 299, 1279]
    case = Attn(hb.ATTN_SELF, kvd, G, KVH, T, [c - 1 for c in curs for _ in (0, 1)], seed=1000 + attn_nz)
    worst = 0.0
    for step in range(3):
        now = [c + step for c in curs if c + step <= T]
        assert now == [[1, 64, 299, 1279], [2, 65, 300, 1280], [3, 66, 301]][step]
        qkv = case.draw_qkv(now)
        before = case.planes()
        out, nslab = case.launch(qkv, curs=now, n_rows=2 * len(now))
        nz = launch_nz(2 * len(now), KVH, T, attn_nz)
        worst = max(worst, check_self(case, qkv, now, out, nslab, before, nz=nz))
    report(f"B {kvd} attn_nz={attn_nz or 'default'}", worst)


# ---- C. group widths ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kvd", KVDS)
@pytest.mark.parametrize("G", [1, 2])
@pytest.mark.parametrize("attn_nz", [0, 2])
def test_self_group_widths(kvd, G, attn_nz, tuning):
    """C: GQA groups 1 and 2 (k_attn's prefetching loop, k_attn_mfma<1|2, .>), ragged cur = 37, 129, 640.  At attn_nz 2
    and cur 640 the new slot's unit is the last of five rounds of its workgroup."""
    if attn_nz:
        tuning("attn_nz", attn_nz)
    KVH, T, curs = 2, 1280, [37, 129, 640]
    nz = launch_nz(2 * len(curs), KVH, T, attn_nz)
    report(f"C {kvd} G={G} attn_nz={attn_nz or 'default'}", self_twice(kvd, G, KVH, curs, T, nz=nz, seed=10 * G + attn_nz))


# ---- D. cross-attention edges -------------------------------------------------------------------------------------
D_LENS = [0, 1, 31, 32, 33, 256, 257, 1024]
D_CURS = [3, 17, 100, 5, 900, 64, 1, 333]
D_CAP, D_H = 1024, 4


def run_cross(kvd, *, gpw=1, head_map=None, act_f32=0, seed=0):
    nz = launch_nz(len(D_LENS), D_H, D_CAP)
    assert nz == 8
    case, q, out, nslab, before = run_attn(hb.ATTN_CROSS, kvd, 1, D_H, D_CURS, D_CAP, lens=D_LENS, head_map=head_map, act_f32=act_f32, seed=seed)
    return check_cross(case, q, D_CURS, D_LENS, out, nslab, before, nz=nz, gpw=gpw, head_map=head_map), out


@pytest.mark.parametrize("kvd", KVDS)
def test_cross_edges(kvd):
    """D: texts of 0, 1, 31, 32, 33, 256, 257 and 1024 bytes in one launch.  On the MFMA kernel 256 keys stay in one
    workgroup and 257 are split over 3; the last arriver of a split pair still writes the unconditional row's zeros."""
    if kvd != "f32":
        assert slabs(kvd, 256, 8) == 1 and slabs(kvd, 257, 8) == 3 and slabs(kvd, 1024, 8) == 8
    else:
        assert slabs(kvd, 64, 8) == 1 and slabs(kvd, 257, 8) == 5 and slabs(kvd, 1024, 8) == 8
    report(f"D {kvd}", run_cross(kvd, seed=31)[0])


@pytest.mark.parametrize("kvd", KVDS)
@pytest.mark.parametrize("gpw", [2, 3])
def test_cross_edges_gpw(kvd, gpw, tuning):
    """D with attn_gpw_cross (k_attn ignores it; the restated rule says so too)"""
    tuning("attn_gpw_cross", gpw)
    if kvd != "f32":
        assert [slabs(kvd, n, 8, gpw) for n in (256, 257, 1024)] == {2: [1, 2, 4], 3: [1, 1, 3]}[gpw]
    report(f"D {kvd} attn_gpw_cross={gpw}", run_cross(kvd, gpw=gpw, seed=32 + gpw)[0])


@pytest.mark.parametrize("kvd", KVDS)
def test_cross_edges_head_map(kvd):
    """D for a head-pruned layer: head 1 is dead, the live heads go to positions 2, 0, 1 of the compacted o_proj input;
    position 3 keeps the sentinel in the conditional and the unconditional row, and the dead head publishes nothing."""
    report(f"D {kvd} head_map", run_cross(kvd, head_map=[2, -1, 0, 1], seed=41)[0])


@pytest.mark.parametrize("kvd", KVDS)
def test_cross_edges_act_f32(kvd):
    """D with fp32 activation tiles as the output: checked like the planes, and holding exactly what the planes sum to;
    the unconditional rows' tiles are zero (check_cross)."""
    w0, planes = run_cross(kvd, seed=51)
    w1, tiles = run_cross(kvd, act_f32=1, seed=51)
    assert torch.equal(planes, tiles) and planes.abs().max().item() > 0
    report(f"D {kvd} act_f32", max(w0, w1))
