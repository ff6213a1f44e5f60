"""The prefill kernels at prefill sizes, through the C ABI, against float64 restatements.

* dia_gemm above 128 rows, where plane inputs go to the wave-specialised tiled kernel (k_gemm_tile_ws), with every epilogue
  the engine's prefill uses: SCALE_STORE (with and without strip_map), RESID_EMIT (gnext, ssq_out, planes, with and without
  cmap), SWIGLU_EMIT and CROSSKV over a packed batch (row_b / seg_off, fp32 and bf16 blocked-V caches, merged layers).
* dia_dec_prefill_embed / _kv / _attn (csrc/prefill.hip) on packed CFG segments of 2..517 rows, and the decode step that
  follows the prefill on the caches it wrote.
* dia_embed_text called the way the encoder prefill calls it: per utterance, into the packed buffers.
* the argument checks of the prefill entry points, with real buffers behind every pointer.

Tolerances (those of test_gpu_kernels.py): fp32 results within 2e-5 of the output scale (max(1, max |ref|)), attention
outputs within 2e-5.  bf16 cache entries are the rounding of an fp32 result: within one bf16 ulp of the float64 value plus
what the fp32 computation itself may be off by (see bf16_bound).  Every test prints its worst error."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from dia_hip import binding as hb
from dia_hip import layout as lay

TOL = 2e-5
HD = 128


def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    return torch.device("cuda:0")


def bf16r(t):
    return t.bfloat16().float()


def ceil(v, m):
    return (v + m - 1) // m * m


def strip_ssq(x, mpad):
    """fp32 strip sums of squares [D/16][mpad] of x [M, D] (the layout of every ssq array)"""
    M, D = x.shape
    s = torch.zeros(D // 16, mpad, dtype=torch.float32, device=x.device)
    s[:, :M] = (x.double() ** 2).reshape(M, D // 16, 16).sum(-1).T.float()
    return s


def rel_err(got, ref):
    return (got.double() - ref).abs().max().item() / max(1.0, ref.abs().max().item())


def rope(x, c, s):
    """x [..., 128] float64, c / s broadcastable to [..., 64]"""
    return torch.cat([x[..., :64] * c - x[..., 64:] * s, x[..., :64] * s + x[..., 64:] * c], dim=-1)


def rope_fp32_err(x, c, s):
    """bound of an fp32 RoPE's own rounding: two products and a sum, each rounded to 2^-24 relative, so at most
    2^-23 (|x1 c| + |x2 s|) for the first half and 2^-23 (|x1 s| + |x2 c|) for the second"""
    x1, x2, c, s = x[..., :64].abs(), x[..., 64:].abs(), c.abs(), s.abs()
    return 2.0 ** -23 * torch.cat([x1 * c + x2 * s, x1 * s + x2 * c], dim=-1)


def bf16_ulp(ref):
    """one bf16 ulp at the magnitude of ref (8 significant bits)"""
    e = torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -126)))
    return torch.pow(2.0, e - 7)


def bf16_bound(ref, fp32_err):
    """A bf16 cache entry is the round-to-nearest of an fp32 result.  The rounding costs half an ulp; the fp32 result may
    sit on the far side of a rounding boundary, so one ulp of the float64 value is allowed.  That argument needs the fp32
    error to be below half an ulp, which fails where the value is near 0 (cancellation): there the ulp shrinks with the value
    and the fp32 error does not.  So the bound adds fp32_err, the error the fp32 computation is allowed by itself (the fp32
    variant of the same check, or the rounding bound of the RoPE products).  Above ~1e-2 the ulp term dominates."""
    return bf16_ulp(ref) + fp32_err


def check_bf16(name, got, ref, fp32_err):
    d = (got.double() - ref).abs()
    ulp = bf16_ulp(ref)
    worst = (d / ulp).max().item()
    beyond = int((d > ulp).sum().item())
    print(f"{name}: worst {worst:.3f} bf16 ulp, {beyond} of {d.numel()} beyond one ulp (largest such |ref| "
          f"{(ref.abs()[d > ulp].max().item() if beyond else 0.0):.2e}), max |err| {d.max().item():.2e}")
    assert (d <= bf16_bound(ref, fp32_err)).all(), (name, worst, beyond)


def timed_gemm(g):
    """dia_gemm through dia_gemm_timed: returns the name of the kernel that ran"""
    L = hb.lib()
    ms = C.c_float()
    hb.check(L.dia_gemm_timed(C.byref(g), None, C.byref(ms)), "dia_gemm_timed")
    torch.cuda.synchronize()
    return L.dia_timed_kernel_name(0).decode()


def gemm_args(A, M, Wt, kt, ns, epi):
    g = hb.GemmArgs()
    g.A, g.a_plane_stride, g.a_ktiles, g.M = hb.ptr(A), A[0].numel(), A.shape[2], M
    g.W, g.KT, g.nstrips, g.epi = hb.ptr(Wt), kt, ns, epi
    return g


# variant -> (tuning knobs, expected kernel name prefix).  tile_v 4 / 5 are the other producer / ring-depth forms of the tiled
# kernel; tile_min_blocks = 1 sends a narrow N (too few 64 x 256 blocks for the default) to it; a huge value keeps k_gemm.
VARIANTS = {
    "tile": ({}, "k_gemm_tile_ws<2, 2, 4>"),
    "v4": ({"tile_v": 4}, "k_gemm_tile_ws<2, 2, 2>"),
    "v5": ({"tile_v": 5}, "k_gemm_tile_ws<2, 4, 4>"),
    "narrow": ({"tile_min_blocks": 1}, "k_gemm_tile_ws<2, 2, 4>"),
    "generic": ({"tile_min_blocks": 1 << 30}, "k_gemm<"),
}


def apply_variant(variant, tuning):
    knobs, want = VARIANTS[variant]
    for k, v in knobs.items():
        tuning(k, v)
    return want


def check_kernel(name, want):
    print("kernel", name)
    assert name.startswith(want), (name, want)


def tile_blocks(M, ns):
    return ceil((M + 15) // 16, 4) // 4 * ((ns + 15) // 16)


# ---------------------------------------------------------------------------------------------------
# 1. dia_gemm at prefill sizes
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,K,N,live,variant", [
    (129, 1024, 4096, 0, "tile"), (144, 2048, 4112, 0, "tile"), (200, 4096, 4096, 24, "tile"), (255, 4096, 3088, 0, "tile"),
    (256, 8192, 3072, 0, "tile"), (257, 2048, 4096, 20, "tile"), (1216, 1024, 1040, 0, "tile"),
    (257, 1024, 2560, 0, "v4"), (257, 1024, 2560, 0, "v5"), (257, 1024, 256, 0, "narrow"), (257, 1024, 2560, 0, "generic")])
def test_gemm_prefill_scale_store(M, K, N, live, variant, tuning):
    """SCALE_STORE (q/k/v, cross-q of the prefill).  live > 0: only `live` of the N/128 heads are computed (strip_map), the
    columns of the others stay untouched."""
    d = dev()
    torch.manual_seed(M + K + N + live)
    want = apply_variant(variant, tuning)
    Mg = ceil(M, 64)                                   # rows the grid covers (4 m-tiles per workgroup)
    x = torch.randn(M, K, device=d) * 2.0
    gw = bf16r(1.0 + 0.1 * torch.randn(K, device=d))
    xg = x * gw                                        # the fp32 input the planes hold
    W = bf16r(torch.randn(K, N, device=d) * 0.05)
    if live:
        lh = torch.zeros(N // HD, dtype=torch.bool)
        lh[torch.randperm(N // HD)[:live]] = True
        strips = [s for h in torch.nonzero(lh).flatten().tolist() for s in range(h * 8, h * 8 + 8)]
        cols = (torch.tensor(strips)[:, None] * 16 + torch.arange(16)[None, :]).reshape(-1).to(d)
        Wt, kt, ns = lay.tile_weight(W[:, cols])
        smap = torch.tensor(strips, dtype=torch.int32, device=d)
    else:
        Wt, kt, ns = lay.tile_weight(W)
        cols, smap = None, None
    if variant in ("tile", "v4", "v5"):
        assert tile_blocks(M, ns) >= 48 and M > 128
    ldo = ceil(N, 16)
    ssq = strip_ssq(x, Mg)
    out = torch.full((Mg, ldo), float("nan"), device=d)
    A = lay.pack_planes(xg)
    g = gemm_args(A, M, Wt, kt, ns, hb.EPI_SCALE_STORE)
    g.ssq_in, g.ssq_in_n, g.inv_d, g.eps, g.ssq_ld = hb.ptr(ssq), ssq.shape[0], 1.0 / K, 1e-5, Mg
    g.out, g.ldo, g.strip_map = hb.ptr(out), ldo, hb.ptr(smap)
    check_kernel(timed_gemm(g), want)
    inv = torch.rsqrt(ssq[:, :M].double().sum(0) / K + 1e-5)[:, None]
    ref = (xg.double() @ W.double()) * inv
    written = torch.zeros(ldo, dtype=torch.bool, device=d)
    written[cols if cols is not None else torch.arange(N, device=d)] = True
    err = rel_err(out[:M, :N][:, written[:N]], ref[:, written[:N]])
    print(f"scale_store M={M} K={K} N={N} live={live} {variant}: err {err:.2e} (tol {TOL})")
    assert err <= TOL, err
    if N < ldo:
        assert (out[:M, N:] == 0).all()                # the zero-padded columns of the last strip
    assert torch.isnan(out[:M, :N][:, ~written[:N]]).all()   # dropped heads: not written
    assert torch.isnan(out[M:]).all()                  # rows >= M: not written


@pytest.mark.parametrize("M,K,D,mapped,variant", [
    (144, 2048, 4096, False, "tile"), (255, 4096, 3072, False, "tile"), (257, 8192, 3072, True, "tile"),
    (1216, 8192, 2048, True, "tile"), (1216, 2048, 1040, False, "tile"),
    (257, 1024, 3072, False, "v4"), (257, 1024, 3072, True, "v5"), (257, 1024, 256, False, "narrow"), (257, 1024, 3072, True, "generic")])
def test_gemm_prefill_resid_emit(M, K, D, mapped, variant, tuning):
    """RESID_EMIT (o, co, wo of the prefill): x += a . W, planes of x * g_next (at cmap[n], or dropped), strip sums of x"""
    d = dev()
    torch.manual_seed(M + K + D + int(mapped))
    want = apply_variant(variant, tuning)
    Mg = ceil(M, 64)
    a = torch.randn(M, K, device=d)
    W = bf16r(torch.randn(K, D, device=d) * 0.03)
    Wt, kt, ns = lay.tile_weight(W)
    if variant in ("tile", "v4", "v5"):
        assert tile_blocks(M, ns) >= 48 and M > 128
    x0 = torch.randn(Mg, D, device=d)
    gn = bf16r(1.0 + 0.1 * torch.randn(D, device=d))
    pkt = (D + 31) // 32
    keep = torch.rand(D, device=d) < 0.5
    keep[:3] = torch.tensor([True, False, True], device=d)
    nk = int(keep.sum()) if mapped else D
    cmap = torch.where(keep, torch.cumsum(keep.int(), 0) - 1, torch.full((D,), -1, device=d, dtype=torch.int64)).to(torch.int32)
    sentinel = 3.0
    x = x0.clone()
    P = lay.pack_planes(torch.full((Mg, pkt * 32), sentinel, device=d))
    ssq = torch.full((ns, Mg), sentinel, device=d)
    g = gemm_args(lay.pack_planes(a), M, Wt, kt, ns, hb.EPI_RESID_EMIT)
    g.ssq_ld, g.out, g.ldo, g.gnext = Mg, hb.ptr(x), D, hb.ptr(gn)
    g.P, g.p_plane_stride, g.p_ktiles, g.ssq_out = hb.ptr(P), P[0].numel(), pkt, hb.ptr(ssq)
    if mapped:
        g.cmap = hb.ptr(cmap)
    check_kernel(timed_gemm(g), want)
    ref = x0[:M].double() + a.double() @ W.double()
    err = rel_err(x[:M], ref)
    got = lay.unpack_planes(P, Mg, pkt * 32)
    emitted = got[:M, :nk]
    kept = keep if mapped else torch.ones(D, dtype=torch.bool, device=d)
    err_p = rel_err(emitted, (ref * gn.double())[:, kept])
    want_ss = (ref ** 2).reshape(M, D // 16, 16).sum(-1).T
    err_s = rel_err(ssq[:, :M], want_ss)
    print(f"resid_emit M={M} K={K} D={D} cmap={mapped} {variant}: x {err:.2e}, planes {err_p:.2e}, ssq {err_s:.2e} (tol {TOL})")
    assert err <= TOL and err_p <= TOL and err_s <= TOL, (err, err_p, err_s)
    assert torch.equal(emitted, (x[:M] * gn)[:, kept])         # planes carry the fp32 x * g of the stored x exactly
    assert (got[:M, nk:] == sentinel).all() and (got[M:] == sentinel).all()
    assert torch.equal(x[M:], x0[M:]) and (ssq[:, M:] == sentinel).all()


@pytest.mark.parametrize("M,K,F,variant", [
    (129, 1024, 2048, "tile"), (200, 4096, 1536, "tile"), (256, 8192, 1544, "tile"), (1216, 2048, 4096, "tile"),
    (257, 1024, 1280, "v4"), (257, 1024, 1280, "v5"), (257, 1024, 128, "narrow"), (257, 1024, 1280, "generic")])
def test_gemm_prefill_swiglu_emit(M, K, F, variant, tuning):
    """SWIGLU_EMIT (wi of the prefill): h = silu(gate * inv) * (up * inv) into planes"""
    d = dev()
    torch.manual_seed(M + K + F)
    want = apply_variant(variant, tuning)
    Mg = ceil(M, 64)
    x = torch.randn(M, K, device=d)
    gw = bf16r(1.0 + 0.1 * torch.randn(K, device=d))
    xg = x * gw
    wi = bf16r(torch.randn(K, 2, F, device=d) * 0.05)
    Wt, kt, ns = lay.tile_weight(lay.interleave_gate_up(wi))
    if variant in ("tile", "v4", "v5"):
        assert tile_blocks(M, ns) >= 48 and M > 128
    ssq = strip_ssq(x, Mg)
    pkt = (F + 31) // 32
    sentinel = 5.0
    P = lay.pack_planes(torch.full((Mg, pkt * 32), sentinel, device=d))
    g = gemm_args(lay.pack_planes(xg), M, Wt, kt, ns, hb.EPI_SWIGLU_EMIT)
    g.ssq_in, g.ssq_in_n, g.inv_d, g.eps, g.ssq_ld = hb.ptr(ssq), ssq.shape[0], 1.0 / K, 1e-5, Mg
    g.P, g.p_plane_stride, g.p_ktiles = hb.ptr(P), P[0].numel(), pkt
    check_kernel(timed_gemm(g), want)
    h = xg.double() * torch.rsqrt(ssq[:, :M].double().sum(0) / K + 1e-5)[:, None]
    f = torch.einsum("mk,kgf->mgf", h, wi.double())
    ref = torch.nn.functional.silu(f[:, 0]) * f[:, 1]
    got = lay.unpack_planes(P, Mg, pkt * 32)
    err = rel_err(got[:M, :F], ref)
    print(f"swiglu_emit M={M} K={K} F={F} {variant}: err {err:.2e} (tol {TOL})")
    assert err <= TOL, err
    assert (got[:M, F:] == sentinel).all() and (got[M:] == sentinel).all()


# packed cross-K/V batch: utterance ids (cache rows) in packing order and their text lengths; cache rows 1 and 4 are not in it
CKV_UTT = [5, 2, 0, 7, 3, 6]
CKV_LENS = [33, 0, 1, 200, 31, 32]
CKV_ROWS, CKV_CAP = 8, 256


@pytest.mark.parametrize("kvd,H,layers,variant", [
    ("f32", 16, 1, "tile"), ("bf16", 16, 1, "tile"), ("bf16", 16, 2, "tile"),
    ("bf16", 16, 1, "v4"), ("f32", 16, 1, "v5"), ("bf16", 1, 1, "narrow"), ("bf16", 16, 1, "generic")])
def test_gemm_prefill_crosskv_packed(kvd, H, layers, variant, tuning):
    """CROSSKV over a packed batch (row_b / seg_off): K = RoPE(h . Wk, text position), V = h . Wv into the utterance's cache row.
    layers = 2: both layers' projections in one launch (kv_layer_strips) with heads dropped through strip_map (12 of 16 live in
    layer 0).  Cache slots past each length, the rows of utterances not in the batch and the dropped heads keep a sentinel."""
    d = dev()
    torch.manual_seed(17 + H + layers + len(kvd))
    want = apply_variant(variant, tuning)
    E = 1024
    offs, tot = [], 0
    for Lb in CKV_LENS:
        offs.append(tot)
        tot += ceil(Lb, 32)
    Mp = tot
    rb = np.full((Mp,), -1, dtype=np.int32)
    so = np.full((CKV_ROWS,), 1 << 20, dtype=np.int32)          # (entries of utterances not in the batch are never read)
    for u, o, Lb in zip(CKV_UTT, offs, CKV_LENS):
        rb[o: o + Lb] = u
        so[u] = o
    row_b, seg_off = torch.from_numpy(rb).to(d), torch.from_numpy(so).to(d)
    x = torch.randn(Mp, E, device=d)
    gw = bf16r(1.0 + 0.1 * torch.randn(E, device=d))
    xg = x * gw
    ssq = strip_ssq(x, Mp)
    perm = lay.rope_pair_perm(HD).to(d)
    live = [torch.ones(H, dtype=torch.bool) for _ in range(layers)]
    if layers > 1:
        live[0][torch.randperm(H)[:4]] = False
    wks, wvs, cols, smap = [], [], [], []
    for l in range(layers):
        wk = bf16r(torch.randn(E, H, HD, device=d) * 0.05)
        wv = bf16r(torch.randn(E, H, HD, device=d) * 0.05)
        wks.append(wk); wvs.append(wv)
        Wl = torch.cat([wk[:, :, perm].reshape(E, -1), wv.reshape(E, -1)], dim=1)
        strips = [s for h in torch.nonzero(live[l]).flatten().tolist() for s in range(h * 8, h * 8 + 8)]
        strips += [H * 8 + s for s in strips]
        cols.append(Wl[:, (torch.tensor(strips)[:, None] * 16 + torch.arange(16)[None, :]).reshape(-1).to(d)])
        smap += [l * H * 16 + s for s in strips]
    Wt, kt, ns = lay.tile_weight(torch.cat(cols, dim=1))
    if variant in ("tile", "v4", "v5"):
        assert tile_blocks(Mp, ns) >= 48 and Mp > 128
    cos, sin = [t.to(d) for t in lay.rope_tables(CKV_CAP + 1, HD, 1, 10000)]
    kdt = torch.float32 if kvd == "f32" else torch.bfloat16
    sentinel = 3.0
    kc = torch.full((layers, CKV_ROWS, H, CKV_CAP, HD), sentinel, dtype=kdt, device=d)
    vc = torch.full_like(kc, sentinel)
    g = gemm_args(lay.pack_planes(xg), Mp, Wt, kt, ns, hb.EPI_CROSSKV)
    g.ssq_in, g.ssq_in_n, g.inv_d, g.eps, g.ssq_ld = hb.ptr(ssq), E // 16, 1.0 / E, 1e-5, Mp
    g.kc, g.vc, g.kv_dtype, g.kv_heads, g.kv_cap, g.kv_batch_index = hb.ptr(kc), hb.ptr(vc), (hb.KV_F32 if kvd == "f32" else hb.KV_BF16), H, CKV_CAP, 0
    g.cos_t, g.sin_t, g.kv_vblocked = hb.ptr(cos), hb.ptr(sin), int(kvd == "bf16")
    g.row_b, g.seg_off = hb.ptr(row_b), hb.ptr(seg_off)
    if layers > 1:
        sm = torch.tensor(smap, dtype=torch.int32, device=d)
        g.strip_map, g.kv_layer_strips, g.kv_layer_stride = hb.ptr(sm), H * 16, kc[0].numel()
    check_kernel(timed_gemm(g), want)
    if kvd == "bf16":
        vc = lay.v_from_blocked(vc.reshape(layers, CKV_ROWS, H, CKV_CAP // 32, HD, 32))
    # float64 reference caches: sentinel everywhere, the reference where a value belongs
    h = xg.double() * torch.rsqrt(ssq.double().sum(0) / E + 1e-5)[:, None]
    valid = row_b >= 0
    bi = row_b[valid].long()
    pi = (torch.arange(Mp, device=d)[valid] - seg_off[row_b[valid].long()]).long()
    refk = torch.full(kc.shape, sentinel, dtype=torch.float64, device=d)
    refv = torch.full(kc.shape, sentinel, dtype=torch.float64, device=d)
    written = torch.zeros(kc.shape[:4], dtype=torch.bool, device=d)
    for l in range(layers):
        k = torch.einsum("me,ehd->mhd", h[valid], wks[l].double())
        v = torch.einsum("me,ehd->mhd", h[valid], wvs[l].double())
        kr = rope(k, cos.double()[pi][:, None, :], sin.double()[pi][:, None, :])
        lv = live[l].to(d)
        rk, rv, wr = refk[l], refv[l], written[l]
        rk[bi, :, pi] = torch.where(lv[None, :, None], kr, rk[bi, :, pi])
        rv[bi, :, pi] = torch.where(lv[None, :, None], v, rv[bi, :, pi])
        wr[bi, :, pi] = lv[None, :].expand(bi.numel(), H)
    assert int(written.sum()) == sum(CKV_LENS) * sum(int(lv.sum()) for lv in live)
    untouched_k = kc[~written]
    untouched_v = vc[~written]
    assert (untouched_k == sentinel).all() and (untouched_v == sentinel).all()
    gk, gv, rk, rv = kc[written], vc[written], refk[written], refv[written]
    if kvd == "f32":
        ek, ev = rel_err(gk, rk), rel_err(gv, rv)
        print(f"crosskv f32 H={H} layers={layers} {variant}: K {ek:.2e}, V {ev:.2e} (tol {TOL})")
        assert ek <= TOL and ev <= TOL, (ek, ev)
    else:
        check_bf16(f"crosskv bf16 H={H} layers={layers} {variant} K", gk, rk, TOL * max(1.0, rk.abs().max().item()))
        check_bf16(f"crosskv bf16 H={H} layers={layers} {variant} V", gv, rv, TOL * max(1.0, rv.abs().max().item()))


def test_gemm_prefill_two_plane_weights_above_128_rows():
    """w_planes = 2 (hi / lo bf16 planes of fp32 weights) at 200 rows: the generic kernel, against float64 over hi + lo"""
    d = dev()
    torch.manual_seed(2)
    M, K, N = 200, 2048, 1040
    Mg = ceil(M, 64)
    x = torch.randn(M, K, device=d)
    W = torch.randn(K, N, device=d) * 0.05                       # not bf16-representable
    Wt, kt, ns = lay.tile_weight_bf16x2(W)
    hi, lo = lay.untile_weight_bf16x2(Wt, K, N)
    ssq = strip_ssq(x, Mg)
    out = torch.full((Mg, ceil(N, 16)), float("nan"), device=d)
    A = lay.pack_planes(x)
    g = gemm_args(A, M, Wt, kt, ns, hb.EPI_SCALE_STORE)
    g.w_planes = 2
    g.ssq_in, g.ssq_in_n, g.inv_d, g.eps, g.ssq_ld = hb.ptr(ssq), ssq.shape[0], 1.0 / K, 1e-5, Mg
    g.out, g.ldo = hb.ptr(out), out.shape[1]
    check_kernel(timed_gemm(g), "k_gemm<")
    ref = (x.double() @ (hi.double() + lo.double())) * torch.rsqrt(ssq[:, :M].double().sum(0) / K + 1e-5)[:, None]
    err = rel_err(out[:M, :N], ref)
    print(f"two-plane weights M={M}: err {err:.2e} (tol {TOL})")
    assert err <= TOL, err
    assert torch.isnan(out[M:]).all()


# ---------------------------------------------------------------------------------------------------
# 2. dia_dec_prefill_embed / _kv / _attn
# ---------------------------------------------------------------------------------------------------
QH, KVH, CH = 16, 4, 16                   # the decoder's heads: q 16, kv 4 (group 4), cross 16 (group 1)
D_, C_, V_ = 512, 9, 1028                 # mid config width, channels, audio vocabulary
NQKV = (QH + 2 * KVH) * HD
# segments (self-cache row 2b + c, prompt rows): not in row order, both CFG rows of each of utterances 3, 1, 5, 0, 7, 4;
# utterances 2 and 6 (cache rows 4, 5, 12, 13) are left out
SEGS = [(7, 33), (6, 2), (2, 517), (3, 16), (11, 300), (10, 17), (0, 31), (1, 128), (15, 129), (14, 32), (9, 64), (8, 65)]
NCROWS, TTOK, SCAP = 16, 520, 544         # self-cache rows, token rows, self-cache capacity
TEXT = {3: 33, 1: 0, 5: 320, 0: 1, 7: 129, 4: 300, 2: 50, 6: 50}     # cross: text length per utterance (5: the capacity)
XCAP = 320


def pack(segs, d):
    offs, tot = [], 0
    for _, n in segs:
        offs.append(tot)
        tot += ceil(n, 32)
    rs = np.full((tot,), -1, dtype=np.int32)
    for i, (_, n) in enumerate(segs):
        rs[offs[i]: offs[i] + n] = i
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=d)
    t = dict(rows=tot, offs=offs, row_seg=torch.from_numpy(rs).to(d), seg_off=i32(offs), seg_len=i32([n for _, n in segs]),
             seg_row=i32([r for r, _ in segs]))
    t["pad"] = t["row_seg"] < 0
    return t


def prefill_args(pk):
    a = hb.DecPrefillArgs()
    a.row_seg, a.seg_off, a.seg_len, a.seg_row, a.rows = hb.ptr(pk["row_seg"]), hb.ptr(pk["seg_off"]), hb.ptr(pk["seg_len"]), hb.ptr(pk["seg_row"]), pk["rows"]
    return a


@pytest.mark.parametrize("with_g", [True, False])
def test_dec_prefill_embed(with_g):
    """x[m] = sum_c emb[c][tokens[b][r][c]] (float64), planes = x * g (or x), strip sums of squares; padding rows untouched"""
    d = dev()
    torch.manual_seed(31 + int(with_g))
    pk = pack(SEGS, d)
    rows = pk["rows"]
    tokens = torch.randint(0, V_, (NCROWS // 2, TTOK, C_), dtype=torch.int32, device=d)
    emb = torch.randn(C_, V_, D_, device=d) * 0.5
    gw = bf16r(1.0 + 0.1 * torch.randn(D_, device=d)) if with_g else None
    sentinel = 7.0
    x = torch.full((rows, D_), sentinel, device=d)
    P = lay.pack_planes(torch.full((rows, D_), sentinel, device=d))
    ssq = torch.full((D_ // 16, rows), sentinel, device=d)
    a = prefill_args(pk)
    a.tokens, a.T, a.C, a.V, a.D = hb.ptr(tokens), TTOK, C_, V_, D_
    a.emb, a.g, a.x = hb.ptr(emb), hb.ptr(gw), hb.ptr(x)
    a.P, a.p_plane_stride, a.p_ktiles, a.ssq, a.ssq_ld = hb.ptr(P), P[0].numel(), D_ // 32, hb.ptr(ssq), rows
    hb.check(hb.lib().dia_dec_prefill_embed(C.byref(a), None), "dia_dec_prefill_embed")
    torch.cuda.synchronize()
    ref = torch.zeros(rows, D_, dtype=torch.float64, device=d)
    for (crow, n), o in zip(SEGS, pk["offs"]):
        tk = tokens[crow >> 1, :n].long()                        # [n, C]
        for c in range(C_):
            ref[o: o + n] += emb[c].double()[tk[:, c]]
    live = ~pk["pad"]
    err = rel_err(x[live], ref[live])
    got_p = lay.unpack_planes(P, rows, D_)
    gd = gw.double() if with_g else 1.0
    err_p = rel_err(got_p[live], ref[live] * gd)
    want_ss = (ref[live] ** 2).reshape(-1, D_ // 16, 16).sum(-1).T
    err_s = rel_err(ssq[:, live], want_ss)
    print(f"prefill embed g={with_g}: x {err:.2e}, planes {err_p:.2e}, ssq {err_s:.2e} (tol {TOL})")
    assert err <= TOL and err_p <= TOL and err_s <= TOL, (err, err_p, err_s)
    assert torch.equal(got_p[live], x[live] * gw if with_g else x[live])
    pad = pk["pad"]
    assert (x[pad] == sentinel).all() and (got_p[pad] == sentinel).all() and (ssq[:, pad] == sentinel).all()


def _self_kv(d, pk, segs, qkv, kc, vc, cos, sin, cap):
    a = prefill_args(pk)
    a.q, a.ldq, a.q_off, a.k_off, a.v_off = hb.ptr(qkv), NQKV, 0, QH * HD, (QH + KVH) * HD
    a.q_heads, a.kv_heads, a.kv_cap, a.causal = QH, KVH, cap, 1
    a.kc, a.vc, a.cos_t, a.sin_t = hb.ptr(kc), hb.ptr(vc), hb.ptr(cos), hb.ptr(sin)
    hb.check(hb.lib().dia_dec_prefill_kv(C.byref(a), None), "dia_dec_prefill_kv")
    return a


def _garbage_caches(d, nrows, heads, cap):
    """bf16 caches [rows][heads][cap][128] holding large finite values; V in the blocked layout"""
    kc = (1e3 * torch.randn(nrows, heads, cap, HD, device=d)).bfloat16()
    vc = lay.v_to_blocked((1e3 * torch.randn(nrows, heads, cap, HD, device=d)).bfloat16())
    return kc, vc


def test_dec_prefill_kv():
    """K slot r of the segment's cache row = RoPE(k, r + 1), V slot r = bf16(v) in the blocked layout; every other slot and
    cache row bitwise unchanged"""
    d = dev()
    torch.manual_seed(41)
    pk = pack(SEGS, d)
    rows = pk["rows"]
    qkv = torch.randn(rows, NQKV, device=d) * 2.0
    cos, sin = [t.to(d) for t in lay.rope_tables(SCAP + 2, HD, 1, 10000)]
    kc0, vc0 = _garbage_caches(d, NCROWS, KVH, SCAP)
    kc, vc = kc0.clone(), vc0.clone()
    _self_kv(d, pk, SEGS, qkv, kc, vc, cos, sin, SCAP)
    torch.cuda.synchronize()
    vr, vr0 = lay.v_from_blocked(vc), lay.v_from_blocked(vc0)
    written = torch.zeros(NCROWS, KVH, SCAP, dtype=torch.bool, device=d)
    gk, rk, e32, gv, rv = [], [], [], [], []
    for (crow, n), o in zip(SEGS, pk["offs"]):
        written[crow, :, :n] = True
        k = qkv[o: o + n, QH * HD: (QH + KVH) * HD].double().reshape(n, KVH, HD)
        c, s = cos[1: n + 1].double()[:, None, :], sin[1: n + 1].double()[:, None, :]
        rk.append(rope(k, c, s))
        e32.append(rope_fp32_err(k, c, s))
        gk.append(kc[crow, :, :n].transpose(0, 1))
        v = qkv[o: o + n, (QH + KVH) * HD:].reshape(n, KVH, HD)
        rv.append(v.bfloat16())
        gv.append(vr[crow, :, :n].transpose(0, 1))
    check_bf16("prefill kv K", torch.cat(gk), torch.cat(rk), torch.cat(e32))
    assert torch.equal(torch.cat(gv), torch.cat(rv))            # torch's round-to-nearest-even of v
    assert torch.equal(kc[~written], kc0[~written]) and torch.equal(vr[~written], vr0[~written])


def attn_masked(q, K, V, lim):
    """q [L, Hq, 128], K / V [n, Hkv, 128] float64, lim [L]: query row i sees keys 0 .. lim[i]-1 (none -> 0)"""
    g = q.shape[1] // K.shape[1]
    Ke, Ve = K.repeat_interleave(g, dim=1), V.repeat_interleave(g, dim=1)
    s = torch.einsum("qhd,khd->hqk", q, Ke) / math.sqrt(HD)
    keys = torch.arange(K.shape[0], device=q.device)
    s = s.masked_fill(~(keys[None, :] < lim[:, None])[None], -math.inf)
    p = torch.nan_to_num(torch.softmax(s, dim=-1), nan=0.0)
    return torch.einsum("hqk,khd->qhd", p, Ve)


def test_dec_prefill_attn_causal():
    """causal self-attention of every segment over its own cache row (written by dia_dec_prefill_kv, large finite garbage past
    the segment), against float64 from the bf16 caches; near-miss references (mask one key short / long, q RoPE at r) are far"""
    d = dev()
    torch.manual_seed(43)
    pk = pack(SEGS, d)
    rows = pk["rows"]
    qkv = torch.randn(rows, NQKV, device=d)
    cos, sin = [t.to(d) for t in lay.rope_tables(SCAP + 2, HD, 1, 10000)]
    kc, vc = _garbage_caches(d, NCROWS, KVH, SCAP)
    a = _self_kv(d, pk, SEGS, qkv, kc, vc, cos, sin, SCAP)
    sentinel = 9.0
    P = lay.pack_planes(torch.full((rows, QH * HD), sentinel, device=d))
    a.P, a.p_plane_stride, a.p_ktiles = hb.ptr(P), P[0].numel(), QH * HD // 32
    hb.check(hb.lib().dia_dec_prefill_attn(C.byref(a), None), "dia_dec_prefill_attn")
    torch.cuda.synchronize()
    out = lay.unpack_planes(P, rows, QH * HD).double().reshape(rows, QH, HD)
    vr = lay.v_from_blocked(vc)
    worst, near = 0.0, {"one key short": 0.0, "one key long": 0.0, "q RoPE at r": 0.0}
    for (crow, n), o in zip(SEGS, pk["offs"]):
        qr = qkv[o: o + n, : QH * HD].double().reshape(n, QH, HD)
        q = rope(qr, cos[1: n + 1].double()[:, None, :], sin[1: n + 1].double()[:, None, :])
        q0 = rope(qr, cos[:n].double()[:, None, :], sin[:n].double()[:, None, :])
        K = kc[crow, :, :n].double().transpose(0, 1)
        V = vr[crow, :, :n].double().transpose(0, 1)
        r = torch.arange(n, device=d)
        got = out[o: o + n]
        worst = max(worst, (got - attn_masked(q, K, V, r + 1)).abs().max().item())
        near["one key short"] = max(near["one key short"], (got - attn_masked(q, K, V, r)).abs().max().item())
        near["one key long"] = max(near["one key long"], (got - attn_masked(q, K, V, (r + 2).clamp(max=n))).abs().max().item())
        near["q RoPE at r"] = max(near["q RoPE at r"], (got - attn_masked(q0, K, V, r + 1)).abs().max().item())
    print(f"prefill attn causal: worst {worst:.2e} (tol {TOL}); distance to near misses {near}")
    assert worst <= TOL, worst
    for k, v in near.items():
        assert v >= 100 * TOL, (k, v)
    pad = pk["pad"]
    assert (out[pad] == sentinel).all()


def test_dec_prefill_attn_cross():
    """cross-attention: cond segments over their utterance's text keys (lengths 0, 1, 33, 129, 300 and the capacity; large
    finite garbage past each), uncond segments and text length 0 exactly 0; near miss text_len - 1 is far; padding untouched"""
    d = dev()
    torch.manual_seed(47)
    pk = pack(SEGS, d)
    rows = pk["rows"]
    qc = torch.randn(rows, CH * HD, device=d)
    cos, sin = [t.to(d) for t in lay.rope_tables(SCAP + 2, HD, 1, 10000)]
    nb = NCROWS // 2
    kf = 1e3 * torch.randn(nb, CH, XCAP, HD, device=d)
    vf = 1e3 * torch.randn(nb, CH, XCAP, HD, device=d)
    for b, n in TEXT.items():
        kf[b, :, :n] = torch.randn(CH, n, HD, device=d)
        vf[b, :, :n] = torch.randn(CH, n, HD, device=d)
    kc, vc = kf.bfloat16(), lay.v_to_blocked(vf.bfloat16())
    tl = torch.tensor([TEXT[b] for b in range(nb)], dtype=torch.int32, device=d)
    sentinel = 9.0
    P = lay.pack_planes(torch.full((rows, CH * HD), sentinel, device=d))
    a = prefill_args(pk)
    a.q, a.ldq, a.q_off = hb.ptr(qc), CH * HD, 0
    a.q_heads, a.kv_heads, a.kv_cap, a.causal = CH, CH, XCAP, 0
    a.kc, a.vc, a.cos_t, a.sin_t, a.text_len = hb.ptr(kc), hb.ptr(vc), hb.ptr(cos), hb.ptr(sin), hb.ptr(tl)
    a.P, a.p_plane_stride, a.p_ktiles = hb.ptr(P), P[0].numel(), CH * HD // 32
    hb.check(hb.lib().dia_dec_prefill_attn(C.byref(a), None), "dia_dec_prefill_attn(cross)")
    torch.cuda.synchronize()
    out = lay.unpack_planes(P, rows, CH * HD).double().reshape(rows, CH, HD)
    vr = lay.v_from_blocked(vc)
    worst, near = 0.0, 0.0
    for (crow, n), o in zip(SEGS, pk["offs"]):
        got = out[o: o + n]
        b, tn = crow >> 1, TEXT[crow >> 1]
        if crow % 2 == 0 or tn == 0:
            assert (got == 0).all(), (crow, tn)                 # uncond segment / no text: exactly 0
            continue
        q = rope(qc[o: o + n].double().reshape(n, CH, HD), cos[1: n + 1].double()[:, None, :], sin[1: n + 1].double()[:, None, :])
        K = kc[b, :, :tn].double().transpose(0, 1)
        V = vr[b, :, :tn].double().transpose(0, 1)
        lim = torch.full((n,), tn, device=d)
        worst = max(worst, (got - attn_masked(q, K, V, lim)).abs().max().item())
        near = max(near, (got - attn_masked(q, K, V, lim - 1)).abs().max().item())
    print(f"prefill attn cross: worst {worst:.2e} (tol {TOL}); distance to text_len - 1 {near:.2e}")
    assert worst <= TOL, worst
    assert near >= 100 * TOL, near
    assert (out[pk["pad"]] == sentinel).all()


def test_dec_prefill_then_decode_step():
    """the decode step reads what the prefill wrote: after dia_dec_prefill_kv fills slots 0..n-1 (n = 300 and 129, both CFG
    rows), one dia_attn SELF step (bf16 caches, blocked V) at cur = n + 1 equals float64 attention over those slots plus the
    appended one"""
    d = dev()
    torch.manual_seed(53)
    lens = [300, 129]
    segs = [(1, 300), (3, 129), (0, 300), (2, 129)]
    pk = pack(segs, d)
    R, cap = 4, 320
    cos, sin = [t.to(d) for t in lay.rope_tables(cap + 2, HD, 1, 10000)]
    qkv_p = torch.randn(pk["rows"], NQKV, device=d)
    kc, vc = _garbage_caches(d, R, KVH, cap)
    _self_kv(d, pk, segs, qkv_p, kc, vc, cos, sin, cap)
    torch.cuda.synchronize()
    kpre, vpre = kc.clone(), lay.v_from_blocked(vc)
    qkv = torch.randn(R, NQKV, device=d)
    curs = torch.tensor([n + 1 for n in lens], dtype=torch.int32, device=d)
    P = torch.zeros(3, 1, QH * HD // 32, 64, 8, dtype=torch.bfloat16, device=d)
    at = hb.AttnArgs()
    at.mode, at.kv_dtype, at.n_kv_heads, at.group, at.n_rows, at.kv_cap = hb.ATTN_SELF, hb.KV_BF16, KVH, QH // KVH, R, cap
    at.q, at.ldq, at.q_off, at.k_off, at.v_off = hb.ptr(qkv), NQKV, 0, QH * HD, (QH + KVH) * HD
    at.kc, at.vc, at.cur = hb.ptr(kc), hb.ptr(vc), hb.ptr(curs)
    at.cos_t, at.sin_t, at.rope_rows = hb.ptr(cos), hb.ptr(sin), cos.shape[0]
    at.P, at.p_plane_stride, at.p_ktiles = hb.ptr(P), P[0].numel(), P.shape[2]
    scr = torch.zeros(hb.lib().dia_attn_scratch_floats(R, KVH, cap), device=d)
    tk = torch.zeros(R * KVH, dtype=torch.int32, device=d)
    at.scratch, at.tickets, at.v_blocked = hb.ptr(scr), hb.ptr(tk), 1
    hb.check(hb.lib().dia_attn(C.byref(at), None), "dia_attn")
    torch.cuda.synchronize()
    out = lay.unpack_planes(P, R, QH * HD).double().reshape(R, QH, HD)
    vr = lay.v_from_blocked(vc)
    worst = 0.0
    for r in range(R):
        n = lens[r >> 1]
        c, s = cos[n + 1].double(), sin[n + 1].double()
        q = rope(qkv[r, : QH * HD].double().reshape(QH, HD), c, s)
        kraw = qkv[r, QH * HD: (QH + KVH) * HD].double().reshape(KVH, HD)
        vnew = qkv[r, (QH + KVH) * HD:].reshape(KVH, HD)
        assert torch.equal(kc[r, :, :n], kpre[r, :, :n]) and torch.equal(vr[r, :, :n], vpre[r, :, :n])   # prefill slots kept
        assert torch.equal(vr[r, :, n], vnew.bfloat16())
        check_bf16(f"decode append row {r}", kc[r, :, n], rope(kraw, c, s), rope_fp32_err(kraw, c, s))
        K = kc[r, :, : n + 1].double().transpose(0, 1)                # the prefill's n slots and the appended one
        V = vr[r, :, : n + 1].double().transpose(0, 1)
        ref = attn_masked(q[None], K, V, torch.tensor([n + 1], device=d))[0]
        worst = max(worst, (out[r] - ref).abs().max().item())
    print(f"prefill -> decode step: worst {worst:.2e} (tol {TOL})")
    assert worst <= TOL, worst


# ---------------------------------------------------------------------------------------------------
# 3. dia_embed_text
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mapped", [False, True])
def test_embed_text_packed(mapped):
    """per utterance into the packed buffers as the encoder prefill calls it: x at row offs[b], planes at m-tile offs[b] / 16,
    ssq at column offs[b] with ssq_ld = Mp; mapped: plane columns through a cmap that drops entries"""
    d = dev()
    torch.manual_seed(61 + int(mapped))
    E, Vt = 1024, 256
    lens = [45, 0, 70, 1, 32, 129]
    offs, tot = [], 0
    for Lb in lens:
        offs.append(tot)
        tot += ceil(Lb, 32)
    Mp, kt = tot, E // 32
    table = torch.randn(Vt, E, device=d)
    gw = bf16r(1.0 + 0.1 * torch.randn(E, device=d))
    keep = torch.rand(E, device=d) < 0.6
    keep[:2] = torch.tensor([False, True], device=d)
    nk = int(keep.sum()) if mapped else E
    cmap = torch.where(keep, torch.cumsum(keep.int(), 0) - 1, torch.full((E,), -1, device=d, dtype=torch.int64)).to(torch.int32)
    sentinel = 7.0
    x = torch.full((Mp, E), sentinel, device=d)
    P = lay.pack_planes(torch.full((Mp, E), sentinel, device=d))
    ssq = torch.full((E // 16, Mp), sentinel, device=d)
    ids = [torch.randint(0, Vt, (Lb,), dtype=torch.int32, device=d) for Lb in lens]
    L = hb.lib()
    for b, Lb in enumerate(lens):
        if Lb == 0:
            continue
        o = offs[b]
        hb.check(L.dia_embed_text(hb.ptr(ids[b]), Lb, hb.ptr(table), E, hb.ptr(gw), x.data_ptr() + o * E * 4,
                                  P.data_ptr() + (o // 16) * kt * 512 * 2, P[0].numel(), kt, ssq.data_ptr() + o * 4, Mp,
                                  hb.ptr(cmap) if mapped else None, None), "dia_embed_text")
    torch.cuda.synchronize()
    live = torch.zeros(Mp, dtype=torch.bool, device=d)
    ref = torch.zeros(Mp, E, dtype=torch.float64, device=d)
    for b, Lb in enumerate(lens):
        live[offs[b]: offs[b] + Lb] = True
        ref[offs[b]: offs[b] + Lb] = table.double()[ids[b].long()]
    got_p = lay.unpack_planes(P, Mp, E)
    kept = keep if mapped else torch.ones(E, dtype=torch.bool, device=d)
    err = rel_err(x[live], ref[live])
    err_p = rel_err(got_p[live][:, :nk], (ref[live] * gw.double())[:, kept])
    want_ss = (ref[live] ** 2).reshape(-1, E // 16, 16).sum(-1).T
    err_s = rel_err(ssq[:, live], want_ss)
    print(f"embed_text cmap={mapped}: x {err:.2e}, planes {err_p:.2e}, ssq {err_s:.2e} (tol {TOL})")
    assert err <= TOL and err_p <= TOL and err_s <= TOL, (err, err_p, err_s)
    assert torch.equal(x[live], ref[live].float())                   # a row of the table, as is
    assert torch.equal(got_p[live][:, :nk], (x[live] * gw)[:, kept])
    assert (got_p[live][:, nk:] == sentinel).all()
    assert (x[~live] == sentinel).all() and (got_p[~live] == sentinel).all() and (ssq[:, ~live] == sentinel).all()


# ---------------------------------------------------------------------------------------------------
# 4. argument checks of the prefill entry points, real buffers behind every pointer (a missing check launches on valid memory
#    and fails the assertion; the outputs must not change)
# ---------------------------------------------------------------------------------------------------
def test_dec_prefill_argument_checks():
    d = dev()
    torch.manual_seed(71)
    L = hb.lib()
    segs = [(1, 40), (0, 40)]                 # 96 packed rows (a multiple of 32; 48 is not)
    pk = pack(segs, d)
    rows, cap, Cm, Dm = pk["rows"], 64, 17, 528
    cos, sin = [t.to(d) for t in lay.rope_tables(cap + 2, HD, 1, 10000)]
    tokens = torch.randint(0, V_, (1, TTOK, Cm), dtype=torch.int32, device=d)
    emb = torch.randn(Cm, V_, Dm, device=d)
    sentinel = 7.0
    x = torch.full((rows, Dm), sentinel, device=d)
    Pe = lay.pack_planes(torch.full((rows, Dm), sentinel, device=d))
    ssq = torch.full(((Dm + 15) // 16, rows), sentinel, device=d)
    qkv = torch.randn(rows, NQKV, device=d)
    kc, vc = _garbage_caches(d, 2, KVH, cap)
    kc0, vc0 = kc.clone(), vc.clone()
    Pa = lay.pack_planes(torch.full((rows, QH * HD), sentinel, device=d))
    Pa0 = Pa.clone()
    tl = torch.full((1,), 10, dtype=torch.int32, device=d)

    def embed(**kw):
        a = prefill_args(pk)
        a.tokens, a.T, a.C, a.V, a.D = hb.ptr(tokens), TTOK, C_, V_, D_
        a.emb, a.x = hb.ptr(emb), hb.ptr(x)
        a.P, a.p_plane_stride, a.p_ktiles, a.ssq, a.ssq_ld = hb.ptr(Pe), Pe[0].numel(), Pe.shape[2], hb.ptr(ssq), rows
        for k, v in kw.items():
            setattr(a, k, v)
        return L.dia_dec_prefill_embed(C.byref(a), None)

    def selfargs(**kw):
        a = prefill_args(pk)
        a.q, a.ldq, a.q_off, a.k_off, a.v_off = hb.ptr(qkv), NQKV, 0, QH * HD, (QH + KVH) * HD
        a.q_heads, a.kv_heads, a.kv_cap, a.causal = QH, KVH, cap, 1
        a.kc, a.vc, a.cos_t, a.sin_t = hb.ptr(kc), hb.ptr(vc), hb.ptr(cos), hb.ptr(sin)
        a.P, a.p_plane_stride, a.p_ktiles = hb.ptr(Pa), Pa[0].numel(), QH * HD // 32
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def rejected(rc, what):
        msg = L.dia_last_error().decode()
        print(f"{what}: rc {rc}, {msg}")
        assert rc == -1, (what, rc)

    rejected(embed(rows=48), "embed rows % 32")
    rejected(L.dia_dec_prefill_kv(C.byref(selfargs(rows=48)), None), "kv rows % 32")
    rejected(L.dia_dec_prefill_attn(C.byref(selfargs(rows=48)), None), "attn rows % 32")
    rejected(embed(C=Cm), "C > 16")
    rejected(embed(D=520), "D % 16")
    rejected(embed(p_ktiles=D_ // 32 - 1), "embed p_ktiles")
    rejected(L.dia_dec_prefill_attn(C.byref(selfargs(kv_heads=3)), None), "q_heads % kv_heads")
    rejected(L.dia_dec_prefill_kv(C.byref(selfargs(kv_cap=48)), None), "kv kv_cap % 32")
    rejected(L.dia_dec_prefill_attn(C.byref(selfargs(kv_cap=48)), None), "attn kv_cap % 32")
    rejected(L.dia_dec_prefill_attn(C.byref(selfargs(p_ktiles=QH * HD // 32 - 1)), None), "attn p_ktiles")
    # cross without text_len: only uncond segments (even cache rows), which never read text_len, so a missing check would
    # launch, write zeros and be seen
    pku = pack([(0, 40), (2, 33)], d)
    assert pku["rows"] == rows
    a = selfargs(causal=0, q_heads=CH, kv_heads=CH)
    a.row_seg, a.seg_off, a.seg_len, a.seg_row = hb.ptr(pku["row_seg"]), hb.ptr(pku["seg_off"]), hb.ptr(pku["seg_len"]), hb.ptr(pku["seg_row"])
    kx, vx = _garbage_caches(d, 2, CH, cap)
    a.kc, a.vc = hb.ptr(kx), hb.ptr(vx)
    rejected(L.dia_dec_prefill_attn(C.byref(a), None), "cross without text_len")
    torch.cuda.synchronize()
    # nothing was launched by any of the rejected calls
    assert (x == sentinel).all() and (ssq == sentinel).all() and (lay.unpack_planes(Pe, rows, Dm) == sentinel).all()
    assert torch.equal(kc, kc0) and torch.equal(vc, vc0) and torch.equal(Pa, Pa0)
    # the same cross call with text_len is accepted and writes the uncond zeros
    a.text_len = hb.ptr(tl)
    hb.check(L.dia_dec_prefill_attn(C.byref(a), None), "dia_dec_prefill_attn(cross)")
    torch.cuda.synchronize()
    assert (lay.unpack_planes(Pa, rows, CH * HD)[~pku["pad"]] == 0).all()
