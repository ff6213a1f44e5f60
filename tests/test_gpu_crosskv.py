"""The cross-K/V epilogue of dia_gemm (DIA_EPI_CROSSKV) on every kernel body gemm_impl sends it to and in every cache
format, through the C ABI, against a float64 restatement: K = RoPE(h . Wk) at the TEXT position, V = h . Wv, scattered into
the caches of the utterance a packed row belongs to (row_b / seg_off), optionally through a strip map and for several layers
in one launch.

Kernel bodies (csrc/gemm.hip, gemm_impl): the generic k_gemm (one m-tile, above 128 rows with few blocks, two- or three-plane
weights), the z-form of k_gemm16 (two m-tiles, or K per workgroup other than 1024), k_gemm2t with the shared 32-thread tail
(its own pre-loaded cos / sin) and with the all-thread cross-K/V tail (bf16, blocked V, no strip map), and k_gemm_tile_ws.
Every case states the kernel it expects (_cases, taken from reading gemm_impl) and checks the name the launch reports.

Bounds.  fp32 caches: TOL = 2e-5 of max(1, max |ref|), the figure of every fp32 kernel test here.  bf16 caches: one bf16 ulp of
the float64 value plus the fp32 allowance (bf16_bound, as in test_gpu_prefill.py).  Two-plane bf16 (bf16x2) caches: the format
is a run-time branch of kv_store on the same fp32 value, so the same launch with an fp32 cache gives that value v and the
planes must be bf16(v) and bf16(v - bf16(v)) bit for bit; and hi + lo is within TOL * scale + 2^-17 |ref| of float64, 2^-17
being the relative error include/dia_hip.h states for the format.  Every case pre-fills the caches (and guard areas before,
between and behind the planes) with sentinels and requires every element outside (listed utterance, live head, position below
the length, listed layer) to keep its sentinel.  Every case prints its worst error."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from dia_hip import binding as hb
from dia_hip import layout as lay

TOL = 2e-5
HD = 128
ROWS = 5                        # utterances (cache rows) the caches hold
GUARD = 1024                    # sentinel elements in front of the first plane and behind the last
S_HI, S_LO, S_GUARD = 3.0, -5.0, 7.0          # exact in bf16
FMT_CODE = {"f32": hb.KV_F32, "bf16": hb.KV_BF16, "bf16x2": hb.KV_BF16X2}


def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    return torch.device("cuda:0")


def bf16r(t):
    return t.bfloat16().float()


def ceil(v, m):
    return (v + m - 1) // m * m


def rope(x, c, s):
    """x [..., 128] float64, c / s broadcastable to [..., 64]"""
    return torch.cat([x[..., :64] * c - x[..., 64:] * s, x[..., :64] * s + x[..., 64:] * c], dim=-1)


# ---- the bf16 bound of test_gpu_prefill.py, unchanged --------------------------------------------------------------
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


# ---- the problems --------------------------------------------------------------------------------------------------
# packed batches: (utterance = cache row, text length) in packing order; every segment starts on a 32-row boundary, one
# utterance is empty, the cache rows not named are not in the batch, the rows behind a text are padding (row_b = -1).
# None: no row_b / seg_off — one utterance (kv_batch_index), position = row.
SHAPES = {
    # name: (rows M, K, heads, capacity, batch)
    "8": (8, 1024, 2, 64, None),
    "16": (16, 1024, 2, 64, None),
    "32": (32, 1024, 2, 64, [(3, 20), (1, 0)]),
    "40": (40, 1024, 2, 64, None),
    "96": (96, 1024, 2, 64, [(4, 33), (2, 0), (0, 31)]),
    "128": (128, 1024, 2, 96, [(1, 70), (4, 0), (3, 1)]),
    "160": (160, 1024, 2, 96, [(2, 96), (0, 0), (4, 33)]),
    "48k": (48, 2048, 2, 64, [(0, 30), (3, 0), (2, 9)]),        # K = 2048: 64 k-tiles per workgroup
    "64": (64, 1024, 2, 64, [(3, 32), (0, 0), (1, 20)]),
}
KV_BATCH_INDEX = 2              # the cache row of an unpacked launch


@functools.lru_cache(maxsize=None)
def problem(shape, maps, w_planes):
    """inputs of one launch and its float64 caches, built once per (shape, maps, weight planes) and shared, never changed.
    maps: two layers in one launch (kv_layer_strips) behind a strip map that drops head 0 of layer 0."""
    d = dev()
    M, E, H, cap, batch = SHAPES[shape]
    torch.manual_seed(sum(map(ord, shape)) * 7 + 3 * int(maps) + w_planes)
    layers = 2 if maps else 1
    Mg = ceil(M, 64)                                         # rows a grid of four m-tiles per workgroup covers
    x = torch.randn(M, E, device=d)
    gw = bf16r(1.0 + 0.1 * torch.randn(E, device=d))
    xg = x * gw
    ssq = torch.zeros(E // 16, Mg, dtype=torch.float32, device=d)
    ssq[:, :M] = (x.double() ** 2).reshape(M, E // 16, 16).sum(-1).T.float()
    A = lay.pack_planes(xg, mtiles=Mg // 16)
    rb = np.full((Mg,), -1, dtype=np.int32)
    so = np.full((ROWS,), 1 << 20, dtype=np.int32)           # (entries of utterances not in the batch are never read)
    lens = {}
    if batch is not None:
        off = 0
        for u, Lb in batch:
            rb[off: off + Lb] = u
            so[u] = off
            lens[u] = Lb
            off += ceil(Lb, 32)
        assert off - 32 < M <= off and (rb[M:] < 0).all() and any(Lb == 0 for _, Lb in batch) and len(batch) < ROWS
        assert (rb[:M] < 0).any()                            # padding rows
        row_b, seg_off = torch.from_numpy(rb).to(d), torch.from_numpy(so).to(d)
        rows_live = torch.from_numpy(rb[:M] >= 0).to(d)
        bi = row_b[:M][rows_live].long()
        pi = (torch.arange(M, device=d)[rows_live] - seg_off[bi]).long()
    else:
        assert M <= cap
        row_b = seg_off = None
        lens[KV_BATCH_INDEX] = M
        rows_live = torch.ones(M, dtype=torch.bool, device=d)
        bi = torch.full((M,), KV_BATCH_INDEX, device=d)
        pi = torch.arange(M, device=d)
    perm = lay.rope_pair_perm(HD).to(d)
    inv_perm = torch.argsort(perm)
    live = [torch.ones(H, dtype=torch.bool) for _ in range(layers)]
    if maps:
        live[0][0] = False
    cols, smap, lmaps, weff = [], [], [], []
    for l in range(layers):
        wk = torch.randn(E, H, HD, device=d) * 0.05
        wv = torch.randn(E, H, HD, device=d) * 0.05
        if w_planes <= 1:
            wk, wv = bf16r(wk), bf16r(wv)                    # (two / three planes: weights bf16 cannot hold)
        Wl = torch.cat([wk[:, :, perm].reshape(E, -1), wv.reshape(E, -1)], dim=1)
        strips = [s for h in torch.nonzero(live[l]).flatten().tolist() for s in range(h * 8, h * 8 + 8)]
        strips += [H * 8 + s for s in strips]
        cols.append(Wl[:, (torch.tensor(strips)[:, None] * 16 + torch.arange(16)[None, :]).reshape(-1).to(d)])
        lmaps.append(strips)
        smap += [l * H * 16 + s for s in strips]
        weff.append(Wl)
    if w_planes == 2:
        assert layers == 1 and not maps
        Wt, kt, ns = lay.tile_weight_bf16x2(cols[0])
        hi, lo = lay.untile_weight_bf16x2(Wt, E, 2 * H * HD)
        weff = [hi.double() + lo.double()]                   # the reference multiplies what the two planes hold
    elif w_planes == 3:
        assert layers == 1 and not maps
        Wt, kt, ns = lay.tile_weight_planes(cols[0])         # hi + mid + lo == w exactly
    else:
        Wt, kt, ns = lay.tile_weight(torch.cat(cols, dim=1))
    per_layer = []
    if maps:
        for l in range(layers):
            t, _, n = lay.tile_weight(cols[l])
            per_layer.append((t, n, torch.tensor(lmaps[l], dtype=torch.int32, device=d)))
    cos, sin = [t.to(d) for t in lay.rope_tables(cap + 1, HD, 1, 10000)]
    # float64 caches [layers, ROWS, H, cap, 128] where a value belongs, and the mask of those places
    h64 = xg.double() * torch.rsqrt(ssq[:, :M].double().sum(0) / E + 1e-5)[:, None]       # the scale from ssq as the kernel sees it
    shape5 = (layers, ROWS, H, cap, HD)
    refk = torch.zeros(shape5, dtype=torch.float64, device=d)
    refv = torch.zeros(shape5, dtype=torch.float64, device=d)
    written = torch.zeros(shape5[:4], dtype=torch.bool, device=d)
    for l in range(layers):
        f = h64[rows_live] @ weff[l].double()
        k = f[:, : H * HD].reshape(-1, H, HD)[:, :, inv_perm]
        v = f[:, H * HD:].reshape(-1, H, HD)
        kr = rope(k, cos.double()[pi][:, None, :], sin.double()[pi][:, None, :])          # RoPE by text position; V is not roped
        lv = live[l].to(d)
        refk[l][bi, :, pi] = torch.where(lv[None, :, None], kr, refk[l][bi, :, pi])
        refv[l][bi, :, pi] = torch.where(lv[None, :, None], v, refv[l][bi, :, pi])
        written[l][bi, :, pi] = lv[None, :].expand(bi.numel(), H)
    assert int(written.sum()) == sum(lens.values()) * sum(int(lv.sum()) for lv in live) > 0
    return dict(M=M, E=E, H=H, cap=cap, layers=layers, Mg=Mg, A=A, ssq=ssq, row_b=row_b, seg_off=seg_off, Wt=Wt, kt=kt, ns=ns,
                smap=torch.tensor(smap, dtype=torch.int32, device=d) if maps else None, per_layer=per_layer,
                cos=cos, sin=sin, refk=refk, refv=refv, written=written, w_planes=w_planes)


class Caches:
    """K and V caches of every layer in one allocation each: [guard | plane | (lo plane) | guard], sentinels everywhere"""

    def __init__(self, pb, fmt, vblocked):
        d = dev()
        self.pb, self.fmt, self.vb = pb, fmt, vblocked
        self.planes = 2 if fmt == "bf16x2" else 1
        self.layer = ROWS * pb["H"] * pb["cap"] * HD         # elements of one layer
        self.plane = pb["layers"] * self.layer               # elements of one plane
        dt = torch.float32 if fmt == "f32" else torch.bfloat16
        self.buf = []
        for _ in range(2):
            b = torch.full((2 * GUARD + self.planes * self.plane,), S_GUARD, dtype=dt, device=d)
            b[GUARD: GUARD + self.plane] = S_HI
            if self.planes == 2:
                b[GUARD + self.plane: GUARD + 2 * self.plane] = S_LO
            self.buf.append(b)

    def base(self, which, layer=0):
        b = self.buf[which]
        return b.data_ptr() + (GUARD + layer * self.layer) * b.element_size()

    def plane_of(self, which, p):
        """plane p of K (which = 0) or V (1) as [layers, ROWS, H, cap, 128], V out of the blocked layout"""
        pb = self.pb
        t = self.buf[which][GUARD + p * self.plane: GUARD + (p + 1) * self.plane]
        if which == 1 and self.vb:
            return lay.v_from_blocked(t.reshape(pb["layers"], ROWS, pb["H"], pb["cap"] // 32, HD, 32))
        return t.reshape(pb["layers"], ROWS, pb["H"], pb["cap"], HD)

    def check_untouched(self):
        w = self.pb["written"]
        for which in (0, 1):
            b = self.buf[which]
            assert (b[:GUARD] == S_GUARD).all() and (b[GUARD + self.planes * self.plane:] == S_GUARD).all(), "a guard area was written"
            for p, s in zip(range(self.planes), (S_HI, S_LO)):
                assert (self.plane_of(which, p)[~w] == s).all(), f"{'KV'[which]} plane {p}: an element outside the batch was written"


def launch(pb, c, *, layer=None):
    """one CROSSKV launch into the caches c: the merged launch (layer = None), or one layer of a merged problem alone"""
    g = hb.GemmArgs()
    A = pb["A"]
    g.A, g.a_plane_stride, g.a_ktiles, g.M = hb.ptr(A), A[0].numel(), A.shape[2], pb["M"]
    g.epi, g.w_planes = hb.EPI_CROSSKV, pb["w_planes"]
    g.ssq_in, g.ssq_in_n, g.inv_d, g.eps, g.ssq_ld = hb.ptr(pb["ssq"]), pb["E"] // 16, 1.0 / pb["E"], 1e-5, pb["Mg"]
    g.kv_dtype, g.kv_heads, g.kv_cap, g.kv_batch_index = FMT_CODE[c.fmt], pb["H"], pb["cap"], KV_BATCH_INDEX if pb["row_b"] is None else 0
    g.cos_t, g.sin_t, g.kv_vblocked = hb.ptr(pb["cos"]), hb.ptr(pb["sin"]), int(c.vb)
    g.row_b, g.seg_off = hb.ptr(pb["row_b"]), hb.ptr(pb["seg_off"])
    g.kv_plane_stride = c.plane if c.planes == 2 else 0
    if layer is None:
        g.W, g.KT, g.nstrips = hb.ptr(pb["Wt"]), pb["kt"], pb["ns"]
        g.kc, g.vc = c.base(0), c.base(1)
        if pb["smap"] is not None:
            g.strip_map, g.kv_layer_strips, g.kv_layer_stride = hb.ptr(pb["smap"]), pb["H"] * 16, c.layer
    else:
        t, n, sm = pb["per_layer"][layer]
        g.W, g.KT, g.nstrips, g.strip_map = hb.ptr(t), pb["kt"], n, hb.ptr(sm)
        g.kc, g.vc = c.base(0, layer), c.base(1, layer)
    return timed_gemm(g)


def bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


# ---- the table -----------------------------------------------------------------------------------------------------
GENERIC, ZFORM, TILE = "k_gemm<", "k_gemm16<", "k_gemm_tile_ws<"
# k_gemm2t<KPW, AF32, SPLITK, NW, CKV, EPI, SK2>: the all-thread cross-K/V tail is CKV = true; the shared 32-thread tail is the
# plain half form (CKV = false, run-time epilogue EPI = -1)
G2T_CKV, G2T_SHARED = "k_gemm2t<8, false, false, 4, true,", "k_gemm2t<8, false, false, 4, false, -1,"
F32, BF16, X2 = ("f32", 0), ("bf16", 1), ("bf16x2", 1)              # (format, V blocked): what dia_attn reads
F32_BLK, X2_ROW = ("f32", 1), ("bf16x2", 0)                          # what only the epilogue supports

# gemm_impl, for plane inputs without split-K (m-tiles = ceil(M / 16), ktw = K / 32):
#   one m-tile: CROSSKV is not a fast epilogue, so k_gemm16 does not take it                            -> k_gemm
#   3..8 m-tiles and ktw == 32: k_gemm2t (prefill_ok); CKV tail for bf16 + blocked V + no strip map + knob gemm_2t != 4,
#     else the half form with the shared tail                                                           -> k_gemm2t
#   2..8 m-tiles otherwise (two m-tiles; ktw == 64, where prefill_ok wants ktw == 32): the z-form       -> k_gemm16
#   above 8 m-tiles: the tiled kernel when its 64 x 256 blocks reach tile_min_blocks, else               -> k_gemm_tile_ws / k_gemm
#   w_planes = 2 (not fp32 tiles) or 3: the generic kernel whatever the shape                            -> k_gemm
KNOB_TILE, KNOB_GENERIC, KNOB_SHARED = {"tile_min_blocks": 1}, {"tile_min_blocks": 1 << 30}, {"gemm_2t": 4}


def _cases():
    out = []

    def add(shape, fmt, want, knobs=None, maps=False, w_planes=0, tag=""):
        name = f"{shape}-{fmt[0]}{'-blockedV' if fmt == F32_BLK else '-rowV' if fmt == X2_ROW else ''}{'-maps' if maps else ''}{tag}"
        out.append(pytest.param(shape, fmt, want, knobs or {}, maps, w_planes, id=name))

    for shape, want, knobs, tag in (("8", GENERIC, None, ""), ("16", GENERIC, None, ""), ("32", ZFORM, None, ""), ("40", None, None, ""),
                                    ("96", None, None, ""), ("128", None, None, ""), ("160", TILE, KNOB_TILE, "-tile"),
                                    ("160", GENERIC, KNOB_GENERIC, "-generic"), ("48k", ZFORM, None, "")):
        for fmt in (F32, BF16, X2):
            add(shape, fmt, want or (G2T_CKV if fmt == BF16 else G2T_SHARED), knobs, tag=tag)
    # formats only the epilogue supports, once per path
    for shape, want, knobs, tag in (("16", GENERIC, None, ""), ("32", ZFORM, None, ""), ("96", G2T_SHARED, None, ""), ("160", TILE, KNOB_TILE, "-tile")):
        add(shape, F32_BLK, want, knobs, tag=tag)
        add(shape, X2_ROW, want, knobs, tag=tag)
    # the shared tail on the shapes that default to the all-thread tail
    add("96", BF16, G2T_SHARED, KNOB_SHARED, tag="-2t4")
    add("128", BF16, G2T_SHARED, KNOB_SHARED, tag="-2t4")
    # two layers in one launch behind a strip map (a strip map keeps bf16 + blocked V off the all-thread tail)
    for shape, want, knobs, tag in (("32", ZFORM, None, ""), ("96", G2T_SHARED, None, ""), ("160", TILE, KNOB_TILE, "-tile")):
        for fmt in (F32, BF16, X2):
            add(shape, fmt, want, knobs, maps=True, tag=tag)
    # two- and three-plane weights
    add("64", X2, GENERIC, w_planes=2, tag="-w2")
    add("64", X2, GENERIC, w_planes=3, tag="-w3")
    return out


@pytest.mark.parametrize("shape,fmt,want,knobs,maps,w_planes", _cases())
def test_gemm_crosskv_paths(shape, fmt, want, knobs, maps, w_planes, tuning):
    """One CROSSKV launch per (kernel path, cache format): kernel name, nothing stray, the values against float64.
    bf16x2: the planes against the fp32 value of the same kernel, bit for bit.  maps: the merged launch against one launch per
    layer, bit for bit.  Knob gemm_2t = 4 on bf16: the cache equals the hi plane of the bf16x2 run, bit for bit."""
    kvd, vb = fmt
    for k, v in knobs.items():
        tuning(k, v)
    pb = problem(shape, maps, w_planes)
    name_id = f"crosskv {shape} {kvd}{' blockedV' if vb else ' rowV'}{' maps' if maps else ''}{f' w_planes={w_planes}' if w_planes else ''} {knobs or ''}"
    c = Caches(pb, kvd, vb)
    name = launch(pb, c)
    print("kernel", name)
    assert name.startswith(want), (name, want)
    c.check_untouched()
    w, refk, refv = pb["written"], pb["refk"][pb["written"]], pb["refv"][pb["written"]]
    sk, sv = max(1.0, refk.abs().max().item()), max(1.0, refv.abs().max().item())
    if kvd == "f32":
        gk, gv = c.plane_of(0, 0)[w].double(), c.plane_of(1, 0)[w].double()
        ek, ev = (gk - refk).abs().max().item() / sk, (gv - refv).abs().max().item() / sv
        print(f"{name_id}: K {ek:.2e}, V {ev:.2e} (tol {TOL})")
        assert ek <= TOL and ev <= TOL, (ek, ev)
    elif kvd == "bf16":
        check_bf16(f"{name_id} K", c.plane_of(0, 0)[w], refk, TOL * sk)
        check_bf16(f"{name_id} V", c.plane_of(1, 0)[w], refv, TOL * sv)
    else:
        # 1. the fp32 value of the same kernel instantiation, split as kv_store splits it
        f = Caches(pb, "f32", vb)
        name_f = launch(pb, f)
        assert name_f == name, (name_f, name)
        for which in (0, 1):
            v32 = f.plane_of(which, 0)[w]
            hi = v32.bfloat16()
            lo = (v32 - hi.float()).bfloat16()               # (the subtraction is exact in fp32)
            assert torch.equal(bits(c.plane_of(which, 0)[w]), bits(hi)), f"{name_id} {'KV'[which]}: hi plane is not bf16(v)"
            assert torch.equal(bits(c.plane_of(which, 1)[w]), bits(lo)), f"{name_id} {'KV'[which]}: lo plane is not bf16(v - hi)"
        # 2. hi + lo against float64
        worst = []
        for which, ref, s in ((0, refk, sk), (1, refv, sv)):
            got = c.plane_of(which, 0)[w].double() + c.plane_of(which, 1)[w].double()
            dlt = (got - ref).abs()
            worst.append((dlt / s).max().item())
            assert (dlt <= TOL * s + 2.0 ** -17 * ref.abs()).all(), (name_id, "KV"[which], worst[-1])
        print(f"{name_id}: hi + lo K {worst[0]:.2e}, V {worst[1]:.2e} of the scale (bound {TOL} + 2^-17 |ref|)")
    if knobs.get("gemm_2t") == 4 and kvd == "bf16":
        x2 = Caches(pb, "bf16x2", vb)
        assert launch(pb, x2) == name
        for which in (0, 1):
            assert torch.equal(bits(c.plane_of(which, 0)), bits(x2.plane_of(which, 0))), f"{name_id} {'KV'[which]}: bf16 cache != hi plane of the bf16x2 run"
    if maps:
        per = Caches(pb, kvd, vb)
        for l in range(pb["layers"]):
            launch(pb, per, layer=l)
        per.check_untouched()
        for which in (0, 1):
            assert torch.equal(bits(c.buf[which]), bits(per.buf[which])), f"{name_id} {'KV'[which]}: merged launch != one launch per layer"


# ---- writer -> reader ----------------------------------------------------------------------------------------------
LOOP_LENS, LOOP_CAP, LOOP_H, LOOP_CURS = [40, 70], 96, 4, [5, 60]
SENTINEL_OUT = 5.0
SCALE = 1.0 / math.sqrt(128.0)


def attn64(q, K, V):
    """q [H, 128], K / V [H, keys, 128] float64 -> [H, 128]"""
    p = torch.softmax(torch.einsum("hd,htd->ht", q, K) * SCALE, dim=-1)
    return torch.einsum("ht,htd->hd", p, V)


@pytest.mark.parametrize("kvd", ["f32", "bf16", "bf16x2"])
def test_crosskv_caches_read_by_cross_attention(kvd):
    """CROSSKV writes the caches of two utterances (40 and 70 text bytes, capacity 96, 4 heads) in the layout dia_attn requires
    for the format; dia_attn (CROSS) reads them; the output is compared with float64 attention over the float64 K / V of the same
    projection — no host layout helper between the writer and the reader.  Bound 2e-5 for f32 and bf16x2.

    bf16: test_gpu_attn_decode.py has no bound against an unrounded reference (every bf16 comparison there is against the
    values the cache holds, to 2e-5), and the rounding of K and V alone moves the output by 2.0e-3 here, so none is made up:
    the writer is held to one bf16 ulp of the float64 projection (check_bf16), the reader to that file's 2e-5 of float64
    attention over the values the writer stored, V taken out of the blocked layout by the index rule of include/dia_hip.h
    ([key / 32][128 dims][32 keys]) written out below; the distance to the unrounded reference is printed."""
    d = dev()
    torch.manual_seed(29)
    E, H, cap, B = 1024, LOOP_H, LOOP_CAP, len(LOOP_LENS)
    offs = [0, ceil(LOOP_LENS[0], 32)]
    Mp = offs[1] + ceil(LOOP_LENS[1], 32)
    rb = np.full((Mp,), -1, dtype=np.int32)
    for b, (o, Lb) in enumerate(zip(offs, LOOP_LENS)):
        rb[o: o + Lb] = b
    row_b, seg_off = torch.from_numpy(rb).to(d), torch.tensor(offs, dtype=torch.int32, device=d)
    x = torch.randn(Mp, E, device=d)
    gw = bf16r(1.0 + 0.1 * torch.randn(E, device=d))
    xg = x * gw
    ssq = torch.zeros(E // 16, Mp, device=d)
    ssq[:] = (x.double() ** 2).reshape(Mp, E // 16, 16).sum(-1).T.float()
    wk = bf16r(torch.randn(E, H, HD, device=d) * 0.03)                  # K, V ~ N(0, 1), the scale of the attention tests
    wv = bf16r(torch.randn(E, H, HD, device=d) * 0.03)
    perm = lay.rope_pair_perm(HD).to(d)
    Wt, kt, ns = lay.tile_weight(torch.cat([wk[:, :, perm].reshape(E, -1), wv.reshape(E, -1)], dim=1))
    cos, sin = [t.to(d) for t in lay.rope_tables(cap + 1, HD, 1, 10000)]
    two, blocked = kvd == "bf16x2", kvd != "f32"
    plane = B * H * cap * HD
    dt = torch.float32 if kvd == "f32" else torch.bfloat16
    kc = torch.full(((2 if two else 1) * plane,), 3.0, dtype=dt, device=d)
    vc = torch.full_like(kc, 3.0)
    A = lay.pack_planes(xg, mtiles=ceil(Mp, 64) // 16)
    g = hb.GemmArgs()
    g.A, g.a_plane_stride, g.a_ktiles, g.M = hb.ptr(A), A[0].numel(), A.shape[2], Mp
    g.W, g.KT, g.nstrips, g.epi = hb.ptr(Wt), kt, ns, hb.EPI_CROSSKV
    g.ssq_in, g.ssq_in_n, g.inv_d, g.eps, g.ssq_ld = hb.ptr(ssq), E // 16, 1.0 / E, 1e-5, Mp
    g.kc, g.vc, g.kv_dtype, g.kv_heads, g.kv_cap, g.kv_batch_index = hb.ptr(kc), hb.ptr(vc), FMT_CODE[kvd], H, cap, 0
    g.cos_t, g.sin_t, g.kv_vblocked, g.kv_plane_stride = hb.ptr(cos), hb.ptr(sin), int(blocked), plane if two else 0
    g.row_b, g.seg_off = hb.ptr(row_b), hb.ptr(seg_off)
    print("kernel", timed_gemm(g))
    # the reader
    q = torch.randn(2 * B, H * HD, device=d)
    cur = torch.tensor(LOOP_CURS, dtype=torch.int32, device=d)
    ln = torch.tensor(LOOP_LENS, dtype=torch.int32, device=d)
    P = lay.pack_planes(torch.full((16, H * HD), SENTINEL_OUT, device=d))
    scr = torch.zeros(hb.lib().dia_attn_scratch_floats(B, H, cap), device=d)
    tk = torch.zeros(B * H, dtype=torch.int32, device=d)
    a = hb.AttnArgs()
    a.mode, a.kv_dtype, a.n_kv_heads, a.group, a.n_rows, a.kv_cap = hb.ATTN_CROSS, FMT_CODE[kvd], H, 1, B, cap
    a.q, a.ldq, a.q_off = hb.ptr(q), H * HD, 0
    a.kc, a.vc, a.cur, a.len = hb.ptr(kc), hb.ptr(vc), hb.ptr(cur), hb.ptr(ln)
    a.cos_t, a.sin_t, a.rope_rows = hb.ptr(cos), hb.ptr(sin), cos.shape[0]
    a.P, a.p_plane_stride, a.p_ktiles = hb.ptr(P), P[0].numel(), H * 4
    a.scratch, a.tickets = hb.ptr(scr), hb.ptr(tk)
    a.v_blocked, a.kv_plane_stride = int(blocked), plane if two else 0
    hb.check(hb.lib().dia_attn(C.byref(a), None), "dia_attn")
    torch.cuda.synchronize()
    assert (tk == 0).all()
    out = lay.unpack_planes(P, 16, H * HD).double().reshape(16, H, HD)
    assert (out[2 * B:] == SENTINEL_OUT).all()
    # float64 K / V of the projection
    h64 = xg.double() * torch.rsqrt(ssq.double().sum(0) / E + 1e-5)[:, None]
    qc = rope(q.double().reshape(2 * B, H, HD)[1::2], cos.double()[cur.long()][:, None, :], sin.double()[cur.long()][:, None, :])
    worst = worst_unrounded = 0.0
    for b, (o, Lb) in enumerate(zip(offs, LOOP_LENS)):
        hb_ = h64[o: o + Lb]
        k64 = rope(torch.einsum("me,ehd->mhd", hb_, wk.double()), cos.double()[:Lb][:, None, :], sin.double()[:Lb][:, None, :]).transpose(0, 1)
        v64 = torch.einsum("me,ehd->mhd", hb_, wv.double()).transpose(0, 1)                 # [H, keys, 128]
        ref = attn64(qc[b], k64, v64)
        assert (out[2 * b] == 0).all()                                                      # the unconditional row
        e_unr = (out[2 * b + 1] - ref).abs().max().item()
        worst_unrounded = max(worst_unrounded, e_unr)
        if kvd != "bf16":
            worst = max(worst, e_unr)
            continue
        kh = kc.reshape(B, H, cap, HD)[b, :, :Lb]
        t_ = torch.arange(Lb, device=d)
        idx = ((b * H + torch.arange(H, device=d))[:, None, None] * cap * HD + (t_ // 32)[None, :, None] * (HD * 32)
               + torch.arange(HD, device=d)[None, None, :] * 32 + (t_ % 32)[None, :, None])
        vh = vc[idx]
        check_bf16(f"loop bf16 utterance {b} K", kh, k64, TOL * max(1.0, k64.abs().max().item()))
        check_bf16(f"loop bf16 utterance {b} V", vh, v64, TOL * max(1.0, v64.abs().max().item()))
        worst = max(worst, (out[2 * b + 1] - attn64(qc[b], kh.double(), vh.double())).abs().max().item())
    print(f"crosskv -> attn {kvd}: worst abs error {worst:.3e} (bound {TOL:.0e}); against the unrounded reference {worst_unrounded:.3e}")
    assert worst <= TOL, worst
