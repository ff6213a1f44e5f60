"""The MXFP8 weight stream (dia_gemm_args.w_format = DIA_W_MXFP8, csrc/gemm_mx.hip) on a real MI355X, through the C ABI.
Reference: the float64 product of the fp32 activations with the DEQUANTISED weights (an MXFP8 value is exactly a bf16 value, so
the stream is a second encoding of numbers the dense tiles hold exactly).  Bound: 2e-5 relative to the output scale, the
project's GEMM bound (tests/test_gpu_kernels.py); in every case the dense dia_gemm on tile_weight(dequantised) must meet it
too — it is the yardstick: a case the dense kernel fails is a wrong case, not a wrong feature."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from dia_hip import binding as hb
from dia_hip import layout as lay
from dia_hip.quant import is_mxfp8, mxfp8_round_2d

TOL = 2e-5


def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    return torch.device("cuda:0")


def gemm(X, w, epi, *, fp8, sk=None, ssq=True, x0=None, gnext=None, spw=0, expect=hb.check, ssq_n=8):
    """one dia_gemm launch with fp32 activation tiles in and out; returns (out, emitted activations [M, width], ssq_out, ssq_in)"""
    d = dev()
    M, K = X.shape
    N = w.shape[1]
    Np = (N + 15) // 16 * 16
    A = lay.pack_f32_tiles(X.to(d), ktiles=K // 32)
    Wt, kt, ns_ = lay.tile_weight_fp8(w) if fp8 else lay.tile_weight(w)
    Wt = Wt.to(d)
    g = hb.GemmArgs()
    g.A, g.a_ktiles, g.M = hb.ptr(A), K // 32, M
    g.W, g.KT, g.nstrips, g.epi, g.spw = hb.ptr(Wt), kt, ns_, epi, spw
    g.act_f32 = 3
    g.w_format = hb.W_MXFP8 if fp8 else 0
    ssq_ld = 16
    keep = [A, Wt]
    sin = None
    if ssq:
        sin = (torch.rand(ssq_n, ssq_ld, generator=torch.Generator().manual_seed(M + K)) + 0.5).to(d)
        g.ssq_in, g.ssq_in_n, g.inv_d, g.eps = hb.ptr(sin), ssq_n, 1.0 / (8 * ssq_n), 1e-5
    g.ssq_ld = ssq_ld
    out = P = sso = None
    if epi == hb.EPI_SCALE_STORE:
        out = torch.zeros(M, Np, device=d)
        g.out, g.ldo = hb.ptr(out), Np
    elif epi == hb.EPI_RESID_EMIT:
        out = x0.clone().to(d)
        P = torch.zeros(1, Np // 32, 64, 8, device=d)
        sso = torch.zeros(ns_, ssq_ld, device=d)
        gn = gnext.to(d)
        keep.append(gn)
        g.out, g.ldo, g.gnext, g.P, g.p_ktiles, g.ssq_out = hb.ptr(out), Np, hb.ptr(gn), hb.ptr(P), Np // 32, hb.ptr(sso)
    else:
        P = torch.zeros(1, max(1, Np // 64), 64, 8, device=d)
        g.P, g.p_ktiles = hb.ptr(P), max(1, Np // 64)
    tk = None
    if sk is not None:
        scr = torch.zeros(ns_ * sk * 256, device=d)
        tk = torch.zeros(ns_, dtype=torch.int32, device=d)
        g.sk_scratch, g.sk_tickets, g.sk, g.sk_scratch_floats = hb.ptr(scr), hb.ptr(tk), sk, scr.numel()
        keep += [scr, tk]
    rc = hb.lib().dia_gemm(C.byref(g), None)
    if expect is not hb.check:
        return rc
    hb.check(rc, "dia_gemm")
    torch.cuda.synchronize()
    if tk is not None:
        assert (tk == 0).all()
    emitted = None
    if P is not None:
        width = Np if epi == hb.EPI_RESID_EMIT else Np // 2
        emitted = lay.unpack_f32_tiles(P, M, width).cpu()
    return (out.cpu() if out is not None else None), emitted, (sso.cpu() if sso is not None else None), (sin.cpu() if ssq else None)


def reference(X, w, epi, sin=None, x0=None, gnext=None):
    """float64 restatement of the three decode epilogues"""
    X64, W64 = X.double(), w.double()
    M = X.shape[0]
    inv = torch.ones(M, dtype=torch.float64)
    if sin is not None:
        inv = torch.rsqrt(sin[:, :M].double().sum(dim=0) / (8 * sin.shape[0]) + 1e-5)
    acc = X64 @ W64
    if epi == hb.EPI_SCALE_STORE:
        return acc * inv[:, None], None, None
    if epi == hb.EPI_RESID_EMIT:
        x = x0.double() + acc
        ssq = (x * x).reshape(M, -1, 16).sum(dim=2).T
        return x, x * gnext.double(), ssq
    s = acc.reshape(M, -1, 2, 8) * inv[:, None, None, None]
    gate, up = s[:, :, 0], s[:, :, 1]
    return None, (gate / (1 + torch.exp(-gate)) * up).reshape(M, -1), None


def check_close(got, want, what, tol=TOL):
    scale = max(want.abs().max().item(), 1e-6)
    err = (got.double() - want).abs().max().item()
    print(f"{what}: max err {err:.3e} = {err / scale:.3e} of the output scale {scale:.3e}")
    assert err <= tol * scale, (what, err, scale)


def case(M, K, N, epi, seed, sk=None, spw=0, ssq_n=8):
    gen = torch.Generator().manual_seed(seed)
    X = torch.randn(M, K, generator=gen)
    w = torch.randn(K, N, generator=gen) * 0.05
    w[:, 0] *= 2.0 ** -20                                   # blocks with very different scales inside one strip
    w[32:64, 1] = 0.0                                       # an all-zero block
    w = mxfp8_round_2d(w)                                   # the DEQUANTISED weights: what both kernels and the reference multiply
    assert is_mxfp8(w) and torch.equal(w.bfloat16().float(), w)
    Np = (N + 15) // 16 * 16
    x0 = torch.randn(M, Np, generator=gen) if epi == hb.EPI_RESID_EMIT else None
    gn = (torch.rand(Np, generator=gen) + 0.5) if epi == hb.EPI_RESID_EMIT else None
    ssq = epi != hb.EPI_RESID_EMIT
    f8 = gemm(X, w, epi, fp8=True, sk=sk, ssq=ssq, x0=x0, gnext=gn, spw=spw, ssq_n=ssq_n)
    dn = gemm(X, w, epi, fp8=False, sk=sk, ssq=ssq, x0=x0, gnext=gn, spw=spw, ssq_n=ssq_n)
    wp = torch.zeros(K, Np)
    wp[:, :N] = w
    ro, re, rs = reference(X, wp, epi, sin=f8[3], x0=x0, gnext=gn)
    if ro is not None:
        check_close(dn[0], ro, "dense out")
        check_close(f8[0], ro, "mxfp8 out")
    if re is not None:
        check_close(dn[1], re, "dense emitted")
        check_close(f8[1], re, "mxfp8 emitted")
    if rs is not None:
        check_close(dn[2][:, :M], rs, "dense ssq")
        check_close(f8[2][:, :M], rs, "mxfp8 ssq")


def test_operand_probe():
    """One k-tile at a time: one-hot weights with a distinct scale per (k-tile, column) pin the element order inside a slot, the
    slot halves and the scale block's [column][k-tile] order."""
    K, N, M = 1024, 16, 16
    gen = torch.Generator().manual_seed(11)
    X = torch.randn(M, K, generator=gen)
    for t in (0, 1, 6, 15, 16, 31):
        w = torch.zeros(K, N)
        for c in range(N):
            for j in range(32):
                w[32 * t + j, c] = float(1 + (c + j) % 7) * 2.0 ** ((c % 5) - 3 * (t % 3))
        assert is_mxfp8(w)
        out = gemm(X, w, hb.EPI_SCALE_STORE, fp8=True, ssq=False)[0]
        check_close(out, X.double() @ w.double(), f"probe k-tile {t}", tol=1e-6)


@pytest.mark.parametrize("M", [1, 2, 4, 5, 8, 16])
@pytest.mark.parametrize("K", [512, 2048])
@pytest.mark.parametrize("epi", [0, 1, 2])
def test_mxfp8_gemm_vs_float64_and_dense(M, K, epi):
    case(M, K, 128 if epi != 2 else 256, epi, seed=M * 131 + K + epi)


@pytest.mark.parametrize("M,sk", [(1, 2), (2, 2), (4, 2), (5, 4), (8, 4), (16, 4)])
def test_mxfp8_wo_split_k(M, sk):
    case(M, 8192, 2048, hb.EPI_RESID_EMIT, seed=M + 17 * sk, sk=sk)


@pytest.mark.parametrize("M", [2, 4, 8, 16])
def test_mxfp8_logits_shape(M):
    """the logits head: N = 9 * 1028 (padded to 579 strips), K = 2048: the persistent multi-strip form at every row count"""
    case(M, 2048, 9 * 1028, hb.EPI_SCALE_STORE, seed=M + 5)


@pytest.mark.parametrize("M", [2, 16])
def test_mxfp8_wi_persistent_form(M):
    """wi: 1024 strips (4 strips per workgroup, next strip prefetched), SWIGLU_EMIT"""
    case(M, 2048, 16384, hb.EPI_SWIGLU_EMIT, seed=99 + M)


def test_mxfp8_row_scales_past_128_partials():
    """ssq_in_n = 136 (D = 2176): the row-scale reduction's tail loop behind the 16 partials a thread requests at once (the MX
    kernel has at least two waves, so no thread serves a second row: that branch runs in the 2:4 kernel's K = 512 cases)"""
    case(3, 512, 256, hb.EPI_SCALE_STORE, seed=136, ssq_n=136)


def test_mxfp8_rejections():
    d = dev()
    gen = torch.Generator().manual_seed(3)
    X = torch.randn(4, 512, generator=gen)
    w = mxfp8_round_2d(torch.randn(512, 32, generator=gen))

    def rc_of(mut, Xm=None):
        Xu = X if Xm is None else Xm
        A = lay.pack_f32_tiles(Xu.to(d), ktiles=16)
        Wt, kt, ns = lay.tile_weight_fp8(w)
        Wt = Wt.to(d)
        out = torch.zeros(Xu.shape[0], 32, device=d)
        g = hb.GemmArgs()
        g.A, g.a_ktiles, g.M, g.W, g.KT, g.nstrips, g.epi = hb.ptr(A), 16, Xu.shape[0], hb.ptr(Wt), kt, ns, hb.EPI_SCALE_STORE
        g.out, g.ldo, g.act_f32, g.w_format, g.ssq_ld = hb.ptr(out), 32, 3, hb.W_MXFP8, 32
        mut(g)
        rc = hb.lib().dia_gemm(C.byref(g), None)
        torch.cuda.synchronize()
        return rc, hb.lib().dia_last_error()

    ok, _ = rc_of(lambda g: None)
    assert ok == 0
    dummy = torch.zeros(64, dtype=torch.int32, device=d)
    for mut in (lambda g: setattr(g, "w_planes", 2), lambda g: setattr(g, "w_planes", 3), lambda g: setattr(g, "w_layout", 1),
                lambda g: setattr(g, "sp_blocks", hb.ptr(dummy)), lambda g: setattr(g, "cmap", hb.ptr(dummy)),
                lambda g: setattr(g, "strip_map", hb.ptr(dummy)), lambda g: setattr(g, "act_f32", 0),
                lambda g: setattr(g, "w_format", 7), lambda g: setattr(g, "epi", hb.EPI_CROSSKV), lambda g: setattr(g, "KT", 8)):
        rc, msg = rc_of(mut)
        assert rc == -1, msg
        assert msg
    rc, msg = rc_of(lambda g: None, Xm=torch.randn(17, 512, generator=gen))
    assert rc == -1 and b"16 rows" in msg


_FIRST_CALL = r"""
import ctypes as C, sys, torch
sys.path.insert(0, %r)
from dia_hip import binding as hb, layout as lay
from dia_hip.quant import mxfp8_round_2d
d = torch.device("cuda:0")
gen = torch.Generator().manual_seed(1)
X = torch.randn(2, 4096, generator=gen)
w = mxfp8_round_2d(torch.randn(4096, 64, generator=gen))
A = lay.pack_f32_tiles(X.to(d), ktiles=128)
Wt, kt, ns = lay.tile_weight_fp8(w)
Wt = Wt.to(d)
out = torch.zeros(2, 64, device=d)
g = hb.GemmArgs()
g.A, g.a_ktiles, g.M, g.W, g.KT, g.nstrips, g.epi = hb.ptr(A), 128, 2, hb.ptr(Wt), kt, ns, hb.EPI_SCALE_STORE
g.out, g.ldo, g.act_f32, g.w_format, g.ssq_ld = hb.ptr(out), 64, 3, hb.W_MXFP8, 16
hb.check(hb.lib().dia_gemm(C.byref(g), None), "dia_gemm")
torch.cuda.synchronize()
ref = (X.double() @ w.double())
err = (out.cpu().double() - ref).abs().max().item() / ref.abs().max().item()
assert err < 2e-5, err
print("ok")
"""


def test_mxfp8_gemm_as_first_call():
    """a fresh process whose first library call is an MXFP8 dia_gemm needing > 64 KiB of LDS (4096 K at 2 rows: 96 KiB image)"""
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dia-tts-prune_amd")
    r = subprocess.run([sys.executable, "-c", _FIRST_CALL % root], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-2000:]
