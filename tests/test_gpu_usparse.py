"""The unstructured sparse weight stream (dia_gemm_args.w_format = DIA_W_USPARSE, csrc/gemm_us.hip) on a real MI355X, through the
C ABI.  Reference: the float64 product of the fp32 activations with the bf16 weights (the stream is a second, lossless encoding
of the numbers the dense tiles hold).  Bound: 2e-5 relative to the output scale, the project's GEMM bound
(tests/test_gpu_kernels.py); in every case the dense dia_gemm on tile_weight of the same matrix must meet it too — it is the
yardstick: a case the dense kernel fails is a wrong case, not a wrong feature."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from dia_hip import binding as hb
from dia_hip import layout as lay

TOL = 2e-5


def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    return torch.device("cuda:0")


def gemm(X, w, epi, *, rate, sk=None, ssq=True, x0=None, gnext=None, spw=0, ssq_n=8):
    """one dia_gemm launch with fp32 activation tiles in and out (rate 0: the dense tiles); returns (out, emitted activations
    [M, width], ssq_out, ssq_in)"""
    d = dev()
    M, K = X.shape
    N = w.shape[1]
    Np = (N + 15) // 16 * 16
    A = lay.pack_f32_tiles(X.to(d), ktiles=K // 32)
    Wt, kt, ns_ = lay.tile_weight_us(w, rate) if rate else lay.tile_weight(w)
    Wt = Wt.to(d)
    g = hb.GemmArgs()
    g.A, g.a_ktiles, g.M = hb.ptr(A), K // 32, M
    g.KT, g.nstrips, g.epi, g.spw = kt, ns_, epi, spw
    um = hb.UsMat(stream=hb.ptr(Wt), rate=rate)
    g.W = C.cast(C.pointer(um), C.c_void_p) if rate else hb.ptr(Wt)
    g.act_f32 = 3
    g.w_format = hb.W_USPARSE if rate else 0
    ssq_ld = 16
    keep = [A, Wt, um]
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
        pk = (Np + 31) // 32
        P = torch.zeros(1, pk, 64, 8, device=d)
        sso = torch.zeros(ns_, ssq_ld, device=d)
        gn = gnext.to(d)
        keep.append(gn)
        g.out, g.ldo, g.gnext, g.P, g.p_ktiles, g.ssq_out = hb.ptr(out), Np, hb.ptr(gn), hb.ptr(P), pk, hb.ptr(sso)
    else:
        pk = (Np // 2 + 31) // 32
        P = torch.zeros(1, pk, 64, 8, device=d)
        g.P, g.p_ktiles = hb.ptr(P), pk
    tk = None
    if sk is not None:
        scr = torch.zeros(ns_ * sk * 256, device=d)
        tk = torch.zeros(ns_, dtype=torch.int32, device=d)
        g.sk_scratch, g.sk_tickets, g.sk, g.sk_scratch_floats = hb.ptr(scr), hb.ptr(tk), sk, scr.numel()
        keep += [scr, tk]
    hb.check(hb.lib().dia_gemm(C.byref(g), None), "dia_gemm")
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


def pruned(K, N, zeros, gen):
    """a bf16-representable matrix with the given share of zeros, unstructured"""
    w = (torch.randn(K, N, generator=gen) * 0.05).bfloat16().float()
    return w * (torch.rand(K, N, generator=gen) >= zeros)


def case(M, K, N, epi, seed, zeros, sk=None, spw=0, rates=(4, 2), ssq_n=8):
    gen = torch.Generator().manual_seed(seed)
    X = torch.randn(M, K, generator=gen)
    w = pruned(K, N, zeros, gen)
    if zeros > 0:
        w[32:64, 1] = 0.0                                   # an all-zero k-tile of a column
        w[:, 2] = ((torch.randn(K, generator=gen) * 0.05).abs() + 1e-3).bfloat16().float()     # a fully dense column
    Np = (N + 15) // 16 * 16
    x0 = torch.randn(M, Np, generator=gen) if epi == hb.EPI_RESID_EMIT else None
    gn = (torch.rand(Np, generator=gen) + 0.5) if epi == hb.EPI_RESID_EMIT else None
    ssq = epi != hb.EPI_RESID_EMIT
    dn = gemm(X, w, epi, rate=0, sk=sk, ssq=ssq, x0=x0, gnext=gn, spw=spw, ssq_n=ssq_n)
    wp = torch.zeros(K, Np)
    wp[:, :N] = w
    ro, re, rs = reference(X, wp, epi, sin=dn[3], x0=x0, gnext=gn)
    for rate in rates:
        us = gemm(X, w, epi, rate=rate, sk=sk, ssq=ssq, x0=x0, gnext=gn, spw=spw, ssq_n=ssq_n)
        again = gemm(X, w, epi, rate=rate, sk=sk, ssq=ssq, x0=x0, gnext=gn, spw=spw, ssq_n=ssq_n)
        for a, b in zip(us[:3], again[:3]):                 # fixed summation order: the same bits on every call
            assert (a is None and b is None) or torch.equal(a, b)
        if ro is not None:
            check_close(dn[0], ro, "dense out")
            check_close(us[0], ro, f"usparse R={rate} out")
        if re is not None:
            check_close(dn[1], re, "dense emitted")
            check_close(us[1], re, f"usparse R={rate} emitted")
        if rs is not None:
            check_close(dn[2][:, :M], rs, "dense ssq")
            check_close(us[2][:, :M], rs, f"usparse R={rate} ssq")


def probe_matrix():
    """K = 512, N = 16: pairwise-distinct bf16 values inside every lane-tile (8 consecutive K of a column), and lane-tiles of every
    non-zero count 0..8 with the kept positions moving from lane-tile to lane-tile"""
    K, N = 512, 16
    k, c = torch.arange(K)[:, None], torch.arange(N)[None, :]
    j, lt = k & 7, (k >> 3) * N + c                          # element inside its lane-tile; lane-tile number
    val = (1.0 + j.float() / 8 + ((lt % 7).float() + 1) * 2.0) * torch.where((lt & 1) == 1, -1.0, 1.0)     # distinct in j, bf16-exact
    assert torch.equal(val.bfloat16().float(), val)
    count = lt % 9                                           # non-zeros of the lane-tile
    start = (lt // 9) % 8                                    # where its run of non-zeros begins (wraps around)
    keep = ((j - start) % 8) < count
    w = val * keep
    cnt = (w != 0).reshape(K // 8, 8, N).sum(dim=1)
    assert set(cnt.flatten().tolist()) == set(range(9))
    return w


@pytest.mark.parametrize("rate", [4, 2])
def test_operand_probe(rate):
    """One workgroup, one strip, one group.  The activations are rows of the identity, 4 at a time, so the outputs ARE the matrix:
    exactly, a one-hot row splits into hi = 1, mid = lo = 0.  Pins the mask's bit order, v_perm_b32's byte order and selector
    semantics (0x0c = zero), the order of the window's slots and the overflow entries' indexing."""
    w = probe_matrix()
    eye = torch.eye(512)
    d = dev()
    got = torch.cat([gemm(eye[r: r + 4], w, hb.EPI_SCALE_STORE, rate=rate, ssq=False)[0] for r in range(0, 512, 4)])
    assert torch.equal(got, w), (got != w).nonzero()[:8]


@pytest.mark.parametrize("zeros", [0.5, 0.75])
@pytest.mark.parametrize("M", [1, 2, 4])
@pytest.mark.parametrize("K", [512, 2048])
@pytest.mark.parametrize("epi", [0, 1, 2])
def test_usparse_gemm_vs_float64_and_dense(M, K, epi, zeros):
    """N = 48: three strips; both rates; eager and second call bit-identical"""
    case(M, K, 48, epi, seed=M * 131 + K + epi, zeros=zeros)


@pytest.mark.parametrize("M", [1, 4])
def test_usparse_wo_split_k(M):
    """K = 8192 at sk = 2: 16 k-tiles per wave, 128 per workgroup; the tickets return to zero (gemm() asserts it)"""
    case(M, 8192, 64, hb.EPI_RESID_EMIT, seed=M + 34, zeros=0.6, sk=2)


def test_usparse_logits_persistent_form():
    """513 strips: the first count at which a workgroup walks several strips (3 each, next strip prefetched), SCALE_STORE"""
    case(2, 512, 513 * 16, hb.EPI_SCALE_STORE, seed=7, zeros=0.6, rates=(4,))


def test_usparse_wi_persistent_form():
    """the same with SWIGLU_EMIT (514 strips: a whole number of 32-column plane tiles)"""
    case(2, 512, 514 * 16, hb.EPI_SWIGLU_EMIT, seed=101, zeros=0.6, rates=(2,))


@pytest.mark.parametrize("K", [512, 2048])
def test_usparse_fully_dense_matrix(K):
    """maximal overflow: every lane-tile spills 8 - R values (the loop behind the prefetched entries runs)"""
    case(4, K, 48, hb.EPI_SCALE_STORE, seed=K + 3, zeros=0.0)


def test_usparse_row_scales_past_128_partials():
    """ssq_in_n = 136 (D = 2176): the row-scale reduction's tail loop behind the 16 partials a thread requests at once (the
    kernel has at least two waves, so no thread serves a second row)"""
    case(3, 512, 256, hb.EPI_SCALE_STORE, seed=136, zeros=0.6, rates=(4,), ssq_n=136)


def test_usparse_rejections():
    d = dev()
    gen = torch.Generator().manual_seed(3)
    X = torch.randn(4, 512, generator=gen)
    w = pruned(512, 32, 0.5, gen)
    um = hb.UsMat()

    def rc_of(mut, Xm=None):
        Xu = X if Xm is None else Xm
        A = lay.pack_f32_tiles(Xu.to(d), ktiles=16)
        Wt, kt, ns = lay.tile_weight_us(w, 4)
        Wt = Wt.to(d)
        um.stream, um.rate = hb.ptr(Wt), 4
        out = torch.full((Xu.shape[0], 32), 7.0, device=d)
        g = hb.GemmArgs()
        g.A, g.a_ktiles, g.M, g.W, g.KT, g.nstrips, g.epi = hb.ptr(A), 16, Xu.shape[0], C.cast(C.pointer(um), C.c_void_p), kt, ns, hb.EPI_SCALE_STORE
        g.out, g.ldo, g.act_f32, g.w_format, g.ssq_ld = hb.ptr(out), 32, 3, hb.W_USPARSE, 32
        mut(g)
        rc = hb.lib().dia_gemm(C.byref(g), None)
        torch.cuda.synchronize()
        return rc, hb.lib().dia_last_error(), bool((out == 7.0).all())

    ok, _, untouched = rc_of(lambda g: None)
    assert ok == 0 and not untouched
    dummy = torch.zeros(64, dtype=torch.int32, device=d)
    for mut in (lambda g: setattr(g, "w_planes", 2), lambda g: setattr(g, "w_planes", 3), lambda g: setattr(g, "w_layout", 1),
                lambda g: setattr(g, "sp_blocks", hb.ptr(dummy)), lambda g: setattr(g, "cmap", hb.ptr(dummy)),
                lambda g: setattr(g, "strip_map", hb.ptr(dummy)), lambda g: setattr(g, "act_f32", 0),
                lambda g: setattr(g, "epi", hb.EPI_CROSSKV), lambda g: setattr(g, "KT", 8), lambda g: setattr(um, "rate", 3),
                lambda g: (setattr(g, "sk", 2), setattr(g, "sk_scratch", hb.ptr(dummy)), setattr(g, "sk_tickets", hb.ptr(dummy)))):
        rc, msg, untouched = rc_of(mut)
        assert rc == -1 and b"unstructured sparse stream" in msg and untouched, msg
    rc, msg, untouched = rc_of(lambda g: None, Xm=torch.randn(5, 512, generator=gen))
    assert rc == -1 and b"4 rows" in msg and untouched


_FIRST_CALL = r"""
import ctypes as C, sys, torch
sys.path.insert(0, %r)
from dia_hip import binding as hb, layout as lay
d = torch.device("cuda:0")
gen = torch.Generator().manual_seed(1)
X = torch.randn(2, 4096, generator=gen)
w = torch.randn(4096, 64, generator=gen).bfloat16().float() * (torch.rand(4096, 64, generator=gen) < 0.4)
A = lay.pack_f32_tiles(X.to(d), ktiles=128)
Wt, kt, ns = lay.tile_weight_us(w, 4)
Wt = Wt.to(d)
um = hb.UsMat(stream=hb.ptr(Wt), rate=4)
out = torch.zeros(2, 64, device=d)
g = hb.GemmArgs()
g.A, g.a_ktiles, g.M, g.W, g.KT, g.nstrips, g.epi = hb.ptr(A), 128, 2, C.cast(C.pointer(um), C.c_void_p), kt, ns, hb.EPI_SCALE_STORE
g.out, g.ldo, g.act_f32, g.w_format, g.ssq_ld = hb.ptr(out), 64, 3, hb.W_USPARSE, 16
hb.check(hb.lib().dia_gemm(C.byref(g), None), "dia_gemm")
torch.cuda.synchronize()
ref = (X.double() @ w.double())
err = (out.cpu().double() - ref).abs().max().item() / ref.abs().max().item()
assert err < 2e-5, err
print("ok")
"""


def test_usparse_gemm_as_first_call():
    """a fresh process whose first library call is a stream dia_gemm needing > 64 KiB of LDS (4096 K at 2 rows: 96 KiB image + tables)"""
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dia-tts-prune_amd")
    r = subprocess.run([sys.executable, "-c", _FIRST_CALL % root], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-2000:]
