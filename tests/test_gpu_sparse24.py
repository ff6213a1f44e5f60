"""The 2:4 sparse weight stream (dia_gemm_args.w_format = DIA_W_SPARSE24, csrc/gemm_sparse.hip) on a real MI355X, through the
C ABI, against float64 and against the dense kernels on the same zero-holding matrix.  Tolerance: 2e-5 relative to the output
scale, as the dense GEMM tests."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from dia_hip import binding as hb
from dia_hip import layout as lay
from dia_hip.pruning import is_2of4

W_SPARSE24 = hb.W_SPARSE24


def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    return torch.device("cuda:0")


def prune24(w):
    K, N = w.shape
    g = w.reshape(K // 4, 4, N)
    keep = torch.zeros_like(g, dtype=torch.bool).scatter_(1, g.abs().topk(2, dim=1).indices, True)
    return (g * keep).reshape(K, N).bfloat16().float()


def gemm(X, w, epi, *, sparse, sk=None, ssq=True, x0=None, gnext=None, spw=0, expect=hb.check, ssq_n=8):
    """one dia_gemm launch with fp32 activation tiles in and out; returns (out, emitted activations [M, width], ssq_out)"""
    d = dev()
    M, K = X.shape
    N = w.shape[1]
    ns = (N + 15) // 16
    Np = ns * 16
    A = lay.pack_f32_tiles(X.to(d), ktiles=K // 32)
    if sparse:
        Wt, kt, ns_ = lay.tile_weight_24(w)
    else:
        Wt, kt, ns_ = lay.tile_weight(w)
    Wt = Wt.to(d)
    g = hb.GemmArgs()
    g.A, g.a_ktiles, g.M = hb.ptr(A), K // 32, M
    g.W, g.KT, g.nstrips, g.epi, g.spw = hb.ptr(Wt), kt, ns_, epi, spw
    g.act_f32 = 3
    g.w_format = W_SPARSE24 if sparse else 0
    ssq_ld = 16
    keep = [A, Wt]
    if ssq:
        sin = (torch.rand(ssq_n, ssq_ld, generator=torch.Generator().manual_seed(M + K)) + 0.5).to(d)
        g.ssq_in, g.ssq_in_n, g.ssq_ld, g.inv_d, g.eps = hb.ptr(sin), ssq_n, ssq_ld, 1.0 / (8 * ssq_n), 1e-5
        keep.append(sin)
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
    if sk is not None:
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


def check_close(got, want, tol=2e-5):
    scale = max(want.abs().max().item(), 1e-6)
    err = (got.double() - want).abs().max().item()
    assert err <= tol * scale, (err, scale)


def case(M, K, N, epi, seed, sk=None, spw=0, ssq_n=8):
    gen = torch.Generator().manual_seed(seed)
    X = torch.randn(M, K, generator=gen)
    w = prune24(torch.randn(K, N, generator=gen) * 0.05)
    assert is_2of4(w)
    x0 = torch.randn(M, (N + 15) // 16 * 16, generator=gen) if epi == hb.EPI_RESID_EMIT else None
    gn = (torch.rand(N, generator=gen) + 0.5) if epi == hb.EPI_RESID_EMIT else None
    ssq = epi != hb.EPI_RESID_EMIT
    sp = gemm(X, w, epi, sparse=True, sk=sk, ssq=ssq, x0=x0, gnext=gn, spw=spw, ssq_n=ssq_n)
    dn = gemm(X, w, epi, sparse=False, sk=sk, ssq=ssq, x0=x0, gnext=gn, spw=spw, ssq_n=ssq_n)
    ro, re, rs = reference(X, w, epi, sin=sp[3], x0=x0, gnext=gn)
    if ro is not None:
        check_close(sp[0][:, :N], ro[:, :N])
        check_close(sp[0], dn[0].double())
    if re is not None:
        check_close(sp[1], re)
        check_close(sp[1], dn[1].double())
    if rs is not None:
        check_close(sp[2][:, :M], rs)
        check_close(sp[2][:, :M], dn[2][:, :M].double())


@pytest.mark.parametrize("abid_tile", [0, 1])
def test_operand_probe(abid_tile):
    """One smfmac k-tile: every output column's weights only in sparse k-tile `abid_tile` (even: index bits 0-15, odd: 16-31).
    One-hot weights at each of the 4 positions of every group, then random 2:4 values, against float64 — pins the operand
    layout, the index bit order and abid."""
    K, N, M = 512, 16, 16
    gen = torch.Generator().manual_seed(11 + abid_tile)
    X = torch.randn(M, K, generator=gen)
    k0 = 64 * abid_tile
    for pos in range(4):
        w = torch.zeros(K, N)
        for c in range(N):
            for grp in range(16):
                w[k0 + 4 * grp + pos, c] = float(1 + (c + grp) % 5)
        out = gemm(X, w, hb.EPI_SCALE_STORE, sparse=True, ssq=False)[0]
        check_close(out, X.double() @ w.double(), tol=1e-6)
    w = torch.zeros(K, N)
    w[k0:k0 + 64] = prune24(torch.randn(64, N, generator=gen))
    out = gemm(X, w, hb.EPI_SCALE_STORE, sparse=True, ssq=False)[0]
    check_close(out, X.double() @ w.double(), tol=1e-6)


@pytest.mark.parametrize("M", [1, 2, 4, 6, 16])
@pytest.mark.parametrize("K", [512, 2048, 8192])
@pytest.mark.parametrize("epi", [0, 1, 2])
def test_sparse_gemm_vs_float64_and_dense(M, K, epi):
    case(M, K, 128 if epi != 2 else 256, epi, seed=M * 131 + K + epi)


@pytest.mark.parametrize("M,sk", [(2, 2), (4, 2), (8, 4), (16, 4)])
def test_sparse_wo_split_k(M, sk):
    case(M, 8192, 2048, hb.EPI_RESID_EMIT, seed=M + 17 * sk, sk=sk)


@pytest.mark.parametrize("M", [2, 4, 16])
def test_sparse_logits_shape(M):
    """the logits head: N = 9 * 1028 (padded to 579 strips), K = 2048; at M <= 4 the persistent multi-strip form"""
    case(M, 2048, 9 * 1028, hb.EPI_SCALE_STORE, seed=M + 5)


def test_sparse_wi_persistent_form():
    """wi: 1024 strips at batch 1 (4 strips per workgroup, next strip prefetched), SWIGLU_EMIT"""
    case(2, 2048, 16384, hb.EPI_SWIGLU_EMIT, seed=99)


def test_sparse_row_scales_past_128_partials():
    """ssq_in_n = 136 (D = 2176): the row-scale reduction's tail loop behind the 16 partials a thread requests at once, in a
    one-wave workgroup (K = 512), whose threads also serve rows 8..15 (the M = 16, K = 512 cases above run that branch with
    ssq_in present and every row live)"""
    case(3, 512, 256, hb.EPI_SCALE_STORE, seed=136, ssq_n=136)


def test_sparse_rejections():
    d = dev()
    gen = torch.Generator().manual_seed(3)
    X = torch.randn(4, 512, generator=gen)
    w = prune24(torch.randn(512, 32, generator=gen))

    def rc_of(mut, M=4, epi=hb.EPI_SCALE_STORE, Xm=None):
        Xu = X if Xm is None else Xm
        A = lay.pack_f32_tiles(Xu.to(d), ktiles=16)
        Wt, kt, ns = lay.tile_weight_24(w)
        Wt = Wt.to(d)
        out = torch.zeros(Xu.shape[0], 32, device=d)
        g = hb.GemmArgs()
        g.A, g.a_ktiles, g.M, g.W, g.KT, g.nstrips, g.epi = hb.ptr(A), 16, Xu.shape[0], hb.ptr(Wt), kt, ns, epi
        g.out, g.ldo, g.act_f32, g.w_format, g.ssq_ld = hb.ptr(out), 32, 3, W_SPARSE24, 16
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
                lambda g: setattr(g, "w_format", 7), lambda g: setattr(g, "epi", hb.EPI_CROSSKV)):
        rc, msg = rc_of(mut)
        assert rc == -1, msg
        assert msg
    rc, msg = rc_of(lambda g: None, Xm=torch.randn(17, 512, generator=gen))
    assert rc == -1 and b"16 rows" in msg


_FIRST_CALL = r"""
import ctypes as C, sys, torch
sys.path.insert(0, %r)
from dia_hip import binding as hb, layout as lay
d = torch.device("cuda:0")
gen = torch.Generator().manual_seed(1)
X = torch.randn(2, 4096, generator=gen)
w = torch.randn(4096, 64, generator=gen)
g4 = w.reshape(1024, 4, 64)
w = (g4 * torch.zeros_like(g4, dtype=torch.bool).scatter_(1, g4.abs().topk(2, dim=1).indices, True)).reshape(4096, 64).bfloat16().float()
A = lay.pack_f32_tiles(X.to(d), ktiles=128)
Wt, kt, ns = lay.tile_weight_24(w)
Wt = Wt.to(d)
out = torch.zeros(2, 64, device=d)
g = hb.GemmArgs()
g.A, g.a_ktiles, g.M, g.W, g.KT, g.nstrips, g.epi = hb.ptr(A), 128, 2, hb.ptr(Wt), kt, ns, hb.EPI_SCALE_STORE
g.out, g.ldo, g.act_f32, g.w_format, g.ssq_ld = hb.ptr(out), 64, 3, hb.W_SPARSE24, 16
hb.check(hb.lib().dia_gemm(C.byref(g), None), "dia_gemm")
torch.cuda.synchronize()
ref = (X.double() @ w.double())
err = (out.cpu().double() - ref).abs().max().item() / ref.abs().max().item()
assert err < 2e-5, err
print("ok")
"""


def test_sparse_gemm_as_first_call():
    """a fresh process whose first library call is a sparse dia_gemm needing > 64 KiB of LDS (4096 K at 2 rows: 100 KiB image)"""
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dia-tts-prune_amd")
    r = subprocess.run([sys.executable, "-c", _FIRST_CALL % root], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-2000:]
