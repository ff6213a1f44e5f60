"""Two-plane bf16 weights (dia_gemm_args.w_planes = 2, Dia.fp32_weights = "bf16x2") on a real MI355X: the tuned kernels against
float64 at the kernel level, and a genuine (not bf16-representable) fp32 checkpoint end to end against the oracle on its fp32
weights."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from dia_hip import binding as hb
from dia_hip import config as CF
from dia_hip import layout as lay
from dia_hip.engine import DecodeSession, DeviceWeights
from dia_hip.model import Dia
from dia_hip.tokens import effective_text, encode_text, synthetic_text
from dia_hip.weights import synthetic_state_dict
from oracle import dia_oracle as O

LOGIT_TOL = 1e-3
TEXTS = ["[S1] Dia is an open weights text to dialogue model. [S2] You get full control over scripts and voices.",
         "[S1] Short one.",
         "[S2] A somewhat longer line, with punctuation; and more words to encode."]


def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    return torch.device("cuda:0")


def threads():
    try:
        n = len(os.sched_getaffinity(0))
    except Exception:
        n = os.cpu_count() or 1
    return max(1, min(16, n))


# ---------------------------------------------------------------------------------------------------- kernel level
def gemm_w2(x, W, epi, *, sk=0, gn=None, x0=None):
    """x [M, K] fp32, W [K, N] fp32 -> dia_gemm with w_planes = 2 and fp32 activation tiles; returns (outputs, kernel name)"""
    d = x.device
    M, K = x.shape
    N = W.shape[1]
    Wt, kt2, ns = lay.tile_weight_bf16x2(W)
    assert kt2 == 2 * (K // 32)
    mpad = (M + 15) // 16 * 16
    A = lay.pack_f32_tiles(x)
    g = hb.GemmArgs()
    g.A, g.a_ktiles, g.M = hb.ptr(A), K // 32, M
    g.W, g.KT, g.nstrips, g.epi, g.w_planes = hb.ptr(Wt), kt2, ns, epi, 2
    g.ssq_ld = mpad
    keep = [A, Wt]
    res = {}
    if epi == hb.EPI_SCALE_STORE:
        out = torch.full((M, ns * 16), float("nan"), device=d)
        g.out, g.ldo, g.act_f32 = hb.ptr(out), ns * 16, 1
        res["out"] = out
    elif epi == hb.EPI_RESID_EMIT:
        xr = x0.clone()
        P = torch.zeros(mpad // 16, N // 32, 64, 8, device=d)
        ssq = torch.zeros(ns, mpad, device=d)
        g.out, g.ldo, g.gnext = hb.ptr(xr), N, hb.ptr(gn)
        g.P, g.p_ktiles, g.ssq_out, g.act_f32 = hb.ptr(P), N // 32, hb.ptr(ssq), 3
        res.update(x=xr, P=P, ssq=ssq)
    else:
        P = torch.zeros(mpad // 16, N // 64, 64, 8, device=d)
        g.P, g.p_ktiles, g.act_f32 = hb.ptr(P), N // 64, 3
        res["P"] = P
    if sk:
        scr = torch.zeros(mpad // 16 * ns * sk * 256, device=d)
        tk = torch.zeros(mpad // 16 * ns, dtype=torch.int32, device=d)
        g.sk, g.sk_scratch, g.sk_tickets, g.sk_scratch_floats = sk, hb.ptr(scr), hb.ptr(tk), scr.numel()
        keep += [scr, tk]
    ms = C.c_float()
    hb.check(hb.lib().dia_gemm_timed(C.byref(g), None, C.byref(ms)), "dia_gemm_timed")
    torch.cuda.synchronize()
    if sk:
        assert bool((tk == 0).all())                # the last arriver re-arms the tickets
    return res, hb.lib().dia_timed_kernel_name(0).decode()


def tuned_name(M):
    return "k_gemv_small<8, 16" if M <= 4 else "k_gemm16<8, 16"


@pytest.mark.parametrize("M", [2, 4, 16, 40, 128])
@pytest.mark.parametrize("epi", ["store", "resid", "swiglu"])
def test_gemm_two_planes_vs_float64(M, epi):
    d = dev()
    torch.manual_seed(M * 13 + len(epi))
    K = N = 2048
    x = torch.randn(M, K, device=d)
    W = torch.randn(K, N, device=d) * 0.05          # not bf16-representable
    ref = x.double() @ W.double()
    scale = ref.abs().max().item()
    if epi == "store":
        r, name = gemm_w2(x, W, hb.EPI_SCALE_STORE)
        err = (r["out"][:, :N].double() - ref).abs().max().item()
        # what the one-plane (rounded) tile set would cost on the same operands
        e1 = (x.double() @ W.bfloat16().double() - ref).abs().max().item()
        assert e1 > 1e-3 * scale
    elif epi == "resid":
        x0 = torch.randn(M, N, device=d)
        gn = (1.0 + 0.1 * torch.randn(N, device=d)).bfloat16().float()
        r, name = gemm_w2(x, W, hb.EPI_RESID_EMIT, gn=gn, x0=x0)
        ref = x0.double() + ref
        err = (r["x"].double() - ref).abs().max().item()
        assert torch.equal(lay.unpack_f32_tiles(r["P"], M, N), r["x"] * gn)
    else:
        r, name = gemm_w2(x, W, hb.EPI_SWIGLU_EMIT)
        y = ref.reshape(M, N // 16, 2, 8)
        g_, u_ = y[:, :, 0], y[:, :, 1]
        h = (g_ / (1.0 + torch.exp(-g_)) * u_).reshape(M, N // 2)
        err = (lay.unpack_f32_tiles(r["P"], M, N // 2).double() - h).abs().max().item()
        scale = h.abs().max().item()
    print(f"w_planes=2 M={M} {epi}: {name}, err {err / scale:.2e} of scale")
    assert err <= 3e-5 * scale
    assert "k_gemm<" not in name and name.startswith(tuned_name(M)), name


@pytest.mark.parametrize("M", [2, 4, 16, 40, 128])
def test_gemm_two_planes_wo_split_k(M):
    """wo: K 8192 -> 2048 with RESID_EMIT, split-K 4 (128 weight k-tiles per workgroup) as the engine runs it"""
    d = dev()
    torch.manual_seed(M + 8192)
    K, N = 8192, 2048
    x = torch.randn(M, K, device=d)
    W = torch.randn(K, N, device=d) * 0.05
    x0 = torch.randn(M, N, device=d)
    gn = (1.0 + 0.1 * torch.randn(N, device=d)).bfloat16().float()
    r, name = gemm_w2(x, W, hb.EPI_RESID_EMIT, sk=4, gn=gn, x0=x0)
    ref = x0.double() + x.double() @ W.double()
    err = (r["x"].double() - ref).abs().max().item()
    assert err <= 3e-5 * ref.abs().max().item()
    assert "k_gemm<" not in name and name.startswith(tuned_name(M)), name


@pytest.mark.parametrize("M", [2, 16, 128])
def test_gemm_two_planes_logits_shape(M):
    d = dev()
    torch.manual_seed(M + 9252)
    K, N = 2048, 9252
    x = torch.randn(M, K, device=d)
    W = torch.randn(K, N, device=d) * 0.05
    r, name = gemm_w2(x, W, hb.EPI_SCALE_STORE)
    ref = x.double() @ W.double()
    err = (r["out"][:, :N].double() - ref).abs().max().item()
    assert err <= 3e-5 * ref.abs().max().item()
    assert "k_gemm<" not in name and name.startswith(tuned_name(M)), name


def test_gemm_two_planes_generic_and_rejections():
    """planes in / out (the prefill's format) and ragged K take the generic kernel; the diagonal layout, the sparse stream
    and an odd KT are refused with a reason"""
    d = dev()
    torch.manual_seed(1)
    M, K, N = 20, 96, 80
    x = torch.randn(M, K, device=d)
    W = torch.randn(K, N, device=d) * 0.05
    Wt, kt2, ns = lay.tile_weight_bf16x2(W)
    A = lay.pack_planes(x)
    out = torch.zeros(M, ns * 16, device=d)
    g = hb.GemmArgs()
    g.A, g.a_plane_stride, g.a_ktiles, g.M = hb.ptr(A), A[0].numel(), A.shape[2], M
    g.W, g.KT, g.nstrips, g.epi, g.w_planes = hb.ptr(Wt), kt2, ns, hb.EPI_SCALE_STORE, 2
    g.out, g.ldo = hb.ptr(out), ns * 16
    ms = C.c_float()
    hb.check(hb.lib().dia_gemm_timed(C.byref(g), None, C.byref(ms)), "dia_gemm_timed")
    torch.cuda.synchronize()
    assert hb.lib().dia_timed_kernel_name(0).decode().startswith("k_gemm<")
    ref = x.double() @ W.double()
    assert (out[:, :N].double() - ref).abs().max().item() <= 3e-5 * ref.abs().max().item()
    L = hb.lib()
    g.w_layout = 1
    assert L.dia_gemm(C.byref(g), None) == -1 and b"diagonal" in L.dia_last_error()
    g.w_layout = 0
    g.KT = kt2 - 1
    assert L.dia_gemm(C.byref(g), None) == -1 and b"even KT" in L.dia_last_error()
    g.KT = kt2
    g.sp_toff = hb.ptr(torch.zeros(4, dtype=torch.int32, device=d))
    assert L.dia_gemm(C.byref(g), None) == -1 and b"sparse" in L.dia_last_error()


# ---------------------------------------------------------------------------------------------------- model level
def perturbed(sd, seed=3):
    """a genuine fp32 checkpoint: the synthetic weights plus noise below bf16's resolution"""
    g = torch.Generator().manual_seed(seed)
    return {k: (v + v.abs().mean() * 2.0 ** -10 * torch.randn(v.shape, generator=g)) if v.ndim >= 2 and "embedding" not in k else v.clone()
            for k, v in sd.items()}


def oracle_run(cfg, sd, text, seed, max_tokens, **kw):
    dm = O.Dims.of(cfg)
    nz = O.exp_noise(seed, max_tokens - 1, dm.C, dm.tgt_vocab)
    torch.set_num_threads(threads())
    return O.generate(sd, cfg, text, max_tokens=max_tokens, seed=None, noise=nz, mirror=False, **kw), nz


def teacher_forced(w, cfg, texts, oracle_tokens, noises, max_tokens):
    ids = [encode_text(effective_text(t), cfg) for t in texts]
    s = DecodeSession(w, ids, kv_dtype="f32", max_tokens=max_tokens, noise=torch.stack(noises), teacher_tokens=oracle_tokens)
    s.prefill()
    logits = []
    for _ in range(max_tokens - 1):
        s.decode(1, use_graph=False)
        logits.append(s.logits_host())
    res = s.results()
    s.close()
    return logits, res


def check_vs_oracle(w, cfg, sd, texts, seeds, mt, label, **kw):
    runs = [oracle_run(cfg, sd, t, s_, mt, **kw) for t, s_ in zip(texts, seeds)]
    logits, res = teacher_forced(w, cfg, texts, [r.tokens for r, _ in runs], [nz[: mt - 1] for _, nz in runs], mt)
    worst = 0.0
    for b, (r, _) in enumerate(runs):
        for i in range(len(r.logits)):
            worst = max(worst, float(np.abs(logits[i][b] - r.logits[i]).max()))
        for i, p in enumerate(r.preds):
            assert np.array_equal(res[b].preds[1 + i], p), (b, i)
    print(f"{label}: logits vs oracle on the fp32 weights {worst:.3e}")
    assert worst <= LOGIT_TOL
    return runs


@pytest.fixture(scope="module")
def mid_raw():
    cfg = CF.mid_config()
    raw = perturbed(synthetic_state_dict(cfg, seed=1234, std=0.02))
    Dia.fp32_weights = "bf16x2"
    try:
        dia = Dia.from_state_dict(cfg, raw, "float32", dev())
    finally:
        Dia.fp32_weights = "exact"
    return cfg, raw, dia


def test_mid_two_planes_load_and_batch1(mid_raw, capsys):
    cfg, raw, dia = mid_raw
    assert dia.model.weight_planes == 2 and not dia.weights_rounded and not dia.weights_exact_planes
    assert Dia.fp32_weights == "exact"
    mt = 24
    runs = check_vs_oracle(dia.model, cfg, raw, [TEXTS[0]], [42], mt, "mid, two weight planes, batch 1")
    # free running with the same noise: the oracle's token buffer; graph replay == eager, bitwise
    r, nz = runs[0]
    ids = [encode_text(effective_text(TEXTS[0]), cfg)]
    outs = []
    for use_graph in (False, True):
        s = DecodeSession(dia.model, ids, kv_dtype="f32", max_tokens=mt, noise=torch.stack([nz]))
        s.prefill()
        s.run(use_graph=use_graph, poll=8)
        outs.append(s.results()[0].tokens)
        s.close()
    assert np.array_equal(outs[0], r.tokens)
    assert np.array_equal(outs[0], outs[1])


def test_mid_two_planes_load_note(capsys):
    cfg = CF.mid_config()
    raw = perturbed(synthetic_state_dict(cfg, seed=1234, std=0.02))
    Dia.fp32_weights = "bf16x2"
    try:
        capsys.readouterr()
        dia = Dia.from_state_dict(cfg, raw, "float32", dev())
        out = capsys.readouterr().out
    finally:
        Dia.fp32_weights = "exact"
    assert "Note:" in out and "bf16x2" in out and "2x the weight traffic" in out
    assert dia.model.weight_planes == 2


@pytest.mark.parametrize("B", [3, 20])
def test_mid_two_planes_batches(mid_raw, B):
    cfg, raw, dia = mid_raw
    texts = [TEXTS[i % 3] for i in range(B)]
    seeds = [42 + i for i in range(B)]
    check_vs_oracle(dia.model, cfg, raw, texts, seeds, 8 if B > 3 else 16, f"mid, two weight planes, batch {B}")


def test_mid_two_planes_pruned_compacted():
    from dia_hip.pruning import structured_prune_state_dict

    cfg = CF.mid_config()
    raw = perturbed(synthetic_state_dict(cfg, seed=1234, std=0.02))
    psd, _ = structured_prune_state_dict(cfg, raw, amount=0.5, dim=0, n=2)
    w = DeviceWeights(cfg, psd, dev(), weight_planes=2)
    assert w.compacted and w.weight_planes == 2
    check_vs_oracle(w, cfg, psd, TEXTS, [42, 7, 123], 12, "mid pruned-50 compacted, two weight planes, batch 3")


# ---------------------------------------------------------------------------------------------------- full size
@pytest.fixture(scope="module")
def full_raw():
    cfg = CF.dia_1_6b_config()
    d = dev()
    sd_gpu = synthetic_state_dict(cfg, seed=1234, std=0.02, device=d)
    g = torch.Generator(device=d).manual_seed(3)
    raw_gpu = {k: (v + v.abs().mean() * 2.0 ** -10 * torch.randn(v.shape, generator=g, device=d)) if v.ndim >= 2 and "embedding" not in k else v
               for k, v in sd_gpu.items()}
    del sd_gpu
    w = DeviceWeights(cfg, raw_gpu, d, weight_planes=2)
    raw = {k: v.cpu() for k, v in raw_gpu.items()}
    del raw_gpu
    return cfg, raw, w


def test_full_two_planes_batch1_and_batch8(full_raw):
    cfg, raw, w = full_raw
    check_vs_oracle(w, cfg, raw, [TEXTS[0]], [42], 9, "Dia-1.6B, two weight planes, batch 1", max_steps=8)
    lens = [32, 64, 96, 128, 192, 256, 384, 512]
    texts = [synthetic_text(L, cfg) for L in lens]
    check_vs_oracle(w, cfg, raw, texts, [42 + b for b in range(8)], 4, "Dia-1.6B, two weight planes, batch 8 mixed", max_steps=3)


@pytest.mark.parametrize("B", [1, 8, 64])
def test_full_two_planes_tuned_kernels_only(full_raw, B):
    cfg, raw, w = full_raw
    texts = [synthetic_text(32 + 8 * (b % 8), cfg) for b in range(B)]
    ids = [encode_text(effective_text(t), cfg) for t in texts]
    s = DecodeSession(w, ids, kv_dtype="f32", max_tokens=16, seeds=list(range(B)))
    s.prefill()
    s.decode(1, use_graph=False)
    ms = s.time_step()
    names = s.last_kernel_names
    s.close()
    gemms = [n for n in names if n.startswith("k_gemm") or n.startswith("k_gemv")]
    print(f"Dia-1.6B two weight planes, batch {B}: step {ms.sum() * 1e3:.0f} us, {len(gemms)} GEMM launches, "
          f"{sorted(set(n.split('<')[0] for n in gemms))}")
    assert gemms and not [n for n in gemms if n.startswith("k_gemm<")], sorted(set(gemms))
