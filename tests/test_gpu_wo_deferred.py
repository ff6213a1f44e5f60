"""wo's split-K slices merged by the launch behind it (dia_gemm_wo_deferred, knob wo_defer) at 1-4 rows: the
consumer's staging prologue rebuilds bit for bit what wo's in-launch merge and epilogue leave.  Kernel level through dia_gemm
(Dia-1.6B wo shape, K 8192 -> 2048: the smallest shape for which the dispatcher picks the two-slice k_gemv_small form), then a
3-layer model with Dia-1.6B layer widths, knob on against knob off."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from dia_hip import binding as hb
from dia_hip import config as CF
from dia_hip import layout as lay

D, F, EPS = 2048, 8192, 1e-5


def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    return torch.device("cuda:0")


def bf16r(t):
    return t.bfloat16().float()


def mixed(*shape, seed):
    """values whose magnitudes spread over six decades: the order of the adds shows in the last bits"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    v = torch.randn(*shape, generator=g) * 10.0 ** torch.randint(-3, 3, shape, generator=g).float()
    return v.to(dev())


@pytest.fixture(scope="module")
def mats():
    """wo and the two consumers (q/k/v: 192 strips, one per workgroup; a logits-shaped head: 579 strips, several per workgroup),
    tiled once for all cases"""
    d = dev()
    g = torch.Generator(device="cpu").manual_seed(7)
    Wo = bf16r(torch.randn(F, D, generator=g) * 0.02).to(d)
    cons = {}
    for name, N in (("qkv", 3072), ("logits", 9252)):
        Npad = (N + 15) // 16 * 16
        W = torch.zeros(D, Npad)
        W[:, :N] = bf16r(torch.randn(D, N, generator=g) * 0.03)
        cons[name] = (W.to(d), Npad) + tuple(lay.tile_weight(W.to(d)))
    gn = bf16r(1.0 + 0.1 * torch.randn(D, generator=g)).to(d)
    return Wo, lay.tile_weight(Wo), cons, gn


def launch(g, w, timed=False):
    """one launch through dia_gemm, or through dia_gemm_wo_deferred when w is given; timed: -> the kernel's name"""
    ms = C.c_float(0)
    if w is not None:
        hb.check(hb.lib().dia_gemm_wo_deferred(C.byref(g), C.byref(w), None, C.byref(ms) if timed else None), "dia_gemm_wo_deferred")
    elif timed:
        hb.check(hb.lib().dia_gemm_timed(C.byref(g), None, C.byref(ms)), "dia_gemm_timed")
    else:
        hb.check(hb.lib().dia_gemm(C.byref(g), None), "dia_gemm")
    return hb.lib().dia_timed_kernel_name(0).decode() if timed else None


class Pair:
    """one wo launch and one consumer launch over fixed buffers, in the in-launch or the deferred form"""

    def __init__(self, mats, M, consumer, deferred):
        d = dev()
        Wo, (Wot, kto, nso), cons, gn = mats
        Wc, Npad, Wct, ktc, nsc = cons[consumer]
        self.M, self.deferred, self.Npad, self.gn = M, deferred, Npad, gn
        mpad = 16
        self.h_tiles = torch.zeros(F // 32, 64, 8, device=d)
        self.x = torch.zeros(mpad, D, device=d)                   # in-launch: the residual stream; deferred: x_old
        self.x_new = torch.full((mpad, D), float("nan"), device=d)
        self.planes_x = torch.full((3, 1, D // 32, 64, 8), 7.0, dtype=torch.bfloat16, device=d)
        self.ssq = torch.zeros(D // 16, mpad, device=d)
        self.out = torch.zeros(mpad, Npad, device=d)
        self.scr = torch.full((max(nso * 2 * 256, 2 * mpad * D),), float("nan"), device=d)
        self.tk = torch.zeros(nso, dtype=torch.int32, device=d)
        go = hb.GemmArgs()
        go.A, go.a_ktiles, go.M = hb.ptr(self.h_tiles), F // 32, M
        go.W, go.KT, go.nstrips, go.epi, go.act_f32 = hb.ptr(Wot), kto, nso, hb.EPI_RESID_EMIT, 3
        go.out, go.ldo, go.gnext, go.ssq_out, go.ssq_ld = hb.ptr(self.x), D, hb.ptr(gn), hb.ptr(self.ssq), mpad
        go.P, go.p_plane_stride, go.p_ktiles = hb.ptr(self.planes_x), self.planes_x[0].numel(), D // 32
        go.sk, go.sk_scratch, go.sk_tickets, go.sk_scratch_floats = 2, hb.ptr(self.scr), hb.ptr(self.tk), self.scr.numel()
        gc = hb.GemmArgs()
        gc.A, gc.a_ktiles, gc.M = hb.ptr(self.planes_x), D // 32, M
        gc.W, gc.KT, gc.nstrips, gc.epi, gc.act_f32 = hb.ptr(Wct), ktc, nsc, hb.EPI_SCALE_STORE, 1
        gc.ssq_in, gc.ssq_in_n, gc.ssq_ld, gc.inv_d, gc.eps = hb.ptr(self.ssq), D // 16, mpad, 1.0 / D, EPS
        gc.out, gc.ldo = hb.ptr(self.out), Npad
        self.wo = self.wc = None
        if deferred:
            self.wo, self.wc = hb.WoDeferArgs(), hb.WoDeferArgs()
            self.wo.defer, self.wo.nslices, self.wo.slices, self.wo.slice_stride = 1, 2, hb.ptr(self.scr), mpad * D
            self.wc.nslices, self.wc.slices, self.wc.slice_stride = 2, hb.ptr(self.scr), mpad * D
            self.wc.xold, self.wc.xnew, self.wc.ldx, gc.gnext = hb.ptr(self.x), hb.ptr(self.x_new), D, hb.ptr(gn)
        self.go, self.gc = go, gc

    def run(self, h, x0, names=False):
        """-> (x_new, consumer output) of the M valid rows"""
        self.h_tiles.copy_(lay.pack_f32_tiles(h)[0])
        self.x.zero_()
        self.x[: self.M] = x0
        self.names = (launch(self.go, self.wo, names), launch(self.gc, self.wc, names))
        torch.cuda.synchronize()
        xn = (self.x_new if self.deferred else self.x)[: self.M].clone()
        return xn, self.out[: self.M].clone()


def check_f64(mats, consumer, h, x0, xn, out):
    Wo, _, cons, gn = mats
    Wc = cons[consumer][0]
    x_ref = x0.double() + h.double() @ Wo.double()
    assert (xn.double() - x_ref).abs().max().item() <= 2e-5 * max(1.0, x_ref.abs().max().item())
    inv_ref = torch.rsqrt((x_ref ** 2).mean(-1, keepdim=True) + EPS)
    raw = (x_ref * gn.double()) @ Wc.double()
    ref = raw * inv_ref
    assert (out.double() - ref).abs().max().item() <= 2e-5 * max(1.0, ref.abs().max().item())
    # the inverse RMS itself, read off the column where each row's unscaled product is largest
    j = raw.abs().argmax(-1, keepdim=True)
    inv = out.double().gather(1, j) / raw.gather(1, j)
    assert ((inv - inv_ref).abs() / inv_ref).max().item() <= 2e-5


@pytest.mark.parametrize("consumer", ["qkv", "logits"])
@pytest.mark.parametrize("M", [1, 2, 3, 4])
def test_deferred_merge_equals_in_launch_merge(mats, M, consumer):
    h, x0 = mixed(M, F, seed=10 + M), mixed(M, D, seed=20 + M)
    ref, dfr = Pair(mats, M, consumer, False), Pair(mats, M, consumer, True)
    x_a, o_a = ref.run(h, x0, names=True)
    x_b, o_b = dfr.run(h, x0, names=True)
    rs = 2 if M <= 2 else 4
    multi = "true" if consumer == "logits" else "false"
    assert ref.names[0].endswith(f"k_gemv_small<16, 8, {rs}, false, true, true, false, 0>"), ref.names
    assert dfr.names[0].endswith(f"k_gemv_small<16, 8, {rs}, false, true, true, false, 1>"), dfr.names
    assert ref.names[1].endswith(f"k_gemv_small<8, 8, {rs}, {multi}, true, true, false, 0>"), ref.names
    assert dfr.names[1].endswith(f"k_gemv_small<8, 8, {rs}, {multi}, true, true, false, 2>"), dfr.names
    assert (dfr.tk == 0).all() and torch.isnan(dfr.x_new[M:]).all()        # no ticket taken, no row past M written
    assert torch.equal(dfr.x[:M], x0)                                       # the old row stays as it was
    assert torch.equal(x_a, x_b)
    assert torch.equal(o_a, o_b)
    assert o_b.abs().max().item() > 0
    check_f64(mats, consumer, h, x0, x_b, o_b)


def test_second_launch_reads_nothing_stale(mats):
    """twice in a row into the same buffers with new inputs: the second result is that of the second inputs alone"""
    M = 3
    ref, dfr = Pair(mats, M, "qkv", False), Pair(mats, M, "qkv", True)
    for rep in range(2):
        h, x0 = mixed(M, F, seed=100 + rep), mixed(M, D, seed=200 + rep)
        x_a, o_a = ref.run(h, x0)
        x_b, o_b = dfr.run(h, x0)
        assert torch.equal(x_a, x_b) and torch.equal(o_a, o_b), rep
    check_f64(mats, "qkv", h, x0, x_b, o_b)


def test_unservable_deferred_calls_are_refused(mats):
    """what the deferred kernels do not serve returns DIA_E_ARG (the engine then keeps the in-launch merge)"""
    p = Pair(mats, 2, "qkv", True)
    L = hb.lib()
    p.go.M = 6
    assert L.dia_gemm_wo_deferred(C.byref(p.go), C.byref(p.wo), None, None) == -1
    p.go.M, p.go.sk = 2, 4
    assert L.dia_gemm_wo_deferred(C.byref(p.go), C.byref(p.wo), None, None) == -1
    p.wc.xnew = p.wc.xold
    assert L.dia_gemm_wo_deferred(C.byref(p.gc), C.byref(p.wc), None, None) == -1
    assert L.dia_gemm_wo_deferred(C.byref(p.gc), None, None, None) == -1
    torch.cuda.synchronize()


# ---- model level: 3 layers of Dia-1.6B widths, synthetic seeded weights ----------------------------------------------------------

def model_cfg():
    c = CF.dia_1_6b_config()
    m = c.model
    return c.model_copy(update={
        "model": m.model_copy(update={"encoder": m.encoder.model_copy(update={"n_layer": 1}), "decoder": m.decoder.model_copy(update={"n_layer": 3})}),
        "data": c.data.model_copy(update={"text_length": 128, "audio_length": 128})})


@pytest.fixture(scope="module")
def model():
    from dia_hip.weights import synthetic_state_dict
    cfg = model_cfg()
    return cfg, synthetic_state_dict(cfg, seed=1234, std=0.02)


@pytest.fixture(scope="module")
def dense(model):
    from dia_hip.engine import DeviceWeights
    cfg, sd = model
    return DeviceWeights(cfg, sd, dev())


def session(w, cfg, B, *, teacher=None, kv_dtype="f32", mt=80):
    from dia_hip.engine import DecodeSession
    from dia_hip.tokens import effective_text, encode_text, synthetic_text
    ids = [encode_text(effective_text(synthetic_text(32 + 16 * b, cfg)), cfg) for b in range(B)]
    s = DecodeSession(w, ids, kv_dtype=kv_dtype, max_tokens=mt, seeds=list(range(B)), ignore_eos=True, teacher_tokens=teacher)
    s.prefill()
    return s


def forms(s):
    """(wo launches in the deferred producer form, launches in the deferred consumer form) of one step"""
    s.time_step()
    small = [n for n in s.last_kernel_names if "k_gemv_small<" in n]
    return sum(n.endswith(", 1>") for n in small), sum(n.endswith(", 2>") for n in small)


def run_both(w, cfg, B, **kw):
    """knob off / on: logits of 8 teacher-forced steps, tokens of a 64-step seeded free run (graph and eager)"""
    V, Cn = cfg.model.tgt_vocab_size, cfg.data.channels
    rng = np.random.default_rng(5)
    teacher = [rng.integers(0, V - 4, size=(10, Cn)).astype(np.int32) for _ in range(B)]
    res = {}
    for knob in (0, 1):
        hb.set_tuning("wo_defer", knob)
        try:
            s = session(w, cfg, B, teacher=teacher, **kw)
            lg = []
            for _ in range(8):
                s.decode(1, use_graph=False)
                lg.append(s.logits_host().copy())
            n_launch, f = s.launches_per_step(), forms(s)
            s.close()
            toks = []
            for graph in (True, False):
                s = session(w, cfg, B, **kw)
                s.decode(64, use_graph=graph)
                s.sync()
                toks.append([r.tokens.copy() for r in s.results()])
                s.close()
        finally:
            hb.set_tuning("wo_defer", -1)
        res[knob] = (lg, toks, n_launch, f)
    return res


def assert_same(res):
    (lg0, tk0, n0, _), (lg1, tk1, n1, _) = res[0], res[1]
    assert n0 == n1
    for a, b in zip(lg0, lg1):
        assert np.array_equal(a, b) and np.isfinite(a).all() and np.abs(a).max() > 0
    for run in (tk0[0], tk0[1], tk1[0], tk1[1]):           # graph / eager, knob off / on: one token stream
        for a, b in zip(tk0[0], run):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("B,kv", [(1, "f32"), (2, "f32"), (1, "bf16"), (2, "bf16x2")])
def test_model_knob_on_equals_knob_off(model, dense, B, kv):
    cfg, _ = model
    res = run_both(dense, cfg, B, kv_dtype=kv)
    nl = cfg.model.decoder.n_layer
    assert res[0][3] == (0, 0)
    assert res[1][3] == (nl, nl)            # every wo, and behind each the next layer's q/k/v projection or the logits head
    assert res[1][2] == nl * 8 + 2
    assert_same(res)


def test_model_batch_3_keeps_the_in_launch_merge(model, dense):
    cfg, _ = model
    res = run_both(dense, cfg, 3)
    assert res[0][3] == (0, 0) and res[1][3] == (0, 0)
    assert_same(res)


@pytest.mark.parametrize("variant", ["compacted", "weight_planes", "sparse24", "mxfp8"])
def test_model_variants_keep_the_in_launch_merge(model, variant):
    from dia_hip.engine import DeviceWeights
    from dia_hip.pruning import semi_structured_prune_state_dict, structured_prune_state_dict
    from dia_hip.quant import mxfp8_quantize_state_dict
    cfg, sd = model
    if variant == "compacted":
        w = DeviceWeights(cfg, structured_prune_state_dict(cfg, sd, 0.5)[0], dev())
    elif variant == "weight_planes":
        w = DeviceWeights(cfg, sd, dev(), weight_planes=2)
    elif variant == "sparse24":
        w = DeviceWeights(cfg, semi_structured_prune_state_dict(cfg, sd), dev(), sparse="2:4")
    else:
        w = DeviceWeights(cfg, mxfp8_quantize_state_dict(cfg, sd), dev(), quant="mxfp8")
    res = run_both(w, cfg, 1)
    assert res[0][3] == (0, 0) and res[1][3] == (0, 0)
    assert_same(res)
