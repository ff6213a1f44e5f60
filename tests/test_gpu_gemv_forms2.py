"""The one-shape forms of wo's deferred pair, which kept the generic 1-4-row GEMV body until now (csrc/gemm.hip, LeadForm): the producer
and its consumer (q/k/v onto 192 strips, a logits-shaped head walking several strips per workgroup).  Each runs
under the instantiation name of the generic kernel it replaces; the knob gemv_spec = 0 puts the generic code back.  The same inputs give
the same bits with the knob on and off (out, emitted tiles, strip sums, x_new, wo's slices), both sit within 2e-5 * max(1, |ref|max) of
a float64 reference (the bound of tests/test_gpu_gemv_specialised.py), and nothing outside the valid rows and columns is written.
Then a 2-layer decoder of Dia-1.6B widths at batch 1 and 2: logits of 4 teacher-forced steps and tokens of a 16-step seeded run, graph
replay and eager, identical between the knobs.

The consumer writes x_new only where it has at least 128 workgroups (one per strip of the row: dia_gemm_wo_deferred refuses anything
else, with either knob).  The head cut to 64 strips (two per workgroup, 32 workgroups) therefore runs without x_new, and a head of 259
strips (two per workgroup, 130 workgroups, the last one with a single strip) runs with it.

wi as a form of its own was built and lost its A/B (profiles/r09_gemv_forms_ab.txt): it is not in the library.  wi still runs
here at 1, 2 and 4 rows under every value of the knob, which this change turned from on / off into a mask: same launch, same name, same
bits, float64 bound, sentinels.

Both bodies of a deferred launch report one instantiation name, so the tests read dia_last_gemv_form() to see which one ran: 3 / 4 with
the knob on, 0 with it off."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from dia_hip import binding as hb
from dia_hip import config as CF
from dia_hip import layout as lay

D, F, EPS, MPAD = 2048, 8192, 1e-5, 16
SENT = -77.25
HEADS = {"qkv": (192, 0, True), "head64": (64, 2, False), "head259": (259, 2, True)}      # strips, spw, writes x_new


def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    return torch.device("cuda:0")


def bf16r(t):
    return t.bfloat16().float()


def bound(ref):
    return 2e-5 * max(1.0, ref.abs().max().item())


def timed(g, w=None):
    """one launch -> its kernel name"""
    ms = C.c_float(0)
    if w is not None:
        hb.check(hb.lib().dia_gemm_wo_deferred(C.byref(g), C.byref(w), None, C.byref(ms)), "dia_gemm_wo_deferred")
    else:
        hb.check(hb.lib().dia_gemm_timed(C.byref(g), None, C.byref(ms)), "dia_gemm_timed")
    torch.cuda.synchronize()
    return hb.lib().dia_timed_kernel_name(0).decode()


def form():
    """which body the last call launched: 0 generic, 3 / 4 the consumer / producer form"""
    return hb.lib().dia_last_gemv_form()


@pytest.fixture(scope="module")
def mats():
    d = dev()
    g = torch.Generator(device="cpu").manual_seed(23)
    Wo = bf16r(torch.randn(F, D, generator=g) * 0.02).to(d)
    Wc = bf16r(torch.randn(D, 259 * 16, generator=g) * 0.03).to(d)          # every consumer: its first strips
    gn = bf16r(1.0 + 0.1 * torch.randn(D, generator=g)).to(d)
    return {"Wo": Wo, "Wot": lay.tile_weight(Wo)[0], "Wc": Wc, "Wct": lay.tile_weight(Wc)[0], "gn": gn}


def inputs(M, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    h = (torch.randn(M, F, generator=g) * 10.0 ** torch.randint(-3, 2, (M, F), generator=g).float()).to(dev())
    x0 = torch.randn(M, D, generator=g).to(dev())
    return h, x0


class Producer:
    """wo as the deferred producer: K = 8192 -> 2048 in two slices; every buffer it may and may not write starts as a sentinel"""

    def __init__(self, mats, M, h, x0):
        d = dev()
        self.M, self.x0 = M, x0
        self.A = lay.pack_f32_tiles(h)
        self.x = torch.full((MPAD, D), SENT, device=d)
        self.x[:M] = x0
        self.P = torch.full((1, D // 32, 64, 8), 7.0, device=d)
        self.ssq = torch.full((D // 16, MPAD), SENT, device=d)
        self.slices = torch.full((2 * MPAD * D,), SENT, device=d)
        self.tk = torch.zeros(D // 16, dtype=torch.int32, device=d)
        self.skscr = torch.full(((D // 16) * 2 * 256,), SENT, device=d)
        g = hb.GemmArgs()
        g.A, g.a_ktiles, g.M = hb.ptr(self.A), F // 32, M
        g.W, g.KT, g.nstrips, g.epi, g.act_f32 = hb.ptr(mats["Wot"]), F // 32, D // 16, hb.EPI_RESID_EMIT, 3
        g.out, g.ldo, g.gnext, g.ssq_out, g.ssq_ld = hb.ptr(self.x), D, hb.ptr(mats["gn"]), hb.ptr(self.ssq), MPAD
        g.P, g.p_plane_stride, g.p_ktiles = hb.ptr(self.P), self.P.numel(), D // 32
        g.sk, g.sk_scratch, g.sk_tickets, g.sk_scratch_floats = 2, hb.ptr(self.skscr), hb.ptr(self.tk), self.skscr.numel()
        w = hb.WoDeferArgs()
        w.defer, w.nslices, w.slices, w.slice_stride = 1, 2, hb.ptr(self.slices), MPAD * D
        self.g, self.w = g, w

    def run(self):
        self.slices.fill_(SENT)
        name = timed(self.g, self.w)
        return name, self.slices.clone()

    def rows(self, slices):
        """the two slices as [2][16][D]"""
        return torch.stack([lay.unpack_f32_tiles(slices[s * MPAD * D:(s + 1) * MPAD * D].view(1, D // 32, 64, 8), MPAD, D) for s in range(2)])


@pytest.mark.parametrize("M", [1, 2, 3, 4])
def test_producer_form_equals_generic_form(mats, tuning, M):
    h, x0 = inputs(M, 300 + M)
    p = Producer(mats, M, h, x0)
    n_new, s_new = p.run()
    f_new = form()
    tuning("gemv_spec", 0)
    n_old, s_old = p.run()
    f_old = form()
    tuning("gemv_spec", 2)                                                  # the consumer's bit alone: the producer stays generic
    p.run()
    f_other = form()
    tuning("gemv_spec", -1)
    assert (f_new, f_old, f_other) == (4, 0, 0)
    want = f"k_gemv_small<16, 8, {2 if M <= 2 else 4}, false, true, true, false, 1>"
    assert n_new == want and n_old == want, (n_new, n_old)
    assert torch.equal(s_new, s_old)
    r = p.rows(s_new)
    assert (r[:, M:] == SENT).all()                                         # rows past M of both slices
    assert torch.equal(p.x[:M], x0) and (p.x[M:] == SENT).all()             # no residual added, nothing emitted, no strip sums, no ticket
    assert (p.P == 7.0).all() and (p.ssq == SENT).all() and (p.tk == 0).all() and (p.skscr == SENT).all()
    hd, Wd = h.double(), mats["Wo"].double()
    for s in range(2):
        ref = hd[:, s * F // 2:(s + 1) * F // 2] @ Wd[s * F // 2:(s + 1) * F // 2]
        err = (r[s, :M].double() - ref).abs().max().item()
        print(f"producer M {M} slice {s}: err {err:.3e} (bound {bound(ref):.3e})")
        assert err <= bound(ref)


class Consumer:
    def __init__(self, mats, M, head, slices, x0):
        d = dev()
        ns, spw, xnew = HEADS[head]
        self.M, self.ns, self.N, self.writes = M, ns, ns * 16, xnew
        self.slices, self.x_old = slices, torch.full((MPAD, D), SENT, device=d)
        self.x_old[:M] = x0
        self.x_new = torch.full((MPAD, D), SENT, device=d)                  # the alternate residual buffer
        self.out = torch.full((MPAD, self.N + 16), SENT, device=d)
        self.ssq = torch.full((D // 16, MPAD), SENT, device=d)              # never read (the consumer rebuilds the sums), never written
        self.A = torch.full((1, D // 32, 64, 8), float("nan"), device=d)    # never read either: the image is rebuilt from the slices
        g = hb.GemmArgs()
        g.A, g.a_ktiles, g.M = hb.ptr(self.A), D // 32, M
        g.W, g.KT, g.nstrips, g.epi, g.act_f32, g.spw = hb.ptr(mats["Wct"]), D // 32, ns, hb.EPI_SCALE_STORE, 1, spw
        g.ssq_in, g.ssq_in_n, g.ssq_ld, g.inv_d, g.eps = hb.ptr(self.ssq), D // 16, MPAD, 1.0 / D, EPS
        g.out, g.ldo, g.gnext = hb.ptr(self.out), self.N + 16, hb.ptr(mats["gn"])
        w = hb.WoDeferArgs()
        w.nslices, w.slices, w.slice_stride = 2, hb.ptr(slices), MPAD * D
        w.xold, w.xnew, w.ldx = hb.ptr(self.x_old), hb.ptr(self.x_new) if xnew else None, D
        self.g, self.w = g, w

    def run(self):
        self.out.fill_(SENT)
        self.x_new.fill_(SENT)
        name = timed(self.g, self.w)
        return name, self.out.clone(), self.x_new.clone()


@pytest.fixture(scope="module")
def produced(mats):
    """wo's slices for every row count, made once by the producer (default knob) and left unchanged"""
    res = {}
    for M in (1, 2, 3, 4):
        h, x0 = inputs(M, 400 + M)
        res[M] = (h, x0, Producer(mats, M, h, x0).run()[1])
    return res


@pytest.mark.parametrize("head", list(HEADS))
@pytest.mark.parametrize("M", [1, 2, 3, 4])
def test_consumer_form_equals_generic_form(mats, produced, tuning, M, head):
    h, x0, slices = produced[M]
    c = Consumer(mats, M, head, slices, x0)
    n_new, o_new, x_new = c.run()
    f_new = form()
    tuning("gemv_spec", 0)
    n_old, o_old, x_old = c.run()
    f_old = form()
    tuning("gemv_spec", 4)                                                  # the producer's bit alone: the consumer stays generic
    c.run()
    f_other = form()
    tuning("gemv_spec", -1)
    assert (f_new, f_old, f_other) == (3, 0, 0)
    multi = "false" if head == "qkv" else "true"
    want = f"k_gemv_small<8, 8, {2 if M <= 2 else 4}, {multi}, true, true, false, 2>"
    assert n_new == want and n_old == want, (n_new, n_old)
    assert torch.equal(o_new, o_old) and torch.equal(x_new, x_old)
    N = c.N
    assert (o_new[M:] == SENT).all() and (o_new[:, N:] == SENT).all()
    assert (x_new[M:] == SENT).all() and (c.ssq == SENT).all()
    assert torch.equal(c.x_old[:M], x0) and (c.x_old[M:] == SENT).all()
    x_ref = x0.double() + h.double() @ mats["Wo"].double()
    if c.writes:
        err = (x_new[:M].double() - x_ref).abs().max().item()
        print(f"consumer {head} M {M}: x_new err {err:.3e} (bound {bound(x_ref):.3e})")
        assert err <= bound(x_ref)
    else:
        assert (x_new == SENT).all()
    ref = ((x_ref * mats["gn"].double()) @ mats["Wc"][:, :N].double()) * torch.rsqrt((x_ref ** 2).mean(-1, keepdim=True) + EPS)
    err = (o_new[:M, :N].double() - ref).abs().max().item()
    print(f"consumer {head} M {M}: out err {err:.3e} (bound {bound(ref):.3e})")
    assert err <= bound(ref) and o_new[:M, :N].abs().max().item() > 0


def test_head_of_64_strips_cannot_write_x_new(mats, produced):
    """32 workgroups cannot write back the 128 strips of the row: refused with either knob, as before"""
    h, x0, slices = produced[2]
    c = Consumer(mats, 2, "head64", slices, x0)
    c.w.xnew = hb.ptr(c.x_new)
    assert hb.lib().dia_gemm_wo_deferred(C.byref(c.g), C.byref(c.w), None, None) == -1
    torch.cuda.synchronize()


# ---- wi: no form of its own, one launch whatever the knob says ---------------------------------------------------------------------

WI_NS = 2 * F // 16                                                         # 1024 strips: 8 gate columns, then the 8 matching up columns


@pytest.fixture(scope="module")
def wi_mats():
    g = torch.Generator(device="cpu").manual_seed(29)
    W = bf16r(torch.randn(D, 2 * F, generator=g) * 0.03).to(dev())
    return W, lay.tile_weight(W)[0]


@pytest.mark.parametrize("M", [1, 2, 4])
def test_wi_is_one_launch_under_every_knob_value(wi_mats, tuning, M):
    d = dev()
    W, Wt = wi_mats
    g0 = torch.Generator(device="cpu").manual_seed(500 + M)
    x = (torch.randn(M, D, generator=g0) * 2.0).to(d)
    xp = torch.full((MPAD, D), float("nan"), device=d)
    xp[:M] = x
    A = lay.pack_f32_tiles(xp)
    ssq_in = torch.full((D // 16, MPAD), float("nan"), device=d)
    ssq_in[:, :M] = (x.double() ** 2).reshape(M, D // 16, 16).sum(-1).T.float()
    pkt = F // 32 + 1                                                       # one k-tile of emitted columns past the F the launch owns

    def run():
        out = torch.full((MPAD, 2 * F + 16), SENT, device=d)
        ssq_o = torch.full((WI_NS, MPAD), SENT, device=d)
        P = torch.full((1, pkt, 64, 8), 7.0, device=d)
        g = hb.GemmArgs()
        g.A, g.a_plane_stride, g.a_ktiles, g.M = hb.ptr(A), (D // 32) * 512, D // 32, M
        g.W, g.KT, g.nstrips, g.epi, g.act_f32 = hb.ptr(Wt), D // 32, WI_NS, hb.EPI_SWIGLU_EMIT, 3
        g.ssq_in, g.ssq_in_n, g.ssq_ld, g.inv_d, g.eps = hb.ptr(ssq_in), D // 16, MPAD, 1.0 / D, EPS
        g.out, g.ldo, g.ssq_out = hb.ptr(out), 2 * F + 16, hb.ptr(ssq_o)
        g.P, g.p_plane_stride, g.p_ktiles = hb.ptr(P), P.numel(), pkt
        name = timed(g)
        return name, form(), out, ssq_o, lay.unpack_f32_tiles(P, MPAD, pkt * 32)

    res = {}
    for knob in (-1, 0, 1, 2, 4):
        tuning("gemv_spec", knob)
        res[knob] = run()
    tuning("gemv_spec", -1)
    name, _, out, ssq_o, em = res[-1]
    assert name.startswith(f"k_gemv_small<16, 4, {2 if M <= 2 else 4}, true, true, true, false, 0>"), name
    for knob, r in res.items():
        assert r[0] == name and r[1] == 0, (knob, r[0], r[1])
        assert torch.equal(r[4], em) and torch.equal(r[2], out) and torch.equal(r[3], ssq_o)
    fill = torch.full((1, pkt, 64, 8), 7.0, device=d)
    assert (out == SENT).all() and (ssq_o == SENT).all()                    # SWIGLU emits only
    assert torch.equal(em[M:], lay.unpack_f32_tiles(fill, MPAD, pkt * 32)[M:])          # pad rows
    assert (em[:M, F:] == 7.0).all()                                        # columns past the F emitted ones
    xd = x.double()
    inv = torch.rsqrt((xd ** 2).mean(-1, keepdim=True) + EPS)
    f = ((xd * inv) @ W.double()).reshape(M, WI_NS, 2, 8)
    ref = torch.nn.functional.silu(f[:, :, 0].reshape(M, F)) * f[:, :, 1].reshape(M, F)
    err = (em[:M, :F].double() - ref).abs().max().item()
    print(f"wi M {M}: emitted err {err:.3e} (bound {bound(ref):.3e})")
    assert err <= bound(ref) and torch.isfinite(em[:M, :F]).all() and em[:M, :F].abs().max().item() > 0


# ---- model level: 2 decoder layers of Dia-1.6B widths ------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def model():
    from dia_hip.engine import DeviceWeights
    from dia_hip.weights import synthetic_state_dict
    c = CF.dia_1_6b_config()
    m = c.model
    cfg = c.model_copy(update={
        "model": m.model_copy(update={"encoder": m.encoder.model_copy(update={"n_layer": 1}), "decoder": m.decoder.model_copy(update={"n_layer": 2})}),
        "data": c.data.model_copy(update={"text_length": 128, "audio_length": 128})})
    return cfg, DeviceWeights(cfg, synthetic_state_dict(cfg, seed=1234, std=0.02), dev())


def session(w, cfg, B, teacher=None):
    from dia_hip.engine import DecodeSession
    from dia_hip.tokens import effective_text, encode_text, synthetic_text
    ids = [encode_text(effective_text(synthetic_text(32 + 16 * b, cfg)), cfg) for b in range(B)]
    s = DecodeSession(w, ids, kv_dtype="bf16", max_tokens=32, seeds=list(range(B)), ignore_eos=True, teacher_tokens=teacher)
    s.prefill()
    return s


@pytest.mark.parametrize("B", [1, 2])
def test_model_knob_on_equals_knob_off(model, tuning, B):
    cfg, w = model
    V, Cn, nl = cfg.model.tgt_vocab_size, cfg.data.channels, cfg.model.decoder.n_layer
    rng = np.random.default_rng(5)
    teacher = [rng.integers(0, V - 4, size=(6, Cn)).astype(np.int32) for _ in range(B)]
    res = {}
    for knob in (-1, 0):
        tuning("gemv_spec", knob)
        s = session(w, cfg, B, teacher)
        lg = []
        for _ in range(4):
            s.decode(1, use_graph=False)
            lg.append(s.logits_host().copy())
        s.time_step()
        names = list(s.last_kernel_names)
        s.close()
        toks = []
        for graph in (True, False):
            s = session(w, cfg, B)
            s.decode(16, use_graph=graph)
            s.sync()
            toks.append([r.tokens.copy() for r in s.results()])
            s.close()
        res[knob] = (lg, toks, names)
    # the deferred pair and wi keep their names and their counts under either knob
    def forms(names):
        small = [n for n in names if "k_gemv_small<" in n]
        return (sum(n.endswith(", 1>") for n in small), sum(n.endswith(", 2>") for n in small), sum(n.startswith("k_gemv_small<16, 4,") for n in small))
    assert forms(res[-1][2]) == forms(res[0][2]) == (nl, nl, nl), res[-1][2]
    assert len(res[-1][2]) == len(res[0][2])
    for a, b in zip(res[-1][0], res[0][0]):
        assert np.array_equal(a, b) and np.isfinite(a).all() and np.abs(a).max() > 0
    for run in (res[-1][1][1], res[0][1][0], res[0][1][1]):   # eager / knob off: the token stream of the graph-replayed run
        for a, b in zip(res[-1][1][0], run):
            assert np.array_equal(a, b)
