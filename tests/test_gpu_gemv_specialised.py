"""The per-epilogue forms of the 1-4-row projection GEMV at K = 2048 (csrc/gemm.hip, k_gemv_small<RS, ScaleStore> and
k_gemv_small<RS, ResidEmit>, one strip per workgroup) against the generic instantiation k_gemv_small<8, 8, RS, false, true, true, false, 0>,
which the knob gemv_spec = 0 puts back: the same inputs give the same bits (out, emitted tiles, strip sums of squares), both
sit within 2e-5 * max(1, |ref|max) of a float64 reference, and what the new forms do not serve keeps the generic name.  Then a
2-layer decoder of Dia-1.6B widths at batch 1 and 2: logits of 8 teacher-forced steps and tokens of a 32-step seeded free run
(graph replay and eager) identical with the knob on and off.

The row-major strip-sum layout of the same issue was built and measured and is not kept (profiles/r07_gemv_specialised_ab.txt):
the strip sums keep their [strip][row] layout everywhere, so there is no second layout to compare."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from dia_hip import binding as hb
from dia_hip import config as CF
from dia_hip import layout as lay

K, NMAX, EPS = 2048, 3072, 1e-5
STORE, RESID = hb.EPI_SCALE_STORE, hb.EPI_RESID_EMIT
SENT = -77.25


def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    return torch.device("cuda:0")


def bf16r(t):
    return t.bfloat16().float()


def generic_name(rs):
    return f"k_gemv_small<8, 8, {rs}, false, true, true, false, 0>"


def spec_name(rs, epi):
    return f"k_gemv_small<{rs}, {'ScaleStore' if epi == STORE else 'ResidEmit'}>"


@pytest.fixture(scope="module")
def mats():
    d = dev()
    g = torch.Generator(device="cpu").manual_seed(11)
    W = bf16r(torch.randn(K, NMAX, generator=g) * 0.03).to(d)
    gn = bf16r(1.0 + 0.1 * torch.randn(NMAX, generator=g)).to(d)
    return W, lay.tile_weight(W)[0], W.double(), gn


class Call:
    """one dia_gemm descriptor over fixed inputs; run() fills fresh outputs and returns (kernel name, out, tiles, ssq_out)"""

    def __init__(self, mats, M, ns, epi, seed, *, cmap=None, ssq_n=None, nw=0, spw=0):
        d = dev()
        self.W, self.Wt, self.Wd, self.gn = mats
        self.M, self.ns, self.epi, self.N = M, ns, epi, ns * 16
        self.mpad = mpad = (M + 15) // 16 * 16
        gen = torch.Generator(device="cpu").manual_seed(seed)
        self.x = (torch.randn(M, K, generator=gen) * (1.0 if epi == RESID else 2.0)).to(d)
        xp = torch.full((mpad, K), float("nan"), device=d)
        xp[:M] = self.x
        self.A = lay.pack_f32_tiles(xp)
        self.x0 = torch.randn(M, self.N, generator=gen).to(d)
        self.ssq_in = torch.full((K // 16, mpad), float("nan"), device=d)
        self.ssq_in[:, :M] = (self.x.double() ** 2).reshape(M, K // 16, 16).sum(-1).T.float()
        self.cmap, self.ssq_n, self.nw, self.spw = cmap, ssq_n, nw, spw

    def run(self):
        d, M, N, ns, mpad = dev(), self.M, self.N, self.ns, self.mpad
        out = torch.full((mpad, N + 16), SENT, device=d)
        ssq_o = torch.full((ns, mpad), SENT, device=d)
        P = torch.full((mpad // 16, N // 32, 64, 8), 7.0, device=d)
        g = hb.GemmArgs()
        g.A, g.a_ktiles, g.a_plane_stride, g.M = hb.ptr(self.A), K // 32, (mpad // 16) * (K // 32) * 512, M
        g.W, g.KT, g.nstrips, g.epi, g.nw, g.spw = hb.ptr(self.Wt), K // 32, ns, self.epi, self.nw, self.spw
        g.ssq_ld, g.out, g.ldo = mpad, hb.ptr(out), N + 16
        if self.epi == STORE:
            g.act_f32 = 1
            g.ssq_in, g.ssq_in_n, g.inv_d, g.eps = hb.ptr(self.ssq_in), self.ssq_n or K // 16, 1.0 / K, EPS
        else:
            g.act_f32 = 3
            out[:M, :N] = self.x0
            g.gnext, g.ssq_out = hb.ptr(self.gn), hb.ptr(ssq_o)
            g.P, g.p_plane_stride, g.p_ktiles = hb.ptr(P), P.numel(), N // 32
            if self.cmap is not None:
                g.cmap = hb.ptr(self.cmap)
        ms = C.c_float()
        hb.check(hb.lib().dia_gemm_timed(C.byref(g), None, C.byref(ms)), "dia_gemm_timed")
        torch.cuda.synchronize()
        return hb.lib().dia_timed_kernel_name(0).decode(), out, P, ssq_o

    def check_f64(self, out, P, ssq_o):
        M, N, ns = self.M, self.N, self.ns
        xd, Wd = self.x.double(), self.Wd[:, :N]
        assert (out[M:] == SENT).all() and (out[:, N:] == SENT).all()
        if self.epi == STORE:
            ref = (xd @ Wd) * torch.rsqrt((xd ** 2).mean(-1, keepdim=True) + EPS)
            assert (ssq_o == SENT).all() and (P == 7.0).all()
        else:
            ref = self.x0.double() + xd @ Wd
            want = (out[:M, :N].double() ** 2).reshape(M, ns, 16).sum(-1).T
            assert (ssq_o[:, :M].double() - want).abs().max().item() <= 1e-5 * want.max().item()
            assert (ssq_o[:, M:] == SENT).all()
            assert torch.equal(lay.unpack_f32_tiles(P, self.mpad, N)[:M], out[:M, :N] * self.gn[:N])
        err = (out[:M, :N].double() - ref).abs().max().item()
        bound = 2e-5 * max(1.0, ref.abs().max().item())
        print(f"M {M} strips {ns} epi {self.epi}: err {err:.3e} (bound {bound:.3e})")
        assert err <= bound


def both(call, tuning):
    """(new form's results, generic form's results) of one call"""
    new = call.run()
    tuning("gemv_spec", 0)
    old = call.run()
    tuning("gemv_spec", -1)
    return new, old


@pytest.mark.parametrize("M", [1, 2, 3, 4])
@pytest.mark.parametrize("ns,epi", [(128, STORE), (128, RESID), (192, RESID), (130, STORE), (130, RESID)],
                         ids=["store128", "resid128", "resid192", "store130", "resid130"])
def test_specialised_form_equals_generic_form(mats, tuning, M, ns, epi):
    rs = 2 if M <= 2 else 4
    call = Call(mats, M, ns, epi, seed=100 * ns + 10 * epi + M)
    new, old = both(call, tuning)
    assert new[0] == spec_name(rs, epi), new[0]
    assert old[0] == generic_name(rs), old[0]
    for a, b in zip(new[1:], old[1:]):
        assert torch.equal(a, b)
    call.check_f64(*new[1:])
    call.check_f64(*old[1:])


@pytest.mark.parametrize("M", [2, 4])
def test_store_over_fewer_strip_sums(mats, tuning, M):
    """row scales over 96 of the 128 strip sums (a caller that norms a narrower row): the clamped requests past the count add nothing"""
    call = Call(mats, M, 128, STORE, seed=7 + M, ssq_n=96)
    new, old = both(call, tuning)
    assert new[0] == spec_name(2 if M <= 2 else 4, STORE) and old[0] == generic_name(2 if M <= 2 else 4)
    assert torch.equal(new[1], old[1])
    xd = call.x.double()
    inv = torch.rsqrt((xd[:, : 96 * 16] ** 2).sum(-1, keepdim=True) / K + EPS)
    ref = (xd @ call.Wd[:, : call.N]) * inv
    assert (new[1][:M, : call.N].double() - ref).abs().max().item() <= 2e-5 * max(1.0, ref.abs().max().item())


def test_what_the_new_forms_leave_to_the_generic_one(mats):
    """one strip per workgroup, so there is no partial last group to serve (130 strips run the new forms, above): q/k/v's SCALE_STORE
    at 192 strips (pinned by tests/test_gpu_wo_deferred.py), a compaction map on the edge, an explicit wave count, several strips per
    workgroup and 5 rows keep the names they had"""
    d = dev()
    ident = torch.arange(2048, dtype=torch.int32, device=d)
    cases = [(Call(mats, 4, 192, STORE, 3), generic_name(4)), (Call(mats, 2, 192, STORE, 2), generic_name(2)), (Call(mats, 2, 128, RESID, 4, cmap=ident), generic_name(2)),
             (Call(mats, 2, 128, STORE, 5, nw=8), generic_name(2)),
             (Call(mats, 2, 128, RESID, 6, spw=2), "k_gemv_small<8, 8, 2, true, true, true, false, 0>"),
             (Call(mats, 5, 128, STORE, 7), "k_gemm16<")]
    for call, want in cases:
        name, out, P, ssq_o = call.run()
        assert name == want or (want.endswith("<") and name.startswith(want)), (name, want)
        call.check_f64(out, P, ssq_o)


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
    s = DecodeSession(w, ids, kv_dtype="bf16", max_tokens=48, seeds=list(range(B)), ignore_eos=True, teacher_tokens=teacher)
    s.prefill()
    return s


@pytest.mark.parametrize("B", [1, 2])
def test_model_knob_on_equals_knob_off(model, tuning, B):
    cfg, w = model
    V, Cn, nl = cfg.model.tgt_vocab_size, cfg.data.channels, cfg.model.decoder.n_layer
    rng = np.random.default_rng(5)
    teacher = [rng.integers(0, V - 4, size=(10, Cn)).astype(np.int32) for _ in range(B)]
    res = {}
    for knob in (-1, 0):
        tuning("gemv_spec", knob)
        s = session(w, cfg, B, teacher)
        lg = []
        for _ in range(8):
            s.decode(1, use_graph=False)
            lg.append(s.logits_host().copy())
        s.time_step()
        names = list(s.last_kernel_names)
        s.close()
        toks = []
        for graph in (True, False):
            s = session(w, cfg, B)
            s.decode(32, use_graph=graph)
            s.sync()
            toks.append([r.tokens.copy() for r in s.results()])
            s.close()
        res[knob] = (lg, toks, names)
    rs = 2 if 2 * B <= 2 else 4
    spec = lambda names: (sum(n == spec_name(rs, STORE) for n in names), sum(n == spec_name(rs, RESID) for n in names))
    assert spec(res[-1][2]) == (nl, 2 * nl), res[-1][2]        # cq; o and co
    assert spec(res[0][2]) == (0, 0) and len(res[0][2]) == len(res[-1][2])
    for a, b in zip(res[-1][0], res[0][0]):
        assert np.array_equal(a, b) and np.isfinite(a).all() and np.abs(a).max() > 0
    for run in (res[-1][1][1], res[0][1][0], res[0][1][1]):   # eager / knob off: the token stream of the graph-replayed run
        for a, b in zip(res[-1][1][0], run):
            assert np.array_equal(a, b)
