"""Teacher-forced scoring on a real MI355X (csrc/score.hip, DESIGN.md "Scoring").

Kernel: dia_score against float64 log-softmax / entropy over oracle.guided_logits of the same fp32 logits.
Bound (derived, not measured): |d lp| <= 2e-5, |d H| <= 5e-5 — (l - m) rounds to <= 32 * 2^-24 ~ 2e-6 while |l - m| < 64, a
<= 1088-term fp32 sum of expf plus logf adds a few 1e-6, and the fp32 result itself carries half an ulp (<= 3.8e-6 below 64).
The bound is one on fp32 numbers below 64 in magnitude, so the logits keep the guided row in that range: the conditional row
is normal * 6 with spikes to +-30 and the unconditional row is that row plus normal * 1 — the two rows of a real step are the
same network on the same tokens — so that guidance at s = 3 moves a logit by a few units, not by 3 x 60.
Measured (MI355X): max |d lp| 7.4e-6 — 2.1e-6 over the targets with |lp| < 32; the larger ones are tail targets with lp in
(-128, -32), where one fp32 ulp is 3.8e-6 .. 7.6e-6 — and max |d H| 3.0e-7; in the step 1.2e-6 and 7.7e-7 (DESIGN.md "Scoring").

Step: the smallest model the HIP path runs is the `mid` fixture (the attention kernels are built for head_dim 128, which the
`tiny` config of tests/golden/ref_tiny.npz does not have): the weights of tests/golden/ref_mid.npz — the checkpoint
tests/test_gpu_mxfp8_model.py builds — fp32 K/V, batch 2 with different texts, 12 teacher-forced rows, one utterance with a
3-frame audio prompt."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from dia_hip import binding as hb
from dia_hip import config as C
from dia_hip import score as S
from dia_hip.engine import DecodeSession, DeviceWeights
from dia_hip.tokens import effective_text, encode_text
from dia_hip.weights import synthetic_state_dict
from oracle import dia_oracle as O

LP_TOL, H_TOL = 2e-5, 5e-5
DEV = "cuda:0"


def ref_scores(lg2, s, dm):
    """float64 (log_softmax(co) [C, V], log_softmax(g) [C, V], entropy of softmax(g) [C]) of fp32 logits [2, C, V]"""
    lg2 = torch.from_numpy(np.ascontiguousarray(lg2, dtype=np.float32))
    g = O.guided_logits(lg2.clone(), float(s), dm).double()
    lc = torch.log_softmax(lg2[1].double(), dim=-1)
    lgd = torch.log_softmax(g, dim=-1)
    p = lgd.exp()
    h = -torch.where(p > 0, p * lgd, torch.zeros_like(p)).sum(dim=-1)
    return lc.numpy(), lgd.numpy(), h.numpy()


def expect_rows(lg2, s, dm, targets):
    """[C, 3] float64 of what dia_score writes for `targets` [C] (NaN for a target outside the vocabulary)"""
    lc, lgd, h = ref_scores(lg2, s, dm)
    out = np.full((len(targets), 3), np.nan)
    for c, t in enumerate(targets):
        if 0 <= t < lc.shape[1]:
            out[c] = lc[c, t], lgd[c, t], h[c]
    return out


def compare(got, want, worst):
    """got fp32 / want float64, same shape [..., 3]: NaN and -inf where expected, the finite ones inside the kernel bound;
    worst = [max |d lp|, max |d H|, max |d lp| over the targets with |lp| < 32], updated"""
    got = got.astype(np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(np.isneginf(got), np.isneginf(want))
    fin = np.isfinite(want)
    assert np.isfinite(got[fin]).all()
    d = np.where(fin, np.abs(np.where(fin, got, 0.0) - np.where(fin, want, 0.0)), 0.0)
    worst[0] = max(worst[0], float(d[..., :2].max()))
    worst[1] = max(worst[1], float(d[..., 2].max()))
    near = fin[..., :2] & (np.abs(np.where(fin, want, 0.0))[..., :2] < 32)
    worst[2] = max(worst[2], float(np.where(near, d[..., :2], 0.0).max()))


# ------------------------------------------------------------------------------------------------ kernel
KINDS = ("argmax", "tail", "eos", "pad", "neg1", "V", "rand", "bos")
# (B, C, V, eos, pad, bos): the ids of Dia where the vocabulary holds them; V = 1026 with eos = 1024 leaves only PAD behind EOS
# (V <= eos + 2), BOS then sits below; the small vocabularies keep all three inside
SHAPES = [(1, 9, 1028, 1024, 1025, 1026), (3, 9, 1028, 1024, 1025, 1026), (2, 1, 64, 60, 61, 62), (2, 2, 65, 61, 62, 63),
          (1, 12, 1088, 1024, 1025, 1026), (2, 9, 1026, 1024, 1025, 1023)]


@pytest.mark.parametrize("s", [0.0, 3.0])
@pytest.mark.parametrize("B,Cn,V,eos,pad,bos", SHAPES)
def test_kernel_against_float64(B, Cn, V, eos, pad, bos, s):
    L = hb.lib()
    dm = types.SimpleNamespace(eos=eos, pad=pad, bos=bos, tgt_vocab=V)
    rs = np.random.RandomState(0)
    ld = 16 * -(-(Cn * V) // 16)
    co = rs.normal(size=(B, Cn, V)) * 6
    for b in range(B):
        for c in range(Cn):
            at = rs.choice(V, size=6, replace=False)
            co[b, c, at] = np.where(rs.rand(6) < 0.5, 30.0, -30.0)
    un = co + rs.normal(size=co.shape)
    lg = np.stack([un, co], axis=1).astype(np.float32)                     # [B, 2, C, V]
    dev_lg = torch.full((2 * B, ld), 777.0, dtype=torch.float32, device=DEV)
    dev_lg[:, : Cn * V] = torch.from_numpy(lg.reshape(2 * B, Cn * V)).to(DEV)
    refs = [ref_scores(lg[b], s, dm) for b in range(B)]

    nk = len(KINDS)
    T = nk + 2                                                             # row 0: BOS; row 1: never scored; rows 2 .. T-1: one per round
    def target(kind, b, c):
        g = refs[b][1][c]
        fin = np.isfinite(g)
        return {"argmax": int(np.argmax(g)), "tail": int(np.argmin(np.where(fin, g, np.inf))), "eos": eos, "pad": pad, "neg1": -1,
                "V": V, "rand": int(rs.randint(0, V)), "bos": bos}[kind]
    tok = np.full((B, T, Cn), bos, dtype=np.int32)
    want = np.full((B, T, Cn, 3), np.nan)
    for b in range(B):
        for r in range(nk):
            t = 2 + (r + b) % nk
            tg = [target(KINDS[(r + c) % nk], b, c) for c in range(Cn)]
            tok[b, t] = tg
            want[b, t] = expect_rows(lg[b], s, dm, tg)
    # what the issue names must be among the targets of every case: EOS on channel 0 (finite) and on channel 1 (-inf), PAD (-inf)
    assert (tok[:, 2:, 0] == eos).any() and (Cn < 2 or (tok[:, 2:, 1] == eos).any()) and (tok[:, 2:] == pad).any()
    assert np.isneginf(want[..., 1]).any() and np.isnan(want[:, 2:]).any() and np.isfinite(want[:, 2:, 0, 1]).any()

    GUARD = 64
    n_out = B * T * Cn * 3
    buf = torch.full((GUARD + n_out + GUARD,), 12345.0, dtype=torch.float32, device=DEV)
    buf[GUARD: GUARD + n_out] = float("nan")
    dev_tok = torch.from_numpy(tok).to(DEV)
    st = torch.cuda.Stream(device=DEV)

    def launch(cur, first):
        a = hb.ScoreArgs()
        a.logits, a.ld_logits, a.B, a.T, a.C, a.V = hb.ptr(dev_lg), ld, B, T, Cn, V
        a.cfg_scale, a.eos, a.pad, a.bos = s, eos, pad, bos
        a.tokens = hb.ptr(dev_tok)
        cur_t = torch.tensor(cur, dtype=torch.int32, device=DEV)
        fs_t = torch.tensor(first, dtype=torch.int32, device=DEV) if first is not None else None
        a.cur, a.first_step, a.out = hb.ptr(cur_t), hb.ptr(fs_t), buf.data_ptr() + 4 * GUARD
        torch.cuda.synchronize()
        hb.check(L.dia_score(ctypes.byref(a), ctypes.c_void_p(st.cuda_stream)), "dia_score")
        st.synchronize()

    for r in range(nk):
        launch([2 + (r + b) % nk for b in range(B)], None if r % 2 else [1 + (b % 2) for b in range(B)])
    # one utterance below its first_step (a replay row: nothing written) next to one at the last row and one past the buffer
    launch([1, T - 1, T][:B], [2, 1, 1][:B])
    host = buf.cpu().numpy()
    assert (host[:GUARD] == 12345.0).all() and (host[GUARD + n_out:] == 12345.0).all()
    got = host[GUARD: GUARD + n_out].reshape(B, T, Cn, 3)
    assert np.isnan(got[:, :2]).all()                                      # the NaN fill of rows no launch scored
    worst = [0.0, 0.0, 0.0]
    compare(got, want, worst)
    print(f"B={B} C={Cn} V={V} s={s}: max |d lp| {worst[0]:.3e} ({worst[2]:.3e} where |lp| < 32), max |d H| {worst[1]:.3e}")
    assert worst[0] <= LP_TOL and worst[1] <= H_TOL, worst

    # per-utterance guidance scales give the same numbers as the scalar
    buf2 = torch.full((n_out,), float("nan"), dtype=torch.float32, device=DEV)
    a = hb.ScoreArgs()
    a.logits, a.ld_logits, a.B, a.T, a.C, a.V = hb.ptr(dev_lg), ld, B, T, Cn, V
    a.cfg_scale, a.eos, a.pad, a.bos, a.tokens = -1.0, eos, pad, bos, hb.ptr(dev_tok)
    cur_t = torch.full((B,), T - 1, dtype=torch.int32, device=DEV)
    sc_t = torch.full((B,), s, dtype=torch.float32, device=DEV)
    a.cur, a.cfg_scales, a.out = hb.ptr(cur_t), hb.ptr(sc_t), hb.ptr(buf2)
    torch.cuda.synchronize()
    hb.check(L.dia_score(ctypes.byref(a), ctypes.c_void_p(st.cuda_stream)), "dia_score")
    st.synchronize()
    assert np.array_equal(buf2.cpu().numpy().reshape(B, T, Cn, 3)[:, T - 1], got[:, T - 1], equal_nan=True)


def test_refusals_launch_nothing():
    L = hb.lib()
    out = torch.full((2 * 4 * 13 * 3,), 5.0, dtype=torch.float32, device=DEV)
    lg = torch.zeros(4, 13 * 1089 + 15, dtype=torch.float32, device=DEV)
    tok = torch.zeros(2, 4, 13, dtype=torch.int32, device=DEV)
    cur = torch.ones(2, dtype=torch.int32, device=DEV)
    for kw in (dict(C=13), dict(V=1089), dict(out=None)):
        a = hb.ScoreArgs()
        a.logits, a.ld_logits, a.B, a.T, a.C, a.V = hb.ptr(lg), lg.shape[1], 2, 4, 9, 1028
        a.eos, a.pad, a.bos, a.tokens, a.cur, a.out = 1024, 1025, 1026, hb.ptr(tok), hb.ptr(cur), hb.ptr(out)
        for k, v in kw.items():
            setattr(a, k, v)
        assert L.dia_score(ctypes.byref(a), None) == -1, kw
    torch.cuda.synchronize()
    assert bool((out == 5.0).all().item())


# ------------------------------------------------------------------------------------------------ in the step
TEXTS = ["[S1] Dia is an open weights text to dialogue model. [S2] You get full control over scripts and voices.",
         "[S1] Hello there. [S2] Hi, how are you?"]
ROWS, S_CFG = 12, 3.0


@pytest.fixture(scope="module")
def mid():
    cfg = C.mid_config()
    sd = synthetic_state_dict(cfg, seed=1234, std=0.02)                     # weight_seed / weight_std of tests/golden/ref_mid.npz
    rs = np.random.RandomState(5)
    prompt = rs.randint(0, 1024, size=(3, cfg.data.channels)).astype(np.int32)
    rows = [S.teacher_rows(cfg, rs.randint(0, 1024, size=(11, cfg.data.channels)))[:ROWS],
            S.teacher_rows(cfg, rs.randint(0, 1024, size=(8, cfg.data.channels)), prompt=prompt)[:ROWS]]
    first = [1, S.check_prompt_rows(cfg, rows[1], prompt)]
    assert first == [1, 4] and all(r.shape == (ROWS, 9) for r in rows)
    return types.SimpleNamespace(cfg=cfg, sd=sd, w=DeviceWeights(cfg, sd, torch.device(DEV)), rows=rows, first=first,
                                 prompts=[None, prompt], ids=[encode_text(effective_text(t), cfg) for t in TEXTS])


def run_session(m, w, *, score, graph, keep_logits=False):
    s = DecodeSession(w, m.ids, kv_dtype="f32", max_tokens=ROWS, cfg_scale=S_CFG, temperature=0.0, teacher_tokens=m.rows,
                      audio_prompts=m.prompts, score=score)
    s.prefill()
    steps = []
    if keep_logits:
        for _ in range(ROWS - 1):
            s.decode(1, use_graph=graph)
            steps.append(s.logits_host().copy())
    else:
        s.decode(ROWS - 1, use_graph=graph)
    s.sync()
    out = types.SimpleNamespace(scores=s.scores_host().copy() if score else None, tokens=s.tokens.cpu().numpy(), pred=s.pred.cpu().numpy(),
                                fsm=s.fsm.cpu().numpy(), logits=s.logits_host().copy(), steps=steps, launches=s.launches_per_step())
    s.close()
    return out


def check_against_own_logits(m, run):
    """(a): the scores equal float64 scores of the step's own downloaded logits; (d): nothing below first_step"""
    dm = O.Dims.of(m.cfg)
    worst = [0.0, 0.0, 0.0]
    for b in range(2):
        want = np.full((ROWS, dm.C, 3), np.nan)
        for i, lg in enumerate(run.steps):
            cur = i + 1
            if cur >= m.first[b]:
                want[cur] = expect_rows(lg[b], S_CFG, dm, m.rows[b][cur])
        compare(run.scores[b, :ROWS], want, worst)
        assert np.isnan(run.scores[b, : m.first[b]]).all() and np.isnan(run.scores[b, ROWS:]).all()
        assert np.isfinite(run.scores[b, m.first[b]: ROWS, 0]).all()        # channel 0 holds codes from its first scored row on
    print(f"step scores vs float64 of the step's logits: max |d lp| {worst[0]:.3e}, max |d H| {worst[1]:.3e}")
    assert worst[0] <= LP_TOL and worst[1] <= H_TOL, worst


@pytest.fixture(scope="module")
def eager(mid):
    return run_session(mid, mid.w, score=True, graph=False, keep_logits=True)


@pytest.fixture(scope="module")
def graph(mid):
    return run_session(mid, mid.w, score=True, graph=True)


def test_step_scores_match_the_steps_own_logits(mid, eager):
    check_against_own_logits(mid, eager)


def test_step_graph_equals_eager(eager, graph):
    assert np.array_equal(eager.scores.view(np.uint32), graph.scores.view(np.uint32))


def test_step_without_score_is_unchanged(mid, graph):
    plain = run_session(mid, mid.w, score=False, graph=True)
    for k in ("tokens", "pred", "fsm"):
        assert np.array_equal(getattr(plain, k), getattr(graph, k)), k
    assert np.array_equal(plain.logits.view(np.uint32), graph.logits.view(np.uint32))
    assert graph.launches == plain.launches + 1


def test_set_score_after_a_step_is_a_state_error(mid):
    s = DecodeSession(mid.w, mid.ids, kv_dtype="f32", max_tokens=ROWS, temperature=0.0, teacher_tokens=mid.rows)
    s.prefill()
    free = DecodeSession(mid.w, mid.ids, kv_dtype="f32", max_tokens=ROWS, temperature=0.0)
    out = torch.zeros(2, s.T, s.C, 3, device=DEV)
    a = hb.ScoreArgs()
    a.logits, a.ld_logits, a.B, a.T, a.C, a.V = hb.ptr(s.logits), s.ld_logits, 2, s.T, s.C, s.V
    a.eos, a.pad, a.bos = 1024, 1025, 1026
    a.tokens, a.cur, a.out = hb.ptr(s.tokens), hb.ptr(s.cur), hb.ptr(out)
    L = hb.lib()
    assert L.dia_engine_set_score(free._engine, ctypes.byref(a)) == -1 and b"teacher" in L.dia_last_error()
    free.close()
    s.decode(1, use_graph=False)
    assert L.dia_engine_set_score(s._engine, ctypes.byref(a)) == -3
    assert L.dia_engine_set_score(s._engine, None) == -3
    s.close()
    with pytest.raises(hb.DiaHipError):
        s2 = DecodeSession(mid.w, mid.ids, kv_dtype="f32", max_tokens=ROWS, temperature=0.0, teacher_tokens=mid.rows)
        try:
            s2.scores_host()
        finally:
            s2.close()


@pytest.fixture(scope="module")
def oracle_logits(mid):
    """the oracle's decode_step logits for the same forced rows: [b][cur - 1] = fp32 [2, C, V]"""
    try:
        torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
    except Exception:
        pass
    dm = O.Dims.of(mid.cfg)
    out = []
    for b in range(2):
        st = O.prepare(mid.sd, dm, O.text_tokens(effective_text(TEXTS[b]), dm), False)
        out.append([O.decode_step(mid.sd, st, mid.rows[b][cur - 1], cur).numpy().copy() for cur in range(1, ROWS)])
    return out


def test_step_scores_against_the_oracle(mid, eager, oracle_logits):
    """(e): guidance amplifies a logit deviation by at most 1 + 2s and log-softmax is 2-Lipschitz in the sup norm, so with
    delta = max |logits_hip - logits_oracle| measured here: |d lp_cfg| <= 2 (1 + 2s) delta + 2e-5"""
    dm = O.Dims.of(mid.cfg)
    delta = max(float(np.abs(eager.steps[i][b] - oracle_logits[b][i]).max()) for b in range(2) for i in range(ROWS - 1))
    bound = 2 * (1 + 2 * S_CFG) * delta + LP_TOL
    worst, n = 0.0, 0
    for b in range(2):
        for cur in range(mid.first[b], ROWS):
            want = expect_rows(oracle_logits[b][cur - 1], S_CFG, dm, mid.rows[b][cur])[:, 1]
            got = eager.scores[b, cur, :, 1].astype(np.float64)
            assert np.array_equal(np.isneginf(got), np.isneginf(want)) and not np.isnan(got).any()
            fin = np.isfinite(want)
            worst = max(worst, float(np.abs(got[fin] - want[fin]).max()))
            n += int(fin.sum())
    print(f"delta {delta:.3e}, bound {bound:.3e}, max |d lp_cfg| vs oracle {worst:.3e} over {n} targets")
    assert delta <= 1e-3 and n > 0 and worst <= bound, (delta, worst, bound)


def close_results(a, b):
    for k in ("lp_cond", "lp_cfg", "entropy_cfg"):
        x, y = getattr(a, k).astype(np.float64), getattr(b, k).astype(np.float64)
        assert np.array_equal(np.isnan(x), np.isnan(y)) and np.array_equal(np.isneginf(x), np.isneginf(y)), k
        fin = np.isfinite(x)
        assert np.abs(x[fin] - y[fin]).max() <= (H_TOL if k == "entropy_cfg" else LP_TOL), k
    assert np.array_equal(a.valid, b.valid) and a.n_valid == b.n_valid
    for k in ("nll_cond", "nll_cfg"):
        assert abs(getattr(a, k) - getattr(b, k)) <= LP_TOL, k
    assert abs(a.mean_entropy_cfg - b.mean_entropy_cfg) <= H_TOL


def test_dia_score_public_surface(mid, eager):
    from dia_hip.model import Dia
    dia = Dia.from_state_dict(mid.cfg, mid.sd, "float32", torch.device(DEV))
    singles = []
    for b in range(2):
        r = dia.score(TEXTS[b], mid.rows[b], audio_prompt=mid.prompts[b], cfg_scale=S_CFG)
        want = S.summarise(eager.scores[b, :ROWS], S.valid_mask(mid.rows[b], mid.first[b], mid.cfg.data))
        close_results(r, want)
        assert r.n_valid > 0 and np.isfinite(r.nll_cfg) and r.perplexity_cfg == pytest.approx(np.exp(r.nll_cfg))
        singles.append(r)
    assert singles[1].n_valid < singles[0].n_valid and not singles[1].valid[:4].any()      # the prompt rows are not scored
    both = dia.score_batch(TEXTS, [mid.rows[0], mid.rows[1][:10]], audio_prompts=mid.prompts, cfg_scale=S_CFG)
    close_results(both[0], singles[0])
    short = dia.score(TEXTS[1], mid.rows[1][:10], audio_prompt=mid.prompts[1], cfg_scale=S_CFG)      # a shorter utterance in the batch
    close_results(both[1], short)
    assert both[1].lp_cfg.shape == (10, 9)
    with pytest.raises(ValueError):
        dia.score(TEXTS[0], np.zeros((5, 8), np.int32))


def test_step_scores_with_the_mxfp8_stream(mid, tuning):
    """the hook composes with the per-matrix weight stream: (a) on an MXFP8 checkpoint's own logits; nothing about quality"""
    from dia_hip.quant import mxfp8_quantize_state_dict
    tuning("mxfp8", 0x7f7f)
    sd8 = mxfp8_quantize_state_dict(mid.cfg, mid.sd)
    w8 = DeviceWeights(mid.cfg, sd8, torch.device(DEV), quant="mxfp8")
    s = DecodeSession(w8, mid.ids, kv_dtype="f32", max_tokens=ROWS, temperature=0.0, teacher_tokens=mid.rows, score=True)
    s.prefill()
    s.time_step()
    # (an MX launch keeps its format: "k_gemm_mx<Fp8, 8, 4, false>" -> "k_gemm_mx<Fp8")
    names = set(n.split(",")[0] if n.startswith("k_gemm_mx<") else n.split("<")[0].split("::")[-1] for n in s.last_kernel_names)
    s.close()
    assert "k_gemm_mx<Fp8" in names and "k_score" in names, names
    check_against_own_logits(mid, run_session(mid, w8, score=True, graph=False, keep_logits=True))
