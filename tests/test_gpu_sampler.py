"""csrc/sample.hip step by step on a real MI355X: the token state machine over whole utterances, sampling under real guidance,
the per-slot instantiation k_sample<true>, probabilities that underflow, the edges of the route choice, other shapes,
dia_embed_tokens and dia_slot_admit / dia_slot_retire called directly.

The step's logits are SCRIPTED: they do not depend on the tokens drawn, so every draw of a multi-step run is computed on the
CPU beforehand by the oracle's own loop (oracle.dia_oracle.token_loop, the function generate() runs) fed from the script.
Everything is compared exactly: tokens, pred, cur, fsm[:, :5], the embedded row x (sequential fp32 sum in channel order) and
the planes (x * g).  The one tolerance is ssq: a strip is a sum of 16 non-negative fp32 terms, worst case about 16 * 2^-24,
compared with a float64 sum within 2^-20 relative.

Fragile draws.  Device expf and CPU exp may differ in the last bit; a draw can flip only where the reference sits on an edge.
For every sampled draw the oracle reports (sample_next_token(trace=...)) the smallest relative |cumsum[r] - top_p| and the
relative gap between the two largest p / q; every test asserts BEFORE any launch that neither is below 2^-20, and then compares
every draw.  Margins of the committed seeds (smallest over the test's draws: cut, gap), from the oracle alone:
  state machine: eos_sampled 2.1e-6, 4.1e-4; eos_again_in_countdown 3.0e-5, 1.5e-3; forced_eos 3.8e-6, 1.3e-3; ignore_eos 8.0e-6,
    1.7e-3; max_tokens_2 4.5e-5, 1.4e-2; max_delay + 1 3.1e-5, 8.7e-4; max_delay + 2 4.0e-6, 8.7e-5; prompt_replay 2.1e-6, 4.8e-4;
    teacher 2.8e-6, 1.0e-3
  guidance: cfg 1.5 1.7e-6, 7.5e-5; cfg 3.0 1.5e-6, 1.5e-4; cfg 4.0 1.1e-6, 5.6e-4
  slots 1.8e-5, 9.1e-3; underflow 2.8e-4, 1.2e-2; candidate counts 5.7e-4, 4.0e-3; top_k 64 / 65 / 100 9.6e-6, 8.1e-3
  shapes: C4_V260 1.5e-5, 1.7e-3; C9_V1088 1.1e-4, 1.6e-2; C12_V1028 1.3e-4, 6.2e-3; C4_D4096 3.4e-5, 8.9e-4
"""
import ctypes as C
import dataclasses
import itertools
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from dia_hip import binding as hb
from dia_hip import layout as lay
from oracle import dia_oracle as O

EDGE = 2.0 ** -20
SENT = 7.0                                  # poison of x / planes / ssq (exact in bf16)
DELAY9 = [0, 8, 9, 10, 11, 12, 13, 14, 15]


def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    return torch.device("cuda:0")


def bf16r(t):
    return t.bfloat16().float()


def ceil16(v):
    return (v + 15) // 16 * 16


def dims(C_=9, V=1028, T=64, eos=1024, pad=1025, bos=1026, delay=None):
    kw = {f.name: 0 for f in dataclasses.fields(O.Dims)}
    kw.update(T=T, C=C_, eos=eos, pad=pad, bos=bos, delay=list(delay or DELAY9[:C_]), tgt_vocab=V)
    return O.Dims(**kw)


_tables = {}


def tables(C_, V, D):
    """embedding tables and the norm weight (CPU fp32, bf16-representable), one set per shape"""
    if (C_, V, D) not in _tables:
        g = torch.Generator().manual_seed(1000 + C_ + V + D)
        _tables[(C_, V, D)] = (bf16r(torch.randn(C_, V, D, generator=g) * 0.1), bf16r(1 + 0.1 * torch.randn(D, generator=g)))
    return _tables[(C_, V, D)]


class Rig:
    """one sampler session: dia_sample_args over device buffers, one launch per step(), read() brings the state back"""

    def __init__(self, dm, B, D, tokens, *, max_tokens, cfg_scale=3.0, temperature=0.0, top_p=0.95, top_k=35, ignore_eos=0,
                 teacher=0, noise=None, first_step=None, slot=None, parked=()):
        d = dev()
        self.dm, self.B, self.D, self.M = dm, B, D, ceil16(2 * B)
        T, C_, V = dm.T, dm.C, dm.tgt_vocab
        self.ld = ceil16(C_ * V)
        self.lg = torch.zeros(self.M, self.ld, device=d)
        self.tok = torch.from_numpy(np.ascontiguousarray(tokens, dtype=np.int32)).to(d)
        assert self.tok.shape == (B, T, C_)
        self.pred = torch.full((B, T, C_), -1, dtype=torch.int32, device=d)
        self.cur = torch.ones(B, dtype=torch.int32, device=d)
        self.fsm = torch.zeros(B, 8, dtype=torch.int32, device=d)
        self.fsm[:, 1], self.fsm[:, 2] = -1, max(dm.delay)
        for b in parked:
            self.fsm[b, 3] = 1
        emb, gw = tables(C_, V, D)
        self.emb_h, self.g_h = emb, gw
        self.emb, self.gw = emb.to(d), gw.to(d)
        self.x = torch.full((self.M, D), SENT, device=d)
        self.P = lay.pack_planes(torch.full((self.M, D), SENT, device=d))
        self.ssq = torch.full((D // 16, self.M), SENT, device=d)
        self.dl = torch.tensor(dm.delay, dtype=torch.int32, device=d)
        self.noise = None if noise is None else noise.to(d).contiguous()
        self.fs = None if first_step is None else torch.tensor(first_step, dtype=torch.int32, device=d)
        s = self.s = hb.SampleArgs()
        s.logits, s.ld_logits, s.B, s.T, s.C, s.V, s.max_tokens = hb.ptr(self.lg), self.ld, B, T, C_, V, max_tokens
        s.cfg_scale, s.temperature, s.top_p, s.top_k = cfg_scale, temperature, top_p, top_k
        s.eos, s.pad, s.bos, s.max_delay, s.ignore_eos, s.teacher = dm.eos, dm.pad, dm.bos, max(dm.delay), ignore_eos, teacher
        s.delay, s.noise, s.noise_steps = hb.ptr(self.dl), hb.ptr(self.noise), (0 if noise is None else noise.shape[1])
        s.tokens, s.pred, s.cur, s.fsm, s.first_step = hb.ptr(self.tok), hb.ptr(self.pred), hb.ptr(self.cur), hb.ptr(self.fsm), hb.ptr(self.fs)
        e = s.embed
        e.D, e.emb, e.g, e.x = D, hb.ptr(self.emb), hb.ptr(self.gw), hb.ptr(self.x)
        e.P, e.p_plane_stride, e.p_ktiles, e.ssq_ld, e.ssq = hb.ptr(self.P), self.P[0].numel(), D // 32, self.M, hb.ptr(self.ssq)
        if slot is not None:                      # per-slot values: the k_sample<true> instantiation
            self.slot = [torch.tensor(slot[k], dtype=t, device=d) for k, t in
                         (("cfg_scale", torch.float32), ("temperature", torch.float32), ("top_p", torch.float32),
                          ("top_k", torch.int32), ("max_tokens", torch.int32))]
            s.slot_cfg_scale, s.slot_temperature, s.slot_top_p, s.slot_top_k, s.slot_max_tokens = (hb.ptr(t) for t in self.slot)

    def step(self, logits):
        B, dm = self.B, self.dm
        self.lg[: 2 * B, : dm.C * dm.tgt_vocab] = logits.reshape(2 * B, -1).to(self.lg.device)
        hb.check(hb.lib().dia_sample(C.byref(self.s), None), "dia_sample")
        torch.cuda.synchronize()

    def read(self):
        return dict(tok=self.tok.cpu().numpy(), pred=self.pred.cpu().numpy(), cur=self.cur.cpu().numpy(),
                    fsm=self.fsm[:, :5].cpu().numpy(), x=self.x.cpu(), planes=lay.unpack_planes(self.P, self.M, self.D).cpu(),
                    ssq=self.ssq.cpu())


def check_embedding(rig, got, prev, b, row, where):
    """row: the token row whose embedding rows 2b, 2b+1 must hold now; None: they are what they were"""
    for m in (2 * b, 2 * b + 1):
        if row is None:
            assert torch.equal(got["x"][m], prev["x"][m]) and torch.equal(got["planes"][m], prev["planes"][m]) and \
                torch.equal(got["ssq"][:, m], prev["ssq"][:, m]), ("embedding moved", where, b)
            continue
        e = rig.emb_h[0, int(row[0])].clone()
        for c in range(1, rig.dm.C):              # sequential fp32 sum in channel order (layers.py:691-696)
            e = e + rig.emb_h[c, int(row[c])]
        assert torch.equal(got["x"][m], e), ("x", where, b)
        assert torch.equal(got["planes"][m], e * rig.g_h), ("planes", where, b)
        want = (e.double() ** 2).reshape(-1, 16).sum(-1)
        err = ((got["ssq"][:, m].double() - want).abs() / want).max().item()
        assert err <= EDGE, ("ssq", where, b, err)


def run_oracle(dm, tokens0, script, *, first_step, max_tokens, cfg_scale, temperature, top_p, top_k, noise, ignore_eos=False,
               teacher=False, limit=None):
    """token_loop for every utterance of a session on the scripted logits [launch, 2B, C, V] (the launch that works on row
    cur is cur - 1).  Per-utterance values may be lists.  Returns (steps per utterance, (smallest cut, smallest gap))."""
    B = tokens0.shape[0]
    per = lambda v, b: v[b] if isinstance(v, (list, tuple)) else v
    out, trace = [], []
    for b in range(B):
        tok = tokens0[b].copy()
        tk = per(top_k, b)
        loop = O.token_loop(dm, tok, per(first_step, b), per(max_tokens, b), lambda row, cur, b=b: script[cur - 1, 2 * b: 2 * b + 2],
                            cfg_scale=per(cfg_scale, b), temperature=per(temperature, b), top_p=per(top_p, b),
                            top_k=tk if tk > 0 else None, noise=None if noise is None else noise[b],
                            forced_tokens=tokens0[b].copy() if teacher else None, ignore_eos=ignore_eos, trace=trace)
        out.append(list(itertools.islice(loop, limit)))
    cut = min([t[0] for t in trace], default=math.inf)
    gap = min([t[1] for t in trace], default=math.inf)
    return out, (cut, gap)


def assert_margins(m, what):
    print(f"margins {what}: cut {m[0]:.3g}, gap {m[1]:.3g}")
    assert m[0] >= EDGE and m[1] >= EDGE, ("a reference draw sits on an edge: choose another seed", what, m)


def drive(rig, exp, script, tokens0, *, extra=3, parked=(), shadows=None, until_finished=True):
    """launch until every utterance has finished and `extra` launches more; after EVERY launch the whole device state against
    the oracle's steps.  shadows: {b: Rig of batch 1} launched in lockstep on utterance b's logits, compared bitwise.
    until_finished=False: `exp` is a run cut short; its steps are driven and every utterance must still be going after them."""
    B, md = rig.B, max(rig.dm.delay)
    want_tok, want_pred = tokens0.astype(np.int32).copy(), np.full(tokens0.shape, -1, dtype=np.int32)
    want_cur = np.ones(B, dtype=np.int32)
    want_fsm = np.tile(np.array([0, -1, md, 0, 0], dtype=np.int32), (B, 1))
    for b in parked:
        want_fsm[b, 3] = 1
    prev = rig.read()
    n = max(len(e) for b, e in enumerate(exp) if b not in parked)
    for k in range(n + (extra if until_finished else 0)):
        lg = script[min(k, script.shape[0] - 1)]
        rig.step(lg)
        got = rig.read()
        for b in range(B):
            moved = False
            if b not in parked and k < len(exp[b]):
                s = exp[b][k]
                assert s.cur == want_cur[b] == k + 1
                want_tok[b, s.cur] = s.row
                if not s.replay:
                    want_pred[b, s.cur] = s.pred
                want_fsm[b] = [int(s.eos_detected), s.eos_countdown, s.bos_countdown, int(s.finished), s.last_step]
                moved = not s.finished
                if moved:
                    want_cur[b] = s.cur + 1
            check_embedding(rig, got, prev, b, want_tok[b, want_cur[b] - 1] if moved else None, k)
            if shadows and b in shadows:
                sh = shadows[b]
                sh.step(lg[2 * b: 2 * b + 2])
                one = sh.read()
                for key in ("tok", "pred", "cur", "fsm"):
                    assert np.array_equal(one[key][0], got[key][b]), ("batch-1 closed form differs", key, k, b)
                assert torch.equal(one["x"][:2], got["x"][2 * b: 2 * b + 2]), ("batch-1 closed form differs: x", k, b)
        assert np.array_equal(got["pred"], want_pred), ("pred", k, np.argwhere(got["pred"] != want_pred)[:4])
        assert np.array_equal(got["tok"], want_tok), ("tokens", k, np.argwhere(got["tok"] != want_tok)[:4])
        assert np.array_equal(got["cur"], want_cur), ("cur", k, got["cur"], want_cur)
        assert np.array_equal(got["fsm"], want_fsm), ("fsm", k, got["fsm"], want_fsm)
        prev = got
    live = [b for b in range(B) if b not in parked]
    assert all(exp[b][-1].finished == until_finished for b in live) and (got["fsm"][live, 3] == int(until_finished)).all()


def fresh_tokens(dm, B, prompts=None):
    """[B, T, C] token buffers as a session starts them: the delayed prefill, -1 behind it; and first_step per utterance"""
    tok = np.full((B, dm.T, dm.C), -1, dtype=np.int32)
    first = []
    for b in range(B):
        pre, fs = O.delayed_prefill(dm, None if not prompts or prompts[b] is None else prompts[b])
        rows = min(pre.shape[0], dm.T)
        tok[b, :rows] = pre[:rows]
        first.append(fs)
    return tok, first


def make_script(dm, B, launches, seed, spikes=()):
    """scripted logits [launches, 2B, C, V], uncond != cond; the EOS logit of channel 0 is out of reach except at the
    (launch, utterance) pairs of `spikes`, where guidance lifts it far above everything"""
    g = torch.Generator().manual_seed(seed)
    cond = torch.randn(launches, B, dm.C, dm.tgt_vocab, generator=g) * 2.0
    unc = cond - 0.5 * torch.randn(launches, B, dm.C, dm.tgt_vocab, generator=g)
    cond[:, :, 0, dm.eos] = -30.0
    unc[:, :, 0, dm.eos] = -30.0
    for k, b in spikes:
        if k < launches:
            cond[k, b, 0, dm.eos], unc[k, b, 0, dm.eos] = 60.0, 0.0
    return torch.stack([unc, cond], dim=2).reshape(launches, 2 * B, dm.C, dm.tgt_vocab)


def noise_for(B, steps, dm, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.empty(B, steps, dm.C, dm.tgt_vocab).exponential_(1.0, generator=g)


# ---------------------------------------------------------------------------------------------------
# a. the state machine of a closed batch, every step, against token_loop
# ---------------------------------------------------------------------------------------------------
SAMPLED = dict(temperature=1.3, top_p=0.95, top_k=35)
GREEDY = dict(temperature=0.0, top_p=0.95, top_k=35)
EOS_AT = [(4, 0), (19, 1), (16, 2), (24, 3)]                      # (launch, utterance): natural EOS at row launch + 1
FSM_CASES = {
    # name: (max_tokens, sampling, spikes, extra session values, seed)
    "eos_greedy": (48, GREEDY, EOS_AT, {}, 1),
    "eos_sampled": (48, SAMPLED, EOS_AT, {}, 2),
    "eos_again_in_countdown": (48, SAMPLED, EOS_AT + [(k + 4, b) for k, b in EOS_AT] + [(18, 2)], {}, 3),
    "forced_eos": (64, SAMPLED, [], {}, 24),
    "ignore_eos": (40, SAMPLED, EOS_AT, dict(ignore_eos=1), 5),
    "max_tokens_2": (2, SAMPLED, [], {}, 6),
    "max_tokens_max_delay_plus_1": (16, SAMPLED, [(3, 1)], {}, 17),
    "max_tokens_max_delay_plus_2": (17, SAMPLED, [(3, 1)], {}, 8),
    "prompt_replay": (56, SAMPLED, [(30, 0), (12, 2), (40, 3)], dict(prompts=[3, 0, 6, 10]), 9),   # utterance 2: EOS in its BOS window
    "teacher": (40, SAMPLED, EOS_AT, dict(teacher=1), 10),
}


def fsm_case(name):
    mt, samp, spikes, extra, seed = FSM_CASES[name]
    dm, B = dims(), 4
    extra = dict(extra)
    g = torch.Generator().manual_seed(500 + seed)
    prompts = None
    if "prompts" in extra:
        prompts = [None if n == 0 else torch.randint(0, 1024, (n, dm.C), generator=g).numpy().astype(np.int32)
                   for n in extra.pop("prompts")]
    tok, first = fresh_tokens(dm, B, prompts)
    if prompts:
        tok[3, first[3] + 2, [0, 4]] = -1                        # two unwritten entries inside utterance 3's BOS window
    if extra.get("teacher"):
        tok = torch.randint(0, 1024, tok.shape, generator=g).numpy().astype(np.int32)
    script = make_script(dm, B, mt - 1, seed, spikes)
    noise = None if samp["temperature"] == 0.0 else noise_for(B, mt - 1, dm, 900 + seed)
    exp, margins = run_oracle(dm, tok, script, first_step=first, max_tokens=mt, cfg_scale=3.0, noise=noise,
                              ignore_eos=bool(extra.get("ignore_eos")), teacher=bool(extra.get("teacher")), **samp)
    return dm, B, mt, samp, extra, tok, first, script, noise, exp, margins


@pytest.mark.parametrize("name", list(FSM_CASES))
def test_state_machine_closed_batch_every_step(name):
    dm, B, mt, samp, extra, tok, first, script, noise, exp, margins = fsm_case(name)
    assert_margins(margins, name)
    ends = [e[-1] for e in exp]
    md = max(dm.delay)
    # the script does what the case is named for (the oracle's own run says so)
    if name.startswith("eos_"):
        for k, b in EOS_AT:
            assert exp[b][k].pred[0] == dm.eos and exp[b][k].eos_countdown == md - 1 and ends[b].last_step == k + md - 1
    if name == "eos_again_in_countdown":
        assert exp[2][18].pred[0] == dm.eos and exp[2][18].row[0] == dm.eos and exp[2][17].row[0] == dm.pad
    if name == "forced_eos":
        assert all(e[mt - md - 3].eos_detected is False and e[mt - md - 2].eos_detected for e in exp)
        assert all(s.last_step == mt - 2 and s.eos_countdown == 0 for s in ends)
    if name == "ignore_eos":                                     # only the forced EOS ends it
        assert all(not any(s.eos_detected for s in e[: mt - md - 2]) and e[-1].last_step == mt - 2 for e in exp)
    if name == "teacher":
        assert all(s.last_step == mt - 1 and not s.eos_detected for s in ends)
    if name in ("ignore_eos", "teacher"):
        assert all(exp[b][k].pred[0] == dm.eos for k, b in EOS_AT)
    if name.startswith("max_tokens"):
        assert all(len(e) == mt - 1 and e[-1].last_step == (mt - 2 if mt == md + 2 else mt - 1) for e in exp)
    if name == "prompt_replay":
        assert [sum(s.replay for s in e) for e in exp] == [3, 0, 6, 10]
        assert exp[2][12].pred[0] == dm.eos and exp[2][12].bos_countdown > 0 and exp[2][12].row[0] != dm.eos
        assert ends[2].last_step == 12 + md - 1 and exp[3][first[3] + 1].row[0] == exp[3][first[3] + 1].pred[0]
    rig = Rig(dm, B, 96, tok, max_tokens=mt, cfg_scale=3.0, noise=noise, first_step=first if name == "prompt_replay" else None,
              ignore_eos=extra.get("ignore_eos", 0), teacher=extra.get("teacher", 0), **samp)
    drive(rig, exp, script, tok)


# ---------------------------------------------------------------------------------------------------
# b. guidance under sampling
# ---------------------------------------------------------------------------------------------------
ROUTES = [(1.3, 0.95, 35), (1.0, 0.5, 10), (0.7, 1.0, 0), (1.3, 0.9, 0), (2.0, 0.3, 50), (1.0, 0.95, 64), (1.3, 0.8, 100),
          (0.5, 0.95, 1), (1.3, 1.0, 35), (1.7, 0.99, 63), (1.0, 0.6, 5)]     # test_sampler_randomized_vs_oracle's list


def oracle_step(dm, B, rows, noise0, *, cfg_scale, temperature, top_p, top_k):
    """the oracle's draw on [2B, C, V] logits: (pred [B, C], margins), refusing inputs with a fragile draw"""
    trace, want = [], []
    for b in range(B):
        lg = O.guided_logits(rows[2 * b: 2 * b + 2].clone(), cfg_scale, dm)
        want.append(O.sample_next_token(lg, temperature, top_p, top_k if top_k > 0 else None, noise=noise0[b], trace=trace))
    margins = (min([t[0] for t in trace], default=math.inf), min([t[1] for t in trace], default=math.inf))
    assert margins[0] >= EDGE and margins[1] >= EDGE, ("a reference draw sits on an edge", margins)
    return torch.stack(want).numpy(), margins


def device_step(dm, B, rows, noise0, *, cfg_scale, temperature, top_p, top_k, D=64):
    """one launch at cur = 1 on [2B, C, V] logits: pred [B, C]"""
    tok, _ = fresh_tokens(dm, B)
    noise = torch.ones(B, dm.T - 1, dm.C, dm.tgt_vocab)
    noise[:, 0] = noise0
    rig = Rig(dm, B, D, tok, max_tokens=dm.T, cfg_scale=cfg_scale, temperature=temperature, top_p=top_p, top_k=top_k,
              noise=noise, ignore_eos=1)
    rig.step(rows)
    got = rig.read()
    assert (got["cur"] == 2).all()
    return got["pred"][:, 1]


@pytest.mark.parametrize("cfg_scale", [1.5, 3.0, 4.0])
def test_guided_sampling_every_route(cfg_scale):
    dm, B = dims(T=8), 16
    g = torch.Generator().manual_seed(int(cfg_scale * 10) + 200)
    bad, worst, todo = [], (math.inf, math.inf), []
    for T_, tp, tk in ROUTES:
        cond = torch.randn(B, dm.C, dm.tgt_vocab, generator=g) * float(torch.empty(1).uniform_(0.5, 2.0, generator=g))
        unc = cond - torch.randn(B, dm.C, dm.tgt_vocab, generator=g) * 0.4
        rows = torch.stack([unc, cond], dim=1).reshape(2 * B, dm.C, dm.tgt_vocab)
        q = torch.empty(B, dm.C, dm.tgt_vocab).exponential_(1.0, generator=g)
        want, m = oracle_step(dm, B, rows, q, cfg_scale=cfg_scale, temperature=T_, top_p=tp, top_k=tk)
        worst = (min(worst[0], m[0]), min(worst[1], m[1]))
        todo.append((T_, tp, tk, rows, q, want))
    print(f"margins guided cfg {cfg_scale}: cut {worst[0]:.3g}, gap {worst[1]:.3g}")
    for T_, tp, tk, rows, q, want in todo:
        got = device_step(dm, B, rows, q, cfg_scale=cfg_scale, temperature=T_, top_p=tp, top_k=tk)
        if not np.array_equal(got, want):
            bad.append((T_, tp, tk, int((got != want).sum())))
    assert not bad, bad


def find_contraction_case(s):
    """deterministic search: fp32 (c, u) with t = fl(c - u) whose exact c + s * t lies more than half an ulp above the two-rounding
    fl(c + fl(s * t)): a fused multiply-add returns a larger value there"""
    rng = np.random.default_rng(12345)
    s32 = np.float32(s)
    for _ in range(64):
        c = (rng.standard_normal(4096) * 4).astype(np.float32)
        u = (rng.standard_normal(4096) * 4).astype(np.float32)
        t = c - u
        two = c + s32 * t
        exact = c.astype(np.float64) + np.float64(s32) * t.astype(np.float64)
        hit = np.nonzero((exact - two.astype(np.float64) > 0.6 * np.spacing(np.abs(two)).astype(np.float64)) & (two > 1.0))[0]
        if hit.size:
            i = hit[0]
            return c[i], u[i], two[i]
    raise AssertionError("no contraction case found")


def test_guidance_is_not_contracted_into_an_fma():
    """greedy at cfg_scale 3: entry LO holds the value v exactly (cond == uncond), entry HI > LO reaches the same v through
    fl(c + fl(s * t)) but a larger one through a fused fl(c + s * t): the first index wins only without contraction"""
    s = 3.0
    c, u, v = find_contraction_case(s)
    t = np.float32(c - u)
    assert np.float32(c + np.float32(np.float32(s) * t)) == v                                     # two roundings: the tie
    exact = Fraction(float(c)) + Fraction(s) * Fraction(float(t))
    assert exact > Fraction(float(v)) + Fraction(float(np.spacing(v))) / 2                        # one rounding: above v
    dm, B = dims(T=8), 2
    lo, hi = [37, 411], [700, 1023]
    cond = torch.full((B, dm.C, dm.tgt_vocab), float(v) - 6.0)
    unc = cond.clone()
    for b in range(B):
        cond[b, :, lo[b]] = unc[b, :, lo[b]] = float(v)
        cond[b, :, hi[b]], unc[b, :, hi[b]] = float(c), float(u)
    rows = torch.stack([unc, cond], dim=1).reshape(2 * B, dm.C, dm.tgt_vocab)
    want = torch.stack([O.sample_next_token(O.guided_logits(rows[2 * b: 2 * b + 2].clone(), s, dm), 0.0, 0.95, 35) for b in range(B)])
    assert all((want[b] == lo[b]).all() for b in range(B))
    tok, _ = fresh_tokens(dm, B)
    rig = Rig(dm, B, 64, tok, max_tokens=dm.T, cfg_scale=s, ignore_eos=1, **GREEDY)
    rig.step(rows)
    assert np.array_equal(rig.read()["pred"][:, 1], want.numpy())


def find_division_case(temp):
    """deterministic search: adjacent fp32 a < b with fl(a / T) == fl(b / T) but fl(a * fl(1 / T)) != fl(b * fl(1 / T))"""
    T32 = np.float32(temp)
    r = np.float32(1.0) / T32
    a = np.arange(1 << 16, dtype=np.float32) * np.float32(2.0 ** -14) + np.float32(2.0)          # [2, 6): exact steps
    b = np.nextafter(a, np.float32(np.inf))
    hit = np.nonzero((a / T32 == b / T32) & (a * r != b * r))[0]
    assert hit.size, "no division case found"
    return a[hit[0]], b[hit[0]]


def test_temperature_divides():
    """top_k 1 at temperature 1.3: two entries are one ulp apart and equal after the division, so both survive the cut and the
    noise decides for the higher index; multiplied by fl(1 / T) they differ, and only the lower index would survive"""
    temp = 1.3
    a, b_ = find_division_case(temp)
    T32, r = np.float32(temp), np.float32(1.0) / np.float32(temp)
    assert a < b_ and a / T32 == b_ / T32 and b_ * r > a * r
    dm, B = dims(T=8), 2
    lo, hi = [200, 5], [800, 64 + 5]                             # second utterance: both in one lane
    cond = torch.full((B, dm.C, dm.tgt_vocab), -10.0)
    q = torch.ones(B, dm.C, dm.tgt_vocab)
    for b in range(B):
        cond[b, :, lo[b]], cond[b, :, hi[b]] = float(b_), float(a)
        q[b, :, hi[b]] = 0.25
    rows = torch.stack([cond, cond], dim=1).reshape(2 * B, dm.C, dm.tgt_vocab)
    kw = dict(cfg_scale=0.0, temperature=temp, top_p=1.0, top_k=1)
    want, _ = oracle_step(dm, B, rows, q, **kw)
    assert all((want[b] == hi[b]).all() for b in range(B))
    assert np.array_equal(device_step(dm, B, rows, q, **kw), want)


# ---------------------------------------------------------------------------------------------------
# c. k_sample<true>: eight slots with their own values
# ---------------------------------------------------------------------------------------------------
def slot_case():
    dm, B = dims(T=32), 8
    slot = dict(cfg_scale=[3.0, 1.5, 4.0, 2.0, 3.0, 0.0, 2.5, 3.5],
                temperature=[1.3, 0.0, 1.0, 0.7, 1.3, 2.0, 0.0, 1.1],
                top_p=[0.95, 0.95, 1.0, 0.5, 0.9, 0.8, 1.0, 0.99],
                top_k=[35, 35, 0, 1, 64, 65, 10, 100],       # slot 1 is greedy and slot 6 parked: the six others draw with all six
                max_tokens=[18, 9, 14, 2, 17, 12, 32, 16])
    g = torch.Generator().manual_seed(77)
    lens = [0, 2, 0, 0, 4, 1, 0, 3]
    prompts = [None if n == 0 else torch.randint(0, 1024, (n, dm.C), generator=g).numpy().astype(np.int32) for n in lens]
    tok, first = fresh_tokens(dm, B, prompts)
    parked = (6,)
    script = make_script(dm, B, dm.T - 1, 31, [(2, 0), (5, 4), (3, 7)])
    noise = noise_for(B, dm.T - 1, dm, 32)
    exp, margins = run_oracle(dm, tok, script, first_step=first, noise=noise, **slot)
    return dm, B, slot, tok, first, parked, script, noise, exp, margins


def test_slot_sampler_equals_oracle_and_closed_form():
    dm, B, slot, tok, first, parked, script, noise, exp, margins = slot_case()
    assert_margins(margins, "slots")
    assert exp[0][2].pred[0] == dm.eos and exp[4][5].pred[0] == dm.eos
    rig = Rig(dm, B, 64, tok, max_tokens=dm.T, cfg_scale=-1.0, temperature=-1.0, top_p=-1.0, top_k=7, noise=noise, first_step=first,
              slot=slot, parked=parked)                          # the scalars of the closed form are not read
    shadows = {b: Rig(dm, 1, 64, tok[b: b + 1], max_tokens=slot["max_tokens"][b], cfg_scale=slot["cfg_scale"][b],
                      temperature=slot["temperature"][b], top_p=slot["top_p"][b], top_k=slot["top_k"][b],
                      noise=noise[b: b + 1], first_step=[first[b]]) for b in range(B) if b not in parked}
    # a shadow is launched as long as its slot is (a few launches over its end included: nothing may move in either)
    drive(rig, exp, script, tok, parked=parked, shadows=shadows, extra=2)


# ---------------------------------------------------------------------------------------------------
# d. underflow and the edges of the route choice
# ---------------------------------------------------------------------------------------------------
def same_rows(cond):
    B = cond.shape[0]
    return torch.stack([cond, cond], dim=1).reshape(2 * B, *cond.shape[1:])      # uncond == cond: guided == cond at any scale


@pytest.mark.parametrize("temperature,top_p,top_k,layout", [
    (1.3, 0.9, 0, "wide"),          # 17-register route, a handful of survivors with a probability above 0
    (1.0, 0.9, 35, "ladder"),       # compact route, survivors 200 apart: all but the first underflow
    (1.3, 1.0, 0, "wide"),          # no cut at all: the final softmax underflows
])
def test_probabilities_that_underflow(temperature, top_p, top_k, layout):
    dm, B = dims(T=8), 4
    g = torch.Generator().manual_seed(41)
    if layout == "wide":
        cond = torch.empty(B, dm.C, dm.tgt_vocab).uniform_(-400.0, 0.0, generator=g) * temperature
    else:
        cond = torch.empty(B, dm.C, dm.tgt_vocab).uniform_(-9000.0, -8000.0, generator=g)
        for b in range(B):
            for c in range(dm.C):
                at = torch.randperm(1024, generator=g)[:35]
                cond[b, c, at] = -200.0 * torch.arange(35, dtype=torch.float32) + torch.rand(35, generator=g)
    x = cond[..., :1024] / temperature
    assert ((x.max(-1, keepdim=True).values - x) > 104.0).float().mean() > 0.5      # most of the vocabulary underflows in fp32
    q = torch.empty(B, dm.C, dm.tgt_vocab).exponential_(1.0, generator=g)
    want, m = oracle_step(dm, B, same_rows(cond), q, cfg_scale=3.0, temperature=temperature, top_p=top_p, top_k=top_k)
    print(f"margins underflow {layout} {top_p} {top_k}: cut {m[0]:.3g}, gap {m[1]:.3g}")
    assert np.array_equal(device_step(dm, B, same_rows(cond), q, cfg_scale=3.0, temperature=temperature, top_p=top_p, top_k=top_k), want)


def candidate_layout(total, g, V=1028):
    """one channel's logits for top_k 35: `total` values at or above the 35th largest lane maximum (lane = index % 64).  29 lanes
    carry distinct maxima 10..38, five lanes 5.0, one lane 0.0 (the bound); six more 5.0 sit as second entries: the 35th largest
    value overall is 5.0, with ties on both sides of rank 35; fillers in (0, 5) bring the count to `total`"""
    x = -50.0 - torch.rand(V, generator=g)
    lanes = torch.randperm(64, generator=g)
    top = [10.0 + j for j in range(29)] + [5.0] * 5 + [0.0]
    for j, v in enumerate(top):
        x[int(lanes[j]) + 64 * int(torch.randint(0, 11, (1,), generator=g))] = v
    free = [int(lanes[j]) + 64 * i for j in range(29) for i in range(11) if x[int(lanes[j]) + 64 * i] < -40]
    order = torch.randperm(len(free), generator=g)
    more = [5.0] * 6 + [0.5 + 0.1 * j for j in range(total - 41)]
    for j, v in enumerate(more):
        x[free[int(order[j])]] = v
    return x


@pytest.mark.parametrize("total", [64, 65])
def test_candidate_count_at_the_lane_bound(total):
    """exactly 64 candidates take the one-per-lane cut, exactly 65 the bitwise search; the true 35th value (5.0) lies above the
    lane bound (0.0) and its tie group of 11 straddles rank 35: 40 survivors either way"""
    dm, B, temp = dims(T=8), 4, 1.3
    g = torch.Generator().manual_seed(total)
    cond = torch.stack([torch.stack([candidate_layout(total, g) for _ in range(dm.C)]) for _ in range(B)])
    x = (cond / temp).numpy().copy()
    x[..., [dm.pad, dm.bos]] = -np.inf
    x[:, 1:, dm.eos] = -np.inf
    lane_max = np.pad(x, ((0, 0), (0, 0), (0, 1088 - 1028)), constant_values=-np.inf).reshape(B, dm.C, 17, 64).max(2)
    t0 = np.sort(lane_max, -1)[..., -35]
    assert ((x >= t0[..., None]).sum(-1) == total).all()
    kth = np.sort(x, -1)[..., -35]
    assert (kth > t0).all() and ((x == kth[..., None]).sum(-1) == 11).all() and ((x >= kth[..., None]).sum(-1) == 40).all()
    q = torch.empty(B, dm.C, dm.tgt_vocab).exponential_(1.0, generator=g)
    want, m = oracle_step(dm, B, same_rows(cond), q, cfg_scale=3.0, temperature=temp, top_p=0.9, top_k=35)
    print(f"margins candidates {total}: cut {m[0]:.3g}, gap {m[1]:.3g}")
    assert np.array_equal(device_step(dm, B, same_rows(cond), q, cfg_scale=3.0, temperature=temp, top_p=0.9, top_k=35), want)


def search_stops_at(x, k):
    """the bit at which a search for the k-th largest over order-preserving keys first counts exactly k (None: never)"""
    u = x.astype(np.float32).view(np.uint32).astype(np.uint64)
    key = np.where(u & 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000)
    pre = 0
    for bit in range(31, -1, -1):
        cand = pre | (1 << bit)
        cn = int((key >= cand).sum())
        if cn >= k:
            pre = cand
        if cn == k:
            return bit
    return None


@pytest.mark.parametrize("top_k,top_p,ties", [(64, 0.95, False), (65, 0.95, False), (100, 0.9, False), (100, 1.0, True)])
def test_top_k_64_65_and_the_search_exit(top_k, top_p, ties):
    """top_k 64 (lane-maxima route) and 65 (bitwise search) on the SAME logits; top_k 100 on distinct values, where the search
    stops early at a count of exactly k, and on a 1/4 grid, where ties at the k-th value keep most channels from ever counting exactly k"""
    dm, B, temp = dims(T=8), 8, 1.0
    g = torch.Generator().manual_seed(5)
    cond = torch.randn(B, dm.C, dm.tgt_vocab, generator=g) * 3.0
    if ties:
        cond = (cond * 4).round() / 4
    x = cond.numpy().copy()
    x[..., [dm.pad, dm.bos]] = -np.inf
    x[:, 1:, dm.eos] = -np.inf
    stops = [search_stops_at(x[b, c], top_k) for b in range(B) for c in range(dm.C)]
    if top_k == 100:
        assert sum(s is None for s in stops) > 36 if ties else all(s is not None and s > 0 for s in stops), stops
    q = torch.empty(B, dm.C, dm.tgt_vocab).exponential_(1.0, generator=g)
    want, m = oracle_step(dm, B, same_rows(cond), q, cfg_scale=3.0, temperature=temp, top_p=top_p, top_k=top_k)
    print(f"margins top_k {top_k} ties {ties}: cut {m[0]:.3g}, gap {m[1]:.3g}")
    assert np.array_equal(device_step(dm, B, same_rows(cond), q, cfg_scale=3.0, temperature=temp, top_p=top_p, top_k=top_k), want)


# ---------------------------------------------------------------------------------------------------
# e. shapes other than C 9, V 1028
# ---------------------------------------------------------------------------------------------------
SHAPES = {
    "C4_V260": (dims(4, 260, 32, 256, 257, 258, [0, 2, 3, 5]), 64),
    "C9_V1088": (dims(9, 1088, 32), 64),                        # V == 17 * 64: no clamped lane
    "C12_V1028": (dims(12, 1028, 32, delay=[0, 8, 9, 10, 11, 12, 13, 14, 15, 15, 4, 1]), 64),   # the most channels that fit the LDS
    "C4_D4096": (dims(4, 260, 32, 256, 257, 258, [0, 2, 3, 5]), 4096),   # two passes of the embedding loop
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_other_shapes_three_sampled_steps(name):
    dm, D = SHAPES[name]
    B, mt = 3, dm.T
    tok, first = fresh_tokens(dm, B)
    script = make_script(dm, B, 3, 60 + len(name), [(1, 2)])
    noise = noise_for(B, mt - 1, dm, 61)
    exp, margins = run_oracle(dm, tok, script, first_step=first, max_tokens=mt, cfg_scale=3.0, noise=noise, limit=3, **SAMPLED)
    assert_margins(margins, name)
    assert exp[2][1].pred[0] == dm.eos
    rig = Rig(dm, B, D, tok, max_tokens=mt, cfg_scale=3.0, noise=noise, **SAMPLED)
    drive(rig, exp, script, tok, until_finished=False)


# ---------------------------------------------------------------------------------------------------
# f. dia_embed_tokens
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act_f32", [0, 1])
@pytest.mark.parametrize("mapped", [False, True])
@pytest.mark.parametrize("slots", [None, [3, 0]])
def test_embed_tokens_direct(act_f32, mapped, slots):
    d = dev()
    B, T, C_, V, D = 5, 16, 9, 1028, 96
    M = ceil16(2 * B)
    g = torch.Generator().manual_seed(71)
    emb_h, g_h = tables(C_, V, D)
    emb, gw = emb_h.to(d), g_h.to(d)
    tok_h = torch.randint(0, V, (B, T, C_), generator=g, dtype=torch.int32)
    cur_h = torch.tensor([1, 5, 2, 16, 9], dtype=torch.int32)
    keep = torch.rand(D, generator=g) < 0.6
    keep[:2] = torch.tensor([False, True])
    nk = int(keep.sum()) if mapped else D
    cmap = torch.where(keep, torch.cumsum(keep.int(), 0) - 1, torch.full((D,), -1, dtype=torch.int64)).to(torch.int32).to(d)
    tok, cur = tok_h.to(d), cur_h.to(d)
    x = torch.full((M, D), SENT, device=d)
    poison = torch.full((M, D), SENT, device=d)
    P = lay.pack_f32_tiles(poison) if act_f32 else lay.pack_planes(poison)
    ssq = torch.full((D // 16, M), SENT, device=d)
    sl = None if slots is None else torch.tensor(slots, dtype=torch.int32, device=d)
    e = hb.EmbedArgs()
    e.tokens, e.cur, e.B, e.T, e.C, e.V, e.D, e.act_f32 = hb.ptr(tok), hb.ptr(cur), B, T, C_, V, D, act_f32
    e.emb, e.g, e.x, e.P = hb.ptr(emb), hb.ptr(gw), hb.ptr(x), hb.ptr(P)
    e.p_plane_stride, e.p_ktiles, e.ssq_ld, e.ssq = (0 if act_f32 else P[0].numel()), D // 32, M, hb.ptr(ssq)
    e.cmap = hb.ptr(cmap) if mapped else None
    e.slots, e.n_slots = hb.ptr(sl), (0 if slots is None else len(slots))
    hb.check(hb.lib().dia_embed_tokens(C.byref(e), None), "dia_embed_tokens")
    torch.cuda.synchronize()
    got_x = x.cpu()
    got_p = (lay.unpack_f32_tiles(P, M, D) if act_f32 else lay.unpack_planes(P, M, D)).cpu()
    got_s = ssq.cpu()
    listed = range(B) if slots is None else slots
    kept = keep if mapped else torch.ones(D, dtype=torch.bool)
    for b in range(B):
        for m in (2 * b, 2 * b + 1):
            if b not in listed:
                assert (got_x[m] == SENT).all() and (got_p[m] == SENT).all() and (got_s[:, m] == SENT).all(), b
                continue
            row = tok_h[b, int(cur_h[b]) - 1]
            v = emb_h[0, int(row[0])].clone()
            for c in range(1, C_):
                v = v + emb_h[c, int(row[c])]
            assert torch.equal(got_x[m], v), b
            assert torch.equal(got_p[m, :nk], (v * g_h)[kept]) and (got_p[m, nk:] == SENT).all(), b
            want = (v.double() ** 2).reshape(-1, 16).sum(-1)
            assert ((got_s[:, m].double() - want).abs() / want).max().item() <= EDGE, b
    assert (got_x[2 * B:] == SENT).all() and (got_p[2 * B:] == SENT).all() and (got_s[:, 2 * B:] == SENT).all()


# ---------------------------------------------------------------------------------------------------
# g. dia_slot_admit / dia_slot_retire
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,C_", [(64, 9), (41, 9), (512, 9), (513, 9)])
def test_slot_admit_and_retire_direct(T, C_):
    """(64, 9) and (512, 9): 16-byte stores (one and two chunks per slot); (41, 9) and (513, 9): T * C is no multiple of 4,
    the scalar stores.  Prefixes of 1, 2 and 7 rows of 9 end inside a 16-byte store, at its 1st, 2nd and 3rd lane."""
    d = dev()
    B, n, S, md, ld = 5, 3, 32, 15, 16
    g = torch.Generator().manual_seed(T)
    ints = lambda *shape: torch.randint(2000, 3000, shape, generator=g, dtype=torch.int32).to(d)
    dv = dict(tokens=ints(B, T, C_), pred=ints(B, T, C_), cur=ints(B), fsm=ints(B, 8), d_first_step=ints(B), d_text_len=ints(B),
              slot_top_k=ints(B), slot_max_tokens=ints(B))
    for k in ("slot_cfg_scale", "slot_temperature", "slot_top_p"):
        dv[k] = torch.rand(B, generator=g).to(d) + 50.0
    prefix = torch.randint(0, 1024, (n, ld, C_), generator=g, dtype=torch.int32).to(d)
    host = dict(slot=[4, 0, 2], text_len=[8, 32, 0], first_step=[1, 2, 7], prefix_rows=[1, 2, 7], max_tokens=[T, 2, 30],
                top_k=[35, 0, 100], cfg_scale=[3.0, 0.0, 1.5], temperature=[1.3, 0.0, 0.7], top_p=[0.95, 1.0, 0.5])
    a = hb.SlotAdmitArgs()
    a.B, a.T, a.C, a.S, a.max_delay, a.n, a.prefix_ld, a.prefix = B, T, C_, S, md, n, ld, hb.ptr(prefix)
    keep = []
    for k, v in host.items():
        arr = ((C.c_float if k in ("cfg_scale", "temperature", "top_p") else C.c_int32) * n)(*v)
        keep.append(arr)
        setattr(a, k, arr)
    for k, t in dv.items():
        setattr(a, k, hb.ptr(t))
    want = {k: t.cpu().clone() for k, t in dv.items()}
    hb.check(hb.lib().dia_slot_admit(C.byref(a), None), "dia_slot_admit")
    torch.cuda.synchronize()
    for i, b in enumerate(host["slot"]):
        rows = host["prefix_rows"][i]
        want["tokens"][b] = -1
        want["tokens"][b, :rows] = prefix[i, :rows].cpu()
        want["pred"][b] = -1
        want["cur"][b] = 1
        want["fsm"][b] = torch.tensor([0, -1, md, 0, 0, 0, 0, 0], dtype=torch.int32)
        want["d_first_step"][b], want["d_text_len"][b] = host["first_step"][i], host["text_len"][i]
        want["slot_top_k"][b], want["slot_max_tokens"][b] = host["top_k"][i], host["max_tokens"][i]
        for k in ("cfg_scale", "temperature", "top_p"):
            want["slot_" + k][b] = torch.tensor(host[k][i], dtype=torch.float32)
    for k, t in dv.items():
        assert torch.equal(t.cpu(), want[k]), ("admit", k)
    # retire two of them, out of order: cur, fsm[3] and text_len only
    r = hb.SlotAdmitArgs()
    r.B, r.n = B, 2
    gone = (C.c_int32 * 2)(2, 4)
    r.slot, r.cur, r.fsm, r.d_text_len = gone, hb.ptr(dv["cur"]), hb.ptr(dv["fsm"]), hb.ptr(dv["d_text_len"])
    dv["cur"][2], dv["cur"][4] = 9, 11                           # as if they had run
    want["cur"][2], want["cur"][4] = 9, 11
    hb.check(hb.lib().dia_slot_retire(C.byref(r), None), "dia_slot_retire")
    torch.cuda.synchronize()
    for b in (2, 4):
        want["cur"][b], want["fsm"][b, 3], want["d_text_len"][b] = 1, 1, 0
    for k, t in dv.items():
        assert torch.equal(t.cpu(), want[k]), ("retire", k)
