"""DecodeSession(self_kv="fp8") on the mid synthetic model (DESIGN.md "FP8 self K/V"): graph replay against eager launches and
against itself, a slot session against solo runs, the audio-prompt replay against teacher-forced steps, together with
cross_kv="fp8", under score=True, the bytes of the self caches, and the default session launch for launch."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from dia_hip import binding as hb
from dia_hip import config as CF


def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def mid():
    from dia_hip.engine import DeviceWeights
    from dia_hip.weights import synthetic_state_dict
    cfg = CF.mid_config()
    return cfg, DeviceWeights(cfg, synthetic_state_dict(cfg, seed=1234, std=0.02), dev())


def ids_of(n, seed):
    return np.random.RandomState(seed).randint(32, 127, size=(n,)).astype(np.int32)


def run_steps(w, steps, use_graph, **kw):
    from dia_hip.engine import DecodeSession
    s = DecodeSession(w, [ids_of(12, 1), ids_of(45, 2)], kv_dtype="bf16", max_tokens=steps + 4, seeds=[11, 12], ignore_eos=True, **kw)
    try:
        s.prefill()
        s.decode(steps, use_graph=use_graph)
        s.sync()
        assert s.cur.tolist() == [steps + 1, steps + 1]
        toks, logits = [r.tokens.copy() for r in s.results()], s.logits_host().copy()
        names = (s.time_step(), list(s.last_kernel_names))[1] if not use_graph else None       # (one more step, timed: its kernel names)
        return toks, logits, names, s.launches_per_step()
    finally:
        s.close()


def test_graph_equals_eager_and_repeats(mid):
    cfg, w = mid
    tg, lg, _, n_launch = run_steps(w, 40, True, self_kv="fp8")
    te, le, names, _ = run_steps(w, 40, False, self_kv="fp8")
    t2, l2, _, _ = run_steps(w, 40, True, self_kv="fp8")
    assert np.isfinite(lg).all() and np.abs(lg).max() > 0
    for a, b, c in zip(tg, te, t2):
        assert np.array_equal(a, b) and np.array_equal(a, c) and (a[1:41] >= 0).all()
    assert np.array_equal(lg, le) and np.array_equal(lg, l2)
    # launch for launch the bf16 session's step but for the self-attention kernel, and as many launches
    _, _, names_b, n_launch_b = run_steps(w, 4, False)
    nl = cfg.model.decoder.n_layer
    assert n_launch == n_launch_b and len(names) == len(names_b)
    assert sum(n.startswith("k_attn_self_f8<4>") for n in names) == nl and not any(n.startswith("k_attn_self_f8") for n in names_b)
    for nf, nb in zip(names, names_b):
        assert nb.startswith("k_attn_mfma<4, 1>") if nf.startswith("k_attn_self_f8") else nf == nb, (nf, nb)


def test_default_session_enqueues_the_parents_kernels(mid):
    """self_kv="bf16" == a session built without the keyword, kernel name for kernel name; no fp8 buffer exists"""
    from dia_hip.engine import DecodeSession
    cfg, w = mid
    _, _, names_kw, _ = run_steps(w, 4, False, self_kv="bf16")
    _, _, names_no, _ = run_steps(w, 4, False)
    assert names_kw == names_no and not any("self_f8" in n for n in names_kw)
    s = DecodeSession(w, [ids_of(12, 1)], kv_dtype="bf16", max_tokens=8)
    try:
        assert s.self_kv == "bf16" and s.f8_self is None and s.k_self[0] is not None
    finally:
        s.close()


def test_slots_equal_solo_runs(mid):
    """three slots, four requests of different lengths: the fourth is admitted into the slot the first one to finish leaves (its
    fp8 self cache still holds that request's keys and scales beyond the new request's length).  Each result == the same request
    alone in a fresh session of the same shape, bitwise, with its own seed and sampling parameters"""
    from dia_hip.engine import DecodeSession, Request
    cfg, w = mid
    reqs = [Request(ids_of(30, 3), seed=42, max_tokens=30), Request(ids_of(25, 4), seed=7, max_tokens=12, temperature=0.9, top_k=50),
            Request(ids_of(9, 5), seed=9, max_tokens=22), Request(ids_of(50, 6), seed=5, max_tokens=26, top_p=0.8)]

    def session():
        return DecodeSession.open(w, 3, s_cap=64, kv_dtype="bf16", max_tokens=30, self_kv="fp8")

    s = session()
    try:
        out = s.serve(reqs, poll=4)
        assert s.k_self[0] is None and (s.f8_self.ks != 0).any()
    finally:
        s.close()
    for r, got in zip(reqs, out):
        solo = session()
        try:
            want = solo.serve([r], poll=4)[0]
        finally:
            solo.close()
        assert np.array_equal(got.tokens, want.tokens) and np.array_equal(got.preds, want.preds) and got.last_step == want.last_step
        assert np.array_equal(got.codes, want.codes) and got.codes.size > 0


def test_audio_prompt_replays_through_the_step(mid):
    """a 6-frame audio prompt: no batched prefill onto fp8 caches, the prompt rows go through the decode step and every prompted key
    is quantised like a generated one — the same tokens and logits as a session that is fed those rows as teacher-forced steps"""
    from dia_hip.engine import DecodeSession
    cfg, w = mid
    prompt = np.random.RandomState(2).randint(0, 1024, size=(6, cfg.data.channels)).astype(np.int32)
    ids = [ids_of(33, 8)]
    kw = dict(kv_dtype="bf16", max_tokens=40, temperature=0.0, ignore_eos=True, self_kv="fp8")
    a = DecodeSession(w, ids, audio_prompts=[prompt], **kw)
    try:
        assert a.first_steps[0] > 2 and not a._prompt_prefill_batched()
        a.prefill()
        a.sync()
        assert int(a.cur[0].item()) == 1                              # nothing was prefilled: the replay starts at step 1
        steps = 36
        a.decode(steps, use_graph=True)
        ra, la = a.results()[0], a.logits_host().copy()
        fs = a.first_steps[0]
    finally:
        a.close()
    # the same session without the keyword prefills the prompt in one batch (what the fp8 mode declines)
    p = DecodeSession(w, ids, audio_prompts=[prompt], **{**kw, "self_kv": "bf16"})
    try:
        assert p._prompt_prefill_batched()
    finally:
        p.close()
    b = DecodeSession(w, ids, teacher_tokens=[ra.tokens[: steps + 1]], **kw)
    try:
        assert not b._prompt_prefill_batched()
        b.prefill()
        b.decode(steps, use_graph=True)
        rb, lb = b.results()[0], b.logits_host().copy()
    finally:
        b.close()
    assert fs < steps and (ra.tokens[fs: steps + 1] >= 0).all()
    assert np.array_equal(ra.preds[fs: steps + 1], rb.preds[fs: steps + 1]) and np.array_equal(la, lb)
    assert np.array_equal(ra.tokens[: steps + 1], rb.tokens[: steps + 1])


def test_with_cross_fp8_and_scoring(mid):
    from dia_hip.engine import DecodeSession
    cfg, w = mid
    a = run_steps(w, 12, True, self_kv="fp8", cross_kv="fp8")
    b = run_steps(w, 12, True, self_kv="fp8", cross_kv="fp8")
    assert np.isfinite(a[1]).all() and np.array_equal(a[1], b[1]) and all(np.array_equal(x, y) for x, y in zip(a[0], b[0]))
    _, _, names, _ = run_steps(w, 2, False, self_kv="fp8", cross_kv="fp8")
    nl = cfg.model.decoder.n_layer
    assert names.count("k_attn_mfma_f8") == nl and sum(n.startswith("k_attn_self_f8<4>") for n in names) == nl
    # score=True: finite log-probabilities for every scored row
    V, Cn = cfg.model.tgt_vocab_size, cfg.data.channels
    rng = np.random.default_rng(5)
    ids = [ids_of(5, 1), ids_of(40, 2)]
    teacher = [rng.integers(0, V - 4, size=(14, Cn)).astype(np.int32) for _ in ids]
    s = DecodeSession(w, ids, kv_dtype="bf16", max_tokens=16, temperature=0.0, teacher_tokens=teacher, score=True, self_kv="fp8")
    try:
        s.prefill()
        s.decode(12, use_graph=True)
        sc = s.scores_host()
        scored = ~np.isnan(sc[..., 0])
        assert scored.sum() > 0 and np.isfinite(sc[scored]).all() and (sc[scored][:, 0] <= 0).all()
        nll = -sc[scored][:, 0].mean()
        assert np.isfinite(nll) and nll > 0
    finally:
        s.close()


def test_self_cache_bytes_and_engine_refusals(mid):
    from dia_hip.engine import DecodeSession
    cfg, w = mid
    ids = [ids_of(20, 1), ids_of(8, 2)]
    f = DecodeSession(w, ids, kv_dtype="bf16", max_tokens=8, self_kv="fp8")
    b = DecodeSession(w, ids, kv_dtype="bf16", max_tokens=8)
    try:
        assert f.R == b.R and f.T == b.T
        ratio = f.self_cache_bytes / b.self_cache_bytes
        print(f"self cache bytes: fp8 {f.self_cache_bytes}, bf16 {b.self_cache_bytes}, ratio {ratio:.5f}")
        assert ratio == (1 + 1 / 32) / 2 and ratio <= 0.52
        assert f.step_bytes(100) < b.step_bytes(100)
        assert all(t is None for t in f.k_self + f.v_self) and f._layers[0].k_self is None and f._layers[0].v_self is None
        assert all(int(t.count_nonzero()) == 0 for t in (f.f8_self.k8, f.f8_self.v8, f.f8_self.ks, f.f8_self.vs))     # zeroed once
        f.prefill()
        f.decode(1)
        f.sync()
        assert hb.lib().dia_engine_set_self_fp8(f._engine, None) == -3          # DIA_E_STATE: a step has been issued
        assert (f.f8_self.ks[:, :, :, 0] > 0).all() and (f.f8_self.ks[:, :, :, 1:] == 0).all()      # one key per row, head and layer
    finally:
        f.close()
        b.close()
    # the engine hook on an fp32-K/V engine and on a bf16 one whose V is row-major
    p = (hb.KvFp8Ptrs * cfg.model.decoder.n_layer)()
    buf = torch.zeros(64, device=dev())
    for q in p:
        q.k8 = q.v8 = q.ks = q.vs = hb.ptr(buf)
    for kw in (dict(kv_dtype="f32"), dict(kv_dtype="bf16", attention="valu"), dict(kv_dtype="bf16x2")):
        s = DecodeSession(w, ids, max_tokens=8, **kw)
        try:
            assert hb.lib().dia_engine_set_self_fp8(s._engine, p) == -1 and b"bf16 K/V" in hb.lib().dia_last_error()
        finally:
            s.close()
