"""prompt_prefill="batched" on the mid synthetic model (DESIGN.md "Prompt prefill at admission and onto fp8 caches"): the batched
prompt prefill onto self_kv="fp8" caches against the replay, and at slot admission — the live neighbour untouched, the admitted
request bitwise that of a fresh session, the same last step with first_step - 1 fewer steps issued, stale caches, an fp8 slot
session, frame streaming — and the default routing as it was.  Prompts of 40 frames (crosses a 32-key granule) and of 1 frame."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from dia_hip import config as CF
from dia_hip import tokens as TK
from dia_hip.engine import DecodeSession, Request

S_CAP = 64
FRAMES = 40


def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def mid():
    from dia_hip.engine import DeviceWeights
    from dia_hip.weights import synthetic_state_dict
    cfg = CF.mid_config()
    assert cfg.data.audio_length % 32 == 0
    return cfg, DeviceWeights(cfg, synthetic_state_dict(cfg, seed=1234, std=0.02), dev())


def ids_of(n, seed):
    return np.random.RandomState(seed).randint(32, 127, size=(n,)).astype(np.int32)


def prompt_of(cfg, frames, seed):
    return np.random.RandomState(seed).randint(0, 1024, size=(frames, cfg.data.channels)).astype(np.int32)


def same_result(a, b):
    return (a.last_step == b.last_step and np.array_equal(a.tokens, b.tokens) and np.array_equal(a.preds, b.preds)
            and np.array_equal(a.codes, b.codes))


def self_caches(s, b, n):
    """the fp8 self caches of utterance b (both CFG rows), keys [0, n), on the host: k8, v8 in key order, ks, vs"""
    from dia_hip import layout as lay
    rows = slice(2 * b, 2 * b + 2)
    return [s.f8_self.k8[:, rows, :, :n].cpu(), lay.v_from_blocked(s.f8_self.v8[:, rows]).cpu()[:, :, :, :n],
            s.f8_self.ks[:, rows, :, :n].cpu(), s.f8_self.vs[:, rows, :, :n].cpu()]


def test_closed_fp8_session_batched_against_replay(mid):
    """the batched prefill onto fp8 caches sits inside the format's own noise: its first sampled logits differ from the replay's by no
    more than the same replay's differ from a self_kv="bf16" replay session (margin 1x; both references are existing code)"""
    cfg, w = mid
    ids = [ids_of(33, 8), ids_of(20, 9)]
    prompts = [prompt_of(cfg, FRAMES, 2), prompt_of(cfg, 1, 3)]
    kw = dict(kv_dtype="bf16", max_tokens=72, temperature=0.0, ignore_eos=True, audio_prompts=prompts)
    out = {}
    for name, extra in (("replay", dict(self_kv="fp8", prompt_prefill="auto")), ("batched", dict(self_kv="fp8", prompt_prefill="batched")),
                        ("bf16", dict(self_kv="bf16", prompt_prefill="replay"))):
        s = DecodeSession(w, ids, **kw, **extra)
        try:
            fs = s.first_steps[0]
            assert fs == FRAMES + 1 and s.first_steps[1] == 2
            assert s._prompt_prefill_batched() == (name == "batched")
            s.prefill()
            s.sync()
            cur = s.cur.cpu().tolist()
            assert cur == ([fs, 1] if name == "batched" else [1, 1]), (name, cur)      # the one-frame prompt stays on the replay path
            s.decode(1 if name == "batched" else fs)                                    # the step at cur = first_step: the first sampled logits
            lg = s.logits_host()[0].copy()
            caches = self_caches(s, 0, FRAMES) if name != "bf16" else None
            s.decode(20)
            toks = s.results()[0].tokens[fs + 1: fs + 21].copy()
            out[name] = (lg, caches, toks)
        finally:
            s.close()
    assert np.isfinite(out["batched"][0]).all() and np.abs(out["batched"][0]).max() > 0
    for what, a, b in zip(("k8", "v8", "ks", "vs"), out["batched"][1], out["replay"][1]):
        print(f"prompt slots of the fp8 caches, {what}: {float((a == b).float().mean()):.5f} of the prefill's values equal the replay's")
    d_prefill = float(np.abs(out["batched"][0] - out["replay"][0]).max())
    d_format = float(np.abs(out["replay"][0] - out["bf16"][0]).max())
    same = float((out["batched"][2] == out["replay"][2]).mean())
    print(f"first sampled logits: batched prefill vs replay (both fp8) {d_prefill:.3e}; fp8 replay vs bf16 replay {d_format:.3e}")
    print(f"greedy tokens of the next 20 steps equal to the replay's: {same:.3f}")
    assert (out["batched"][2] >= 0).all()
    assert d_prefill <= d_format, (d_prefill, d_format)


def slot_b(cfg, mt=FRAMES + 21):
    return Request(ids_of(28, 12), seed=7, max_tokens=mt, temperature=0.9, top_k=100, audio_prompt=prompt_of(cfg, FRAMES, 5))


def test_admission_prefill_in_a_bf16_slot_session(mid):
    """slot A live (greedy, 40 steps); request B (sampled, 40-frame prompt) admitted after A's 16th step"""
    cfg, w = mid
    A = Request(ids_of(30, 11), seed=None, max_tokens=41, temperature=0.0)
    B = slot_b(cfg)
    fs = FRAMES + 1
    mk = lambda mode: DecodeSession.open(w, 2, s_cap=S_CAP, kv_dtype="bf16", max_tokens=64, ignore_eos=True, prompt_prefill=mode)
    # A without B
    s = mk("batched")
    try:
        assert s.admit([A]) == [0]
        s.decode(16)
        s.decode(24)
        a_alone = (s.logits_host()[0].copy(), s.collect(0))
    finally:
        s.close()
    # A with B, prefilled at admission (batched) or replayed (auto)
    got = {}
    for mode in ("batched", "auto"):
        s = mk(mode)
        try:
            assert s.admit([A]) == [0]
            s.decode(16)
            assert s.admit([B]) == [1]
            s.sync()
            cur = s.cur.cpu().tolist()
            assert cur == [17, fs if mode == "batched" else 1], (mode, cur)            # (a) right behind admit()
            n = s._steps_left(1)
            first = 1 if mode == "batched" else fs
            s.decode(first)                                                             # B's step at cur = first_step
            lg_b = s.logits_host()[1].copy()
            s.decode(n - first - 1)
            assert 1 not in s.finished()
            s.decode(1)
            assert 1 in s.finished()
            if n < 24:
                s.decode(24 - n)                                                        # A's 40th step
            lg_a = s.logits_host()[0].copy() if n <= 24 else None
            got[mode] = dict(n=n, lg_b=lg_b, lg_a=lg_a, A=s.collect(0), B=s.collect(1))
        finally:
            s.close()
    # (b) A's tokens, raw samples and last-step logits are those of the run without B
    ra = got["batched"]["A"]
    assert same_result(ra, a_alone[1]) and (ra.tokens[1: ra.last_step + 1] >= 0).all() and ra.last_step >= 39
    assert np.array_equal(got["batched"]["lg_a"], a_alone[0])
    # (c) B == B admitted alone into a fresh session of the same slot count
    s = mk("batched")
    try:
        assert s.admit([B]) == [0]
        s.decode(s._steps_left(0))
        assert s.finished() == [0]
        b_alone = s.collect(0)
    finally:
        s.close()
    rb = got["batched"]["B"]
    assert same_result(rb, b_alone) and (rb.tokens[fs: rb.last_step + 1] >= 0).all() and len(rb.codes) == rb.last_step + 1 - fs >= 19
    # (d) the same last step as the replay-admitted B, with first_step - 1 fewer steps issued
    assert rb.last_step == got["auto"]["B"].last_step
    assert got["auto"]["n"] - got["batched"]["n"] == fs - 1 and got["batched"]["n"] == B.max_tokens - fs
    # (e) B's first sampled logits, prefilled against replayed, within twice the closed-session figure of the same request
    closed = {}
    for mode in ("auto", "replay"):
        c = DecodeSession(w, [B.text_ids], kv_dtype="bf16", max_tokens=64, ignore_eos=True, audio_prompts=[B.audio_prompt], seeds=[7],
                          temperature=0.9, top_k=100, prompt_prefill=mode)
        try:
            assert c._prompt_prefill_batched() == (mode == "auto")
            c.prefill()
            c.decode(1 if mode == "auto" else fs)
            closed[mode] = c.logits_host()[0].copy()
        finally:
            c.close()
    d_closed = float(np.abs(closed["auto"] - closed["replay"]).max())
    d_slot = float(np.abs(got["batched"]["lg_b"] - got["auto"]["lg_b"]).max())
    print(f"B's first sampled logits, prefilled vs replayed: slot session {d_slot:.3e}; closed session (existing code) {d_closed:.3e}")
    assert d_slot <= 2.0 * d_closed, (d_slot, d_closed)


@pytest.mark.parametrize("self_kv", ["bf16", "fp8"])
def test_slot_reuse_over_stale_caches(mid, self_kv):
    """a 40-step utterance, then a prompted request prefilled into the same slot: bitwise the result of a fresh session"""
    cfg, w = mid
    U = Request(ids_of(40, 21), seed=3, max_tokens=41)
    Q = slot_b(cfg)
    res = []
    for reuse in (True, False):
        s = DecodeSession.open(w, 2, s_cap=S_CAP, kv_dtype="bf16", max_tokens=64, ignore_eos=True, self_kv=self_kv, prompt_prefill="batched")
        try:
            if reuse:
                assert s.admit([U]) == [0]
                s.decode(40)
                assert s.finished() == [0] and s.collect(0).last_step >= 39
            assert s.admit([Q]) == [0]
            s.sync()
            assert int(s.cur[0].item()) == FRAMES + 1
            s.decode(s._steps_left(0))
            assert s.finished() == [0]
            res.append(s.collect(0))
        finally:
            s.close()
    assert same_result(res[0], res[1]) and res[0].last_step >= Q.max_tokens - 2
    assert (res[0].tokens[FRAMES + 1: res[0].last_step + 1] >= 0).all()


def test_fp8_slot_session_serves_prompted_and_unprompted_requests(mid):
    """three requests through two slots of a self_kv="fp8" session with the prefill at admission: each result is that of the same
    request served alone in a session of the same shape"""
    cfg, w = mid
    reqs = [Request(ids_of(28, 31), seed=1, max_tokens=FRAMES + 17, audio_prompt=prompt_of(cfg, FRAMES, 6)),
            Request(ids_of(35, 32), seed=2, max_tokens=30, temperature=0.9),
            Request(ids_of(22, 33), seed=3, max_tokens=FRAMES + 13, top_k=50, audio_prompt=prompt_of(cfg, FRAMES, 7))]
    mk = lambda: DecodeSession.open(w, 2, s_cap=S_CAP, kv_dtype="bf16", max_tokens=64, ignore_eos=True, self_kv="fp8", prompt_prefill="batched")
    s = mk()
    try:
        together = s.serve(reqs, poll=8)
        issued = s._issued
    finally:
        s.close()
    for i, r in enumerate(reqs):
        s = mk()
        try:
            alone = s.serve([r], poll=8)[0]
        finally:
            s.close()
        assert same_result(together[i], alone), i
        assert alone.last_step >= r.max_tokens - 2 and (alone.tokens[1: alone.last_step + 1] >= 0).all(), i
    assert issued < sum(r.max_tokens - 1 for r in reqs) - 2 * FRAMES + 30          # (the prompts cost no decode steps)


def test_frame_streaming_from_a_prefilled_slot(mid):
    cfg, w = mid
    Q = slot_b(cfg, mt=FRAMES + 41)
    kw = dict(s_cap=S_CAP, kv_dtype="bf16", max_tokens=96, ignore_eos=True, prompt_prefill="batched")
    s = DecodeSession.open(w, 2, **kw)
    try:
        want = TK.codes_for_codec(s.serve([Q], poll=8)[0].codes, cfg)
    finally:
        s.close()
    s = DecodeSession.open(w, 2, stream_cap=16, **kw)
    try:
        chunks = list(s.stream_iter([Q], chunk=5))
        steps = s._issued
    finally:
        s.close()
    assert 0 < want.shape[-1] <= 40
    assert [c[3] for c in chunks].count(True) == 1 and chunks[-1][3] and all(c[0] == 0 for c in chunks)
    filled = [c for c in chunks if c[2].shape[-1]]
    assert filled[0][1] == 0                                                   # the first chunk starts at the first sampled frame
    pos = 0
    for _, start, codes, _ in filled:
        assert start == pos
        pos += codes.shape[-1]
    assert np.array_equal(np.concatenate([c[2] for c in filled], axis=-1), want)
    assert steps == 40                                                         # rows first_step .. max_tokens - 1, none for the prompt


def test_defaults_untouched(mid):
    """a slot session and an fp8 closed session opened without the keyword route prompts as before: no batched prefill, cur == 1"""
    cfg, w = mid
    s = DecodeSession.open(w, 2, s_cap=S_CAP, kv_dtype="bf16", max_tokens=64, ignore_eos=True)
    try:
        assert s.prompt_prefill == "auto"
        assert s.admit([slot_b(cfg)]) == [0]
        s.sync()
        assert s._prompt_prefill_batched() is False and s.cur.cpu().tolist() == [1, 1]
        assert s._steps_left(0) == FRAMES + 20 and s._live[0]["t0"] == 0
    finally:
        s.close()
    c = DecodeSession(w, [ids_of(33, 8)], kv_dtype="bf16", max_tokens=64, temperature=0.0, self_kv="fp8", audio_prompts=[prompt_of(cfg, FRAMES, 2)])
    try:
        assert c.prompt_prefill == "auto" and c._prompt_prefill_batched() is False
        c.prefill()
        c.sync()
        assert c.cur.cpu().tolist() == [1]
    finally:
        c.close()
