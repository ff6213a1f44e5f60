"""Continuous batching on the device: requests admitted into free slots of a running session produce the token buffers of
their own oracle runs, bit for bit (fp32 K/V) — whatever slot they got, whenever they were admitted and whatever ran there
before.  The yardstick is the one of test_gpu_parity.test_batched_equals_single / test_large_batches_vs_oracle."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from dia_hip import binding as hb
from dia_hip import config as C
from dia_hip.engine import DecodeSession, DeviceWeights, Request
from dia_hip.tokens import effective_text, encode_text
from dia_hip.weights import synthetic_state_dict
from oracle import dia_oracle as O

TEXTS = [
    "[S1] Dia is an open weights text to dialogue model. [S2] You get full control over scripts and voices.",
    "[S1] Hello there. [S2] Hi!",
    "[S1] The quick brown fox jumps over the lazy dog, twice. [S2] Really? [S1] Yes.",
]
S_CAP = 128


@pytest.fixture(scope="module")
def mid():
    cfg = C.mid_config()
    sd = synthetic_state_dict(cfg, seed=1234, std=0.02)
    w = DeviceWeights(cfg, sd, torch.device("cuda:0"))
    return cfg, sd, w


@pytest.fixture(scope="module")
def full():
    cfg = C.dia_1_6b_config()
    dev = torch.device("cuda:0")
    sd_gpu = synthetic_state_dict(cfg, seed=1234, std=0.02, device=dev)
    w = DeviceWeights(cfg, sd_gpu, dev)
    sd = {k: v.cpu() for k, v in sd_gpu.items()}
    return cfg, sd, w


def cpu_threads():
    try:
        n = len(os.sched_getaffinity(0))
    except Exception:
        n = os.cpu_count() or 1
    return max(1, min(16, n))


def text_of_bytes(n, cfg):
    """a text that encodes to exactly n byte tokens"""
    t = "[S1] " + "abcdefghij " * (n // 8)
    while len(encode_text(effective_text(t), cfg)) > n:
        t = t[:-1]
    assert len(encode_text(effective_text(t), cfg)) == n
    return t


def spec(text, seed, mt, **kw):
    """one request: text, seed, max_tokens + sampling overrides (cfg_scale, temperature, top_p, top_k, audio_prompt)"""
    return dict(text=text, seed=seed, mt=mt, **kw)


_oracle_cache = {}


def oracle_of(cfg, sd, sp, **kw):
    """the solo run of a request: oracle.generate with its seed and parameters"""
    key = (id(sd), sp["text"], sp["seed"], sp["mt"], sp.get("cfg_scale", 3.0), sp.get("temperature", 1.3), sp.get("top_p", 0.95),
           sp.get("top_k", 35), None if sp.get("audio_prompt") is None else sp["audio_prompt"].tobytes(), tuple(sorted(kw.items())))
    if key not in _oracle_cache:
        dm = O.Dims.of(cfg)
        nz = O.exp_noise(sp["seed"], sp["mt"] - 1, dm.C, dm.tgt_vocab)
        torch.set_num_threads(cpu_threads())
        _oracle_cache[key] = O.generate(sd, cfg, sp["text"], max_tokens=sp["mt"], noise=nz, mirror=False, keep_logits=False,
                                        cfg_scale=sp.get("cfg_scale", 3.0), temperature=sp.get("temperature", 1.3),
                                        top_p=sp.get("top_p", 0.95), cfg_filter_top_k=sp.get("top_k", 35),
                                        audio_prompt=sp.get("audio_prompt"), **kw)
    return _oracle_cache[key]


def request_of(cfg, sp):
    return Request(encode_text(effective_text(sp["text"]), cfg), seed=sp["seed"], max_tokens=sp["mt"],
                   cfg_scale=sp.get("cfg_scale", 3.0), temperature=sp.get("temperature", 1.3), top_p=sp.get("top_p", 0.95),
                   top_k=sp.get("top_k", 35), audio_prompt=sp.get("audio_prompt"))


def assert_equals_oracle(res, r, mt, what):
    # the oracle stops writing at its max_tokens; rows behind it are -1 in both buffers
    assert np.array_equal(res.tokens, r.tokens), what
    assert res.last_step == r.last_step, what
    assert np.array_equal(res.codes, r.codes), what


def eight_requests(cfg):
    return [spec(TEXTS[0], 42, 40), spec(TEXTS[1], 7, 12), spec(TEXTS[2], 123, 27), spec("", 11, 19),
            spec(text_of_bytes(S_CAP, cfg), 12, 33), spec(TEXTS[1], 8, 40), spec(TEXTS[0], 9, 15), spec(TEXTS[2], 10, 22)]


def test_served_equals_solo(mid):
    """3 slots, 8 requests of 12..40 steps (slots free up at different polls), an empty text and one of s_cap bytes, graph replay:
    every request == its own oracle run, in the given order and reversed."""
    cfg, sd, w = mid
    specs = eight_requests(cfg)
    assert len(encode_text(effective_text(specs[3]["text"]), cfg)) == 0
    runs = [oracle_of(cfg, sd, sp) for sp in specs]
    s = DecodeSession.open(w, 3, s_cap=S_CAP, kv_dtype="f32", max_tokens=40)
    try:
        out = s.serve([request_of(cfg, sp) for sp in specs], poll=8, use_graph=True)
        for i, (res, r) in enumerate(zip(out, runs)):
            assert_equals_oracle(res, r, specs[i]["mt"], ("forward", i))
        assert s.free_slots() == [0, 1, 2]
        out = s.serve([request_of(cfg, sp) for sp in reversed(specs)], poll=8, use_graph=True)
        for i, (res, r) in enumerate(zip(out, reversed(runs))):
            assert_equals_oracle(res, r, None, ("reversed", i))
    finally:
        s.close()
    with pytest.raises(ValueError):
        s2 = DecodeSession.open(w, 1, s_cap=64, kv_dtype="f32", max_tokens=16)
        try:
            s2.serve([request_of(cfg, spec(TEXTS[0], 1, 12))])           # 100+ bytes into a 64-byte session
        finally:
            s2.close()


def test_per_request_sampling_parameters(mid):
    """greedy next to sampled slots, top-k 35 / 100 (the > 64 route) / 0, top-p on and off, different guidance scales: each request
    == its oracle run with the same parameters."""
    cfg, sd, w = mid
    specs = [spec(TEXTS[0], 42, 30, temperature=0.0), spec(TEXTS[1], 7, 24, temperature=1.0, top_p=1.0, top_k=0),
             spec(TEXTS[2], 5, 36, temperature=0.8, top_p=0.5, top_k=100, cfg_scale=2.0), spec(TEXTS[0], 9, 20, cfg_scale=4.0),
             spec(TEXTS[2], 3, 28, temperature=1.3, top_p=0.9, top_k=100), spec(TEXTS[1], 4, 18, temperature=0.0, cfg_scale=1.5),
             spec(TEXTS[0], 6, 26, temperature=0.7, top_p=0.95, top_k=1)]
    runs = [oracle_of(cfg, sd, sp) for sp in specs]
    s = DecodeSession.open(w, 3, s_cap=S_CAP, kv_dtype="f32", max_tokens=40)
    try:
        out = s.serve([request_of(cfg, sp) for sp in specs], poll=8)
    finally:
        s.close()
    for i, (res, r) in enumerate(zip(out, runs)):
        assert_equals_oracle(res, r, specs[i]["mt"], i)


def test_slot_arrays_with_session_scalars_equal_the_scalar_session(mid):
    """the per-slot instantiation of the sampler with every slot at the session's values == the closed batch's, bitwise"""
    cfg, sd, w = mid
    mt, seeds = 30, [42, 7]
    ids = [encode_text(effective_text(t), cfg) for t in TEXTS[:2]]
    a = DecodeSession(w, ids, kv_dtype="f32", max_tokens=mt, seeds=seeds, cfg_scale=2.5, temperature=1.1, top_p=0.9, top_k=50,
                      s_cap=S_CAP)
    a.prefill()
    a.decode(mt - 1)
    want_logits, want = a.logits_host().copy(), a.results()
    a.close()
    b = DecodeSession.open(w, 2, s_cap=S_CAP, kv_dtype="f32", max_tokens=mt)
    try:
        b.admit([Request(i, seed=sd_, max_tokens=mt, cfg_scale=2.5, temperature=1.1, top_p=0.9, top_k=50) for i, sd_ in zip(ids, seeds)])
        b.decode(mt - 1)
        got_logits = b.logits_host().copy()
        got = [b.collect(0), b.collect(1)]
    finally:
        b.close()
    assert np.array_equal(got_logits, want_logits)
    for g, w_ in zip(got, want):
        assert np.array_equal(g.tokens, w_.tokens) and np.array_equal(g.preds, w_.preds) and g.last_step == w_.last_step


@pytest.mark.parametrize("kv", ["f32", "bf16", "bf16x2"])
def test_slot_reuse_over_stale_caches(mid, kv):
    """One slot: a 40-step utterance with the longest text, then a 12-step one with the shortest — and once more with an audio
    prompt on the short one (replay path).  The second result == the same request in a FRESH session of the same K/V format,
    bitwise: what the first utterance left in the self and cross caches is weighted by exactly 0."""
    cfg, sd, w = mid
    long_ = spec(text_of_bytes(S_CAP, cfg), 42, 41)
    prompt = np.random.RandomState(5).randint(0, 1024, size=(7, cfg.data.channels)).astype(np.int32)
    shorts = [spec(TEXTS[1], 7, 13), spec(TEXTS[1], 8, 22, audio_prompt=prompt)]

    def serve(specs):
        s = DecodeSession.open(w, 1, s_cap=S_CAP, kv_dtype=kv, max_tokens=41)
        try:
            return s.serve([request_of(cfg, sp) for sp in specs], poll=8)
        finally:
            s.close()

    out = serve([long_, shorts[0], long_, shorts[1]])
    for sp, got in zip(shorts, (out[1], out[3])):
        fresh = serve([sp])[0]
        assert np.array_equal(got.tokens, fresh.tokens) and np.array_equal(got.preds, fresh.preds)
        assert got.last_step == fresh.last_step and np.array_equal(got.codes, fresh.codes)
        if kv == "f32":
            assert_equals_oracle(got, oracle_of(cfg, sd, sp), sp["mt"], sp["seed"])


def test_admission_does_not_disturb_a_live_slot(mid):
    """Two slots: A runs 40 steps alone; in a second session B is admitted into the other slot after A's 16th step.  A's token
    buffer, raw samples and the logits of its last step are identical — an admission that rewrote x, ssq or noise rows of a
    live slot would show here."""
    cfg, sd, w = mid
    A = Request(encode_text(effective_text(TEXTS[0]), cfg), seed=42, max_tokens=60)
    B = Request(encode_text(effective_text(TEXTS[2]), cfg), seed=7, max_tokens=60, temperature=0.9, top_k=100)
    got = []
    for with_b in (False, True):
        s = DecodeSession.open(w, 2, s_cap=S_CAP, kv_dtype="f32", max_tokens=60, ignore_eos=True)
        try:
            assert s.admit([A]) == [0]
            s.decode(16)
            if with_b:
                assert s.admit([B]) == [1]
            s.decode(24)
            lg = s.logits_host()[0].copy()
            cur = s.cur.cpu().numpy().copy()
            got.append((s.collect(0), lg, cur))
        finally:
            s.close()
    assert got[0][2][0] == got[1][2][0] == 41 and got[1][2][1] == 25 and got[0][2][1] == 1
    assert np.array_equal(got[0][0].tokens, got[1][0].tokens) and np.array_equal(got[0][0].preds, got[1][0].preds)
    assert np.array_equal(got[0][1], got[1][1])
    assert (got[0][0].tokens[1:41] >= 0).all()


def test_parked_slots_are_cheap_and_harmless(mid):
    """8 slots, one live utterance == its oracle run; after retire the slot's device state is cur 1, text_len 0, done"""
    cfg, sd, w = mid
    sp = spec(TEXTS[0], 42, 40)
    r = oracle_of(cfg, sd, sp)
    s = DecodeSession.open(w, 8, s_cap=S_CAP, kv_dtype="f32", max_tokens=40)
    try:
        s.admit([request_of(cfg, spec(TEXTS[1], 1, 8))] * 5)             # slots 0..4 busy: the utterance lands in slot 5
        assert s.admit([request_of(cfg, sp)]) == [5]
        while 5 not in s.finished():
            s.decode(8)
        s.sync()
        assert int(s.cur[5].item()) > 1 and int(s.text_len[5].item()) == len(request_of(cfg, sp).text_ids)
        res = s.collect(5)
        for b in range(5):
            s.collect(b)
        s.retire(range(6))
        s.sync()
        assert s.cur.cpu().tolist() == [1] * 8 and s.text_len.cpu().tolist() == [0] * 8 and s.fsm[:, 3].cpu().tolist() == [1] * 8
        s.decode(3)                                                      # a step over parked slots only: nothing moves
        s.sync()
        assert s.cur.cpu().tolist() == [1] * 8 and bool(torch.isfinite(s.logits).all())
        # and a session that only ever held this one utterance
        assert s.admit([request_of(cfg, sp)]) == [0]
        while not s.finished():
            s.decode(8)
        again = s.collect(0)
    finally:
        s.close()
    assert_equals_oracle(res, r, 40, "slot 5")
    assert_equals_oracle(again, r, 40, "slot 0 after retire")


def test_ten_slots_24_requests_vs_oracle(mid):
    """20 rows (two m-tiles: the k_gemm2t / z-form range): 24 requests dealt from three oracle runs, each == its run"""
    cfg, sd, w = mid
    base = [spec(t, sd_, mt) for t, sd_, mt in zip(TEXTS, (42, 7, 123), (24, 17, 21))]
    runs = [oracle_of(cfg, sd, sp) for sp in base]
    s = DecodeSession.open(w, 10, s_cap=S_CAP, kv_dtype="f32", max_tokens=24)
    try:
        out = s.serve([request_of(cfg, base[i % 3]) for i in range(24)], poll=8)
    finally:
        s.close()
    for i, res in enumerate(out):
        assert_equals_oracle(res, runs[i % 3], base[i % 3]["mt"], i)


def test_full_size_two_slots_vs_oracle(full):
    """Dia-1.6B shapes, 2 slots, 4 requests of at most 8 steps, fp32 K/V: tokens == oracle"""
    cfg, sd, w = full
    specs = [spec(TEXTS[0], 42, 9), spec(TEXTS[1], 7, 6), spec(TEXTS[2], 123, 8), spec(TEXTS[1], 5, 7, temperature=0.0)]
    runs = [oracle_of(cfg, sd, sp) for sp in specs]
    s = DecodeSession.open(w, 2, s_cap=S_CAP, kv_dtype="f32", max_tokens=9)
    try:
        out = s.serve([request_of(cfg, sp) for sp in specs], poll=4)
    finally:
        s.close()
    for i, (res, r) in enumerate(zip(out, runs)):
        assert_equals_oracle(res, r, specs[i]["mt"], i)
