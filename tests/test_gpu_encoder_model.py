"""The encoder pass end to end (DecodeSession._encode: dia_embed_text, the packed GEMMs, dia_enc_attn per layer, the cross-K/V
launch) against tests/enc_ref.py in float64, on the mid config widened to text_length 1024: a closed batch of ragged texts
up to the full length, slot admissions whose utterance numbers are not the packing order, and a pruned checkpoint whose
encoder layers keep different head counts.  Bound: the 1e-4 of test_encoder_and_cross_kv_mid.  Texts are random byte tokens
(1..255): the pass never looks at what they spell."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import enc_ref as R
from dia_hip import config as C
from dia_hip.engine import DecodeSession, DeviceWeights, Request
from dia_hip.weights import synthetic_state_dict

TOL = 1e-4                 # test_encoder_and_cross_kv_mid's bound on enc_out and the cross K/V
FILL = -3.25               # what the cross caches hold before the pass under test


def long_text_config():
    """mid_config() with the model's text_length"""
    cfg = C.mid_config()
    return cfg.model_copy(update={"data": cfg.data.model_copy(update={"text_length": 1024})})


def byte_ids(n, seed):
    return np.random.RandomState(seed).randint(1, 256, size=(n,)).astype(np.int32)


@pytest.fixture(scope="module")
def mid1k():
    cfg = long_text_config()
    assert cfg.data.text_length == 1024
    sd = synthetic_state_dict(cfg, seed=1234, std=0.02)
    w = DeviceWeights(cfg, sd, torch.device("cuda:0"))
    return cfg, sd, w, R.device_weights(sd)


_refs = {}


def reference(cfg, sd64, ids, key):
    """(enc_out, cross K/V of every decoder layer) in float64 for one text, computed once per text"""
    k = (key, ids.tobytes())
    if k not in _refs:
        enc = R.encoder_ref(sd64, cfg, ids)
        _refs[k] = (enc, R.cross_kv_ref(sd64, cfg, enc))
    return _refs[k]


def err_of(got, want, what):
    """max-abs error of a device tensor against its float64 reference, held to TOL where it is computed: a NaN fails here (a
    running max() over Python floats would keep its old value)"""
    got = got.cpu().double()
    assert tuple(got.shape) == tuple(want.shape), what
    assert torch.isfinite(got).all(), what
    err = (got - want).abs().max().item()
    assert err <= TOL, (what, err)
    return err


def cross_err(s, b, L, kv, heads=None):
    """max-abs error of utterance b's rows 0..L-1 of the first and the last decoder layer's cross caches; heads: per layer
    index (0, -1) the heads to compare (default: all)"""
    worst = 0.0
    for li in (0, -1):
        hs = slice(None) if heads is None else heads[li]
        k, v = kv[li]
        worst = max(worst, err_of(s.k_cross[li][b, :, :L][hs], k[hs], ("k_cross", li, b)))
        worst = max(worst, err_of(s.v_cross[li][b, :, :L][hs], v[hs], ("v_cross", li, b)))
    return worst


def fill_cross(s):
    s.sync()
    s.k_cross_all.fill_(FILL); s.v_cross_all.fill_(FILL)
    torch.cuda.synchronize()


def test_closed_batch_ragged_up_to_text_length(mid1k):
    """texts of 1024, 0, 1, 33 and 257 bytes in one prefill: enc_out and the first / last layer's cross K/V of every utterance
    against float64, and the cache rows behind every text's end exactly as they were before the pass"""
    cfg, sd, w, sd64 = mid1k
    lens = [1024, 0, 1, 33, 257]
    ids = [byte_ids(n, 100 + n) for n in lens]
    s = DecodeSession(w, ids, kv_dtype="f32", max_tokens=8, temperature=0.0)
    try:
        assert s.S == 1024
        fill_cross(s)
        s.prefill(keep_encoder_out=True); s.sync()
        worst_enc = worst_kv = 0.0
        for b, L in enumerate(lens):
            for li in (0, -1):
                assert (s.k_cross[li][b, :, L:] == FILL).all() and (s.v_cross[li][b, :, L:] == FILL).all(), (b, li)
            if L == 0:
                assert s.enc_out[b] is None
                continue
            enc, kv = reference(cfg, sd64, ids[b], "dense")
            worst_enc = max(worst_enc, err_of(s.enc_out[b], enc, ("enc_out", b)))
            worst_kv = max(worst_kv, cross_err(s, b, L, kv))
        print(f"closed batch {lens}: enc_out max-abs err vs float64 {worst_enc:.3e}, cross K/V {worst_kv:.3e}")
        assert worst_enc <= TOL and worst_kv <= TOL
    finally:
        s.close()


def test_slot_admissions_with_unordered_slot_numbers(mid1k):
    """A 4-slot session, two admissions whose (slot, request) lists are [2, 0] and then [3] — DecodeSession._admit, the layer
    under admit() that takes the slots as given (admit() itself hands out free slots in ascending order) — so the packed
    rows of _encode carry utterance numbers that are not their packing order, and seg_off / seg_len have entries of slots
    that are not in the call.  The admitted slots' cross caches against float64; the rows of every other slot bitwise
    untouched by the call.  (tests/test_gpu_slots.py checks admissions through the tokens that come out, at 128-byte
    texts; it asserts neither of these on the caches.)"""
    cfg, sd, w, sd64 = mid1k
    s = DecodeSession.open(w, 4, kv_dtype="f32", max_tokens=8)
    try:
        assert s.S == 1024 and s.B == 4
        fill_cross(s)
        rounds = [[(2, byte_ids(1024, 7)), (0, byte_ids(33, 8))], [(3, byte_ids(257, 9))]]
        worst = 0.0
        for pairs in rounds:
            before_k, before_v = s.k_cross_all.clone(), s.v_cross_all.clone()
            s._admit([(b, s._as_request(Request(t, seed=1, max_tokens=8))) for b, t in pairs])
            s.sync()
            called = [b for b, _ in pairs]
            for b in range(s.B):
                if b not in called:             # [layer, slot, head, key, dim]
                    assert torch.equal(s.k_cross_all[:, b], before_k[:, b]) and torch.equal(s.v_cross_all[:, b], before_v[:, b]), (called, b)
            for b, t in pairs:
                _, kv = reference(cfg, sd64, t, "dense")
                worst = max(worst, cross_err(s, b, len(t), kv))
                for li in (0, -1):
                    assert (s.k_cross[li][b, :, len(t):] == FILL).all() and (s.v_cross[li][b, :, len(t):] == FILL).all()
        print(f"slot admissions [2, 0] then [3]: cross K/V max-abs err vs float64 {worst:.3e}")
        assert worst <= TOL
    finally:
        s.close()


def test_pruned_encoder_layers_with_different_head_counts(mid1k):
    """a structured-pruned checkpoint (structured_prune_state_dict at 50 % along dim 0, loaded compacted, as in
    test_structured_pruned_checkpoint_is_compacted_and_matches_reference) whose first encoder layer keeps all 4 heads — its
    o_proj is the dense one — and whose second keeps 2: the second layer's attention finds the first layer's 4-head K/V planes
    in the scratch.  A 700-byte text against float64 on the pruned weights; the cross caches are compared in the heads the
    compacted decoder keeps (the others are never written or read)."""
    from dia_hip.pruning import structured_prune_state_dict
    cfg, sd, _, _ = mid1k
    psd, _ = structured_prune_state_dict(cfg, sd, amount=0.5, dim=0, n=2)
    name = "encoder.layers.0.self_attention.o_proj.weight"
    psd[name] = sd[name].clone()
    w = DeviceWeights(cfg, psd, torch.device("cuda:0"))
    assert w.enc_compacted and [EL["heads"] for EL in w.enc_layers] == [4, 2]
    sd64 = R.device_weights(psd)
    ids = byte_ids(700, 11)
    s = DecodeSession(w, [ids], kv_dtype="f32", max_tokens=8, temperature=0.0)
    try:
        s.prefill(keep_encoder_out=True); s.sync()
        enc, kv = reference(cfg, sd64, ids, "pruned")
        err_enc = err_of(s.enc_out[0], enc, "enc_out")
        d = cfg.model.decoder
        live = {}
        for li in (0, -1):
            co = psd[f"decoder.layers.{li % d.n_layer}.cross_attention.o_proj.weight"].reshape(d.cross_query_heads, -1)
            live[li] = torch.nonzero(co.abs().sum(dim=1) > 0).flatten()
            assert 0 < live[li].numel() < d.cross_query_heads
        err_kv = cross_err(s, 0, 700, kv, heads=live)
        print(f"pruned encoder (4 then 2 heads), 700 bytes: enc_out max-abs err vs float64 {err_enc:.3e}, cross K/V {err_kv:.3e}")
        assert err_enc <= TOL and err_kv <= TOL
    finally:
        s.close()
