"""The one-shape forms of the decode step's two attention launches (csrc/attn.hip: the cross form behind k_attn_mfma<1, 1>, the self form
behind k_attn_mfma<4, 1>; knob attn_spec, 0 = the generic body everywhere) against the generic body of the SAME library: the same inputs
give the same bits — the output and, for self, the whole cache with the appended slot — and both stay inside the bound that
tests/test_gpu_attn_decode.py applies against its float64 reference (its TOL, its harness, its checks).  Two bodies share one
instantiation name, so the tests ask the host rule itself (dia_attn_form: pure, the function dia_attn decides with) which body a launch of
these shapes takes under the knob in force (0 generic, 1 cross, 2 self); that the two bodies are different code shows in the A/B.

The cross form serves caches of at most 256 keys of capacity: every length such a cache can hold is one chunk.  A text of 257 keys needs
a larger cache and must be served by the generic kernel, with or without a head_map; so must fp32 and two-plane caches and a compacted
checkpoint at model level."""
import ctypes as C

import numpy as np
import pytest
import torch

import test_gpu_attn_decode as AD
from dia_hip import binding as hb
from dia_hip import config as CF

pytestmark = pytest.mark.gpu

SELF, CROSS = hb.ATTN_SELF, hb.ATTN_CROSS
GENERIC, F_CROSS, F_SELF = 0, 1, 2


def form_of(mode, kvd, G, KVH, n_rows, kv_cap, head_map=False):
    """the body dia_attn launches for these shapes under the current attn_spec (csrc/attn.hip attn_form_of)"""
    a = hb.AttnArgs()
    a.mode, a.kv_dtype, a.group, a.n_kv_heads, a.n_rows, a.kv_cap = mode, AD.KVD_CODE[kvd], G, KVH, n_rows, kv_cap
    a.v_blocked = int(kvd != "f32")
    a.head_map = _DUMMY.ctypes.data if head_map else None
    L = hb.lib()
    L.dia_attn_form.argtypes, L.dia_attn_form.restype = [C.POINTER(hb.AttnArgs)], C.c_int
    return L.dia_attn_form(C.byref(a))


_DUMMY = np.zeros(16, dtype=np.int32)


def cap_for(nkeys):
    return max(32, -(-nkeys // 32) * 32)


def cross_pair(tuning, lens, kv_cap, head_map=None, seed=0):
    """the same CROSS launch (16 heads, one utterance per length) under the default and under attn_spec = 0"""
    curs = [7 + 5 * b for b in range(len(lens))]
    res = {}
    for knob in (-1, 0):
        tuning("attn_spec", knob)
        case, q, out, nslab, before = AD.run_attn(CROSS, "bf16", 1, 16, curs, kv_cap, lens=lens, head_map=head_map, seed=seed)
        nz = AD.launch_nz(len(lens), 16, kv_cap)
        worst = AD.check_cross(case, q, curs, lens, out, nslab, before, nz=nz, head_map=head_map)
        res[knob] = (out, form_of(CROSS, "bf16", 1, 16, len(lens), kv_cap, head_map is not None), worst)
    tuning("attn_spec", -1)
    return res


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("nkeys", [1, 31, 32, 33, 98, 255, 256])
def test_cross_form_equals_generic(tuning, nkeys, B):
    lens = [nkeys] if B == 1 else [nkeys, max(1, nkeys // 2)]
    res = cross_pair(tuning, lens, cap_for(nkeys), seed=nkeys)
    assert res[-1][1] == F_CROSS and res[0][1] == GENERIC, (res[-1][1], res[0][1])
    assert torch.equal(res[-1][0], res[0][0]), "the cross form's output differs from the generic body's"
    print(f"cross {nkeys} keys x {B}: max-abs err form {res[-1][2]:.2e} generic {res[0][2]:.2e}")
    assert res[-1][2] <= AD.TOL and res[0][2] <= AD.TOL


@pytest.mark.parametrize("with_map", [False, True])
def test_cross_257_keys_are_the_generic_kernels(tuning, with_map):
    hm = None
    if with_map:                                   # heads 3 and 9 pruned, the rest compacted
        hm, n = [], 0
        for h in range(16):
            hm.append(-1 if h in (3, 9) else n)
            n += h not in (3, 9)
    res = cross_pair(tuning, [257, 98], cap_for(257), head_map=hm, seed=3)
    assert res[-1][1] == GENERIC and res[0][1] == GENERIC
    assert torch.equal(res[-1][0], res[0][0])
    assert res[-1][2] <= AD.TOL


def test_cross_head_map_at_a_short_text_is_the_generic_kernels(tuning):
    hm = [h - (h > 5) if h != 5 else -1 for h in range(16)]
    res = cross_pair(tuning, [98], 128, head_map=hm, seed=4)
    assert res[-1][1] == GENERIC and torch.equal(res[-1][0], res[0][0]) and res[-1][2] <= AD.TOL


def self_pair(tuning, curs, kv_cap, seed):
    """the same SELF launch (4 kv heads x group 4) under the default and under attn_spec = 0: same caches, same q|k|v rows"""
    res = {}
    qkv = None
    for knob in (-1, 0):
        tuning("attn_spec", knob)
        case, qkv, out, nslab, before = AD.run_attn(SELF, "bf16", 4, 4, curs, kv_cap, seed=seed, q=qkv)
        nz = AD.launch_nz(2 * len(curs), 4, kv_cap)
        worst = AD.check_self(case, qkv, curs, out, nslab, before, nz=nz)
        res[knob] = (out, form_of(SELF, "bf16", 4, 4, 2 * len(curs), kv_cap), worst, case.kc.clone(), case.vc.clone())
    tuning("attn_spec", -1)
    return res


SELF_CASES = [[c] for c in (1, 2, 32, 33, 256, 257, 288, 513, 1040)] + [[c, c] for c in (1, 2, 32, 33, 256, 257, 288, 513, 1040)] + [[33, 257], [1040, 1]]


@pytest.mark.parametrize("curs", SELF_CASES, ids=lambda c: "cur_" + "_".join(map(str, c)))
def test_self_form_equals_generic(tuning, curs):
    res = self_pair(tuning, curs, cap_for(max(curs)) if max(curs) > 256 else 288, seed=sum(curs))
    assert res[-1][1] == F_SELF and res[0][1] == GENERIC, (res[-1][1], res[0][1])
    assert torch.equal(res[-1][0], res[0][0]), "the self form's output differs from the generic body's"
    assert torch.equal(res[-1][3].view(torch.int16), res[0][3].view(torch.int16)) and torch.equal(res[-1][4].view(torch.int16), res[0][4].view(torch.int16)), "caches differ"
    print(f"self cur {curs}: max-abs err form {res[-1][2]:.2e} generic {res[0][2]:.2e}")
    assert res[-1][2] <= AD.TOL and res[0][2] <= AD.TOL


@pytest.mark.parametrize("bit,want", [(1, (F_CROSS, GENERIC)), (2, (GENERIC, F_SELF))])
def test_each_bit_of_the_knob_selects_its_form_alone(tuning, bit, want):
    """and the launch under one bit alone gives the bits of the launch under attn_spec = 0"""
    outs = {}
    for knob in (bit, 0):
        tuning("attn_spec", knob)
        forms = (form_of(CROSS, "bf16", 1, 16, 1, 128), form_of(SELF, "bf16", 4, 4, 2, 288))
        assert forms == (want if knob else (GENERIC, GENERIC))
        outs[knob] = (AD.run_attn(CROSS, "bf16", 1, 16, [9], 128, lens=[98], seed=1)[2], AD.run_attn(SELF, "bf16", 4, 4, [40], 288, seed=2)[2])
    assert torch.equal(outs[bit][0], outs[0][0]) and torch.equal(outs[bit][1], outs[0][1])


# ---- model level: 2 decoder layers of Dia-1.6B widths ------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def model():
    from dia_hip.weights import synthetic_state_dict
    c = CF.dia_1_6b_config()
    m = c.model
    cfg = c.model_copy(update={
        "model": m.model_copy(update={"encoder": m.encoder.model_copy(update={"n_layer": 1}), "decoder": m.decoder.model_copy(update={"n_layer": 2})}),
        "data": c.data.model_copy(update={"text_length": 128, "audio_length": 128})})
    return cfg, synthetic_state_dict(cfg, seed=1234, std=0.02)


def session_forms(s, w, cfg, kv):
    """the bodies the session's two attention launches take per decoder layer: the rule asked with the session's own shapes"""
    d = cfg.model.decoder
    out = []
    for L in w.dec_layers:
        out.append((form_of(CROSS, kv, 1, d.cross_query_heads, s.B, s.S, L["hmap_cross"] is not None),
                    form_of(SELF, kv, d.gqa_query_heads // d.kv_heads, d.kv_heads, 2 * s.B, s.T, L["hmap_self"] is not None)))
    return out


def decode40(cfg, w, B, kv):
    from dia_hip.engine import DecodeSession
    from dia_hip.tokens import effective_text, encode_text, synthetic_text
    ids = [encode_text(effective_text(synthetic_text(98, cfg)), cfg)[:98] for _ in range(B)]
    s = DecodeSession(w, ids, kv_dtype=kv, max_tokens=48, seeds=list(range(B)), ignore_eos=True)
    s.prefill()
    forms = session_forms(s, w, cfg, kv)
    lg = []
    for _ in range(40):
        s.decode(1, use_graph=False)
        lg.append(s.logits_host().copy())
    toks = [r.tokens.copy() for r in s.results()]
    s.close()
    return lg, toks, forms


@pytest.mark.parametrize("variant", ["bf16", "f32", "compacted"])
@pytest.mark.parametrize("B", [1, 2])
def test_model_knob_on_equals_knob_off(model, tuning, B, variant):
    from dia_hip.engine import DeviceWeights
    cfg, sd = model
    if variant == "compacted":                     # pruned heads -> head_map on both attention launches
        from dia_hip.pruning import structured_prune_state_dict
        sd, _ = structured_prune_state_dict(cfg, sd, amount=0.5, dim=0, n=2)
    w = DeviceWeights(cfg, sd, AD.dev(), compact="auto")
    res = {}
    for knob in (-1, 0):
        tuning("attn_spec", knob)
        res[knob] = decode40(cfg, w, B, "f32" if variant == "f32" else "bf16")
    tuning("attn_spec", -1)
    nl = cfg.model.decoder.n_layer
    assert res[0][2] == [(GENERIC, GENERIC)] * nl
    assert res[-1][2] == ([(F_CROSS, F_SELF)] if variant == "bf16" else [(GENERIC, GENERIC)]) * nl, res[-1][2]      # f32 caches, head maps: fall through
    for a, b in zip(res[-1][0], res[0][0]):
        assert np.array_equal(a, b) and np.isfinite(a).all() and np.abs(a).max() > 0
    for a, b in zip(res[-1][1], res[0][1]):
        assert np.array_equal(a, b)
