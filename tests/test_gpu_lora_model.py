"""Per-request LoRA adapters, unmerged, through the whole decode path (DESIGN.md "Per-request adapters").  The reference value is
the oracle on merge_lora_state_dict(sd, adapter) — the merged fp32 weights, which is what the reference's PEFT arithmetic means.
Logit bound: 1e-3, the north-star bound of tests/test_gpu_parity.py; the K/V-format bounds and the scoring bound are the ones of
tests/test_gpu_parity.py and tests/test_gpu_score.py."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from dia_hip import binding as hb
from dia_hip import config as C
from dia_hip import score as S
from dia_hip.engine import DecodeSession, DeviceWeights, Request
from dia_hip.lora import AdapterBank, merge_lora_state_dict
from dia_hip.tokens import effective_text, encode_text
from dia_hip.weights import synthetic_state_dict
from oracle import dia_oracle as O

DEV = "cuda:0"
LOGIT_TOL = 1e-3            # north-star tolerance (tests/test_gpu_parity.py)
BF16_KV_TOL = 1e-2          # bf16 K/V on this model (tests/test_gpu_parity.py test_bf16_kv_mode_mid)
LP_TOL = 2e-5               # tests/test_gpu_score.py
MT = 21                     # 20 teacher-forced steps
TEXTS = [
    "[S1] Dia is an open weights text to dialogue model. [S2] You get full control over scripts and voices.",
    "[S1] Hello there. [S2] Hi!",
    "[S1] The quick brown fox jumps over the lazy dog, twice. [S2] Really? [S1] Yes.",
]


def cpu_threads():
    try:
        n = len(os.sched_getaffinity(0))
    except Exception:
        n = os.cpu_count() or 1
    return max(1, min(16, n))


def write_qv_adapter(root, name, cfg, sd, seed, r=8, alpha=16, amp=0.05):
    """a q_proj / v_proj adapter (the reference's default target set) on EVERY attention block: encoder, decoder self and cross"""
    g = torch.Generator().manual_seed(seed)
    e, d = cfg.model.encoder, cfg.model.decoder
    paths = [f"encoder.layers.{l}.self_attention.{p}_proj" for l in range(e.n_layer) for p in "qv"]
    paths += [f"decoder.layers.{l}.{blk}.{p}_proj" for l in range(d.n_layer) for blk in ("self_attention", "cross_attention") for p in "qv"]
    t = {}
    for path in paths:
        w = sd[path + ".weight"]
        n_in, n_out = w.shape[0], w.numel() // w.shape[0]
        t[f"base_model.model.{path}.lora_A.weight"] = amp * torch.randn(r, n_in, generator=g)
        t[f"base_model.model.{path}.lora_B.weight"] = amp * torch.randn(n_out, r, generator=g)
    dd = os.path.join(root, name)
    os.makedirs(dd, exist_ok=True)
    json.dump(dict(r=r, lora_alpha=alpha, target_modules=["q_proj", "v_proj"]), open(os.path.join(dd, "adapter_config.json"), "w"))
    torch.save(t, os.path.join(dd, "adapter_model.bin"))
    return dd


class Env:
    pass


@pytest.fixture(scope="module")
def mid(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("adapters"))
    m = Env()
    m.cfg = C.mid_config()
    m.sd = synthetic_state_dict(m.cfg, seed=1234, std=0.02)
    m.w = DeviceWeights(m.cfg, m.sd, torch.device(DEV))
    m.dirs = dict(A=write_qv_adapter(root, "A", m.cfg, m.sd, 1), B=write_qv_adapter(root, "B", m.cfg, m.sd, 2))
    m.bank = AdapterBank(m.cfg, DEV)
    for k, v in m.dirs.items():
        m.bank.add(k, v)
    m.merged = {None: m.sd, "A": merge_lora_state_dict(m.sd, m.dirs["A"]), "B": merge_lora_state_dict(m.sd, m.dirs["B"])}
    m.dm = O.Dims.of(m.cfg)
    m.oracle = {}
    return m


def oracle_run(m, ti, adapter, seed=42, mt=MT):
    """the oracle's free run of TEXTS[ti] on the weights merged with `adapter` (computed once, shared)"""
    key = (ti, adapter, seed, mt)
    if key not in m.oracle:
        torch.set_num_threads(cpu_threads())
        nz = O.exp_noise(seed, mt - 1, m.dm.C, m.dm.tgt_vocab)
        m.oracle[key] = (O.generate(m.merged[adapter], m.cfg, TEXTS[ti], max_tokens=mt, noise=nz, mirror=False), nz)
    return m.oracle[key]


def teacher_forced(m, w, tis, adapters, runs, kv="f32", bank="auto", graph=False, mt=MT):
    """per-step logits [steps][B, 2, C, V] and results of a closed batch forced along the oracle runs' tokens"""
    ids = [encode_text(effective_text(TEXTS[t]), m.cfg) for t in tis]
    bank = (m.bank if any(a is not None for a in adapters) else None) if bank == "auto" else bank
    s = DecodeSession(w, ids, kv_dtype=kv, max_tokens=mt, noise=torch.stack([nz for _, nz in runs]), teacher_tokens=[r.tokens for r, _ in runs],
                      adapters=bank, adapter_ids=adapters if bank is not None else None)
    try:
        s.prefill()
        logits = []
        for _ in range(mt - 1):
            s.decode(1, use_graph=graph)
            logits.append(s.logits_host())
        return logits, s.results()
    finally:
        s.close()


def worst_err(logits, b, r):
    return max(float(np.abs(logits[i][b] - r.logits[i]).max()) for i in range(len(r.logits)))


@pytest.mark.parametrize("tis,adapters", [([0], ["A"]), ([0, 1, 2], ["A", None, "B"])], ids=["batch1", "batch3"])
def test_parity_with_the_oracle_on_merged_weights(mid, tis, adapters):
    """fp32 K/V, teacher-forced for 20 steps: logits within 1e-3 of the oracle on the MERGED weights, every sample identical —
    and the same run without the adapter misses that oracle by more than 1e-2, as the oracle's own base run does"""
    runs = [oracle_run(mid, t, a) for t, a in zip(tis, adapters)]
    logits, res = teacher_forced(mid, mid.w, tis, adapters, runs)
    for b, (r, _) in enumerate(runs):
        err = worst_err(logits, b, r)
        print(f"adapter {adapters[b]}: logits max-abs err vs the oracle on merged weights {err:.3e}")
        assert err <= LOGIT_TOL, (b, err)
        for i, p in enumerate(r.preds):
            assert np.array_equal(res[b].preds[1 + i], p), (b, i)
    # the adapter matters: CPU, the oracle alone — base and merged logits along the same forced tokens
    r, nz = runs[0]
    torch.set_num_threads(cpu_threads())
    base = O.generate(mid.sd, mid.cfg, TEXTS[tis[0]], max_tokens=MT, noise=nz, mirror=False, forced_tokens=r.tokens)
    moved = max(float(np.abs(a_ - b_).max()) for a_, b_ in zip(base.logits, r.logits))
    assert moved > 1e-2, moved
    # ... and so does the device path without it
    logits0, _ = teacher_forced(mid, mid.w, tis[:1], [None], runs[:1])
    miss = worst_err(logits0, 0, r)
    print(f"oracle base vs merged {moved:.3e}; device without the adapter vs merged oracle {miss:.3e}")
    assert miss > 1e-2, miss


def test_graph_replay_equals_eager(mid):
    runs = [oracle_run(mid, 0, "A"), oracle_run(mid, 1, "B")]
    le, re_ = teacher_forced(mid, mid.w, [0, 1], ["A", "B"], runs, graph=False)
    lg, rg = teacher_forced(mid, mid.w, [0, 1], ["A", "B"], runs, graph=True)
    for b in range(2):
        assert np.array_equal(re_[b].preds, rg[b].preds) and np.array_equal(re_[b].tokens, rg[b].tokens)
    assert all(np.array_equal(a_, b_) for a_, b_ in zip(le, lg))


@pytest.mark.parametrize("kv,tol", [("bf16x2", LOGIT_TOL), ("bf16", BF16_KV_TOL)])
def test_cache_formats(mid, kv, tol):
    """the same adapter session with two-plane and plain bf16 K/V (blocked V, the cross-cache read-modify-write in that format):
    logits within the format's bound of the fp32-K/V run of the same session"""
    runs = [oracle_run(mid, 0, "A"), oracle_run(mid, 2, None), oracle_run(mid, 1, "B")]
    ref, _ = teacher_forced(mid, mid.w, [0, 2, 1], ["A", None, "B"], runs)
    got, _ = teacher_forced(mid, mid.w, [0, 2, 1], ["A", None, "B"], runs, kv=kv)
    worst = max(float(np.abs(a_ - b_).max()) for a_, b_ in zip(ref, got))
    print(f"{kv} K/V vs fp32 K/V under adapters: logits max-abs diff {worst:.3e}")
    assert worst <= tol, worst


def request(m, ti, seed, mt, adapter):
    return Request(encode_text(effective_text(TEXTS[ti]), m.cfg), seed=seed, max_tokens=mt, adapter=adapter)


def test_slots(mid):
    """3 slots, requests with adapters [A, None, B, A, None]: the fourth is admitted into the slot the first one (A, short) frees,
    the fifth (base) into that slot again behind the fourth (A, short).  Every request's tokens are those of the same request alone
    in a one-slot session with the same bank; a base request's tokens are those of a session opened WITHOUT a bank, bit for bit —
    also in a slot that held adapter A before (a stale adapter_of_slot or a cross-cache correction added twice would show here)."""
    specs = [(0, 42, 8, "A"), (1, 7, 30, None), (2, 123, 30, "B"), (1, 9, 8, "A"), (0, 11, 20, None)]
    s = DecodeSession.open(mid.w, 3, s_cap=128, kv_dtype="f32", max_tokens=30, adapters=mid.bank)
    try:
        out = s.serve([request(mid, *sp) for sp in specs], poll=4, use_graph=True)
        assert s._adapter_host.tolist() == [-1, -1, -1] and s.adapter_of_slot.cpu().tolist() == [-1, -1, -1]
    finally:
        s.close()
    for i, sp in enumerate(specs):
        solo = DecodeSession.open(mid.w, 1, s_cap=128, kv_dtype="f32", max_tokens=30, adapters=mid.bank if sp[3] is not None else None)
        try:
            want = solo.serve([request(mid, *sp)], poll=4, use_graph=True)[0]
        finally:
            solo.close()
        assert np.array_equal(out[i].tokens, want.tokens) and out[i].last_step == want.last_step, i
        assert np.array_equal(out[i].codes, want.codes), i
    # the adapters change what is generated (else the comparisons above would show nothing)
    base = DecodeSession.open(mid.w, 1, s_cap=128, kv_dtype="f32", max_tokens=30)
    try:
        plain = base.serve([request(mid, 2, 123, 30, None)], poll=4)[0]
        with pytest.raises(ValueError):
            base.serve([request(mid, 2, 123, 30, "B")])
    finally:
        base.close()
    assert not np.array_equal(plain.tokens, out[2].tokens)


def test_mxfp8_base_with_adapter(mid):
    """an MXFP8-quantised base streams its e4m3 form underneath; the adapter stays fp32 beside it: within 1e-3 of the oracle on
    (quantised base, merged)"""
    from dia_hip.quant import mxfp8_quantize_state_dict
    sd8 = mxfp8_quantize_state_dict(mid.cfg, mid.sd)
    w8 = DeviceWeights(mid.cfg, sd8, torch.device(DEV), quant="mxfp8")
    merged8 = merge_lora_state_dict(sd8, mid.dirs["A"])
    torch.set_num_threads(cpu_threads())
    nz = O.exp_noise(5, MT - 1, mid.dm.C, mid.dm.tgt_vocab)
    r = O.generate(merged8, mid.cfg, TEXTS[1], max_tokens=MT, noise=nz, mirror=False)
    logits, res = teacher_forced(mid, w8, [1], ["A"], [(r, nz)])
    err = worst_err(logits, 0, r)
    print(f"MXFP8 base + adapter: logits max-abs err {err:.3e}")
    assert err <= LOGIT_TOL, err
    for i, p in enumerate(r.preds):
        assert np.array_equal(res[0].preds[1 + i], p), i


def test_score_under_an_adapter(mid):
    """Dia.score(text, codes, adapter="A") — a Dia on the DEFAULT device, as the loaders and the CLI make it — against the host-side
    NLL of the oracle's merged logits, with the bound of tests/test_gpu_score.py: guidance amplifies a logit deviation by at most
    1 + 2s and log-softmax is 2-Lipschitz in the sup norm, so with delta = max |logits_hip - logits_oracle| measured here on the same
    forced rows: |d lp_cfg| <= 2 (1 + 2s) delta + 2e-5 per position — and the base model scores these codes far outside it"""
    from dia_hip.model import Dia
    s_cfg = 3.0
    r, nz = oracle_run(mid, 0, "A")
    rows = r.tokens[:MT]
    logits, _ = teacher_forced(mid, mid.w, [0], ["A"], [(r, nz)])
    delta = worst_err(logits, 0, r)
    bound = 2 * (1 + 2 * s_cfg) * delta + LP_TOL
    dia = Dia.from_state_dict(mid.cfg, mid.sd, "float32")
    assert dia.device.index is None                                 # "cuda": what a session tensor reports as cuda:0
    assert dia.load_adapters(mid.dirs) == [0, 1]
    got = dia.score(TEXTS[0], rows, cfg_scale=s_cfg, adapter="A")
    base = dia.score(TEXTS[0], rows, cfg_scale=s_cfg)
    with pytest.raises(ValueError):
        dia.score(TEXTS[0], rows, adapter="nobody")
    torch.set_num_threads(cpu_threads())
    st = O.prepare(mid.merged["A"], mid.dm, O.text_tokens(effective_text(TEXTS[0]), mid.dm), False)
    worst, n, nll = 0.0, 0, []
    for cur in range(1, MT):
        lg2 = O.decode_step(mid.merged["A"], st, rows[cur - 1], cur)
        lgd = torch.log_softmax(O.guided_logits(lg2.clone(), s_cfg, mid.dm).double(), dim=-1).numpy()
        for c in range(mid.dm.C):
            if got.valid[cur, c]:
                want = lgd[c, rows[cur, c]]
                worst = max(worst, abs(float(got.lp_cfg[cur, c]) - want))
                nll.append(-want)
                n += 1
    print(f"score under adapter A: delta {delta:.3e}, bound {bound:.3e}, max |d lp_cfg| {worst:.3e} over {n} targets; "
          f"nll {got.nll_cfg:.4f} vs base {base.nll_cfg:.4f}")
    assert delta <= LOGIT_TOL and n > 0 and n == got.n_valid and worst <= bound, (delta, worst, bound)
    assert abs(got.nll_cfg - float(np.mean(nll))) <= bound
    both = got.valid & np.isfinite(base.lp_cfg) & np.isfinite(got.lp_cfg)
    assert float(np.abs(base.lp_cfg[both] - got.lp_cfg[both]).max()) > 1e-2       # the base model scores these codes differently


def test_generate_under_an_adapter_on_the_default_device(mid):
    """the public generation calls of a Dia made without a device argument: generate_codes(adapter=) (a closed batch of one) and
    generate_batch(adapters=, slots=1) (the slot path) give the same codes, another adapter and the base model give other ones, and
    a list of the wrong length is a ValueError"""
    from dia_hip.model import Dia
    dia = Dia.from_state_dict(mid.cfg, mid.sd, "float32")
    dia.load_adapters(mid.dirs)
    a1 = dia.generate_codes(TEXTS[1], max_tokens=40, seed=3, adapter="A")
    a2 = dia.generate_batch([TEXTS[1]], max_tokens=40, seeds=[3], adapters=["A"], slots=1)[0]
    b1 = dia.generate_codes(TEXTS[1], max_tokens=40, seed=3, adapter="B")
    p1 = dia.generate_codes(TEXTS[1], max_tokens=40, seed=3)
    assert a1.shape[-1] > 0 and np.array_equal(a1, a2)
    assert not np.array_equal(a1, b1) and not np.array_equal(a1, p1)
    with pytest.raises(ValueError):
        list(dia.generate_stream([TEXTS[1], TEXTS[0]], slots=1, max_tokens=8, adapters=["A"]))
    with pytest.raises(ValueError):
        dia.generate_batch([TEXTS[1]], adapters=["A", "B"])


# ---- the deferred-wo form: 3 layers of Dia-1.6B widths (D = 2048, <= 4 rows), where odd layers read x_alt ------------------------
@pytest.fixture(scope="module")
def wide(tmp_path_factory):
    c = C.dia_1_6b_config()
    m = Env()
    m.cfg = c.model_copy(update={
        "model": c.model.model_copy(update={"encoder": c.model.encoder.model_copy(update={"n_layer": 1}),
                                            "decoder": c.model.decoder.model_copy(update={"n_layer": 3})}),
        "data": c.data.model_copy(update={"text_length": 128, "audio_length": 128})})
    m.sd = synthetic_state_dict(m.cfg, seed=1234, std=0.02)
    m.w = DeviceWeights(m.cfg, m.sd, torch.device(DEV))
    m.dirs = dict(A=write_qv_adapter(str(tmp_path_factory.mktemp("wide")), "A", m.cfg, m.sd, 4, amp=0.02))
    m.bank = AdapterBank(m.cfg, DEV)
    m.bank.add("A", m.dirs["A"])
    m.merged = {None: m.sd, "A": merge_lora_state_dict(m.sd, m.dirs["A"])}
    m.dm = O.Dims.of(m.cfg)
    m.oracle = {}
    return m


@pytest.mark.parametrize("B", [1, 2])
def test_deferred_wo_form_reads_the_right_residual_buffer(wide, B):
    """batch 1 / 2 at D = 2048: with the knob wo_defer on, every wo's merge is deferred and the residual stream of odd layers is
    x_alt — the corrections must read that buffer.  Logits of 6 teacher-forced steps within 1e-3 of the oracle on the merged
    weights in both forms, and bit for bit the same in both (the deferred form rebuilds x bit for bit).  The encoder (E = 1024)
    and every cross-K/V correction run the 1024-wide kernel instantiations here"""
    mt = 7
    tis, adapters = [0, 1][:B], ["A", None][:B]
    runs = [oracle_run(wide, t, a, mt=mt) for t, a in zip(tis, adapters)]
    out = {}
    for knob in (0, 1):
        hb.set_tuning("wo_defer", knob)
        try:
            out[knob], _ = teacher_forced(wide, wide.w, tis, adapters, runs, mt=mt)
            ids = [encode_text(effective_text(TEXTS[t]), wide.cfg) for t in tis]
            s = DecodeSession(wide.w, ids, kv_dtype="f32", max_tokens=mt, adapters=wide.bank, adapter_ids=adapters)
            try:
                s.prefill()
                s.time_step()
                small = [n for n in s.last_kernel_names if "k_gemv_small<" in n]
                forms = (sum(n.endswith(", 1>") for n in small), sum(n.endswith(", 2>") for n in small))
                n_lora = sum("k_lora<" in n for n in s.last_kernel_names)
            finally:
                s.close()
        finally:
            hb.set_tuning("wo_defer", -1)
        nl = wide.cfg.model.decoder.n_layer
        assert forms == ((nl, nl) if knob else (0, 0)) and n_lora == 2 * nl, (knob, forms, n_lora)
        for b, (r, _) in enumerate(runs):
            err = worst_err(out[knob], b, r)
            print(f"wo_defer={knob} batch {B} adapter {adapters[b]}: logits max-abs err {err:.3e}")
            assert err <= LOGIT_TOL, (knob, b, err)
    assert all(np.array_equal(a_, b_) for a_, b_ in zip(out[0], out[1]))
    r0 = runs[0][0]
    base = O.generate(wide.sd, wide.cfg, TEXTS[0], max_tokens=mt, noise=runs[0][1], mirror=False, forced_tokens=r0.tokens)
    assert max(float(np.abs(a_ - b_).max()) for a_, b_ in zip(base.logits, r0.logits)) > 1e-2


def test_launch_counts_and_refusals(mid):
    """a session without a bank launches what it always launched (8 launches per layer, the logits head, the sampler); a bank adds
    exactly two per layer; set_lora after a step is a state error; a compacted checkpoint with a bank raises"""
    n_layer = mid.cfg.model.decoder.n_layer
    ids = [encode_text(effective_text(TEXTS[1]), mid.cfg)]
    plain = DecodeSession(mid.w, ids, kv_dtype="f32", max_tokens=8)
    lora = DecodeSession(mid.w, ids, kv_dtype="f32", max_tokens=8, adapters=mid.bank, adapter_ids=["B"])
    try:
        assert plain.launches_per_step() == 8 * n_layer + 2
        assert lora.launches_per_step() == plain.launches_per_step() + 2 * n_layer
        lora.prefill()
        lora.decode(1, use_graph=False)
        assert len(lora.profile_step()) == lora.launches_per_step()
        assert hb.lib().dia_engine_set_lora(lora._engine, None) == -3
        with pytest.raises(RuntimeError, match="fixed once a session"):
            mid.bank.add("C", mid.dirs["A"])
        with pytest.raises(ValueError):
            DecodeSession(mid.w, ids, kv_dtype="f32", max_tokens=8, adapters=mid.bank, adapter_ids=["A", "B"])
        with pytest.raises(ValueError):
            DecodeSession(mid.w, ids, kv_dtype="f32", max_tokens=8, adapter_ids=["A"])
    finally:
        plain.close()
        lora.close()
    # structured pruning: zero two query heads of layer 0 -> the loader compacts -> adapters are refused
    sdp = dict(mid.sd)
    wq = sdp["decoder.layers.0.self_attention.q_proj.weight"].clone()
    wq[:, :4] = 0
    wo = sdp["decoder.layers.0.self_attention.o_proj.weight"].clone()
    wo[:4] = 0
    sdp["decoder.layers.0.self_attention.q_proj.weight"], sdp["decoder.layers.0.self_attention.o_proj.weight"] = wq, wo
    wp = DeviceWeights(mid.cfg, sdp, torch.device(DEV))
    assert wp.compacted
    with pytest.raises(hb.DiaHipError, match="compacted"):
        DecodeSession(wp, ids, kv_dtype="f32", max_tokens=8, adapters=mid.bank, adapter_ids=["A"])
