"""Activation statistics of a running model on a real MI355X (DESIGN.md "Activation statistics"): DecodeSession(calibrate=True) and
Dia.calibrate against the float32 oracle's capture (tests/calib_ref.py), for every name of prunable_names.

Model: the `mid` fixture (head_dim 128 — the attention kernels are built for it, which the `tiny` config does not have), synthetic
weights, fp32 K/V, 12 forced rows = 11 steps, texts of three lengths.

Deviation of the sums from the oracle: not derivable (the device and the float32 oracle differ in summation order through the
whole network).  Measured on the MI355X, largest relative deviation per tap over B = 1 (three planes) and B = 3 (fp32 tiles):
MEASURED below — the test prints the per-tap values.  Asserted: 4 x the measured value (the project's usual margin), under the
hard ceiling 1e-3.  Channels whose reference sum lies below 1e-12 of the tap's largest are compared absolutely against that floor.

A finished utterance: teacher forcing acts on no EOS (csrc/sample.hip: the EOS countdown is skipped under `teacher`), so a forced
EOS cannot end an utterance of a closed batch early.  The test sets the utterance's done flag (fsm[b][3]) between two steps
instead, which is the state an EOS leaves, and checks that its rows stop counting at the step dia_score stops writing for it."""
import copy
import ctypes
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import calib_ref as R
from dia_hip import binding as hb
from dia_hip import config as C
from dia_hip import pruning as P
from dia_hip import score as S
from dia_hip.calib import ActStats, decoder_tap_names, encoder_tap_names
from dia_hip.engine import DecodeSession, DeviceWeights
from dia_hip.tokens import effective_text, encode_text
from dia_hip.weights import synthetic_state_dict

DEV = "cuda:0"
TEXTS = ["[S1] Dia is an open weights text to dialogue model. [S2] You get full control over scripts and voices.",
         "[S1] Hello there. [S2] Hi, how are you?",
         "[S1] Pruning keeps what the activations say matters."]
ROWS = 12
# largest relative deviation of a channel sum from the oracle capture per tap, measured on the MI355X (B = 1 planes / B = 3 fp32 tiles):
#   decoder cross o_proj 4.3e-04 / 9.6e-06 (one short text: the attention output of some channels nearly cancels), encoder o_proj
#   5.9e-05 / 1.1e-05, decoder wo 1.3e-05 / 9.2e-06, every other tap below 1e-05.  4 x 4.31e-04 exceeds the ceiling: the ceiling holds
MEASURED = 4.31e-4
TOL = min(4 * MEASURED, 1e-3)
FLOOR = 1e-12


@pytest.fixture(scope="module")
def mid():
    try:
        torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
    except Exception:
        pass
    cfg = C.mid_config()
    sd = synthetic_state_dict(cfg, seed=1234, std=0.02)
    rs = np.random.RandomState(17)
    rows = [S.teacher_rows(cfg, rs.randint(0, 1024, size=(11, cfg.data.channels)))[:ROWS] for _ in TEXTS]
    return types.SimpleNamespace(cfg=cfg, sd=sd, w=DeviceWeights(cfg, sd, torch.device(DEV)), rows=rows,
                                 ids=[encode_text(effective_text(t), cfg) for t in TEXTS])


def run(m, sel, *, calibrate=True, score=False, graph=False, done_after=None):
    """one closed teacher-forced session over the utterances `sel`; done_after = (utterance, steps): its done flag is set by hand
    after that many steps"""
    s = DecodeSession(m.w, [m.ids[i] for i in sel], kv_dtype="f32", max_tokens=ROWS, cfg_scale=3.0, temperature=0.0,
                      teacher_tokens=[m.rows[i] for i in sel], calibrate=calibrate, score=score)
    s.prefill()
    if done_after is None:
        s.decode(ROWS - 1, use_graph=graph)
    else:
        b, k = done_after
        s.decode(k, use_graph=graph)
        s.sync()
        s.fsm[b, 3] = 1
        torch.cuda.synchronize()
        s.decode(ROWS - 1 - k, use_graph=graph)
    s.sync()
    out = types.SimpleNamespace(stats=s.act_stats() if calibrate else None, scores=s.scores_host().copy() if score else None,
                                tokens=s.tokens.cpu().numpy(), pred=s.pred.cpu().numpy(), logits=s.logits_host().copy(),
                                launches=s.launches_per_step())
    s.close()
    return out


def oracle(m, sel, stop_at=None):
    with pytest.MonkeyPatch.context() as mp:
        return R.oracle_stats(mp, m.cfg, m.sd, [TEXTS[i] for i in sel], [m.rows[i] for i in sel], [1] * len(sel), stop_at)


def compare(m, stats, want_sums, want_rows):
    """rows exact; per tap the largest relative deviation of a channel sum (absolute against the floor for the smallest channels)"""
    worst = {}
    for tap in decoder_tap_names(m.cfg) + encoder_tap_names(m.cfg):
        for k in tap:
            assert stats.rows[k] == want_rows[k], (k, stats.rows[k], want_rows[k])
            got, ref = stats.sums[k], want_sums[k]
            assert got.shape == ref.shape and np.isfinite(got).all(), k
            floor = FLOOR * ref.max()
            dev = np.abs(got - ref) / np.maximum(ref, floor)
            kind = k.split(".")[0] + "." + ".".join(k.split(".")[3:])
            worst[kind] = max(worst.get(kind, 0.0), float(dev.max()))
    for kind, v in sorted(worst.items()):
        print(f"  {kind}: {v:.3e}")
    return max(worst.values())


@pytest.mark.parametrize("sel,planes", [((1,), True), ((0, 1, 2), False)])
def test_against_the_oracle_capture(mid, tuning, sel, planes):
    if planes:
        tuning("act_f32", 0)                # three bf16 planes between the kernels of the step
    got = run(mid, sel)
    want_sums, want_rows = oracle(mid, sel)
    lens = [len(mid.ids[i]) for i in sel]
    assert want_rows["decoder.logits_dense.weight"] == 2 * (ROWS - 1) * len(sel)
    assert want_rows["encoder.layers.0.mlp.wo.weight"] == sum(lens) == want_rows["decoder.layers.0.cross_attention.k_proj.weight"]
    assert sorted(got.stats.names()) == sorted(P.prunable_names(mid.cfg))
    worst = compare(mid, got.stats, want_sums, want_rows)
    print(f"B={len(sel)} {'planes' if planes else 'fp32 tiles'}: largest relative deviation {worst:.3e} (asserted {TOL:.1e})")
    assert worst <= TOL, worst


def test_a_finished_utterance_stops_counting(mid):
    sel, b, k = (0, 1, 2), 1, 5
    got = run(mid, sel, score=True, done_after=(b, k))
    # dia_score wrote rows 1 .. k of the finished utterance and nothing behind them; the others ran to the end
    wrote = ~np.isnan(got.scores[:, :ROWS, 0, 0])
    assert wrote[b, 1: k + 1].all() and not wrote[b, k + 1:].any() and wrote[0, 1:].all() and wrote[2, 1:].all()
    want_sums, want_rows = oracle(mid, sel, stop_at=[None, k + 1, None])
    assert want_rows["decoder.logits_dense.weight"] == 2 * (2 * (ROWS - 1) + k)
    assert compare(mid, got.stats, want_sums, want_rows) <= TOL


def test_calibration_writes_no_state_and_counts_launches(mid, tuning):
    tuning("wo_defer", 0)                   # a calibrating engine keeps wo's in-launch merge; the plain one is told to
    for sel in ((0,), (0, 1, 2)):
        cal = run(mid, sel, score=True, graph=True)
        plain = run(mid, sel, calibrate=False, score=True, graph=True)
        for f in ("tokens", "pred"):
            assert np.array_equal(getattr(cal, f), getattr(plain, f)), f
        assert np.array_equal(cal.logits.view(np.uint32), plain.logits.view(np.uint32))
        assert np.array_equal(cal.scores.view(np.uint32), plain.scores.view(np.uint32))
        assert cal.launches == plain.launches + 6 * mid.cfg.model.decoder.n_layer + 1


@pytest.mark.parametrize("sel", [(2,), (0, 1, 2)])
def test_graph_replay_equals_eager(mid, sel):
    a, b = run(mid, sel, graph=False).stats, run(mid, sel, graph=True).stats
    for k in a.names():
        assert a.rows[k] == b.rows[k] and np.array_equal(a.sums[k].view(np.uint64), b.sums[k].view(np.uint64)), k
    assert a.sums["decoder.layers.2.mlp.wo.weight"].max() > 0


def test_refusals(mid):
    kw = dict(kv_dtype="f32", max_tokens=ROWS, temperature=0.0, teacher_tokens=mid.rows[:1], calibrate=True)
    with pytest.raises(ValueError, match="slots"):
        DecodeSession(mid.w, mid.ids[:1], _slotted=True, **kw)
    with pytest.raises(ValueError, match="adapters"):
        DecodeSession(mid.w, mid.ids[:1], adapters=object(), **kw)
    pruned = dict(mid.sd)                   # structured pruning: four zero query heads of layer 0 -> the loader compacts
    wq, wo = (pruned[f"decoder.layers.0.self_attention.{p_}_proj.weight"].clone() for p_ in "qo")
    wq[:, :4] = 0
    wo[:4] = 0
    pruned["decoder.layers.0.self_attention.q_proj.weight"], pruned["decoder.layers.0.self_attention.o_proj.weight"] = wq, wo
    wc = DeviceWeights(mid.cfg, pruned, torch.device(DEV))
    assert wc.compacted
    with pytest.raises(ValueError, match="compacted"):
        DecodeSession(wc, mid.ids[:1], **kw)
    wseg = copy.copy(mid.w)
    wseg.seg_layers = [torch.zeros(1, device=DEV)]                         # what DeviceWeights(seg="on") leaves on a model with ring arenas
    with pytest.raises(ValueError, match="seg='on'"):
        DecodeSession(wseg, mid.ids[:1], **kw)
    with pytest.raises(ValueError, match="teacher_tokens"):
        DecodeSession(mid.w, mid.ids[:1], kv_dtype="f32", max_tokens=ROWS, calibrate=True)
    with pytest.raises(ValueError, match="different lengths"):
        DecodeSession(mid.w, mid.ids[:2], kv_dtype="f32", max_tokens=ROWS, temperature=0.0, teacher_tokens=[mid.rows[0], mid.rows[1][:9]],
                      calibrate=True)
    # the C entry: a free-running engine is refused, and so is any engine once a step has been issued
    L = hb.lib()
    s = DecodeSession(mid.w, mid.ids[:1], **kw)
    free = DecodeSession(mid.w, mid.ids[:1], kv_dtype="f32", max_tokens=ROWS, temperature=0.0)
    c = s._calib
    nd = c["n_dec"]
    acc = (ctypes.c_void_p * nd)(*[hb.ptr(t) for t in c["acc"][:nd]])
    kts = (ctypes.c_int32 * nd)(*c["kt"][:nd])
    ca = hb.CalibArgs(n_layer=mid.cfg.model.decoder.n_layer, acc=ctypes.cast(acc, ctypes.POINTER(ctypes.c_void_p)),
                      kt=ctypes.cast(kts, ctypes.POINTER(ctypes.c_int32)), counters=c["counters"].data_ptr())
    assert L.dia_engine_set_calib(free._engine, ctypes.byref(ca)) == -1 and b"teacher" in L.dia_last_error()
    ca.n_layer += 1
    assert L.dia_engine_set_calib(s._engine, ctypes.byref(ca)) == -1
    ca.n_layer -= 1
    free.close()
    s.prefill()
    s.decode(1, use_graph=False)
    assert L.dia_engine_set_calib(s._engine, ctypes.byref(ca)) == -3
    assert L.dia_engine_set_calib(s._engine, None) == -3
    s.close()
    with pytest.raises(hb.DiaHipError):
        s2 = DecodeSession(mid.w, mid.ids[:1], kv_dtype="f32", max_tokens=ROWS, temperature=0.0, teacher_tokens=mid.rows[:1])
        try:
            s2.act_stats()
        finally:
            s2.close()


def test_calibrate_prune_stream_score(mid, tmp_path):
    """the loop the feature closes: Dia.calibrate -> 2:4 with the statistics -> the sparse stream -> Dia.score.  Synthetic weights:
    nothing is claimed about quality"""
    from dia_hip.model import Dia
    dia = Dia.from_state_dict(mid.cfg, mid.sd, "float32", torch.device(DEV))
    stats = dia.calibrate(TEXTS, mid.rows, batch=2)                        # two sessions, merged
    one = run(mid, (0, 1, 2)).stats
    for k in stats.names():
        assert stats.rows[k] == one.rows[k], k
        assert np.allclose(stats.sums[k], one.sums[k], rtol=1e-3, atol=FLOOR * one.sums[k].max()), k
    path = str(tmp_path / "stats.npz")
    stats.save(path)
    wanda = P.semi_structured_prune_state_dict(mid.cfg, mid.sd, act_stats=ActStats.load(path))
    plain = P.semi_structured_prune_state_dict(mid.cfg, mid.sd)
    differ = sum(int(((wanda[k] != 0) != (plain[k] != 0)).any()) for k in P.prunable_names(mid.cfg))      # kernels with another survivor
    assert differ > 0 and all(P.is_2of4(P._kernel_2d(k, wanda[k].float())) for k in P.prunable_names(mid.cfg))
    old = Dia.sparse_weights
    Dia.sparse_weights = "2:4"
    try:
        sparse = Dia.from_state_dict(mid.cfg, dict(wanda), "float32", torch.device(DEV))
        r = sparse.score(TEXTS[0], mid.rows[0])
    finally:
        Dia.sparse_weights = old
    assert r.n_valid > 0 and np.isfinite(r.nll_cfg) and np.isfinite(r.nll_cond)
