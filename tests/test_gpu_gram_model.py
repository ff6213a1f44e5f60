"""Gram matrices of a running model on a real MI355X (DESIGN.md "Gram matrices and GPTQ"): DecodeSession(calibrate="gram") and
Dia.calibrate(gram=True) against the float32 oracle's capture of X^T X (tests/gram_ref.py), for every tap of the decode step.

Model: the `mid` fixture (head_dim 128), synthetic weights, fp32 K/V, 12 forced rows = 11 steps, texts of three lengths; B = 1 on
three bf16 planes and B = 3 on fp32 tiles.

Deviation of a matrix from the oracle's, |got_ij - ref_ij| / sqrt(ref_ii ref_jj): not derivable (the device and the float32 oracle
differ in summation order through the whole network).  Measured on the MI355X, largest value per tap kind over the two runs:
MEASURED below — the test prints the per-tap values.  Asserted: min(4 x measured, 1e-3), the project's rule.  A channel whose
reference diagonal lies below 1e-12 of the tap's largest enters the denominator at that floor.

A finished utterance: as in test_gpu_calib_model.py, the done flag is set by hand between two steps."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gram_ref as R
from dia_hip import binding as hb
from dia_hip import config as C
from dia_hip import quant as Q
from dia_hip import score as S
from dia_hip.calib import GramStats, decoder_tap_names, gram_tap_keys
from dia_hip.engine import DecodeSession, DeviceWeights
from dia_hip.pruning import _kernel_2d
from dia_hip.tokens import effective_text, encode_text
from dia_hip.weights import synthetic_state_dict

DEV = "cuda:0"
TEXTS = ["[S1] Dia is an open weights text to dialogue model. [S2] You get full control over scripts and voices.",
         "[S1] Hello there. [S2] Hi, how are you?",
         "[S1] Pruning keeps what the activations say matters."]
ROWS = 12
# largest |got - ref| / sqrt(ref_ii ref_jj) per tap kind, measured on the MI355X (B = 1 planes / B = 3 fp32 tiles):
#   co 4.3e-04 / 9.6e-06 (one short text: the cross-attention output of some channels nearly cancels — the value dia_act_stats's test
#   measures on the same tap), wo 1.3e-05 / 9.2e-06, wi 1.1e-05 / 5.7e-06, o 1.1e-05 / 5.4e-06, cq 1.0e-05 / 4.4e-06, logits_dense
#   6.7e-06 / 5.3e-06, qkv 6.1e-06 / 4.5e-06.  4 x 4.31e-04 exceeds the ceiling: the ceiling holds
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


def run(m, sel, *, calibrate="gram", layers=None, score=False, graph=False, done_after=None):
    """one closed teacher-forced session over the utterances `sel`; done_after = (utterance, steps): its done flag is set by hand
    after that many steps"""
    s = DecodeSession(m.w, [m.ids[i] for i in sel], kv_dtype="f32", max_tokens=ROWS, cfg_scale=3.0, temperature=0.0,
                      teacher_tokens=[m.rows[i] for i in sel], calibrate=calibrate, gram_layers=layers, score=score)
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
    out = types.SimpleNamespace(grams=s.gram_stats() if calibrate == "gram" else None, stats=s.act_stats() if calibrate else None,
                                scores=s.scores_host().copy() if score else None, tokens=s.tokens.cpu().numpy(),
                                pred=s.pred.cpu().numpy(), logits=s.logits_host().copy(), launches=s.launches_per_step())
    s.close()
    return out


def oracle(m, sel, stop_at=None):
    names = [tap[0] for tap in decoder_tap_names(m.cfg)]                   # one kernel per tap: the others read the same rows
    with pytest.MonkeyPatch.context() as mp:
        return R.oracle_grams(mp, m.cfg, m.sd, [TEXTS[i] for i in sel], [m.rows[i] for i in sel], names, stop_at)


def compare(m, grams, want, want_rows):
    """rows exact; per tap kind the largest |got - ref| / sqrt(ref_ii ref_jj)"""
    worst = {}
    for key, tap in zip(gram_tap_keys(m.cfg), decoder_tap_names(m.cfg)):
        assert grams.rows[key] == want_rows[tap[0]], (key, grams.rows[key], want_rows[tap[0]])
        got, ref = grams.dense(tap[0]), want[tap[0]]
        assert got.shape == ref.shape and np.isfinite(got).all(), key
        assert np.array_equal(got.view(np.uint64), got.T.copy().view(np.uint64)), key
        d = np.sqrt(np.maximum(np.diagonal(ref), FLOOR * np.diagonal(ref).max()))
        dev = float((np.abs(got - ref) / (d[:, None] * d[None, :])).max())
        kind = key.split(".")[-1]
        worst[kind] = max(worst.get(kind, 0.0), dev)
    for kind, v in sorted(worst.items()):
        print(f"  {kind}: {v:.3e}")
    return max(worst.values())


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


@pytest.mark.parametrize("sel,planes", [((1,), True), ((0, 1, 2), False)])
def test_against_the_oracle_capture(mid, tuning, sel, planes):
    if planes:
        tuning("act_f32", 0)                # three bf16 planes between the kernels of the step
    got = run(mid, sel)
    want, want_rows = oracle(mid, sel)
    assert want_rows["decoder.logits_dense.weight"] == 2 * (ROWS - 1) * len(sel)
    assert got.grams.taps() == gram_tap_keys(mid.cfg) and sorted(got.grams.names()) == sorted(Q.mx_names(mid.cfg))
    worst = compare(mid, got.grams, want, want_rows)
    print(f"B={len(sel)} {'planes' if planes else 'fp32 tiles'}: largest deviation {worst:.3e} (asserted {TOL:.1e})")
    assert worst <= TOL, worst
    # the diagonals are the sums of a calibrate=True session, bit for bit; the encoder taps are there as before
    cal = run(mid, sel, calibrate=True).stats
    assert sorted(got.stats.names()) == sorted(cal.names())
    for k in cal.names():
        assert got.stats.rows[k] == cal.rows[k] and same_bits(got.stats.sums[k], cal.sums[k]), k
    for k in got.grams.names():
        assert same_bits(np.diagonal(got.grams.dense(k)).copy(), cal.sums[k]), k


def test_a_finished_utterance_stops_counting(mid):
    sel, b, k = (0, 1, 2), 1, 5
    got = run(mid, sel, done_after=(b, k))
    want, want_rows = oracle(mid, sel, stop_at=[None, k + 1, None])
    assert want_rows["decoder.logits_dense.weight"] == 2 * (2 * (ROWS - 1) + k)
    assert compare(mid, got.grams, want, want_rows) <= TOL


def test_gram_writes_no_state_counts_launches_and_replays_bitwise(mid, tuning):
    tuning("wo_defer", 0)                   # a tapped engine keeps wo's in-launch merge; the plain one is told to
    n = mid.cfg.model.decoder.n_layer
    for sel in ((0,), (0, 1, 2)):
        g = run(mid, sel, score=True, graph=True)
        plain = run(mid, sel, calibrate=False, score=True, graph=True)
        for f in ("tokens", "pred"):
            assert np.array_equal(getattr(g, f), getattr(plain, f)), f
        assert np.array_equal(g.logits.view(np.uint32), plain.logits.view(np.uint32))
        assert np.array_equal(g.scores.view(np.uint32), plain.scores.view(np.uint32))
        assert g.launches == plain.launches + 6 * n + 1
        eager = run(mid, sel, graph=False)                                 # graph replay == eager, bit for bit
        for t in g.grams.taps():
            assert g.grams.rows[t] == eager.grams.rows[t] and same_bits(g.grams.packed[t], eager.grams.packed[t]), t
        assert np.abs(g.grams.packed[f"decoder.layers.{n - 1}.wo"]).max() > 0
        # one layer selected: six launches, its matrices those of the full run, the other names without a row
        one = run(mid, sel, layers=[1], score=True, graph=True)
        assert one.launches == plain.launches + 6
        assert one.grams.taps() == gram_tap_keys(mid.cfg)[6:12]
        for t in one.grams.taps():
            assert one.grams.rows[t] == g.grams.rows[t] and same_bits(one.grams.packed[t], g.grams.packed[t]), t
        assert one.stats.rows["decoder.layers.0.mlp.wo.weight"] == 0 and one.stats.rows["decoder.layers.1.mlp.wo.weight"] > 0
        head = run(mid, sel, layers=(n, n + 1), score=True, graph=True)
        assert head.launches == plain.launches + 1 and head.grams.taps() == ["decoder.logits_dense"]


def test_refusals(mid):
    kw = dict(kv_dtype="f32", max_tokens=ROWS, temperature=0.0, teacher_tokens=mid.rows[:1], calibrate="gram")
    with pytest.raises(ValueError, match="slots"):
        DecodeSession(mid.w, mid.ids[:1], _slotted=True, **kw)
    with pytest.raises(ValueError, match="adapters"):
        DecodeSession(mid.w, mid.ids[:1], adapters=object(), **kw)
    with pytest.raises(ValueError, match="teacher_tokens"):
        DecodeSession(mid.w, mid.ids[:1], kv_dtype="f32", max_tokens=ROWS, calibrate="gram")
    with pytest.raises(ValueError, match="different lengths"):
        DecodeSession(mid.w, mid.ids[:2], kv_dtype="f32", max_tokens=ROWS, temperature=0.0, teacher_tokens=[mid.rows[0], mid.rows[1][:9]],
                      calibrate="gram")
    with pytest.raises(ValueError, match="gram_layers"):
        DecodeSession(mid.w, mid.ids[:1], gram_layers=[99], **kw)
    # the C entry: a free-running engine, an engine that has dia_engine_set_calib, and any engine once a step has been issued
    L = hb.lib()
    n = mid.cfg.model.decoder.n_layer
    s = DecodeSession(mid.w, mid.ids[:1], **kw)
    free = DecodeSession(mid.w, mid.ids[:1], kv_dtype="f32", max_tokens=ROWS, temperature=0.0)
    cal = DecodeSession(mid.w, mid.ids[:1], **dict(kw, calibrate=True))
    c = s._calib
    nd = c["n_dec"]
    gp = (ctypes.c_void_p * nd)(*[hb.ptr(t) for t in c["gram"]])
    kts = (ctypes.c_int32 * nd)(*c["kt"][:nd])
    ga = hb.GramArgs(n_layer=n, gram=ctypes.cast(gp, ctypes.POINTER(ctypes.c_void_p)), kt=ctypes.cast(kts, ctypes.POINTER(ctypes.c_int32)),
                     counters=c["counters"].data_ptr())
    assert L.dia_engine_set_gram(free._engine, ctypes.byref(ga)) == -1 and b"teacher" in L.dia_last_error()
    assert L.dia_engine_set_gram(cal._engine, ctypes.byref(ga)) == -1 and b"dia_engine_set_calib" in L.dia_last_error()
    # ... and the other way round: a Gram engine takes no dia_engine_set_calib
    cc = cal._calib
    acc = (ctypes.c_void_p * nd)(*[hb.ptr(t) for t in cc["acc"][:nd]])
    ca = hb.CalibArgs(n_layer=n, acc=ctypes.cast(acc, ctypes.POINTER(ctypes.c_void_p)), kt=ctypes.cast(kts, ctypes.POINTER(ctypes.c_int32)),
                      counters=cc["counters"].data_ptr())
    assert L.dia_engine_set_calib(s._engine, ctypes.byref(ca)) == -1 and b"dia_engine_set_gram" in L.dia_last_error()
    ga.n_layer += 1
    assert L.dia_engine_set_gram(s._engine, ctypes.byref(ga)) == -1
    ga.n_layer -= 1
    gp[3] = hb.ptr(c["gram"][3]) + 8                                        # a matrix that is not 16-byte aligned
    assert L.dia_engine_set_gram(s._engine, ctypes.byref(ga)) == -1 and b"16-byte aligned" in L.dia_last_error()
    gp[3] = hb.ptr(c["gram"][3])
    kts[2] = 10 ** 6                                                         # wider than its plane set
    assert L.dia_engine_set_gram(s._engine, ctypes.byref(ga)) == -1 and b"k-tiles" in L.dia_last_error()
    kts[2] = c["kt"][2]
    assert L.dia_engine_set_gram(s._engine, ctypes.byref(ga)) == 0
    free.close()
    cal.close()
    s.prefill()
    s.decode(1, use_graph=False)
    assert L.dia_engine_set_gram(s._engine, ctypes.byref(ga)) == -3
    assert L.dia_engine_set_gram(s._engine, None) == -3
    s.close()
    with pytest.raises(hb.DiaHipError):
        s2 = DecodeSession(mid.w, mid.ids[:1], **dict(kw, calibrate=True))
        try:
            s2.gram_stats()
        finally:
            s2.close()


def test_calibrate_gptq_stream_score(mid, tmp_path):
    """the loop the feature closes: Dia.calibrate(gram=True) -> save / load -> GPTQ onto the MXFP4 grid -> the fp4 stream -> Dia.score.
    Synthetic weights: nothing is claimed about quality"""
    from dia_hip.model import Dia
    dia = Dia.from_state_dict(mid.cfg, mid.sd, "float32", torch.device(DEV))
    stats, grams = dia.calibrate(TEXTS, mid.rows, batch=2, gram=True)      # two sessions, merged
    one = run(mid, (0, 1, 2))
    for t in grams.taps():
        assert grams.rows[t] == one.grams.rows[t], t
    for k in stats.names():
        assert stats.rows[k] == one.stats.rows[k], k
    path = str(tmp_path / "grams.npz")
    grams.save(path)
    loaded = GramStats.load(path)
    assert all(same_bits(loaded.packed[t], grams.packed[t]) for t in grams.taps())
    fsd = {k: v.float() for k, v in mid.sd.items()}
    gptq = Q.gptq_quantize_state_dict(mid.cfg, fsd, loaded, "mxfp4")
    rtn = Q.mxfp4_quantize_state_dict(mid.cfg, fsd)
    e_g = e_r = 0.0
    for k in Q.mx_names(mid.cfg):
        assert Q.is_mxfp4(_kernel_2d(k, gptq[k])), k
        G, w = loaded.dense(k), _kernel_2d(k, fsd[k])
        e_g += Q.calibration_error(G, _kernel_2d(k, gptq[k]) - w)
        e_r += Q.calibration_error(G, _kernel_2d(k, rtn[k]) - w)
    print(f"sum over the kernels of tr(delta^T G delta): GPTQ {e_g:.4e}, round-to-nearest {e_r:.4e}, ratio {e_g / e_r:.3f}")
    assert e_g < e_r
    old = Dia.weight_format
    Dia.weight_format = "mxfp4"
    try:
        q = Dia.from_state_dict(mid.cfg, dict(gptq), "float32", torch.device(DEV))
        r = q.score(TEXTS[0], mid.rows[0])
    finally:
        Dia.weight_format = old
    assert r.n_valid > 0 and np.isfinite(r.nll_cfg) and np.isfinite(r.nll_cond)
