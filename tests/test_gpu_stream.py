"""Frame streaming on the device: dia_emit_frames on a synthetic slot state against the rule of dia_hip/tokens.py, and
DecodeSession.stream_iter / cancel / Dia.stream_frames / cli --stream-chunk against the results of serve() and of the oracle —
the chunks of a request, joined, are the codec input of that request, bit for bit (fp32 K/V)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from dia_hip import binding as hb
from dia_hip import config as C
from dia_hip import tokens as TK
from dia_hip.engine import DecodeSession, DeviceWeights
from dia_hip.model import Dia
from dia_hip.weights import synthetic_state_dict
from test_gpu_slots import S_CAP, TEXTS, eight_requests, oracle_of, request_of, spec

DIA_DELAYS = [0, 8, 9, 10, 11, 12, 13, 14, 15]
CANARY = -7


# ---- 3. the kernel on a synthetic state ----------------------------------------------------------------------------
def emit(dv, slots, shape, cap, reset=False):
    B, T, Cn, md = shape
    a = hb.EmitArgs()
    a.B, a.T, a.C, a.max_delay, a.codebook_size, a.cap = B, T, Cn, md, 1024, cap
    a.n, a.slot, a.flags = len(slots), (ctypes.c_int32 * len(slots))(*slots), hb.EMIT_RESET if reset else 0
    for f in ("tokens", "cur", "fsm", "first_step", "delay", "emitted", "out", "state"):
        setattr(a, f, hb.ptr(dv[f]))
    hb.check(hb.lib().dia_emit_frames(ctypes.byref(a), None), "dia_emit_frames")
    torch.cuda.synchronize()


@pytest.mark.parametrize("delays,cap,fs_null", [(DIA_DELAYS, 7, False), ([0, 1, 3], 1, False), (DIA_DELAYS, 7, True)])
def test_emit_frames_on_a_synthetic_state(delays, cap, fs_null):
    dev = torch.device("cuda:0")
    B, T, Cn, md = 5, 64, len(delays), max(delays)
    listed = [4, 1, 2]
    rs = np.random.RandomState(17)
    tok = rs.randint(-1, 1027, size=(B, T, Cn)).astype(np.int32)
    for row, c, v in ((5, 0, -1), (7, 1, 1025), (20, 0, -1), (21, 1, 1024), (22, 2, 1025), (23, 0, 1026)):
        tok[:, row, c] = v                                                 # -1, EOS, PAD, BOS occur in every slot, at any C
    fs = np.array([1, 1 if fs_null else 6, 1, 2, 1], dtype=np.int32)
    cur = np.array([30, 50, T - 1, 40, 1 + md], dtype=np.int32)            # slot 4 runs: cur - first_step <= max_delay, nothing is ready
    fsm = np.zeros((B, 8), dtype=np.int32)
    fsm[:, 1], fsm[:, 2] = -1, md
    fsm[1, 3], fsm[1, 4] = 1, 40                                           # finished, last + 1 < cur: total follows last
    fsm[2, 3], fsm[2, 4] = 1, T - 1                                        # finished with W = T: the last source row is row T - 1
    host = dict(tokens=tok, cur=cur, fsm=fsm, first_step=fs, delay=np.array(delays, dtype=np.int32),
                emitted=np.array([1234, 0, 0, 1234, 0], dtype=np.int32), out=np.full((B, cap, Cn), CANARY, dtype=np.int32),
                state=np.full((B, 4), -9, dtype=np.int32))
    dv = {k: torch.from_numpy(v.copy()).to(dev) for k, v in host.items()}
    if fs_null:
        dv["first_step"] = None
    emitted = host["emitted"].copy()
    seen = {b: [] for b in listed}                                         # frames handed out so far, per slot

    def call_and_check(slots):
        dv["out"].fill_(CANARY)
        emit(dv, slots, (B, T, Cn, md), cap)
        out, state, em = dv["out"].cpu().numpy(), dv["state"].cpu().numpy(), dv["emitted"].cpu().numpy()
        cur_h, fsm_h = dv["cur"].cpu().numpy(), dv["fsm"].cpu().numpy()
        recs = {}
        for b in range(B):
            if b not in slots:
                assert (out[b] == CANARY).all() and em[b] == emitted[b]
                continue
            fin = int(fsm_h[b, 3])
            ready = TK.ready_frames(cur_h[b], fin, fsm_h[b, 4], fs[b], md)
            n = min(ready - emitted[b], cap)
            assert state[b].tolist() == [emitted[b], n, ready if fin else -1, fin], (b, state[b])
            want = TK.frames_window(tok[b], fs[b], emitted[b], n, delays)[0].T
            assert np.array_equal(out[b, :n], want) and (out[b, n:] == CANARY).all(), b
            assert ((out[b, :n] >= 0) & (out[b, :n] < 1024)).all()
            seen[b].append(out[b, :n].copy())
            emitted[b] += n
            assert em[b] == emitted[b]
            recs[b] = state[b].tolist()
        return recs

    r = call_and_check(listed)
    assert r[4] == [0, 0, -1, 0]                                           # running, nothing final yet
    assert (dv["state"].cpu().numpy()[[0, 3]] == -9).all()
    dv["cur"][4] = 1 + md + 10                                             # ten more steps: a backlog of 10 frames
    torch.cuda.synchronize()
    r = call_and_check(listed)
    assert r[4][:3] == [0, min(cap, 10), -1]
    r2 = call_and_check(listed)
    assert r2[4][:3] == [min(cap, 10), min(cap, 10 - min(cap, 10)), -1]
    for _ in range(T):
        r = call_and_check(listed)
        if all(v[0] + v[1] == v[2] or v[1] == 0 for v in r.values()):
            break
    else:
        raise AssertionError("the listed slots never drained")
    r = call_and_check(listed)                                             # drained: every further call is empty
    assert all(v[1] == 0 for v in r.values())
    assert r[1] == [r[1][2], 0, 41 - fs[1] - md, 1] and r[2] == [T - 1 - md, 0, T - 1 - md, 1] and r[4] == [10, 0, -1, 0]
    cfg_like = type("K", (), {"data": type("D", (), {"delay_pattern": delays, "channels": Cn})})
    for b, W in ((1, 41), (2, T), (4, 1 + md + 10)):
        assert np.array_equal(np.concatenate(seen[b]).T[None], TK.codes_for_codec(tok[b, fs[b]: W], cfg_like)), b
    # reset of one slot: it starts over, the others go on
    emit(dv, [1], (B, T, Cn, md), cap, reset=True)
    assert dv["state"].cpu().numpy()[1].tolist() == [0, 0, -1, 0] and dv["emitted"].cpu().numpy().tolist() == [1234, 0] + emitted[2:].tolist()
    emitted[1] = 0
    r = call_and_check(listed)
    assert r[1][:2] == [0, min(cap, 41 - fs[1] - md)] and r[2][1] == 0 and r[4][1] == 0
    # nothing the sampler owns was written
    for k in ("tokens", "fsm", "first_step", "delay"):
        if dv[k] is not None:
            assert np.array_equal(dv[k].cpu().numpy(), host[k]), k
    cur[4] = 1 + md + 10
    assert np.array_equal(dv["cur"].cpu().numpy(), cur)
    assert (dv["state"].cpu().numpy()[[0, 3]] == -9).all() and (dv["out"].cpu().numpy()[[0, 3]] == CANARY).all()


# ---- 4. model level ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mid():
    cfg = C.mid_config()
    sd = synthetic_state_dict(cfg, seed=1234, std=0.02)
    w = DeviceWeights(cfg, sd, torch.device("cuda:0"))
    return cfg, sd, w


def stream_specs(cfg):
    """test_gpu_slots.eight_requests (12..40 steps, an empty text, one of s_cap bytes) with an audio prompt on the third"""
    specs = eight_requests(cfg)
    prompt = np.random.RandomState(5).randint(0, 1024, size=(5, cfg.data.channels)).astype(np.int32)
    specs[2] = spec(TEXTS[2], 123, 27, audio_prompt=prompt)
    return specs


@pytest.fixture(scope="module")
def served(mid):
    """codes_for_codec of serve() on the eight requests, in a fresh session: the reference of every streaming variant"""
    cfg, sd, w = mid
    specs = stream_specs(cfg)
    s = DecodeSession.open(w, 3, s_cap=S_CAP, kv_dtype="f32", max_tokens=40)
    try:
        out = s.serve([request_of(cfg, sp) for sp in specs], poll=8)
    finally:
        s.close()
    return specs, [TK.codes_for_codec(r.codes, cfg) for r in out]


def joined(chunks, n_req, Cn):
    """per request: its chunks joined, after checking contiguous starts and exactly one final chunk, the last one"""
    out = []
    for i in range(n_req):
        mine = [(st, c, f) for ri, st, c, f in chunks if ri == i]
        assert [f for _, _, f in mine] == [False] * (len(mine) - 1) + [True], i
        pos = 0
        for st, c, _ in mine:
            assert st == pos and c.shape[:2] == (1, Cn) and c.dtype == np.int32
            pos += c.shape[-1]
        out.append(np.concatenate([c for _, c, _ in mine], axis=-1))
    return out


@pytest.mark.parametrize("cap,lag", [(16, 1), (16, 0), (3, 1)])
def test_streamed_chunks_join_to_the_served_codes(mid, served, cap, lag):
    cfg, sd, w = mid
    specs, want = served
    assert want[1].shape[-1] == 0 and want[6].shape[-1] == 0               # 12 / 15 steps: no frame at all
    assert max(w_.shape[-1] for w_ in want) > 16
    s = DecodeSession.open(w, 3, s_cap=S_CAP, kv_dtype="f32", max_tokens=40, stream_cap=cap)
    try:
        reqs = [request_of(cfg, sp) for sp in specs]
        chunks = list(s.stream_iter(reqs, chunk=5, lag=lag))
        assert s.free_slots() == [0, 1, 2]
        again = list(s.stream_iter(reqs, chunk=5, lag=lag))               # slots reused over stale caches, counters reset
    finally:
        s.close()
    got = joined(chunks, len(specs), cfg.data.channels)
    for i, (g, w_) in enumerate(zip(got, want)):
        assert g.dtype == w_.dtype and np.array_equal(g, w_), i
    assert sum(1 for ri, *_ in chunks if ri in (1, 6)) == 2                # one empty final chunk each
    assert all(c.shape[-1] <= cap for _, _, c, _ in chunks)
    if cap == 3:
        most = max(w_.shape[-1] for w_ in want)                            # e.g. 23 frames through a 3-frame staging area
        assert max(sum(1 for ri, *_ in chunks if ri == i) for i in range(8)) >= -(-most // 3)
    assert len(again) == len(chunks)
    assert all(a[:2] == b[:2] and a[3] == b[3] and np.array_equal(a[2], b[2]) for a, b in zip(chunks, again))
    if (cap, lag) == (16, 1):
        for i in (0, 2):                                                   # and the oracle's own run of two of them
            r = oracle_of(cfg, sd, specs[i])
            assert np.array_equal(got[i], TK.codes_for_codec(r.codes, cfg)), i


def test_a_session_without_stream_cap_has_no_streaming_buffers(mid):
    cfg, sd, w = mid
    s = DecodeSession.open(w, 1, s_cap=S_CAP, kv_dtype="f32", max_tokens=16)
    try:
        assert s.stream_cap is None and not hasattr(s, "emit_out") and not hasattr(s, "_emit_side")
        with pytest.raises(hb.DiaHipError):
            list(s.stream_iter([request_of(cfg, spec(TEXTS[1], 1, 12))]))
    finally:
        s.close()


# ---- 5. cancel -----------------------------------------------------------------------------------------------------
def test_cancel_leaves_the_other_requests_alone(mid, served):
    cfg, sd, w = mid
    specs, want = served
    pick = [0, 4, 7]                                                       # 40, 33 and 22 steps
    s = DecodeSession.open(w, 2, s_cap=S_CAP, kv_dtype="f32", max_tokens=40, stream_cap=16)
    try:
        chunks, cancelled_at = [], None
        for ch in s.stream_iter([request_of(cfg, specs[i]) for i in pick], chunk=5, lag=1):
            chunks.append(ch)
            if ch[0] == 0 and ch[2].shape[-1] and cancelled_at is None:
                cancelled_at = len(chunks)
                s.cancel(0)
        assert s.free_slots() == [0, 1]
    finally:
        s.close()
    assert cancelled_at is not None and not any(ri == 0 for ri, *_ in chunks[cancelled_at:])
    for j in (1, 2):
        mine = [c for c in chunks if c[0] == j]
        assert [c[3] for c in mine] == [False] * (len(mine) - 1) + [True]
        assert np.array_equal(np.concatenate([c[2] for c in mine], axis=-1), want[pick[j]]), j


# ---- 6. the public surface -----------------------------------------------------------------------------------------
def test_dia_stream_frames_and_cli(mid, tmp_path):
    cfg, sd, w = mid
    dia = Dia.from_state_dict(cfg, sd, "float32", torch.device("cuda:0"))
    texts, seeds = [TEXTS[0], TEXTS[1]], [42, 7]
    want = dia.generate_batch(texts, max_tokens=36, seeds=seeds, slots=2)
    chunks = list(dia.stream_frames(texts, 2, max_tokens=36, seeds=seeds, chunk=4))
    got = joined(chunks, 2, cfg.data.channels)
    assert want[0].shape[-1] > 4
    for g, w_ in zip(got, want):
        assert np.array_equal(g, w_)
    assert max(c.shape[-1] for _, _, c, _ in chunks) <= 4 and len(chunks) >= 4
    # the CLI, in this process, on the same synthetic model: the file with --stream-chunk is the file without it
    import cli
    mdir = tmp_path / "model"
    mdir.mkdir()
    torch.save(sd, mdir / "pytorch_model.bin")
    cfg.save(mdir / "config.json")
    base = [TEXTS[1], "--no-dac", "--model-path", str(mdir), "--compute-dtype", "float32", "--max-tokens", "30", "--seed", "3"]
    a, b = tmp_path / "plain.npy", tmp_path / "streamed.npy"
    assert cli.main(base + ["--codes-output", str(a)]) == 0
    assert cli.main(base + ["--codes-output", str(b), "--stream-chunk", "4", "--verbose"]) == 0
    assert a.read_bytes() == b.read_bytes() and np.load(a).shape[-1] > 0
    assert not (tmp_path / "streamed.npy.frames").exists()
