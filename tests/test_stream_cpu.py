"""Frame streaming without a GPU: the finality rule of dia_hip/tokens.py (ready_frames / frames_window) against codes_for_codec and
against the oracle's token loop step by step, the ABI and argument validation of dia_emit_frames through the library (which loads
without a device), and the driver loop DecodeSession.stream_iter over a simulated device that follows the same rule."""
import ctypes
import os
import subprocess
import tempfile
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from dia_hip import binding as hb
from dia_hip import config as CF
from dia_hip import tokens as TK
from oracle import dia_oracle as O
from test_slots_cpu import FakeSession, req

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIA_DELAYS = [0, 8, 9, 10, 11, 12, 13, 14, 15]


def shape_cfg(delays):
    return SimpleNamespace(data=SimpleNamespace(delay_pattern=list(delays), channels=len(delays)))


# ---- 1. the finality rule ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("delays,T", [(DIA_DELAYS, 40), ([0, 1, 3], 12)])
def test_windows_over_any_partition_equal_codes_for_codec(delays, T):
    assert list(CF.mid_config().data.delay_pattern) == DIA_DELAYS
    cfg, md, C = shape_cfg(delays), max(delays), len(delays)
    rs = np.random.RandomState(3)
    tok = rs.randint(-1, 1027, size=(T, C)).astype(np.int32)               # -1, EOS, PAD, BOS occur
    for fs in (1, 6):
        for W in range(fs, T + 1):
            want = TK.codes_for_codec(tok[fs:W], cfg)
            ready = TK.ready_frames(W, False, 0, fs, md)
            assert ready == TK.ready_frames(3, True, W - 1, fs, md) == want.shape[-1] == max(0, W - fs - md)
            cuts = [list(range(ready + 1)), [0, ready], sorted({0, ready} | set(rs.randint(0, ready + 1, size=3).tolist()))]
            for cut in cuts:
                parts = [TK.frames_window(tok, fs, a, b - a, delays) for a, b in zip(cut[:-1], cut[1:])]
                got = np.concatenate(parts, axis=-1) if parts else TK.frames_window(tok, fs, 0, 0, delays)
                assert got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got, want), (fs, W, cut)


@pytest.mark.parametrize("ending", ["eos", "max_tokens"])
@pytest.mark.parametrize("fs", [1, 6])
def test_ready_frames_along_the_oracle_token_loop(ending, fs):
    """the (cur, fsm) trajectory the sampler leaves on the device, replayed from oracle.token_loop: ready is monotone, never
    above the final frame count, and every frame below it already has its final value"""
    cfg = CF.mid_config()
    dm = O.Dims.of(cfg)
    md, mt = max(dm.delay), 44
    rs = np.random.RandomState(11)
    prompt = rs.randint(0, 1024, size=(fs - 1, dm.C)).astype(np.int32) if fs > 1 else None
    prefill, first = O.delayed_prefill(dm, prompt)
    assert first == fs
    tok = np.full((dm.T, dm.C), -1, dtype=np.int32)
    tok[: prefill.shape[0]] = prefill
    g = torch.Generator().manual_seed(5)

    def step_logits(row, cur):
        lg = torch.randn(2, dm.C, dm.tgt_vocab, generator=g)
        lg[:, :, 1024:] = -50.0
        if ending == "eos" and cur == fs + 9:
            lg[1, 0, dm.eos] = 100.0
        return lg

    traj = []                                                              # (device cur, finished, last, token buffer) after each step
    for s in O.token_loop(dm, tok, fs, mt, step_logits, cfg_scale=3.0, temperature=0.0, top_p=0.95, top_k=35,
                          ignore_eos=ending != "eos"):
        traj.append((s.cur if s.finished else s.cur + 1, s.finished, s.last_step, tok.copy()))
    cur, fin, last, _ = traj[-1]
    # (at max_tokens the loop starts the end-of-stream countdown itself, max_delay + 1 steps before the buffer's end)
    assert fin and (last == mt - 2 if ending == "max_tokens" else fs + 9 < last < mt - 2)
    final = TK.codes_for_codec(tok[fs: last + 1], cfg)
    total = final.shape[-1]
    assert total > 0 and TK.ready_frames(cur, fin, last, fs, md) == total
    prev = 0
    for cur, fin, last, snap in traj:
        ready = TK.ready_frames(cur, fin, last, fs, md)
        assert prev <= ready <= total
        assert np.array_equal(TK.frames_window(snap, fs, 0, ready, dm.delay), final[:, :, :ready])
        prev = ready


# ---- 2. the library, without a device ------------------------------------------------------------------------------
def test_emit_frames_is_exported_and_the_struct_matches_the_header():
    assert "dia_emit_frames" in hb.EXPORTS and hasattr(hb.lib(), "dia_emit_frames")
    prog = ('#include <stdio.h>\n#include "dia_hip.h"\nint main(void){ printf("%zu %d %d\\n", sizeof(dia_emit_args), DIA_EMIT_RESET, '
            'DIA_ABI_VERSION); return 0; }\n')
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "s.c")
        open(c, "w").write(prog)
        exe = os.path.join(td, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        size, reset, abi = (int(v) for v in subprocess.check_output([exe]).split())
    assert size == ctypes.sizeof(hb.EmitArgs) and reset == hb.EMIT_RESET and abi == hb.ABI_VERSION == 8


def emit_args(slots=(0,), B=4, T=64, Cn=9, md=15, cap=8, flags=0, **kw):
    """a complete dia_emit_args whose device pointers are never dereferenced: every case is refused before a launch"""
    buf = ctypes.create_string_buffer(64)
    addr = ctypes.addressof(buf)
    a = hb.EmitArgs()
    a.B, a.T, a.C, a.max_delay, a.codebook_size, a.cap, a.n, a.flags = B, T, Cn, md, 1024, cap, len(slots), flags
    a.slot = (ctypes.c_int32 * max(len(slots), 1))(*slots)
    for f in ("tokens", "cur", "fsm", "first_step", "delay", "emitted", "out", "state"):
        setattr(a, f, addr)
    for k, v in kw.items():
        setattr(a, k, v)
    a._keep = buf
    return a


def test_emit_frames_validation_without_gpu():
    L = hb.lib()

    def refused(a, word):
        assert L.dia_emit_frames(ctypes.byref(a), None) == -1              # DIA_E_ARG
        assert word in L.dia_last_error().decode(), (word, L.dia_last_error())

    refused(hb.EmitArgs(), "null")
    assert L.dia_emit_frames(None, None) == -1
    for f in ("tokens", "cur", "fsm", "delay", "emitted", "out", "state"):
        refused(emit_args(**{f: None}), "null")
    a = emit_args()
    a.slot = None
    refused(a, "null")
    for f in ("emitted", "state"):
        refused(emit_args(flags=hb.EMIT_RESET, **{f: None}), "null")
    refused(emit_args(n=0), "n must be")
    refused(emit_args(slots=tuple(range(hb.SLOTS_PER_CALL)), B=128, n=hb.SLOTS_PER_CALL + 1), "n must be")
    refused(emit_args(slots=(4,)), "slot 4 outside")
    refused(emit_args(slots=(-1,)), "outside")
    refused(emit_args(slots=(1, 2, 1)), "slot 1 listed twice")
    refused(emit_args(slots=(1, 2, 1), flags=hb.EMIT_RESET), "listed twice")
    refused(emit_args(Cn=0), "C = 0")
    refused(emit_args(Cn=17), "C = 17")
    refused(emit_args(cap=0), "cap = 0")
    refused(emit_args(md=-1), "max_delay = -1")
    refused(emit_args(md=64), "max_delay = 64")
    refused(emit_args(flags=2), "flags")


# ---- 3. the driver loop over a simulated device --------------------------------------------------------------------
def fake_row(seed, row, C):
    """what the simulated sampler writes into token row `row` of the request with this seed: ids in [-1, 1027)"""
    return ((seed * 7919 + row * 104729 + np.arange(C) * 1299709) % 1028 - 1).astype(np.int32)


class FakeStream(FakeSession):
    """FakeSession + a host model of dia_emit_frames (the rule of dia_hip/tokens.py) and of the two pinned copies"""

    def __init__(self, slots, cap, **kw):
        super().__init__(slots, **kw)
        self.stream_cap = cap
        self._owner, self._queue = {}, []
        self.tok_h = np.full((slots, self.T, self.C), -1, dtype=np.int32)
        self.fs_h = np.ones(slots, dtype=np.int32)
        self.emitted_h = np.zeros(slots, dtype=np.int32)
        self.out_h = np.full((slots, cap, self.C), -7, dtype=np.int32)
        self.state_h = np.array([[0, 0, -1, 0]] * slots, dtype=np.int32)
        # like the pinned pairs: two buffers that live as long as the session and are overwritten in place
        self.snap = [(np.zeros_like(self.out_h), np.zeros_like(self.state_h)) for _ in range(2)]
        self.delay = list(self.cfg.data.delay_pattern)

    def _ensure_slot_noise(self, n_steps):
        pass

    def _enqueue_admit(self, pairs, pre):
        super()._enqueue_admit(pairs, pre)
        for (b, _), (rows, pstep) in zip(pairs, pre):
            self.tok_h[b] = -1
            self.tok_h[b, : rows.shape[0]] = rows
            self.fs_h[b] = pstep

    def _enqueue_steps(self, n, use_graph):
        for _ in range(n):
            for b, sl in self._live.items():
                if not self.fsm_h[b, 3] and self.cur_h[b] >= self.fs_h[b]:
                    self.tok_h[b, self.cur_h[b]] = fake_row(sl["req"].seed, int(self.cur_h[b]), self.C)
            super()._enqueue_steps(1, use_graph)
        self.log[-n:] = [("steps", n)]

    def _enqueue_emit(self, slots, reset=False):
        self.log.append(("reset" if reset else "emit", list(slots)))
        for b in slots:
            if reset:
                self.emitted_h[b], self.state_h[b] = 0, [0, 0, -1, 0]
                continue
            fin = int(self.fsm_h[b, 3])
            ready = TK.ready_frames(self.cur_h[b], fin, self.fsm_h[b, 4], self.fs_h[b], self.max_delay)
            em = int(self.emitted_h[b])
            n = min(ready - em, self.stream_cap)
            self.out_h[b, :n] = TK.frames_window(self.tok_h[b], self.fs_h[b], em, n, self.delay)[0].T
            self.state_h[b] = [em, n, ready if fin else -1, fin]
            self.emitted_h[b] = em + n

    def _enqueue_fetch(self, k):
        self.log.append(("fetch", k))
        self.snap[k % 2][0][...] = self.out_h
        self.snap[k % 2][1][...] = self.state_h

    def _wait_fetch(self, k):
        self.log.append(("wait", k))
        return self.snap[k % 2]

    def sync(self):
        pass

    def _raise_if_invalid(self):
        pass


def expected_codes(s, r):
    """codes_for_codec of the simulated utterance of request r: it ends at its max_tokens - 1'th step"""
    from dia_hip.tokens import delayed_prefill
    pre, fs = delayed_prefill(s.cfg, r.audio_prompt)
    tok = np.full((s.T, s.C), -1, dtype=np.int32)
    tok[: pre.shape[0]] = pre
    for row in range(fs, r.max_tokens):
        tok[row] = fake_row(r.seed, row, s.C)
    return TK.codes_for_codec(tok[fs: r.max_tokens], s.cfg)


def joined(chunks, n_req, C):
    """per request: its chunks joined, after checking contiguous starts and exactly one final chunk, the last one"""
    out = []
    for i in range(n_req):
        mine = [(st, c, f) for ri, st, c, f in chunks if ri == i]
        assert [f for _, _, f in mine] == [False] * (len(mine) - 1) + [True], i
        pos = 0
        for st, c, _ in mine:
            assert st == pos and c.shape[:2] == (1, C) and c.dtype == np.int32
            pos += c.shape[-1]
        out.append(np.concatenate([c for _, c, _ in mine], axis=-1))
    return out


MTS = [40, 12, 27, 19, 33, 40, 15, 22]


def stream_requests(s):
    prompt = np.random.RandomState(5).randint(0, 1024, size=(5, s.C)).astype(np.int32)
    return [req(100 + i, m, audio_prompt=prompt if i == 2 else None) for i, m in enumerate(MTS)]


@pytest.mark.parametrize("cap,lag", [(16, 1), (16, 0), (3, 1), (1, 0)])
def test_stream_iter_hands_out_every_frame_once(cap, lag):
    s = FakeStream(3, cap)
    reqs = stream_requests(s)
    chunks = list(s.stream_iter(reqs, chunk=5, lag=lag))
    got = joined(chunks, len(reqs), s.C)
    for i, r in enumerate(reqs):
        assert np.array_equal(got[i], expected_codes(s, s._as_request(r))), i
    assert got[1].shape[-1] == 0 and got[6].shape[-1] == 0                 # 12 and 15 steps: no frame, one empty final chunk
    assert sum(1 for ri, *_ in chunks if ri in (1, 6)) == 2
    assert all(c.shape[-1] <= cap for _, _, c, _ in chunks)
    assert s.free_slots() == [0, 1, 2] and s._parked == {0, 1, 2} and not s._owner
    assert not any(w == "collect" for w, _ in s.log)                       # nothing is downloaded per utterance
    # a reset follows every admission, for the same slots, before anything else is enqueued
    for j, (w, a) in enumerate(s.log):
        if w == "admit":
            assert s.log[j + 1] == ("reset", a)
    # the host waits for iteration k only after iteration k + lag was enqueued, while slots were live
    fetched = -1
    for w, a in s.log:
        if w == "fetch":
            fetched = a
        elif w == "wait":
            assert a <= fetched - lag or a == fetched
    assert all(1 <= a <= 5 for w, a in s.log if w == "steps")
    # a second run on the same session gives the same chunks
    again = list(s.stream_iter(reqs, chunk=5, lag=lag))
    assert len(again) == len(chunks)
    assert all(np.array_equal(a[2], b[2]) and a[:2] == b[:2] and a[3] == b[3] for a, b in zip(chunks, again))


def test_one_request_gives_the_same_chunks_at_lag_0_and_1():
    runs = []
    for lag in (0, 1):
        s = FakeStream(1, 64)
        runs.append(list(s.stream_iter([req(7, 60)], chunk=16, lag=lag)))
    assert len(runs[0]) == len(runs[1]) >= 3
    for a, b in zip(*runs):
        assert a[:2] == b[:2] and a[3] == b[3] and np.array_equal(a[2], b[2])


def test_a_backlog_is_drained_without_decode_steps():
    s = FakeStream(1, 2)
    chunks = list(s.stream_iter([req(7, 40)], chunk=8, lag=1))
    assert np.array_equal(joined(chunks, 1, s.C)[0], expected_codes(s, s._as_request(req(7, 40))))
    assert sum(a for w, a in s.log if w == "steps") == 39                   # the utterance's own steps, none while draining
    assert sum(1 for w, _ in s.log if w == "emit") > 39 // 8 + 1


def test_cancel_frees_the_slot_and_silences_the_request():
    s = FakeStream(2, 16)
    reqs = [req(1, 60), req(2, 40), req(3, 30)]
    it = s.stream_iter(reqs, chunk=5, lag=1)
    chunks, cancelled_at = [], None
    for ch in it:
        chunks.append(ch)
        if ch[0] == 0 and ch[2].shape[-1] and cancelled_at is None:
            cancelled_at = len(chunks)
            s.cancel(0)
    assert cancelled_at is not None and not any(ri == 0 for ri, *_ in chunks[cancelled_at:])
    for i in (1, 2):
        mine = [c for c in chunks if c[0] == i]
        assert np.array_equal(np.concatenate([c[2] for c in mine], axis=-1), expected_codes(s, s._as_request(reqs[i])))
        assert [c[3] for c in mine] == [False] * (len(mine) - 1) + [True]
    assert s.free_slots() == [0, 1] and s._parked == {0, 1}
    # a request cancelled while it waits in the queue is never admitted
    s2 = FakeStream(1, 16)
    it = s2.stream_iter(reqs, chunk=5, lag=0)
    first = next(it)
    s2.cancel(1)
    rest = [first] + list(it)
    assert {ri for ri, *_ in rest} == {0, 2}


def test_stream_iter_needs_streaming_buffers_and_a_known_lag():
    with pytest.raises(hb.DiaHipError):
        list(FakeSession(1).stream_iter([req(1, 10)]))
    with pytest.raises(ValueError):
        list(FakeStream(1, 4).stream_iter([req(1, 10)], lag=2))
    with pytest.raises(ValueError):
        list(FakeStream(1, 4).stream_iter([req(1, 10), req(2, 1)]))          # a bad request: before anything is enqueued


def test_cli_stream_chunk_flag():
    import cli
    p = cli.build_parser()
    assert p.parse_args(["x", "--codes-output", "o.npy"]).stream_chunk == 0
    assert p.parse_args(["x", "--stream-chunk", "4", "--codes-output", "o.npy"]).stream_chunk == 4
    for argv in (["x", "--stream-chunk", "4", "--output", "o.wav"], ["x", "--stream-chunk", "-1", "--codes-output", "o.npy"],
                 ["x", "--stream-chunk", "4", "--codes-output", "o.npy", "--audio-prompt", "p.npy", "--audio-prompt-text", "t"]):
        with pytest.raises(SystemExit):
            cli.main(argv)
