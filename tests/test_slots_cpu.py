"""Continuous batching without a GPU: the slot scheduler of DecodeSession with the device calls stubbed, the per-slot noise
bookkeeping, and the argument validation of dia_slot_admit / dia_slot_retire through the library (which loads without a
device, as test_abi.test_argument_validation_without_gpu does for the older entry points)."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from dia_hip import binding as hb
from dia_hip import config as CF
from dia_hip.engine import DecodeSession, Request

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class FakeSession(DecodeSession):
    """The host side of a slotted session over a simulated device: a slot finishes at its max_tokens - 1'th step (or after
    `ends[request seed]` steps when given), nothing else is computed."""

    def __init__(self, slots, s_cap=64, max_tokens=None, ends=None):
        cfg = CF.tiny_config() if hasattr(CF, "tiny_config") else CF.mid_config()
        self.cfg, self.dev = cfg, torch.device("cpu")
        da = cfg.data
        self.B, self.T, self.C, self.V = slots, da.audio_length, da.channels, cfg.model.tgt_vocab_size
        self.max_tokens = self.T if max_tokens is None else max_tokens
        self.max_delay = max(da.delay_pattern)
        self.S = s_cap
        self.noise_steps = self.max_tokens - 1
        self.noise = torch.zeros(slots, self.noise_steps, self.C, self.V)
        self.sample_params = dict(cfg_scale=3.0, temperature=1.3, top_p=0.95, top_k=35)
        self.lens, self.first_steps = [0] * slots, [1] * slots
        self._issued, self._pinned, self.slotted, self.prefilled, self.seg = 0, [], True, True, False
        self._init_slots()
        self.cur_h = np.ones(slots, dtype=np.int32)
        self.fsm_h = self.fsm.numpy().copy()
        self.ends = ends or {}
        self.log = []                      # ("admit", slots) / ("collect", [slot]) / ("retire", slots) / ("steps", n)
        self.uploads = []                  # (slot, first row, rows)

    def _enqueue_admit(self, pairs, pre):
        self.log.append(("admit", [b for b, _ in pairs]))
        for b, _ in pairs:
            self.cur_h[b] = 1
            self.fsm_h[b] = [0, -1, self.max_delay, 0, 0, 0, 0, 0]

    def _enqueue_retire(self, part):
        self.log.append(("retire", list(part)))
        for b in part:
            self.fsm_h[b, 3], self.cur_h[b] = 1, 1

    def _enqueue_steps(self, n, use_graph):
        self.log.append(("steps", n))
        for _ in range(n):
            for b, sl in self._live.items():
                if self.fsm_h[b, 3]:
                    continue
                last_step = self.ends.get(sl["req"].seed, sl["req"].max_tokens - 1)
                if self.cur_h[b] >= last_step:
                    self.fsm_h[b, 3], self.fsm_h[b, 4] = 1, self.cur_h[b]
                else:
                    self.cur_h[b] += 1

    def _upload_noise(self, b, r0, rows):
        self.uploads.append((b, r0, rows.shape[0]))
        self.noise[b, r0: r0 + rows.shape[0]] = rows

    def _read_state(self):
        return self.fsm_h.copy(), self.cur_h.copy()

    def _read_slot(self, b):
        tok = np.full((self.T, self.C), -1, dtype=np.int32)
        return tok, tok.copy()

    def collect(self, b):
        self.log.append(("collect", [b]))
        return super().collect(b)

    def close(self):
        pass


def req(seed, mt, n_text=5, **kw):
    return Request(np.arange(n_text, dtype=np.int32) % 200 + 1, seed=seed, max_tokens=mt, **kw)


def test_serve_keeps_request_order_and_never_admits_a_live_slot():
    s = FakeSession(3)
    mts = [12, 40, 19, 33, 12, 25, 40, 14]
    out = s.serve([req(100 + i, m) for i, m in enumerate(mts)], poll=8)
    assert [r.last_step for r in out] == [m - 1 for m in mts]              # request i's result at position i
    live = set()
    admitted = 0
    for what, arg in s.log:
        if what == "admit":
            assert not (live & set(arg)), (live, arg)                      # never into a slot that was not collected
            live |= set(arg)
            admitted += len(arg)
        elif what == "collect":
            live -= set(arg)
        elif what == "retire":
            assert not (live & set(arg))                                   # only empty slots are parked
        elif what == "steps":
            assert 1 <= arg <= 8
    assert admitted == len(mts)
    assert s.free_slots() == [0, 1, 2] and s._parked == {0, 1, 2}          # all parked at the end
    # slots were refilled while others were still running: fewer steps than three closed batches run to their longest member
    steps = sum(a for w_, a in s.log if w_ == "steps")
    assert steps < (40 - 1) + (33 - 1) + (40 - 1)


def test_serve_iter_yields_as_utterances_finish():
    s = FakeSession(2)
    order = [i for i, _ in s.serve_iter([req(1, 40), req(2, 10), req(3, 10)], poll=4)]
    assert order == [1, 2, 0]


def test_admit_twice_and_retire_live_are_refused():
    s = FakeSession(2)
    assert s.admit([req(1, 10)]) == [0]
    assert s.admit([req(2, 10)]) == [1]
    with pytest.raises(hb.DiaHipError):
        s.admit([req(3, 10)])                                              # no free slot
    with pytest.raises(hb.DiaHipError):
        s._admit([(0, s._as_request(req(3, 10)))])                         # slot 0 has not been collected
    with pytest.raises(hb.DiaHipError):
        s.retire([0])
    s.decode(9)
    assert s.finished() == [0, 1]
    assert s.collect(0).last_step == 9
    assert s.free_slots() == [0]
    s.retire([0])
    assert 0 in s._parked


def test_bad_requests_raise_before_anything_is_enqueued():
    s = FakeSession(2, s_cap=64, max_tokens=48)
    good = req(1, 20)
    for bad in (req(2, 20, n_text=65), req(2, 1), req(2, s.T + 1), req(2, 49),
                req(2, 20, audio_prompt=np.zeros((3, s.C + 1), dtype=np.int32))):
        with pytest.raises(ValueError):
            s.serve([good, bad])
        with pytest.raises(ValueError):
            s.admit([good, bad])
    assert s.log == [] and s._live == {}
    assert len(s.serve([req(3, 20, n_text=64), req(4, 2), req(5, 48)])) == 3


def test_slot_noise_restarts_with_every_admission():
    s = FakeSession(2, max_tokens=40)
    n = 11

    def fresh(seed, rows):
        g = torch.Generator().manual_seed(seed)
        return torch.empty(rows, s.C, s.V).exponential_(1.0, generator=g)

    s.admit([req(42, 30), req(7, 30, temperature=0.0)])
    s.decode(4)
    s.decode(n - 4)
    assert torch.equal(s.noise[0, :n], fresh(42, n))                       # drawn in two pieces == one fresh generator's first n
    assert all(b == 0 for b, _, _ in s.uploads)                            # the greedy slot draws nothing
    s.decode(40)                                                           # more steps than the request has: capped at max_tokens - 1 rows
    assert s._live[0]["rows"] == 29
    for b in s.finished():
        s.collect(b)
    # the same slot again, another seed, admitted while the session's step counter stands at 51: row 0 is ITS first draw
    s.uploads.clear()
    assert s.admit([req(123, 20)]) == [0]
    s.decode(n)
    assert s.uploads[0][:2] == (0, 0)
    assert torch.equal(s.noise[0, :n], fresh(123, n))
    # a slot admitted later than its neighbour keeps its own row count
    assert s.admit([req(9, 20)]) == [1]
    s.decode(3)
    assert s._live[0]["rows"] == n + 3 and s._live[1]["rows"] == 3
    assert torch.equal(s.noise[1, :3], fresh(9, 3))


# ---- the library, without a device ---------------------------------------------------------------------------------
def test_abi_tails_of_the_slot_feature():
    assert [f[0] for f in hb.EmbedArgs._fields_][-3:] == ["slots", "n_slots", "_pad0"]
    assert [f[0] for f in hb.SampleArgs._fields_][-6:] == ["embed", "slot_cfg_scale", "slot_temperature", "slot_top_p", "slot_top_k",
                                                           "slot_max_tokens"]
    prog = '#include <stdio.h>\n#include "dia_hip.h"\nint main(void){ printf("%zu %d\\n", sizeof(dia_slot_admit_args), DIA_SLOTS_PER_CALL); return 0; }\n'
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "s.c")
        open(c, "w").write(prog)
        exe = os.path.join(td, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        size, per_call = (int(v) for v in subprocess.check_output([exe]).split())
    assert size == ctypes.sizeof(hb.SlotAdmitArgs) and per_call == hb.SLOTS_PER_CALL


def slot_args(n=1, B=4, T=64, Cn=9, S=32, **kw):
    """a complete dia_slot_admit_args whose device pointers are never dereferenced: every case is refused before a launch"""
    buf = ctypes.create_string_buffer(64)
    addr = ctypes.addressof(buf)
    a = hb.SlotAdmitArgs()
    a.B, a.T, a.C, a.S, a.max_delay, a.n = B, T, Cn, S, 15, n
    host = dict(slot=[0] * n, text_len=[8] * n, first_step=[1] * n, prefix_rows=[16] * n, max_tokens=[32] * n, top_k=[35] * n,
                cfg_scale=[3.0] * n, temperature=[1.3] * n, top_p=[0.95] * n)
    host["slot"] = list(range(n))
    keep = [buf]
    for k, v in host.items():
        v = kw.pop(k, v)
        if v is None:
            continue
        arr = ((ctypes.c_float if k in ("cfg_scale", "temperature", "top_p") else ctypes.c_int32) * len(v))(*v)
        keep.append(arr)
        setattr(a, k, arr)
    a.prefix_ld = 16
    for k in ("prefix", "tokens", "pred", "cur", "fsm", "d_first_step", "d_text_len", "slot_cfg_scale", "slot_temperature",
              "slot_top_p", "slot_top_k", "slot_max_tokens"):
        setattr(a, k, addr)
    for k, v in kw.items():
        setattr(a, k, v)
    return a, keep


def test_slot_admit_and_retire_validate_their_arguments_without_a_gpu():
    L = hb.lib()
    assert L.dia_slot_admit(None, None) == -1 and b"null" in L.dia_last_error()
    assert L.dia_slot_retire(None, None) == -1 and b"null" in L.dia_last_error()
    empty = hb.SlotAdmitArgs()
    assert L.dia_slot_admit(ctypes.byref(empty), None) == -1 and b"null" in L.dia_last_error()
    assert L.dia_slot_retire(ctypes.byref(empty), None) == -1 and b"null" in L.dia_last_error()
    cases = [
        (dict(tokens=None), b"null"), (dict(prefix=None), b"null"), (dict(temperature=None), b"null"), (dict(slot_top_k=None), b"null"),
        (dict(slot=[4]), b"slot 4"), (dict(slot=[-1]), b"slot -1"), (dict(n=2, slot=[1, 1]), b"twice"),
        (dict(text_len=[33]), b"text_len 33"), (dict(text_len=[-1]), b"text_len"),
        (dict(max_tokens=[1]), b"max_tokens 1"), (dict(max_tokens=[65]), b"max_tokens 65"),
        (dict(first_step=[0]), b"first_step 0"), (dict(first_step=[65]), b"first_step 65"),
        (dict(prefix_rows=[17]), b"prefix_rows"), (dict(prefix_rows=[0]), b"prefix_rows"), (dict(top_k=[-2]), b"top_k"),
        (dict(n=0), b"n must be"), (dict(n=5, slot=[0, 1, 2, 3, 0]), b"n must be"), (dict(Cn=17), b"shape"),
    ]
    for kw, word in cases:
        n = kw.pop("n", 1)
        if n == 0:
            a, keep = slot_args(1, **kw)
            a.n = 0
        else:
            a, keep = slot_args(n, **kw)
        rc = L.dia_slot_admit(ctypes.byref(a), None)
        msg = L.dia_last_error()
        assert rc == -1 and b"dia_slot_admit" in msg and word in msg, (kw, rc, msg)
    for kw, word in ((dict(slot=[4]), b"slot 4"), (dict(cur=None), b"null"), (dict(d_text_len=None), b"null")):
        a, keep = slot_args(1, **kw)
        rc = L.dia_slot_retire(ctypes.byref(a), None)
        msg = L.dia_last_error()
        assert rc == -1 and b"dia_slot_retire" in msg and word in msg, (kw, rc, msg)


def test_sample_and_embed_validate_the_slot_tails_without_a_gpu():
    L = hb.lib()
    buf = ctypes.create_string_buffer(64)
    addr = ctypes.addressof(buf)
    s = hb.SampleArgs()
    for k in ("logits", "tokens", "pred", "cur", "fsm", "delay", "noise", "first_step"):
        setattr(s, k, addr)
    s.B, s.T, s.C, s.V, s.max_tokens, s.noise_steps, s.temperature = 2, 64, 9, 1028, 32, 31, 1.0
    s.slot_cfg_scale = addr                                                # one of five
    assert L.dia_sample(ctypes.byref(s), None) == -1 and b"all five or none" in L.dia_last_error()
    s.slot_temperature = s.slot_top_p = s.slot_top_k = s.slot_max_tokens = addr
    s.noise = None
    assert L.dia_sample(ctypes.byref(s), None) == -1 and b"noise" in L.dia_last_error()
    s.noise, s.first_step = addr, None
    assert L.dia_sample(ctypes.byref(s), None) == -1 and b"first_step" in L.dia_last_error()
    e = hb.EmbedArgs()
    for k in ("tokens", "cur", "emb", "x", "P", "ssq", "slots"):
        setattr(e, k, addr)
    e.B, e.T, e.C, e.V, e.D, e.p_ktiles = 2, 64, 9, 1028, 64, 2
    for n in (0, 3):
        e.n_slots = n
        assert L.dia_embed_tokens(ctypes.byref(e), None) == -1 and b"n_slots" in L.dia_last_error()


def test_sample_refuses_channel_counts_whose_scratch_exceeds_a_cu():
    """k_sample keeps 3 * 1088 floats of LDS per channel: 13 channels are 169 728 bytes against the 160 KiB of a CU.  The call
    is refused with a message that says so, before any launch (no device here); 12 channels pass this check."""
    L = hb.lib()
    buf = ctypes.create_string_buffer(64)
    addr = ctypes.addressof(buf)
    s = hb.SampleArgs()
    for k in ("logits", "tokens", "pred", "cur", "fsm", "delay"):
        setattr(s, k, addr)
    s.B, s.T, s.V, s.max_tokens = 1, 64, 1028, 65                          # max_tokens > T: the last of dia_sample's checks
    for c in (13, 14, 16):
        s.C = c
        assert L.dia_sample(ctypes.byref(s), None) == -1
        msg = L.dia_last_error()
        assert b"channels > 12" in msg and b"LDS" in msg, msg
    for c, word in ((17, b"channels > 12"), (0, b"an empty shape")):             # in this order: the shape, then the channel bound
        s.C = c
        assert L.dia_sample(ctypes.byref(s), None) == -1
        msg = L.dia_last_error()
        assert word in msg, (c, msg)
    s.C = 12
    assert L.dia_sample(ctypes.byref(s), None) == -1 and b"max_tokens out of range" in L.dia_last_error()
