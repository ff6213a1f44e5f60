"""The prompt prefill onto FP8 self caches and at slot admission, the parts that need no GPU (DESIGN.md "Prompt prefill at
admission and onto fp8 caches"): the two entry points in the header and the binding with the ABI version where it was, every
refusal of dia_dec_prefill_kv_fp8 / dia_dec_prefill_attn_fp8 through the C ABI (dummy pointers, never dereferenced), the
prompt_prefill="batched" checks of DecodeSession / DecodeSession.open (they run before anything touches a device), the keyword's
way through Dia and cli.py, and the step accounting of a prefilled slot on the simulated device of tests/test_slots_cpu.py."""
import ctypes
import inspect
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from dia_hip import binding as hb
from dia_hip import config as CF
from dia_hip.engine import DecodeSession, Request

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("dia_dec_prefill_kv_fp8", "dia_dec_prefill_attn_fp8")


def test_header_declares_the_entries_and_the_binding_resolves_them():
    h = open(os.path.join(ROOT, "include", "dia_hip.h")).read()
    for name in ENTRIES:
        assert re.search(r"int %s\s*\(const dia_dec_prefill_args\* a, const dia_kv_fp8_ptrs\* p, void\* stream\);" % name, h), name
        assert name in hb.EXPORTS and getattr(hb.lib(), name) is not None
    assert re.search(r"#define DIA_ABI_VERSION 8\b", h)
    assert hb.ABI_VERSION == 8 and hb.lib().dia_abi_version() == 8
    # no struct grew
    assert ctypes.sizeof(hb.KvFp8Ptrs) == 32 and ctypes.sizeof(hb.AttnArgs) == 168 and ctypes.sizeof(hb.EngineDesc) == 584
    assert [f[0] for f in hb.DecPrefillArgs._fields_][-3:] == ["cos_t", "sin_t", "text_len"]


def test_one_definition_of_the_quantisation_rule():
    """attn.hip and prefill.hip share kv_fp8.hpp: a prompted key is quantised by the code that quantises a generated one"""
    src = lambda n: open(os.path.join(ROOT, "dia-tts-prune_amd", "csrc", n)).read()
    shared = src("kv_fp8.hpp")
    for fn in ("e4m3_rne", "e4m3_finite", "kv_scale_bits_f32", "wave_umax", "expand_e4m3"):
        define = re.compile(r"__device__ __forceinline__ \w+ %s\(" % fn)
        assert len(define.findall(shared)) == 1, fn
        for unit in ("attn.hip", "prefill.hip"):
            assert not define.search(src(unit)), (fn, unit)
            assert '#include "kv_fp8.hpp"' in src(unit), unit
    for fn in ("e4m3_finite", "kv_scale_bits_f32", "wave_umax", "expand_e4m3"):      # (e4m3_rne: through e4m3_finite)
        assert fn + "(" in src("attn.hip") and fn + "(" in src("prefill.hip"), fn


@pytest.mark.parametrize("entry", ENTRIES)
def test_refusals_without_a_device(entry):
    L = hb.lib()
    fn = getattr(L, entry)
    buf = ctypes.create_string_buffer(256)           # never dereferenced: every case is refused before a launch
    addr = (ctypes.addressof(buf) + 15) & ~15

    def ptrs(**kw):
        p = hb.KvFp8Ptrs(k8=addr, v8=addr, ks=addr, vs=addr)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def args(**kw):
        a = hb.DecPrefillArgs()
        a.row_seg = a.seg_off = a.seg_len = a.seg_row = addr
        a.rows = 64
        a.q = a.cos_t = a.sin_t = a.P = addr                                       # kc == vc == NULL
        a.ldq, a.q_off, a.k_off, a.v_off = 1536, 0, 1024, 1280
        a.q_heads, a.kv_heads, a.kv_cap, a.causal = 8, 2, 160, 1
        a.p_plane_stride, a.p_ktiles = 4 * 32 * 512, 32
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def refused(rc, word, what):
        assert rc == -1, what                                                      # DIA_E_ARG
        assert word in L.dia_last_error(), (what, L.dia_last_error())

    refused(fn(None, ctypes.byref(ptrs()), None), b"null", "a == NULL")
    refused(fn(ctypes.byref(args()), None, None), b"null", "p == NULL")
    assert L.dia_last_error().startswith(entry.encode() + b":")
    for kw in (dict(k8=None), dict(v8=None), dict(ks=None), dict(vs=None)):
        refused(fn(ctypes.byref(args()), ctypes.byref(ptrs(**kw)), None), b"null", kw)
    for kw, word in ((dict(kc=addr), b"kc / vc must be NULL"), (dict(vc=addr), b"kc / vc must be NULL"), (dict(causal=0), b"causal"),
                     (dict(kv_cap=170), b"multiple of 32"), (dict(kv_cap=0), b"multiple of 32"),
                     # the existing kernels' own checks
                     (dict(rows=48), b"rows not a multiple of 32"), (dict(rows=0), b"rows"), (dict(row_seg=None), b"packing"),
                     (dict(seg_off=None), b"packing"), (dict(seg_len=None), b"packing"), (dict(seg_row=None), b"packing"),
                     (dict(q=None), b"bad argument"), (dict(cos_t=None), b"bad argument"), (dict(sin_t=None), b"bad argument"),
                     (dict(kv_heads=0), b"bad argument")):
        refused(fn(ctypes.byref(args(**kw)), ctypes.byref(ptrs()), None), word, kw)
    for kw in (dict(k8=addr + 8), dict(v8=addr + 4), dict(ks=addr + 2), dict(vs=addr + 1)):
        refused(fn(ctypes.byref(args()), ctypes.byref(ptrs(**kw)), None), b"aligned", kw)
    if entry.endswith("attn_fp8"):
        for kw in (dict(P=None), dict(q_heads=0), dict(kv_heads=3), dict(p_ktiles=31), dict(p_plane_stride=12)):
            refused(fn(ctypes.byref(args(**kw)), ctypes.byref(ptrs()), None), b"bad argument", kw)


def test_session_keyword_defaults_and_refusals_by_name():
    from dia_hip.model import Dia
    for fn in (DecodeSession.__init__, DecodeSession.open):
        assert inspect.signature(fn).parameters["prompt_prefill"].default == "auto"
    assert Dia.prompt_prefill == "auto" and DecodeSession.prompt_prefill == "auto"
    src = open(os.path.join(ROOT, "cli.py")).read()
    assert '"--prompt-prefill"' in src and 'choices=["auto", "replay", "batched"]' in src and "Dia.prompt_prefill = args.prompt_prefill" in src
    model = open(os.path.join(ROOT, "dia-tts-prune_amd", "dia_hip", "model.py")).read()
    assert model.count("self_kv=self.self_kv") == model.count("self_kv=self.self_kv, prompt_prefill=self.prompt_prefill") == 4
    # the checks run before the session allocates or touches its device: a stand-in for DeviceWeights is enough to reach them
    cfg = CF.mid_config()
    weights = lambda **kw: SimpleNamespace(**{**dict(cfg=cfg, device=torch.device("cpu"), compacted=False, weight_planes=1), **kw})
    ids = [np.arange(40, 50, dtype=np.int32)]
    rows = [np.zeros((4, cfg.data.channels), dtype=np.int32)]
    cases = ((weights(), dict(kv_dtype="f32"), "kv_dtype 'f32'"), (weights(), dict(kv_dtype="bf16x2"), "kv_dtype 'bf16x2'"),
             (weights(), dict(attention="valu"), "attention='valu'"), (weights(compacted=True), {}, "compacted"),
             (weights(weight_planes=2), {}, "weight_planes = 2"), (weights(), dict(adapters=object()), "adapters="),
             (weights(), dict(teacher_tokens=rows), "teacher_tokens="), (weights(), dict(teacher_tokens=rows, score=True), "score=True"),
             (weights(), dict(self_kv="fp8", kv_dtype="f32"), "kv_dtype 'f32'"))
    for w, kw, word in cases:
        with pytest.raises(ValueError, match=re.escape(word)) as ei:
            DecodeSession(w, ids, max_tokens=8, **{"kv_dtype": "bf16", "prompt_prefill": "batched", **kw})
        assert "prompt_prefill='batched'" in str(ei.value) or "self_kv='fp8'" in str(ei.value), str(ei.value)
    for w, kw, word in cases:
        if "teacher_tokens" in kw:
            continue                                  # (open() takes no forced rows)
        with pytest.raises(ValueError, match=re.escape(word)):
            DecodeSession.open(w, 2, **{"kv_dtype": "bf16", "prompt_prefill": "batched", **kw})
    # an unknown value is still refused, wherever the keyword goes in
    for make in (lambda: DecodeSession(weights(), ids, max_tokens=8, prompt_prefill="packed"),
                 lambda: DecodeSession.open(weights(), 2, prompt_prefill="packed")):
        with pytest.raises(ValueError, match="prompt_prefill must be"):
            make()


# ---- step accounting of a prefilled slot, on the simulated device of tests/test_slots_cpu.py ------------------------------
class FakeSession(DecodeSession):
    """The host side of a slotted session; the simulated device honours what _enqueue_admit would leave behind: a prefilled slot
    stands at cur = first_step, a replayed one at 1, and a slot finishes at step max_tokens - 1."""

    def __init__(self, slots, prompt_prefill, max_tokens=None):
        cfg = CF.mid_config()
        self.cfg, self.dev = cfg, torch.device("cpu")
        da = cfg.data
        self.B, self.T, self.C, self.V = slots, da.audio_length, da.channels, cfg.model.tgt_vocab_size
        self.max_tokens = self.T if max_tokens is None else max_tokens
        self.max_delay = max(da.delay_pattern)
        self.S = 64
        self.noise_steps = self.max_tokens - 1
        self.noise = torch.zeros(slots, self.noise_steps, self.C, self.V)
        self.sample_params = dict(cfg_scale=3.0, temperature=1.3, top_p=0.95, top_k=35)
        self.lens, self.first_steps = [0] * slots, [1] * slots
        self._issued, self._pinned, self.slotted, self.prefilled, self.seg = 0, [], True, True, False
        self.prompt_prefill = prompt_prefill
        self._init_slots()
        self.cur_h = np.ones(slots, dtype=np.int32)
        self.fsm_h = self.fsm.numpy().copy()
        self.steps, self.uploads = 0, []

    def _enqueue_admit(self, pairs, pre):
        for (b, _), (_, pstep) in zip(pairs, pre):
            self.cur_h[b] = pstep if self.prompt_prefill == "batched" and pstep > 2 else 1
            self.fsm_h[b] = [0, -1, self.max_delay, 0, 0, 0, 0, 0]

    def _enqueue_retire(self, part):
        for b in part:
            self.fsm_h[b, 3], self.cur_h[b] = 1, 1

    def _enqueue_steps(self, n, use_graph):
        self.steps += n
        for _ in range(n):
            for b, sl in self._live.items():
                if self.fsm_h[b, 3]:
                    continue
                if sl["gen"] is not None and self.cur_h[b] >= sl["first_step"]:      # a sampling step reads row cur - first_step
                    assert self.cur_h[b] - sl["first_step"] < sl["rows"], "a step ran ahead of its noise"
                if self.cur_h[b] >= sl["req"].max_tokens - 1:
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

    def close(self):
        pass


def prompted(seed, mt, frames):
    cfg = CF.mid_config()
    pr = None if not frames else np.ones((frames, cfg.data.channels), dtype=np.int32)
    return Request(np.arange(5, dtype=np.int32) + 1, seed=seed, max_tokens=mt, audio_prompt=pr)


@pytest.mark.parametrize("frames", [40, 1, 0])
def test_a_prefilled_slot_finishes_at_the_same_step_with_fewer_steps_issued(frames):
    """the same request through a replaying and a prefilling session: same last_step, first_step - 1 fewer steps, and noise row r
    is the request's draw number r in both"""
    mt = 90
    out = {}
    for mode in ("auto", "batched"):
        s = FakeSession(2, mode, max_tokens=96)
        res = s.serve([prompted(7, mt, frames)], poll=8)
        fs = s.first_steps[0]
        out[mode] = (res[0].last_step, s.steps, fs, s.noise[0].clone(), sum(n for _, _, n in s.uploads))
    assert out["auto"][0] == out["batched"][0] == mt - 1
    fs = out["auto"][2]
    assert fs == out["batched"][2] == (frames + 1 if frames else 1)
    skipped = fs - 1 if fs > 2 else 0                                       # a one-frame prompt stays on the replay path
    assert out["auto"][1] - out["batched"][1] == skipped
    g = torch.Generator().manual_seed(7)
    n = mt - fs                                                              # sampling steps fs .. mt - 1
    fresh = torch.empty(n, s.C, s.V).exponential_(1.0, generator=g)
    for mode in out:
        assert torch.equal(out[mode][3][:n], fresh), mode
    assert out["batched"][4] == mt - 1 - skipped                             # no row is drawn for a step that was prefilled


def test_steps_left_and_the_live_neighbour_of_a_prefilled_slot():
    s = FakeSession(2, "batched", max_tokens=96)
    assert s.admit([prompted(1, 60, 0)]) == [0]
    s.decode(16)
    assert s.admit([prompted(2, 80, 40)]) == [1]
    assert s.cur_h[1] == 41 and s._live[1]["t0"] == 16 - 40 and s._live[0]["t0"] == 0
    assert s._steps_left(0) == 59 - 16 and s._steps_left(1) == 79 - 40
    s.decode(39)
    assert s.finished() == [1] and s.collect(1).last_step == 79
    assert s._live[0]["rows"] == 16 + 39 and s._steps_left(0) == 4
