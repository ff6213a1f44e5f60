"""dia_attn, dia_attn_cross_fp8 and dia_attn_self_fp8 refuse an argument combination they cannot serve before any pointer is used
and before any launch, so these run without a GPU: every case starts from a launch the entry would accept, changes what its name
says, and must come back as DIA_E_ARG (-1) with the message of that refusal under the entry's own name.  The pointers are non-null
and point at a small host buffer that nothing may read.  The three entries share one front end and one key split (csrc/attn.hip
attn_front / key_split): the last test pins the split through the scratch refusal of each entry."""
import ctypes as C

import numpy as np
import pytest

from dia_hip import binding as hb

SELF, CROSS, ENC = hb.ATTN_SELF, hb.ATTN_CROSS, hb.ATTN_ENC
F32, BF16, BF16X2 = hb.KV_F32, hb.KV_BF16, hb.KV_BF16X2
_DUMMY = np.zeros(64, dtype=np.float32)
assert _DUMMY.ctypes.data % 8 == 0
_blocked = dict(kv_dtype=BF16, v_blocked=1)
PTRS = ("q", "kc", "vc", "cur", "len", "cos_t", "sin_t", "P", "scratch", "tickets")


def _args(**over):
    """a SELF launch dia_attn accepts: 2 rows, 4 kv heads x group 4, capacity 256 (two key splits -> scratch needed)"""
    a = hb.AttnArgs()
    a.mode, a.kv_dtype, a.n_kv_heads, a.group, a.n_rows, a.kv_cap = SELF, F32, 4, 4, 2, 256
    a.ldq, a.q_off, a.k_off, a.v_off = 24 * 128, 0, 16 * 128, 20 * 128
    a.enc_len, a.rope_rows = 0, 257
    a.p_plane_stride, a.p_ktiles = 64 * 512, 64
    for name in PTRS:
        setattr(a, name, _DUMMY.ctypes.data)
    for k, v in over.items():
        setattr(a, k, v)
    return a


def _cross8(**over):
    """a launch dia_attn_cross_fp8 accepts: 2 rows, 16 heads, group 1, bf16 with the blocked V layout, capacity 160 (two key splits)"""
    return _args(**dict(dict(_blocked, mode=CROSS, group=1, n_kv_heads=16, kv_cap=160, rope_rows=0), **over))


def _self8(**over):
    """a launch dia_attn_self_fp8 accepts: the SELF launch above on bf16 with the blocked V layout, and no bf16 caches (kc == vc == NULL)"""
    return _args(**dict(dict(_blocked, kc=None, vc=None), **over))


def _f8(**over):
    f = hb.KvFp8Ptrs(k8=_DUMMY.ctypes.data, v8=_DUMMY.ctypes.data, ks=_DUMMY.ctypes.data, vs=_DUMMY.ctypes.data)
    for k, v in over.items():
        setattr(f, k, v)
    return f


_cross = dict(mode=CROSS, group=1, n_kv_heads=16)
_enc = dict(mode=ENC, group=1, n_kv_heads=16, n_rows=40, enc_len=40, kv_cap=64)

REFUSALS = [
    # (id, changes to the accepted launch, fragment of dia_last_error())
    *[(f"null_{p}", {p: None}, b"null argument") for p in ("q", "kc", "vc", "P", "cos_t", "sin_t")],
    ("no_rows", dict(n_rows=0), b"empty problem"),
    ("negative_rows", dict(n_rows=-2), b"empty problem"),
    ("no_kv_heads", dict(n_kv_heads=0), b"empty problem"),
    ("plane_stride_not_8", dict(p_plane_stride=64 * 512 + 4), b"plane stride must be a multiple of 8"),
    ("enc_rows_differ_from_len", dict(_enc, n_rows=39), b"ENC needs n_rows == enc_len"),
    ("enc_len_zero", dict(_enc, n_rows=1, enc_len=0), b"ENC needs n_rows == enc_len"),
    ("enc_len_over_cap", dict(_enc, n_rows=65, enc_len=65), b"ENC needs n_rows == enc_len"),
    ("rope_short_self", dict(rope_rows=256), b"RoPE tables shorter"),           # position kv_cap needs kv_cap + 1 rows
    ("rope_short_self_blocked", dict(_blocked, rope_rows=256), b"RoPE tables shorter"),
    ("rope_short_enc", dict(_enc, rope_rows=39), b"RoPE tables shorter"),
    ("kv_cap_zero", dict(kv_cap=0, rope_rows=0), b"kv_cap must be positive"),
    ("kv_cap_negative", dict(kv_cap=-128), b"kv_cap must be positive"),
    ("no_scratch", dict(scratch=None), b"scratch and tickets are required"),
    ("no_tickets", dict(tickets=None), b"scratch and tickets are required"),
    ("no_scratch_cross", dict(_cross, kv_cap=129, scratch=None), b"scratch and tickets are required"),
    ("planes_too_narrow", dict(p_ktiles=63), b"output planes too narrow"),
    ("planes_too_narrow_group1", dict(group=1, p_ktiles=15), b"output planes too narrow"),
    ("x2_not_blocked", dict(kv_dtype=BF16X2, kv_plane_stride=2 * 4 * 256 * 128), b"two-plane bf16 K/V needs the blocked V layout"),
    ("x2_no_plane_stride", dict(kv_dtype=BF16X2, v_blocked=1, kv_plane_stride=0), b"two-plane bf16 K/V needs the blocked V layout"),
    ("x2_plane_stride_not_8", dict(kv_dtype=BF16X2, v_blocked=1, kv_plane_stride=2 * 4 * 256 * 128 + 4), b"two-plane bf16 K/V needs the blocked V layout"),
    ("blocked_f32", dict(v_blocked=1), b"v_blocked needs bf16 K/V"),
    ("blocked_enc", dict(_enc, kv_dtype=BF16, v_blocked=1), b"v_blocked needs bf16 K/V"),
    ("blocked_cap_not_32", dict(_blocked, kv_cap=240, rope_rows=241), b"v_blocked needs bf16 K/V"),
    ("self_no_cur", dict(cur=None), b"SELF needs cur"),
    ("self_no_cur_bf16_rows", dict(kv_dtype=BF16, cur=None), b"SELF needs cur"),
    ("self_no_cur_blocked", dict(_blocked, cur=None), b"SELF needs cur"),
    ("cross_no_len", dict(_cross, len=None), b"CROSS needs cur, len and group 1"),
    ("cross_no_len_blocked", dict(_cross, **_blocked, len=None), b"CROSS needs cur, len and group 1"),
    ("cross_no_cur", dict(_cross, cur=None), b"CROSS needs cur, len and group 1"),
    ("cross_group2", dict(_cross, group=2, n_kv_heads=8), b"CROSS needs cur, len and group 1"),
    ("cross_group2_blocked", dict(_cross, **_blocked, group=2, n_kv_heads=8), b"CROSS needs cur, len and group 1"),
    ("group3", dict(group=3), b"GQA group must be 1, 2 or 4"),
    ("group3_blocked", dict(_blocked, group=3), b"GQA group must be 1, 2 or 4"),
    ("group8", dict(group=8, n_kv_heads=2), b"GQA group must be 1, 2 or 4"),
    ("enc_bf16", dict(_enc, kv_dtype=BF16), b"ENC needs group 1, fp32 scratch K/V"),
    ("enc_group4", dict(_enc, group=4, n_kv_heads=4), b"ENC needs group 1, fp32 scratch K/V"),
    ("unknown_mode", dict(mode=3), b"unknown mode"),
    ("negative_mode", dict(mode=-1), b"unknown mode"),
]


def test_null_args_struct_is_refused():
    L = hb.lib()
    assert L.dia_attn(None, None) == -1
    assert b"null argument" in L.dia_last_error()


@pytest.mark.parametrize("name,over,fragment", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_dia_attn_refuses(name, over, fragment):
    L = hb.lib()
    hb.set_tuning("attn_nz", -1)
    assert L.dia_attn(C.byref(_args(**over)), None) == -1, name
    msg = L.dia_last_error()
    assert msg.startswith(b"dia_attn: ") and fragment in msg, (name, msg)


def test_refusal_ids_are_unique_and_cover_every_message():
    """every refusal message dia_attn can produce is pinned by at least one case"""
    assert len({r[0] for r in REFUSALS}) == len(REFUSALS)
    want = {b"null argument", b"empty problem", b"plane stride must be a multiple of 8", b"ENC needs n_rows == enc_len",
            b"RoPE tables shorter", b"kv_cap must be positive", b"scratch and tickets are required", b"output planes too narrow",
            b"two-plane bf16 K/V needs the blocked V layout", b"v_blocked needs bf16 K/V", b"SELF needs cur",
            b"CROSS needs cur, len and group 1", b"GQA group must be 1, 2 or 4", b"ENC needs group 1, fp32 scratch K/V", b"unknown mode"}
    assert {r[2] for r in REFUSALS} == want


# the dia_kv_fp8_ptrs both FP8 entries refuse: (id, changes to the struct, fragment)
_F8_PTRS = [
    *[(f"null_{p}", {p: None}, b"null argument") for p in ("k8", "v8", "ks", "vs")],
    *[(f"odd_{p}", {p: _DUMMY.ctypes.data + d}, b"k8 / v8 must be 8-byte aligned, ks / vs 4-byte") for p, d in (("k8", 4), ("v8", 2), ("ks", 2), ("vs", 1))],
]

CROSS8_REFUSALS = [
    # (id, changes to the accepted launch, changes to the dia_kv_fp8_ptrs, fragment of dia_last_error())
    *[(f"null_{p}", {p: None}, {}, b"null argument") for p in ("q", "kc", "vc", "P", "cos_t", "sin_t")],
    *[(n, {}, f, m) for n, f, m in _F8_PTRS],
    ("mode_self", dict(mode=SELF), {}, b"mode must be DIA_ATTN_CROSS"),
    ("mode_enc", dict(mode=ENC), {}, b"mode must be DIA_ATTN_CROSS"),
    ("group4", dict(group=4, n_kv_heads=4), {}, b"group must be 1"),
    ("f32", dict(kv_dtype=F32), {}, b"kv_dtype must be DIA_KV_BF16 with the blocked V layout (v_blocked)"),
    ("x2", dict(kv_dtype=BF16X2), {}, b"kv_dtype must be DIA_KV_BF16 with the blocked V layout (v_blocked)"),
    ("not_blocked", dict(v_blocked=0), {}, b"kv_dtype must be DIA_KV_BF16 with the blocked V layout (v_blocked)"),
    ("kv_cap_not_32", dict(kv_cap=170), {}, b"kv_cap must be a positive multiple of 32"),
    ("kv_cap_zero", dict(kv_cap=0), {}, b"kv_cap must be a positive multiple of 32"),
    ("no_rows", dict(n_rows=0), {}, b"empty problem"),
    ("no_kv_heads", dict(n_kv_heads=0), {}, b"empty problem"),
    ("plane_stride_not_8", dict(p_plane_stride=64 * 512 + 4), {}, b"plane stride must be a multiple of 8"),
    ("no_cur", dict(cur=None), {}, b"CROSS needs cur and len"),
    ("no_len", dict(len=None), {}, b"CROSS needs cur and len"),
    ("planes_too_narrow", dict(p_ktiles=63), {}, b"output planes too narrow"),
    ("no_scratch", dict(scratch=None), {}, b"scratch and tickets are required"),
    ("no_tickets", dict(tickets=None), {}, b"scratch and tickets are required"),
]

SELF8_REFUSALS = [
    *[(f"null_{p}", {p: None}, {}, b"null argument") for p in ("q", "P", "cos_t", "sin_t")],
    *[(n, {}, f, m) for n, f, m in _F8_PTRS],
    ("mode_cross", dict(mode=CROSS), {}, b"mode must be DIA_ATTN_SELF"),
    ("mode_enc", dict(mode=ENC), {}, b"mode must be DIA_ATTN_SELF"),
    ("f32", dict(kv_dtype=F32), {}, b"kv_dtype must be DIA_KV_BF16 (one plane)"),
    ("x2", dict(kv_dtype=BF16X2), {}, b"kv_dtype must be DIA_KV_BF16 (one plane)"),
    ("not_blocked", dict(v_blocked=0), {}, b"the blocked V layout (v_blocked) is required"),
    ("kv_cap_not_32", dict(kv_cap=240, rope_rows=241), {}, b"kv_cap must be a positive multiple of 32"),
    ("kv_cap_negative", dict(kv_cap=-128), {}, b"kv_cap must be a positive multiple of 32"),
    ("no_rows", dict(n_rows=0), {}, b"empty problem"),
    ("no_kv_heads", dict(n_kv_heads=0), {}, b"empty problem"),
    ("plane_stride_not_8", dict(p_plane_stride=64 * 512 + 4), {}, b"plane stride must be a multiple of 8"),
    ("no_cur", dict(cur=None), {}, b"SELF needs cur"),
    ("group3", dict(group=3), {}, b"GQA group must be 1, 2 or 4"),
    ("group8", dict(group=8, n_kv_heads=2), {}, b"GQA group must be 1, 2 or 4"),
    ("rope_short", dict(rope_rows=256), {}, b"RoPE tables shorter"),
    ("planes_too_narrow", dict(p_ktiles=63), {}, b"output planes too narrow"),
    ("planes_too_narrow_group1", dict(group=1, p_ktiles=15), {}, b"output planes too narrow"),
    ("no_scratch", dict(scratch=None), {}, b"scratch and tickets are required"),
    ("no_tickets", dict(tickets=None), {}, b"scratch and tickets are required"),
]

_FP8 = [("dia_attn_cross_fp8", _cross8, r) for r in CROSS8_REFUSALS] + [("dia_attn_self_fp8", _self8, r) for r in SELF8_REFUSALS]


@pytest.mark.parametrize("entry", ["dia_attn_cross_fp8", "dia_attn_self_fp8"])
def test_null_structs_are_refused_fp8(entry):
    L = hb.lib()
    base = _cross8 if entry == "dia_attn_cross_fp8" else _self8
    for a, f in ((None, C.byref(_f8())), (C.byref(base()), None), (None, None)):
        assert getattr(L, entry)(a, f, None) == -1
        assert L.dia_last_error() == entry.encode() + b": null argument"


@pytest.mark.parametrize("entry,base,case", _FP8, ids=[f"{e}-{r[0]}" for e, _, r in _FP8])
def test_fp8_entries_refuse(entry, base, case):
    name, over, over_f8, fragment = case
    L = hb.lib()
    hb.set_tuning("attn_nz", -1)
    assert getattr(L, entry)(C.byref(base(**over)), C.byref(_f8(**over_f8)), None) == -1, name
    msg = L.dia_last_error()
    assert msg.startswith(entry.encode() + b": ") and fragment in msg, (name, msg)


def test_fp8_refusal_ids_are_unique_and_cover_every_message():
    """every refusal message the two FP8 entries can produce is pinned by at least one case"""
    common = {b"null argument", b"empty problem", b"plane stride must be a multiple of 8", b"kv_cap must be a positive multiple of 32",
              b"output planes too narrow", b"k8 / v8 must be 8-byte aligned, ks / vs 4-byte", b"scratch and tickets are required"}
    for table, own in ((CROSS8_REFUSALS, {b"mode must be DIA_ATTN_CROSS", b"group must be 1", b"CROSS needs cur and len",
                                          b"kv_dtype must be DIA_KV_BF16 with the blocked V layout (v_blocked)"}),
                       (SELF8_REFUSALS, {b"mode must be DIA_ATTN_SELF", b"kv_dtype must be DIA_KV_BF16 (one plane)", b"SELF needs cur",
                                         b"the blocked V layout (v_blocked) is required", b"GQA group must be 1, 2 or 4", b"RoPE tables shorter"})):
        assert len({r[0] for r in table}) == len(table)
        assert {r[3] for r in table} == common | own


def test_the_three_entries_split_the_keys_alike():
    """One key split serves the three entries: without scratch, 160 keys of capacity (two 128-key chunks) stop every entry at the
    scratch refusal.  128 keys (one chunk) need no scratch: dia_attn passes that refusal and stops at the next one, the plane width.
    The FP8 entries raise the scratch refusal last, so nothing later could stop a 128-key call short of a launch: that half is
    dia_attn's alone."""
    L = hb.lib()
    hb.set_tuning("attn_nz", -1)
    for entry, a, f in (("dia_attn", _args(kv_cap=160, scratch=None, p_ktiles=63), None), ("dia_attn_cross_fp8", _cross8(scratch=None), _f8()),
                        ("dia_attn_self_fp8", _self8(kv_cap=160, scratch=None), _f8())):
        assert a.kv_cap == 160
        assert (L.dia_attn(C.byref(a), None) if f is None else getattr(L, entry)(C.byref(a), C.byref(f), None)) == -1, entry
        assert L.dia_last_error() == entry.encode() + b": more than 128 keys possible: scratch and tickets are required"
    assert L.dia_attn(C.byref(_args(kv_cap=128, scratch=None, p_ktiles=63)), None) == -1
    assert L.dia_last_error() == b"dia_attn: output planes too narrow"
