"""The host rule that decides between a one-shape form of k_attn_mfma and the generic kernel (csrc/attn.hip attn_form_of, read through
dia_attn_form): the rule alone, nothing is launched and no pointer is followed, so this runs without a GPU.  0 = generic, 1 = the cross
form, 2 = the self form.  Every case starts from a launch a form serves and changes one fact the form has compiled in."""
import ctypes as C

import numpy as np
import pytest

from dia_hip import binding as hb

GENERIC, F_CROSS, F_SELF = 0, 1, 2
_DUMMY = np.zeros(64, dtype=np.float32)


def form(**over):
    a = hb.AttnArgs()
    a.kv_dtype, a.v_blocked, a.head_map = hb.KV_BF16, 1, None
    for k, v in over.items():
        setattr(a, k, v)
    L = hb.lib()
    L.dia_attn_form.argtypes = [C.POINTER(hb.AttnArgs)]
    L.dia_attn_form.restype = C.c_int
    return L.dia_attn_form(C.byref(a))


CROSS = dict(mode=hb.ATTN_CROSS, group=1, n_kv_heads=16, n_rows=1, kv_cap=128)
SELF = dict(mode=hb.ATTN_SELF, group=4, n_kv_heads=4, n_rows=2, kv_cap=3072)


def test_the_two_hot_launches_take_their_forms():
    assert form(**CROSS) == F_CROSS and form(**SELF) == F_SELF
    assert form(**dict(CROSS, n_rows=2)) == F_CROSS and form(**dict(SELF, n_rows=4)) == F_SELF
    assert form(**dict(CROSS, kv_cap=32)) == F_CROSS and form(**dict(CROSS, kv_cap=256)) == F_CROSS       # 256 keys: still one chunk


@pytest.mark.parametrize("base,change", [
    (CROSS, dict(kv_cap=288)),                      # 257 keys and more: the keys may be split
    (CROSS, dict(kv_cap=1024)),
    (CROSS, dict(n_rows=3)),                        # more than 4 rows
    (CROSS, dict(head_map=_DUMMY.ctypes.data)),
    (CROSS, dict(kv_dtype=hb.KV_F32, v_blocked=0)),
    (CROSS, dict(kv_dtype=hb.KV_BF16X2)),
    (CROSS, dict(v_blocked=0)),
    (CROSS, dict(group=2)),
    (SELF, dict(group=2)),
    (SELF, dict(group=1)),
    (SELF, dict(n_rows=6)),
    (SELF, dict(head_map=_DUMMY.ctypes.data)),
    (SELF, dict(kv_dtype=hb.KV_BF16X2)),
    (SELF, dict(kv_dtype=hb.KV_F32, v_blocked=0)),
    (SELF, dict(kv_cap=3080)),                      # not a multiple of 32 (dia_attn refuses it anyway)
    (SELF, dict(n_kv_heads=4096, kv_cap=8192)),     # a cache row past 2^31 elements: the forms index rows with an int stride
    (SELF, dict(mode=hb.ATTN_ENC)),
])
def test_anything_else_is_the_generic_kernels(base, change):
    assert form(**dict(base, **change)) == GENERIC


def test_the_knob_is_a_mask(tuning):
    for v, want in ((0, (GENERIC, GENERIC)), (1, (F_CROSS, GENERIC)), (2, (GENERIC, F_SELF)), (3, (F_CROSS, F_SELF)), (-1, (F_CROSS, F_SELF))):
        tuning("attn_spec", v)
        assert (form(**CROSS), form(**SELF)) == want, v
    assert hb.lib().dia_attn_form(None) == GENERIC
