"""The decoder prompt-prefill entry points reject a packing they cannot serve before any pointer is used, so these run
without a GPU: missing packing arrays and a packed row count that is not a multiple of 32.  (The checks that need real
buffers behind the pointers are in test_gpu_prefill.py.)"""
import ctypes as C

import numpy as np

from dia_hip import binding as hb

ENTRY = ("dia_dec_prefill_embed", "dia_dec_prefill_kv", "dia_dec_prefill_attn")


def _packing(rows):
    row_seg = np.full((rows,), -1, dtype=np.int32)
    row_seg[:20] = 0
    seg = np.zeros((1,), dtype=np.int32)
    seg_len = np.full((1,), 20, dtype=np.int32)
    keep = (row_seg, seg, seg_len)
    a = hb.DecPrefillArgs()
    a.row_seg, a.seg_off, a.seg_len, a.seg_row = (t.ctypes.data for t in (row_seg, seg, seg_len, seg))
    a.rows = rows
    return a, keep


def test_prefill_rejects_missing_packing_arrays():
    L = hb.lib()
    for name in ENTRY:
        for field in ("row_seg", "seg_off", "seg_len", "seg_row"):
            a, keep = _packing(32)
            setattr(a, field, None)
            assert getattr(L, name)(C.byref(a), None) == -1, (name, field)
            assert b"packing arrays missing" in L.dia_last_error()
        assert getattr(L, name)(None, None) == -1, name


def test_prefill_rejects_rows_not_multiple_of_32():
    L = hb.lib()
    for name in ENTRY:
        for rows in (0, -32, 16, 48, 33):
            a, keep = _packing(max(rows, 64))
            a.rows = rows
            assert getattr(L, name)(C.byref(a), None) == -1, (name, rows)
            assert b"multiple of 32" in L.dia_last_error()
