"""The side struct of dia_gemm_wo_deferred (dia_wo_defer_args / binding.WoDeferArgs) sits outside the structs tests/test_abi.py
compares: its size and every field offset on the C side against the ctypes mirror, and the refusals that need no GPU."""
import ctypes
import os
import subprocess
import tempfile

from dia_hip import binding as hb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_wo_defer_args_layout_matches_header():
    names = [f[0] for f in hb.WoDeferArgs._fields_]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "dia_hip.h"\nint main(void){ printf("%zu", sizeof(dia_wo_defer_args));\n'
    prog += "".join(f'printf(" %zu", offsetof(dia_wo_defer_args, {n}));\n' for n in names) + "return 0; }\n"
    with tempfile.TemporaryDirectory() as td:
        c, exe = os.path.join(td, "s.c"), os.path.join(td, "s")
        open(c, "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(v) for v in subprocess.check_output([exe]).split()]
    assert got == [ctypes.sizeof(hb.WoDeferArgs)] + [getattr(hb.WoDeferArgs, n).offset for n in names]
    assert names == ["slices", "slice_stride", "nslices", "defer", "xold", "xnew", "ldx", "_pad0"]


def test_wo_deferred_refusals_without_gpu():
    L = hb.lib()
    buf = ctypes.create_string_buffer(64)            # never dereferenced: every case is refused before a launch
    addr = ctypes.addressof(buf)
    g, w = hb.GemmArgs(), hb.WoDeferArgs()
    assert L.dia_gemm_wo_deferred(ctypes.byref(g), None, None, None) == -1
    assert L.dia_gemm_wo_deferred(ctypes.byref(g), ctypes.byref(w), None, None) == -1          # null A / W
    g.A, g.W, g.M, g.KT, g.nstrips, g.a_ktiles = addr, addr, 2, 256, 128, 256
    g.w_format = hb.W_MXFP8
    assert L.dia_gemm_wo_deferred(ctypes.byref(g), ctypes.byref(w), None, None) == -1
    assert b"dense" in L.dia_last_error()
    assert L.dia_engine_set_x_alt(None, None) == -1
