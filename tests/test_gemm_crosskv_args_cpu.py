"""dia_gemm's CROSSKV epilogue refuses a cache description it cannot serve before any pointer is used and before any
launch, so these run without a GPU.  Every case starts from one description of a two-plane bf16 (DIA_KV_BF16X2) cache
that passes the CROSSKV checks, changes what its name says, and must come back as DIA_E_ARG (-1) with a message naming
the field.  The starting description itself is stopped by the check that FOLLOWS the CROSSKV ones (its ssq_ld is too
small on purpose), so it never reaches a launch either: it shows that the kv_dtype / kv_plane_stride checks let a
valid two-plane description through.  The pointers are non-null and point at a small host buffer nothing may read."""
import ctypes as C

import numpy as np
import pytest

from dia_hip import binding as hb

_DUMMY = np.zeros(64, dtype=np.float32)
HEADS, CAP, ROWS = 2, 64, 4
PLANE = ROWS * HEADS * CAP * 128                 # elements of one plane of a cache


def _args(**over):
    """CROSSKV over 40 rows of K = 1024 into a two-plane bf16 cache with blocked V; ssq_ld = 0 is what stops it"""
    p = _DUMMY.ctypes.data
    g = hb.GemmArgs()
    g.A, g.a_plane_stride, g.a_ktiles, g.M = p, 3 * 32 * 512, 32, 40
    g.W, g.KT, g.nstrips, g.epi = p, 32, HEADS * 16, hb.EPI_CROSSKV
    g.ssq_in, g.ssq_in_n, g.inv_d, g.eps, g.ssq_ld = p, 64, 1.0 / 1024, 1e-5, 0
    g.kc, g.vc, g.kv_dtype, g.kv_heads, g.kv_cap, g.kv_batch_index = p, p, hb.KV_BF16X2, HEADS, CAP, 1
    g.cos_t, g.sin_t, g.kv_vblocked, g.kv_plane_stride = p, p, 1, PLANE
    for k, v in over.items():
        setattr(g, k, v)
    return g


KV_DTYPE, STRIDE = b"kv_dtype", b"kv_plane_stride"
REFUSALS = [
    # (id, changes to the description, field the message must name)
    ("kv_dtype_3", dict(kv_dtype=3), KV_DTYPE),
    ("kv_dtype_negative", dict(kv_dtype=-1), KV_DTYPE),
    ("kv_dtype_large", dict(kv_dtype=1 << 20), KV_DTYPE),
    ("kv_dtype_3_row_v", dict(kv_dtype=3, kv_vblocked=0, kv_plane_stride=0), KV_DTYPE),
    ("x2_no_plane_stride", dict(kv_plane_stride=0), STRIDE),
    ("x2_no_plane_stride_row_v", dict(kv_plane_stride=0, kv_vblocked=0), STRIDE),
    ("x2_negative_plane_stride", dict(kv_plane_stride=-PLANE), STRIDE),
    ("x2_plane_stride_not_8", dict(kv_plane_stride=PLANE + 4), STRIDE),
    ("x2_plane_stride_1", dict(kv_plane_stride=1), STRIDE),
    ("x2_no_plane_stride_layers", dict(kv_plane_stride=0, nstrips=2 * HEADS * 16, kv_layer_strips=HEADS * 16, kv_layer_stride=2 * PLANE), STRIDE),
]


@pytest.mark.parametrize("name,over,field", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_dia_gemm_crosskv_refuses(name, over, field):
    L = hb.lib()
    assert L.dia_gemm(C.byref(_args(**over)), None) == -1, name
    msg = L.dia_last_error()
    assert msg.startswith(b"dia_gemm: CROSSKV") and field in msg, (name, msg)


@pytest.mark.parametrize("over", [dict(), dict(kv_vblocked=0), dict(kv_plane_stride=8), dict(kv_plane_stride=PLANE + 8),
                                  dict(kv_dtype=hb.KV_F32, kv_plane_stride=0, kv_vblocked=0), dict(kv_dtype=hb.KV_BF16, kv_plane_stride=0),
                                  dict(kv_dtype=hb.KV_BF16, kv_plane_stride=4)],
                         ids=["x2_blocked", "x2_row_v", "x2_stride_8", "x2_stride_gap", "f32_no_stride", "bf16_no_stride", "bf16_stride_ignored"])
def test_valid_cache_descriptions_pass_the_crosskv_checks(over):
    """refused, but by the check behind the CROSSKV ones (ssq_ld), not for the cache format or the plane stride: the
    plane stride binds DIA_KV_BF16X2 only"""
    L = hb.lib()
    assert L.dia_gemm(C.byref(_args(**over)), None) == -1
    msg = L.dia_last_error()
    assert msg == b"dia_gemm: ssq_ld smaller than padded rows", msg
    assert KV_DTYPE not in msg and STRIDE not in msg


def test_refusal_ids_are_unique_and_cover_both_fields():
    assert len({r[0] for r in REFUSALS}) == len(REFUSALS)
    assert {r[2] for r in REFUSALS} == {KV_DTYPE, STRIDE}
