"""dia_act_stats on a real MI355X (csrc/calib.hip, DESIGN.md "Activation statistics") against tests/calib_ref.py.

Accuracy bound (derived, not measured): per channel |acc - ref| <= 16 * 2^-24 * ref.  The reference takes the float32 row scale
of the header's expression and does everything else in float64.  The device rounds v = x * scale once (2^-24 relative), its
scale may differ from the restated one by at most 2 ulp (2 * 2^-23: the division and the square root), and squaring doubles a
relative error: 2 * (2^-24 + 4 * 2^-24) = 10 * 2^-24, below 16 * 2^-24.  The float64 adds contribute M * 2^-53.  All terms of a sum
are non-negative, so the bound on every term is the bound on the sum.
Measured (MI355X): printed per case by the test; see DESIGN.md."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import calib_ref as R
from dia_hip import binding as hb
from dia_hip import layout as LY

DEV = "cuda:0"
TOL = 16 * 2.0 ** -24
GUARD = 16
EPS = 1e-5


class Plane:
    """x [M, K] on the device in one of the two activation formats, rows M .. rows_pad - 1 of the tiles filled with NaN"""

    def __init__(self, x, fmt, rows_pad, ktiles=None):
        M, K = x.shape
        full = np.full((rows_pad, K), np.nan, dtype=np.float32)
        full[:M] = x
        t = torch.from_numpy(full).to(DEV)
        self.fmt, self.M, self.K, self.rows_pad = fmt, M, K, rows_pad
        self.kt = ktiles if ktiles is not None else K // 32
        self.t = (LY.pack_f32_tiles if fmt == "f32" else LY.pack_planes)(t, self.kt, rows_pad // 16).contiguous()
        self.stride = 0 if fmt == "f32" else self.t[0].numel()


def launch(st, pl, acc, counter, *, M=None, ssq=None, n=0, mask=None, cur=None, first=None, fsm=None, T=0, used=0):
    """one dia_act_stats; acc: float64 device tensor with GUARD doubles on either side, counter: int64 device tensor [1]"""
    a = hb.ActStatsArgs()
    a.x, a.plane_stride, a.ktiles, a.ktiles_used = hb.ptr(pl.t), pl.stride, pl.kt, used
    a.M, a.rows_pad, a.act_f32 = pl.M if M is None else M, pl.rows_pad, int(pl.fmt == "f32")
    if ssq is not None:
        a.ssq_in, a.ssq_in_n, a.ssq_ld, a.inv_d, a.eps = hb.ptr(ssq), n, pl.rows_pad, 1.0 / pl.K, EPS
    a.row_mask = hb.ptr(mask)
    if cur is not None:
        a.rows_per_slot, a.cur, a.first_step, a.fsm, a.T = 2, hb.ptr(cur), hb.ptr(first), hb.ptr(fsm), T
    a.acc, a.counter = acc.data_ptr() + 8 * GUARD, hb.ptr(counter)
    torch.cuda.synchronize()                # the operands were written on torch's stream
    hb.check(hb.lib().dia_act_stats(ctypes.byref(a), ctypes.c_void_p(st.cuda_stream)), "dia_act_stats")
    st.synchronize()                        # ... and the caller may drop them right away


def new_acc(K):
    acc = torch.full((K + 2 * GUARD,), 777.0, dtype=torch.float64, device=DEV)
    acc[GUARD: GUARD + K] = 0
    return acc, torch.zeros(1, dtype=torch.int64, device=DEV)


def read(st, acc, counter, K):
    st.synchronize()
    h = acc.cpu().numpy()
    assert (h[:GUARD] == 777.0).all() and (h[GUARD + K:] == 777.0).all()
    return h[GUARD: GUARD + K].copy(), int(counter.item())


def dev(a, dt):
    return None if a is None else torch.tensor(np.asarray(a), dtype=dt, device=DEV)


def rel_err(got, want):
    assert np.isfinite(got).all()
    assert (got[want == 0] == 0).all()
    nz = want > 0
    return float((np.abs(got[nz] - want[nz]) / want[nz]).max()) if nz.any() else 0.0


def make_x(rs, M, K):
    x = (rs.normal(size=(M, K)) * np.exp(rs.normal(size=(1, K)) * 1.5)).astype(np.float32)     # channel norms spread over decades
    x[:, 3] = 0                                                                                # an all-zero column
    return x


SHAPES = [(K, M, "planes") for K in (64, 2048, 8192) for M in (1, 2, 4)] + [(K, M, "f32") for K in (64, 2048, 8192) for M in (5, 16, 17, 33)]


@pytest.mark.parametrize("K,M,fmt", SHAPES)
def test_against_float64(K, M, fmt):
    rs = np.random.RandomState(K + 31 * M)
    rows_pad = 16 * (-(-M // 16)) + (16 if M % 16 == 0 else 0)              # always at least one padding row (NaN)
    x = make_x(rs, M, K)
    pl = Plane(x, fmt, rows_pad)
    st = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    for n in (0, 128, 256):
        ssq_h = scale = None
        if n:
            ssq_h = (rs.gamma(2.0, 1.0, size=(n, rows_pad)) * K / n).astype(np.float32)
            ssq_h[:, M:] = np.nan
            scale = R.row_scale_f32(ssq_h, n, np.float32(1.0 / K), np.float32(EPS), M)
        acc, cnt = new_acc(K)
        ssq_d = dev(ssq_h, torch.float32)
        torch.cuda.synchronize()
        launch(st, pl, acc, cnt, ssq=ssq_d, n=n)
        got, rows = read(st, acc, cnt, K)
        want, nrows = R.kernel_ref(x, np.ones(M, dtype=bool), scale)
        e = rel_err(got, want)
        print(f"K={K} M={M} {fmt} partials={n}: max rel err {e:.3e} (bound {TOL:.3e})")
        assert rows == nrows == M and got[3] == 0.0
        assert e <= TOL, (n, e)


@pytest.mark.parametrize("fmt,M", [("planes", 4), ("f32", 6), ("f32", 33)])
def test_gate_and_row_mask(fmt, M):
    K, T = 64, 12
    B = -(-M // 2)
    rs = np.random.RandomState(M)
    x = make_x(rs, M, K)
    pl = Plane(x, fmt, 16 * (-(-M // 16)) + 16)
    st = torch.cuda.Stream(device=DEV)
    # per utterance (cur, first, done), cycled over the utterances and shifted per scenario: below first, at first, at the last
    # row, one past the buffer, finished
    kinds = [(2, 3, 0), (3, 3, 0), (T - 1, 1, 0), (T, 1, 0), (5, 1, 1)]
    counts = []
    for shift in range(len(kinds)):
        for use_mask, use_gate, with_first, with_fsm in ((False, True, True, True), (True, False, False, False), (True, True, True, True),
                                                         (False, True, False, False)):
            sel = [kinds[(b + shift) % len(kinds)] for b in range(B)]
            cur, first, done = ([s[i] for s in sel] for i in range(3))
            mask = (rs.rand(M) < 0.6).astype(np.uint8) if use_mask else None
            fsm = np.zeros((B, 8), dtype=np.int32)
            fsm[:, 3] = done
            on = R.gate(M, mask, cur if use_gate else None, first if with_first else None, done if with_fsm else None, T)
            acc, cnt = new_acc(K)
            args = dict(mask=dev(mask, torch.uint8))
            if use_gate:
                args.update(cur=dev(cur, torch.int32), first=dev(first, torch.int32) if with_first else None,
                            fsm=dev(fsm, torch.int32) if with_fsm else None, T=T)
            torch.cuda.synchronize()
            launch(st, pl, acc, cnt, **args)
            got, rows = read(st, acc, cnt, K)
            want, nrows = R.kernel_ref(x, on)
            assert rows == nrows, (shift, use_mask, use_gate, rows, nrows)
            assert rel_err(got, want) <= TOL
            counts.append(nrows)
    assert 0 in counts or M > 8
    assert max(counts) > 0 and len(set(counts)) > 2                         # the scenarios do switch rows on and off


def bits(a):
    return a.view(np.uint64)


@pytest.mark.parametrize("fmt", ["f32", "planes"])
def test_bitwise_properties(fmt):
    K, M, n = 2048, 8, 128
    rs = np.random.RandomState(11)
    x = make_x(rs, M, K)
    pl = Plane(x, fmt, 16)
    ssq = dev((rs.gamma(2.0, 1.0, size=(n, 16)) * K / n).astype(np.float32), torch.float32)
    st = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()

    def run(masks, acc=None, cnt=None, plane=pl):
        if acc is None:
            acc, cnt = new_acc(K)
        for m in masks:
            launch(st, plane, acc, cnt, ssq=ssq, n=n, mask=dev(m, torch.uint8))
        return read(st, acc, cnt, K)

    ones = np.ones(M, dtype=np.uint8)
    whole, c1 = run([ones])
    halves, c2 = run([np.r_[ones[:4], 0 * ones[4:]], np.r_[0 * ones[:4], ones[4:]]])
    assert c1 == c2 == 8 and np.array_equal(bits(whole), bits(halves))     # one launch over 8 rows == 4 + 4
    assert whole.max() > 0

    # a row's contribution does not depend on its index: row 2's data and partial sums moved to index 5
    x2 = np.zeros_like(x)
    x2[5] = x[2]
    pl2 = Plane(x2, fmt, 16)
    ssq2 = ssq.clone()
    ssq2[:, 5] = ssq[:, 2]
    a, _ = run([np.eye(M, dtype=np.uint8)[2]])
    acc, cnt = new_acc(K)
    launch(st, pl2, acc, cnt, ssq=ssq2, n=n, mask=dev(np.eye(M, dtype=np.uint8)[5], torch.uint8))
    b, _ = read(st, acc, cnt, K)
    assert np.array_equal(bits(a), bits(b)) and a.max() > 0

    # three accumulating launches of one row each == the host's float64 sum of the three single launches IN THAT ORDER
    singles = [run([np.eye(M, dtype=np.uint8)[r]])[0] for r in (6, 1, 4)]
    chained, c3 = run([np.eye(M, dtype=np.uint8)[r] for r in (6, 1, 4)])
    assert c3 == 3 and np.array_equal(bits(chained), bits((singles[0] + singles[1]) + singles[2]))


def test_narrower_tap_than_its_plane_and_refusals():
    """ktiles_used < ktiles (o_proj's K inside wider attention planes): only the first channels are read and written"""
    K, M = 256, 3
    rs = np.random.RandomState(2)
    x = make_x(rs, M, K)
    pl = Plane(x, "planes", 16)
    st = torch.cuda.Stream(device=DEV)
    acc, cnt = new_acc(K)
    torch.cuda.synchronize()
    launch(st, pl, acc, cnt, used=2)
    got, rows = read(st, acc, cnt, K)
    want, _ = R.kernel_ref(x, np.ones(M, dtype=bool))
    assert rows == 3 and (got[64:] == 0).all() and rel_err(got[:64], want[:64]) <= TOL
    # a refused call launches nothing
    a = hb.ActStatsArgs()
    a.x, a.ktiles, a.M, a.rows_pad, a.act_f32, a.acc, a.counter = hb.ptr(pl.t), pl.kt, 17, 16, 0, acc.data_ptr() + 8 * GUARD, hb.ptr(cnt)
    a.plane_stride = pl.stride
    assert hb.lib().dia_act_stats(ctypes.byref(a), ctypes.c_void_p(st.cuda_stream)) == -1
    again, rows2 = read(st, acc, cnt, K)
    assert rows2 == 3 and np.array_equal(bits(again), bits(got))
