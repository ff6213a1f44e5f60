"""dia_act_gram on a real MI355X (csrc/gram.hip, DESIGN.md "Gram matrices and GPTQ") against tests/gram_ref.py.

Without a row scale the device's result is the reference's bit for bit: v is the float32 input, the product of two widened floats
is exact in double, and both sides add the rows in ascending order with one rounding each.
With a scale (derived, not measured): |got - ref| <= 16 * 2^-24 * sqrt(ref_ii * ref_jj).  The reference multiplies by the float32
scale of the header's expression in float64; the device rounds v = x * scale once (2^-24 relative) with a scale at most 2 ulp
(4 * 2^-24) off, so every v is off by at most 5 * 2^-24 relative and a product by 10 * 2^-24 (+ second order); the sum over the rows
of |v_i v_j| is at most sqrt(G_ii G_jj) by Cauchy-Schwarz.  The float64 adds contribute M * 2^-53.
Measured (MI355X): printed per case by the test."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import calib_ref as CR
import gram_ref as R
from dia_hip import binding as hb
from dia_hip import layout as LY
from dia_hip.calib import gram_diagonal, gram_tiles, unpack_gram

DEV = "cuda:0"
TOL = 16 * 2.0 ** -24
GUARD = 16
EPS = 1e-5
CANARY = 777.0


class Plane:
    """x [M, K] on the device in one of the two activation formats, rows M .. rows_pad - 1 of the tiles filled with NaN"""

    def __init__(self, x, fmt, rows_pad):
        M, K = x.shape
        full = np.full((rows_pad, K), np.nan, dtype=np.float32)
        full[:M] = x
        t = torch.from_numpy(full).to(DEV)
        self.fmt, self.M, self.K, self.rows_pad, self.kt = fmt, M, K, rows_pad, K // 32
        self.t = (LY.pack_f32_tiles if fmt == "f32" else LY.pack_planes)(t, self.kt, rows_pad // 16).contiguous()
        self.stride = 0 if fmt == "f32" else self.t[0].numel()


def fill(a, pl, gram_ptr, counter, *, M=None, ssq=None, n=0, mask=None, cur=None, first=None, fsm=None, T=0, used=0):
    a.x, a.plane_stride, a.ktiles, a.ktiles_used = hb.ptr(pl.t), pl.stride, pl.kt, used
    a.M, a.rows_pad, a.act_f32 = pl.M if M is None else M, pl.rows_pad, int(pl.fmt == "f32")
    if ssq is not None:
        a.ssq_in, a.ssq_in_n, a.ssq_ld, a.inv_d, a.eps = hb.ptr(ssq), n, pl.rows_pad, 1.0 / pl.K, EPS
    a.row_mask = hb.ptr(mask)
    if cur is not None:
        a.rows_per_slot, a.cur, a.first_step, a.fsm, a.T = 2, hb.ptr(cur), hb.ptr(first), hb.ptr(fsm), T
    a.counter = hb.ptr(counter)
    return a


def launch(st, pl, gram, counter, **kw):
    """one dia_act_gram; gram: float64 device tensor with GUARD doubles on either side, counter: int64 device tensor [1]"""
    a = fill(hb.ActGramArgs(), pl, None, counter, **kw)
    a.gram = gram.data_ptr() + 8 * GUARD
    torch.cuda.synchronize()                # the operands were written on torch's stream
    hb.check(hb.lib().dia_act_gram(ctypes.byref(a), ctypes.c_void_p(st.cuda_stream)), "dia_act_gram")
    st.synchronize()                        # ... and the caller may drop them right away


def launch_stats(st, pl, K, **kw):
    """dia_act_stats on the same inputs: float64 [K]"""
    acc = torch.zeros(K, dtype=torch.float64, device=DEV)
    cnt = torch.zeros(1, dtype=torch.int64, device=DEV)
    a = fill(hb.ActStatsArgs(), pl, None, cnt, **kw)
    a.acc = hb.ptr(acc)
    torch.cuda.synchronize()
    hb.check(hb.lib().dia_act_stats(ctypes.byref(a), ctypes.c_void_p(st.cuda_stream)), "dia_act_stats")
    st.synchronize()
    return acc.cpu().numpy()


def new_gram(K, value=0.0):
    n = gram_tiles(K) * 1024
    g = torch.full((n + 2 * GUARD,), CANARY, dtype=torch.float64, device=DEV)
    g[GUARD: GUARD + n] = value
    return g, torch.zeros(1, dtype=torch.int64, device=DEV)


def read(st, g, counter, K):
    """(packed [tiles, 32, 32], counter); the canaries on either side of the packed range must have survived"""
    st.synchronize()
    n = gram_tiles(K) * 1024
    h = g.cpu().numpy()
    assert (h[:GUARD] == CANARY).all() and (h[GUARD + n:] == CANARY).all()
    return h[GUARD: GUARD + n].reshape(-1, 32, 32).copy(), int(counter.item())


def dev(a, dt):
    return None if a is None else torch.tensor(np.asarray(a), dtype=dt, device=DEV)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def make_x(rs, M, K):
    x = (rs.normal(size=(M, K)) * np.exp(rs.normal(size=(1, K)) * 1.5)).astype(np.float32)     # channel norms spread over decades
    x[:, 3] = 0                                                                                # an all-zero column
    return x


def rel_dev(got, ref):
    """largest |got - ref| / sqrt(ref_ii ref_jj); where the denominator is 0 both must be 0"""
    d = np.sqrt(np.diagonal(ref))
    den = d[:, None] * d[None, :]
    assert np.isfinite(got).all()
    assert (got[den == 0] == 0).all()
    nz = den > 0
    return float((np.abs(got - ref)[nz] / den[nz]).max())


# (K of the Gram matrix, K of the plane set, rows, format): one tile; an odd tile count with off-diagonal tiles; every row count at
# an m-tile (16) or chunk (64) edge; the o_proj form (a tap narrower than its planes); the model's own wo (K = 8192 at 2 rows)
SHAPES = ([(32, 32, M, "f32" if M % 2 else "planes") for M in (1, 2, 16, 17, 64, 65, 130)]
          + [(96, 96, M, "planes" if M % 2 else "f32") for M in (1, 2, 16, 17, 64, 65, 130)]
          + [(1024, 1280, 5, "planes"), (1024, 1280, 33, "f32"), (8192, 8192, 2, "planes")])


@pytest.mark.parametrize("K,Kp,M,fmt", SHAPES)
def test_against_float64(K, Kp, M, fmt):
    rs = np.random.RandomState(K + 31 * M)
    rows_pad = 16 * (-(-M // 16)) + (16 if M % 16 == 0 else 0)              # always at least one padding row (NaN)
    x = make_x(rs, M, Kp)
    pl = Plane(x, fmt, rows_pad)
    used = 0 if K == Kp else K // 32
    st = torch.cuda.Stream(device=DEV)
    on = np.ones(M, dtype=bool)
    for n in ((0,) if K >= 8192 else (0, 128)):                              # (the 67M-element case checks the tile decode: bitwise only)
        ssq_h = scale = None
        if n:
            ssq_h = (rs.gamma(2.0, 1.0, size=(n, rows_pad)) * Kp / n).astype(np.float32)
            ssq_h[:, M:] = np.nan
            scale = CR.row_scale_f32(ssq_h, n, np.float32(1.0 / Kp), np.float32(EPS), M)
        ssq_d = dev(ssq_h, torch.float32)
        g, cnt = new_gram(K)
        launch(st, pl, g, cnt, ssq=ssq_d, n=n, used=used)
        packed, rows = read(st, g, cnt, K)
        got = unpack_gram(packed)
        del g
        want, nrows = R.kernel_ref(x[:, :K], on, scale)
        assert rows == nrows == M                                            # the counter is exact
        assert np.array_equal(bits(got), bits(got.T))                        # diagonal tiles are stored whole and symmetric
        assert (got[3] == 0).all() and (got[:, 3] == 0).all()
        if n == 0:
            assert np.array_equal(bits(got), bits(want)), "without a scale the result is the reference's bit for bit"
            print(f"K={K} M={M} {fmt}: bitwise")
        else:
            e = rel_dev(got, want)
            print(f"K={K} M={M} {fmt} partials={n}: max |got - ref| / sqrt(ref_ii ref_jj) {e:.3e} (bound {TOL:.3e})")
            assert e <= TOL, e
        # the diagonal is dia_act_stats's acc on the same inputs, bit for bit
        acc = launch_stats(st, pl, K, ssq=ssq_d, n=n, used=used)
        assert np.array_equal(bits(gram_diagonal(packed)), bits(acc)) and acc.max() > 0
        del got, want, packed


@pytest.mark.parametrize("fmt,M", [("planes", 4), ("f32", 6), ("f32", 33)])
def test_gate_and_row_mask(fmt, M):
    K, T = 96, 12
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
            on = CR.gate(M, mask, cur if use_gate else None, first if with_first else None, done if with_fsm else None, T)
            g, cnt = new_gram(K)
            args = dict(mask=dev(mask, torch.uint8))
            if use_gate:
                args.update(cur=dev(cur, torch.int32), first=dev(first, torch.int32) if with_first else None,
                            fsm=dev(fsm, torch.int32) if with_fsm else None, T=T)
            launch(st, pl, g, cnt, **args)
            packed, rows = read(st, g, cnt, K)
            want, nrows = R.kernel_ref(x, on)
            assert rows == nrows, (shift, use_mask, use_gate, rows, nrows)
            assert np.array_equal(bits(unpack_gram(packed)), bits(want))
            counts.append(nrows)
    assert 0 in counts or M > 8
    assert max(counts) > 0 and len(set(counts)) > 2                         # the scenarios do switch rows on and off


@pytest.mark.parametrize("fmt", ["f32", "planes"])
def test_bitwise_properties(fmt):
    K, M, n = 96, 8, 128
    rs = np.random.RandomState(11)
    x = make_x(rs, M, K)
    pl = Plane(x, fmt, 16)
    ssq = dev((rs.gamma(2.0, 1.0, size=(n, 16)) * K / n).astype(np.float32), torch.float32)
    st = torch.cuda.Stream(device=DEV)

    def run(masks, g=None, cnt=None):
        if g is None:
            g, cnt = new_gram(K)
        for m in masks:
            launch(st, pl, g, cnt, ssq=ssq, n=n, mask=dev(m, torch.uint8))
        return read(st, g, cnt, K)

    ones = np.ones(M, dtype=np.uint8)
    whole, c1 = run([ones])
    halves, c2 = run([np.r_[ones[:4], 0 * ones[4:]], np.r_[0 * ones[:4], ones[4:]]])
    assert c1 == c2 == 8 and np.array_equal(bits(whole), bits(halves))     # rows 0..7 in one launch == 0..3 then 4..7
    assert np.abs(whole).max() > 0

    # zero counted rows: G is left as it is, bit for bit (a pattern no sum would reproduce, NaN among it), the counter stays
    g, cnt = new_gram(K, value=float("nan"))
    g[GUARD + 5] = -3.25
    before, _ = read(st, g, cnt, K)
    after, c0 = run([0 * ones], g, cnt)
    assert c0 == 0 and np.array_equal(bits(before), bits(after))
    # ... and by the gate: every utterance finished
    fsm = np.zeros((M // 2, 8), dtype=np.int32)
    fsm[:, 3] = 1
    launch(st, pl, g, cnt, cur=dev([3] * (M // 2), torch.int32), first=None, fsm=dev(fsm, torch.int32), T=12)
    after, c0 = read(st, g, cnt, K)
    assert c0 == 0 and np.array_equal(bits(before), bits(after))


def test_refusals():
    """every refusal returns DIA_E_ARG with its message and launches nothing"""
    K, M = 64, 3
    x = make_x(np.random.RandomState(2), M, K)
    pl = Plane(x, "planes", 16)
    st = torch.cuda.Stream(device=DEV)
    g, cnt = new_gram(K)
    launch(st, pl, g, cnt)
    good, rows = read(st, g, cnt, K)
    assert rows == 3
    ssq = torch.ones(4, 16, dtype=torch.float32, device=DEV)
    cur = torch.ones(2, dtype=torch.int32, device=DEV)
    L = hb.lib()

    def base():
        a = fill(hb.ActGramArgs(), pl, None, cnt)
        a.gram = g.data_ptr() + 8 * GUARD
        return a

    def set_(**kw):
        def f(a):
            for k, v in kw.items():
                setattr(a, k, v)
        return f

    cases = [(set_(gram=None), b"null gram"), (set_(gram=g.data_ptr() + 8 * GUARD + 8), b"16-byte aligned"),
             (set_(x=None), b"null plane"), (set_(counter=None), b"null counter"), (set_(ktiles=0), b"ktiles <= 0"),
             (set_(ktiles_used=3), b"ktiles_used outside"), (set_(ktiles_used=-1), b"ktiles_used outside"),
             (set_(rows_pad=24), b"rows_pad"), (set_(rows_pad=0), b"rows_pad"), (set_(M=0), b"M <= 0"), (set_(M=17), b"M <= 0"),
             (set_(plane_stride=pl.stride - 1), b"plane_stride"), (set_(ssq_in=hb.ptr(ssq), ssq_in_n=0, ssq_ld=16), b"ssq_in_n"),
             (set_(ssq_in=hb.ptr(ssq), ssq_in_n=4, ssq_ld=2), b"ssq_ld"), (set_(rows_per_slot=3, cur=hb.ptr(cur), T=12), b"rows_per_slot"),
             (set_(rows_per_slot=2, T=12), b"without cur"), (set_(rows_per_slot=2, cur=hb.ptr(cur), T=0), b"without T"),
             (set_(x=hb.ptr(pl.t) + 8), b"16-byte aligned"), (set_(ktiles=4096, ktiles_used=0), b"2048 k-tiles")]
    for change, msg in cases:
        a = base()
        change(a)
        assert L.dia_act_gram(ctypes.byref(a), ctypes.c_void_p(st.cuda_stream)) == -1, msg
        err = L.dia_last_error()
        assert b"dia_act_gram" in err and msg in err, (msg, err)
    assert L.dia_act_gram(None, ctypes.c_void_p(st.cuda_stream)) == -1
    again, rows2 = read(st, g, cnt, K)
    assert rows2 == 3 and np.array_equal(bits(again), bits(good))
