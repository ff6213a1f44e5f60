"""Which decode GEMM instantiation dia_gemm runs, and whether that instantiation is right: every (NW, KPW) pair of
launch_small_rs (k_gemv_small, 1-4 rows) and of launch_g16_any (k_gemm16, 5-16 rows and the z-form over 2-3 m-tiles) is
reached with an explicit g.nw at K = 32 * NW * KPW * sk, named through dia_gemm_timed / dia_timed_kernel_name and compared
with the float64 restatements of tests/test_gpu_kernels.py (2e-5 * max(1, |ref|max)); part B pins the DEFAULT choice
(nw = 0, spw = 0) for the shapes the engine produces, dense and K-compacted, and for a hidden-pruned model step.

Dense one-plane weights, w_layout = 0, through the C ABI only.  Sparse, MXFP, two-plane and diagonal weights, k_gemm2t and
k_gemm_tile_ws have their own files.

The table (ENTRIES): one entry per pair and launch form.
  k_gemv_small: 20 pairs x RS {2, 4} x forms {one strip per workgroup, split-K 2, MULTI with spw = 3}, MULTI with spw = 4 for
                two pairs.
  k_gemm16:     8 fp32-tile + 13 plane pairs x rows {one m-tile, z-form} x forms {one strip, multi-strip, split-K 4,
                split-K 4 with several strips per workgroup (the strip-pair hand-off where KPW == 8 at one m-tile)}.
Entries: 282 reachable, 9 unreachable.  The unreachable ones are run as well: each asserts the kernel that serves the call
instead, or DIA_E_ARG (UNREACHABLE_WHY names the guard).

Every case also checks that nothing else is written: rows >= M and 16 extra columns of `out`, the pad rows of the emitted
planes / tiles and the columns >= M of ssq_out keep their fill value.  (No GEMM test of test_gpu_kernels.py shows a kernel that
defines ssq_out beyond M — test_gemm_resid_emit and its kin look at [:, :M] only, and every epilogue stores under `live` — so
none is excepted.)  The pad rows of the A image and the pad columns of ssq_in hold NaN.

The z-form cases whose workgroup K range is 32 or 64 k-tiles set the knob gemm_2t = 0: by default k_gemm2t takes those
shapes (test_gpu_kernels.py covers it) and k_gemm16 over gridDim.z is what the engine falls back to."""
import ctypes as C
from collections import namedtuple

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from dia_hip import binding as hb
from dia_hip import layout as lay

REACHABLE, UNREACHABLE = 282, 9             # the counts the docstring states (test_table_counts)
E_ARG = -1
STORE, RESID, SWIGLU = hb.EPI_SCALE_STORE, hb.EPI_RESID_EMIT, hb.EPI_SWIGLU_EMIT
EPIS = (STORE, RESID, SWIGLU)
EPI_NAME = {STORE: "store", RESID: "resid", SWIGLU: "swiglu"}
SENT = -77.25                               # fill of out and ssq_out
NAN = float("nan")

# csrc/gemm.hip, launch_small_rs: the (NW, KPW) pairs of k_gemv_small, in its order
SMALL_PAIRS = [(4, 4), (4, 8), (4, 16),
               (8, 1), (8, 2), (8, 3), (8, 4), (8, 5), (8, 6), (8, 7), (8, 8), (8, 10), (8, 12), (8, 14), (8, 16), (8, 32),
               (16, 1), (16, 2), (16, 4), (16, 8)]
# csrc/gemm.hip, launch_g16_any: fp32 tiles on both sides (nw == 8 only) ...
G16_F32_PAIRS = [(8, 1), (8, 2), (8, 3), (8, 4), (8, 5), (8, 6), (8, 7), (8, 8)]
# ... and planes
G16_PLANE_PAIRS = [(16, 1), (16, 2), (16, 4),
                   (8, 1), (8, 2), (8, 3), (8, 4), (8, 5), (8, 6), (8, 7), (8, 8),
                   (4, 4), (4, 8)]
MULTI4_PAIRS = [(8, 2), (16, 1)]            # the two pairs that also run nstrips = 1024 (spw = 4)

UNREACHABLE_WHY = {
    "lds": "gemm_impl: small_smem(8, 256, 4) = 201 KiB exceeds the 150 KiB guard in front of launch_small_rs",
    "small_multi": "launch_small: MULTI is compiled for KPW <= 16 && !(NW == 16 && KPW > 4) only",
    "g16_multi": "launch_g16: the multi-strip forms sit behind if constexpr (!(NW == 16 && KPW >= 4))",
}

# kind "small": rows = RS; kind "g16": rows = "m1" (one m-tile) or "mz" (z-form).  why: None = reachable, else a key of
# UNREACHABLE_WHY.
Entry = namedtuple("Entry", "kind f32 nw kpw rows form why")
ROWS = {2: (1, 2), 4: (3, 4), "m1": (5, 16), "mz": (17, 40)}
SMALL_FORMS = ("one", "sk2", "multi3", "multi4")
G16_FORMS = ("one", "multi", "sk4", "sk4_multi")


def small_multi_compiled(nw, kpw):
    return kpw <= 16 and not (nw == 16 and kpw > 4)


def build_entries():
    out = []
    for nw, kpw in SMALL_PAIRS:
        for rs in (2, 4):
            lds = "lds" if (nw, kpw, rs) == (8, 32, 4) else None
            out.append(Entry("small", None, nw, kpw, rs, "one", lds))
            out.append(Entry("small", None, nw, kpw, rs, "sk2", lds))
            if small_multi_compiled(nw, kpw):
                out.append(Entry("small", None, nw, kpw, rs, "multi3", None))
                if (nw, kpw) in MULTI4_PAIRS:
                    out.append(Entry("small", None, nw, kpw, rs, "multi4", None))
            elif lds is None:               # (<8, 32> at RS = 4 never gets as far as launch_small)
                out.append(Entry("small", None, nw, kpw, rs, "multi3", "small_multi"))
    for f32, pairs in ((True, G16_F32_PAIRS), (False, G16_PLANE_PAIRS)):
        for nw, kpw in pairs:
            for rows in ("m1", "mz"):
                for form in G16_FORMS:
                    why = "g16_multi" if (nw == 16 and kpw >= 4 and form in ("multi", "sk4_multi")) else None
                    out.append(Entry("g16", f32, nw, kpw, rows, form, why))
    return out


ENTRIES = build_entries()

Case = namedtuple("Case", "entry M f32 epi K ns sk spw")


def entry_cases(e, idx):
    """the launches of one entry: its row counts (and, k_gemv_small, both activation formats), the epilogue rotating"""
    rows = ROWS[e.rows]
    cases = []
    if e.kind == "small":
        fi = SMALL_FORMS.index(e.form)
        sk = 2 if e.form == "sk2" else 1
        ns = {"one": 16, "sk2": 16, "multi3": 528, "multi4": 1024}[e.form]
        spw = 0
        if e.why == "small_multi":
            ns, spw = 16, 2                 # spw > 1 is what asks launch_small for MULTI; N = 256 keeps K = 8192 weights small
        for mi, M in enumerate(rows):
            for f32 in (False, True):
                epi = EPIS[(idx + fi + mi + int(f32) + (2 if e.rows == 4 else 0)) % 3]
                cases.append(Case(e, M, f32, epi, 32 * e.nw * e.kpw * sk, ns, sk, spw))
    else:
        fi = G16_FORMS.index(e.form)
        sk = 4 if e.form in ("sk4", "sk4_multi") else 1
        ns = 272 if e.form in ("multi", "sk4_multi") else 16
        spw = 2 if (e.form == "sk4_multi" and e.rows == "m1") else 0        # as wo_split_k sets it; the z-form picks its own
        for mi, M in enumerate(rows):
            epi = EPIS[(idx + fi + mi + (2 if e.rows == "mz" else 0)) % 3]
            cases.append(Case(e, M, e.f32, epi, 32 * e.nw * e.kpw * sk, ns, sk, spw))
    return cases


PAIR_INDEX = {}
for _e in ENTRIES:
    PAIR_INDEX.setdefault((_e.kind, _e.f32, _e.nw, _e.kpw), len(PAIR_INDEX))
CASES = [c for e in ENTRIES for c in entry_cases(e, PAIR_INDEX[(e.kind, e.f32, e.nw, e.kpw)])]


def case_id(c):
    e = c.entry
    fmt = "f32" if c.f32 else "planes"
    return f"{e.kind}-{e.nw}x{e.kpw}-{fmt}-M{c.M}-{e.form}-{EPI_NAME[c.epi]}" + ("-unreachable" if e.why else "")


def b(v):
    return "true" if v else "false"


def expected_kernel(c):
    """the instantiation name dia_timed_kernel_name prints, or E_ARG.  k_gemv_small<NW, KPW, RS, MULTI, AF32, PF32, W2, DF>,
    k_gemm16<NW, KPW, MULTI, MZ, AF32, PF32, PAIR, ALDS, W2>."""
    e = c.entry
    f = b(c.f32)
    if e.kind == "small":
        if e.why == "lds":                  # no k_gemm16 form holds 32 k-tiles per wave: the generic kernel, which has no split-K
            return E_ARG if c.sk > 1 else "k_gemm<1, 8, 32>"
        multi = e.form in ("multi3", "multi4") and e.why is None
        return f"k_gemv_small<{e.nw}, {e.kpw}, {e.rows}, {b(multi)}, {f}, {f}, false, 0>"
    mz = e.rows == "mz"
    multi = e.form in ("multi", "sk4_multi") and e.why is None
    pair = multi and e.form == "sk4_multi" and not mz and e.kpw == 8
    # the mid / lo planes of A in LDS: the z-form of <8, 4> and <8, 8> without split-K, and <8, 8> on fp32 tiles at one m-tile
    alds = multi and e.form == "multi" and e.nw == 8 and ((mz and e.kpw in (4, 8)) or (not mz and e.kpw == 8 and c.f32))
    return f"k_gemm16<{e.nw}, {e.kpw}, {b(multi)}, {b(mz)}, {f}, {f}, {b(pair)}, {b(alds)}, false>"


# ---------------------------------------------------------------------------------------------------------------------------

def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    return torch.device("cuda:0")


def bf16r(t):
    return t.bfloat16().float()


# Part B shapes (below) share the weights
PART_B_IN_K = list(range(256, 2049, 256))
PART_B_WO_K = list(range(1024, 8193, 1024))
PART_B_NS = 128


class Weights:
    """one bf16-valued matrix per K, created once at the widest N any case asks for; a case takes its first N columns (the
    tiles of its first nstrips strips)"""

    def __init__(self):
        self.nmax = {}
        for c in CASES:
            self.nmax[c.K] = max(self.nmax.get(c.K, 0), c.ns * 16)
        for K in PART_B_IN_K + PART_B_WO_K:
            self.nmax[K] = max(self.nmax.get(K, 0), PART_B_NS * 16)
        self.mats = {}
        self.f64 = (None, None)

    def get(self, K):
        if K not in self.mats:
            gen = torch.Generator(device=dev()).manual_seed(1000 + K)
            W = bf16r(torch.randn(K, self.nmax[K], device=dev(), generator=gen) * 0.03)
            self.mats[K] = (W, lay.tile_weight(W)[0])
        return self.mats[K]

    def double(self, K):
        if self.f64[0] != K:
            self.f64 = (None, None)
            self.f64 = (K, self.get(K)[0].double())
        return self.f64[1]


@pytest.fixture(scope="module")
def weights():
    w = Weights()
    yield w
    w.mats.clear()
    w.f64 = (None, None)
    torch.cuda.empty_cache()


def strip_ssq(x, mpad):
    """strip sums of squares [K / 16, mpad] of the rows of x; the columns of the pad rows hold NaN"""
    M, D = x.shape
    s = torch.full((D // 16, mpad), NAN, dtype=torch.float32, device=x.device)
    s[:, :M] = (x.double() ** 2).reshape(M, D // 16, 16).sum(-1).T.float()
    return s


def timed(g):
    """dia_gemm through dia_gemm_timed: (return code, name of the kernel that ran)"""
    L = hb.lib()
    ms = C.c_float()
    try:
        rc = L.dia_gemm_timed(C.byref(g), None, C.byref(ms))
        torch.cuda.synchronize()
    except RuntimeError as err:             # a device error poisons the process: end the session, launch nothing more
        pytest.exit(f"GPU error after dia_gemm_timed: {err}", returncode=3)
    if rc not in (0, E_ARG):
        pytest.exit(f"dia_gemm_timed returned {rc}: {L.dia_last_error().decode()}", returncode=3)
    return rc, (L.dia_timed_kernel_name(0).decode() if rc == 0 else "")


def run_gemm(weights, *, M, K, ns, epi, f32, nw=0, sk=1, spw=0, act_f32=None):
    """One dia_gemm call (two on one scratch and ticket buffer with split-K) checked against float64 and for stray writes.
    Returns the kernel name, or the return code when the call was refused (nothing checked then)."""
    d = dev()
    W, Wt = weights.get(K)
    Wd = weights.double(K)[:, : ns * 16]
    N, kt = ns * 16, K // 32
    mt = (M + 15) // 16
    mpad = mt * 16
    ldo = N + 16
    torch.manual_seed(M * 131 + K + ns + epi)
    resid = epi == RESID
    x = torch.randn(M, K, device=d) * (1.0 if resid else 2.0)
    xp = torch.full((mpad, K), NAN, device=d)
    xp[:M] = x
    A = lay.pack_f32_tiles(xp) if f32 else lay.pack_planes(xp)           # pad rows of the image: NaN in every plane / tile
    assert torch.isnan((lay.unpack_f32_tiles(A, mpad, K) if f32 else lay.unpack_planes(A, mpad, K))[M:]).all()
    D_out = N if resid else (N // 2 if epi == SWIGLU else 0)
    pkt = D_out // 32
    x0 = torch.randn(M, N, device=d)
    gn = bf16r(1.0 + 0.1 * torch.randn(N, device=d))
    ssq_in = None if resid else strip_ssq(x, mpad)

    def unpack(P):
        return lay.unpack_f32_tiles(P, mpad, pkt * 32) if f32 else lay.unpack_planes(P, mpad, pkt * 32)

    scr = tk = None
    if sk > 1:      # as gemm_impl demands for the z-form: a slab set and a ticket row per m-tile
        scr = torch.zeros(mt * ns * sk * 256, device=d)
        tk = torch.zeros(mt * ns, dtype=torch.int32, device=d)
    res, name = [], None
    for _ in range(2 if sk > 1 else 1):
        out = torch.full((mpad, ldo), SENT, device=d)
        if resid:
            out[:M, :N] = x0
        ssq_o = torch.full((ns, mpad), SENT, device=d)
        P = None
        if D_out:       # (7.0 in bf16 = 0x40E0: a finite fill as an fp32 pair too)
            P = torch.full((mt, pkt, 64, 8), 7.0, device=d) if f32 else torch.full((3, mt, pkt, 64, 8), 7.0, dtype=torch.bfloat16, device=d)
        g = hb.GemmArgs()
        g.A, g.a_plane_stride, g.a_ktiles, g.M = hb.ptr(A), mt * kt * 512, kt, M
        g.W, g.KT, g.nstrips, g.epi, g.nw, g.spw = hb.ptr(Wt), kt, ns, epi, nw, spw
        g.act_f32 = (3 if f32 else 0) if act_f32 is None else act_f32
        g.ssq_ld = mpad
        if ssq_in is not None:
            g.ssq_in, g.ssq_in_n, g.inv_d, g.eps = hb.ptr(ssq_in), K // 16, 1.0 / K, 1e-5
        g.out, g.ldo, g.ssq_out = hb.ptr(out), ldo, hb.ptr(ssq_o)
        if resid:
            g.gnext = hb.ptr(gn)
        if P is not None:
            g.P, g.p_plane_stride, g.p_ktiles = hb.ptr(P), mt * pkt * 512, pkt
        if sk > 1:
            g.sk, g.sk_scratch, g.sk_tickets, g.sk_scratch_floats = sk, hb.ptr(scr), hb.ptr(tk), scr.numel()
        rc, nm = timed(g)
        if rc != 0:
            return rc
        name = name or nm
        assert nm == name
        if sk > 1:
            assert (tk == 0).all()                  # the last arriver re-armed every ticket
        res.append((out, P, ssq_o))
    out, P, ssq_o = res[0]
    if len(res) == 2:                               # bit-reproducible whatever the arrival order
        assert torch.equal(out, res[1][0]) and torch.equal(ssq_o, res[1][2])
        assert P is None or torch.equal(P, res[1][1])

    xd = x.double()
    tol = lambda ref: 2e-5 * max(1.0, ref.abs().max().item())
    inv = None if resid else torch.rsqrt((xd ** 2).mean(-1, keepdim=True) + 1e-5)
    # nothing but the M x N result is written to out
    assert (out[M:] == SENT).all() and (out[:, N:] == SENT).all()
    if epi == STORE:
        ref = (xd @ Wd) * inv
        err = (out[:M, :N].double() - ref).abs().max().item()
        print(f"{name}: out err {err:.3e} (bound {tol(ref):.3e})")
        assert err <= tol(ref), (name, err)
    elif resid:
        ref = x0.double() + xd @ Wd
        err = (out[:M, :N].double() - ref).abs().max().item()
        want = (out[:M, :N].double() ** 2).reshape(M, ns, 16).sum(-1).T
        serr = (ssq_o[:, :M].double() - want).abs().max().item()
        print(f"{name}: out err {err:.3e} (bound {tol(ref):.3e}), ssq_out err {serr:.3e} (bound {1e-5 * want.max().item():.3e})")
        assert err <= tol(ref), (name, err)
        assert serr <= 1e-5 * want.max().item(), (name, serr)
        em = unpack(P)
        assert torch.equal(em[:M], out[:M, :N] * gn)                    # the emitted activations carry x * gnext exactly
    else:
        assert (out == SENT).all()
        f = ((xd * inv) @ Wd).reshape(M, ns, 2, 8)                      # a strip: 8 gate columns, then the 8 matching up columns
        ref = torch.nn.functional.silu(f[:, :, 0].reshape(M, ns * 8)) * f[:, :, 1].reshape(M, ns * 8)
        em = unpack(P)
        err = (em[:M].double() - ref).abs().max().item()
        print(f"{name}: emitted err {err:.3e} (bound {tol(ref):.3e})")
        assert err <= tol(ref), (name, err)
    if resid:
        assert (ssq_o[:, M:] == SENT).all()
    else:
        assert (ssq_o == SENT).all()
    if P is not None and M < mpad:                  # pad rows of the emitted planes / tiles keep their fill
        assert torch.equal(unpack(P)[M:], unpack(torch.full_like(P, 7.0))[M:])
    assert torch.isfinite(out[:M, :N]).all() if epi != SWIGLU else torch.isfinite(em[:M]).all()      # no NaN of a pad row leaked
    return name


# ---- the table itself -------------------------------------------------------------------------------------------------------

def test_table_has_every_pair():
    small = {(e.nw, e.kpw) for e in ENTRIES if e.kind == "small"}
    assert small == set(SMALL_PAIRS) and len(SMALL_PAIRS) == 20
    assert {(e.nw, e.kpw) for e in ENTRIES if e.kind == "g16" and e.f32} == set(G16_F32_PAIRS) and len(G16_F32_PAIRS) == 8
    assert {(e.nw, e.kpw) for e in ENTRIES if e.kind == "g16" and not e.f32} == set(G16_PLANE_PAIRS) and len(G16_PLANE_PAIRS) == 13
    for e in ENTRIES:           # every entry is run, reachable or not
        assert any(c.entry is e for c in CASES)
        assert e.why is None or e.why in UNREACHABLE_WHY


def test_table_counts():
    """the counts the module docstring states"""
    assert sum(e.why is None for e in ENTRIES) == REACHABLE
    assert sum(e.why is not None for e in ENTRIES) == UNREACHABLE
    assert f"{REACHABLE} reachable, {UNREACHABLE} unreachable" in __doc__


def test_every_pair_sees_every_epilogue():
    seen = {}
    for c in CASES:
        e = c.entry
        seen.setdefault((e.kind, e.f32, e.nw, e.kpw), set()).add(c.epi)
    assert all(s == set(EPIS) for s in seen.values())
    for e in ENTRIES:           # and so does every form of a pair across its row counts (and formats)
        if e.rows in (2, "m1"):
            other = 4 if e.rows == 2 else "mz"
            both = [c.epi for c in CASES if c.entry.kind == e.kind and c.entry.f32 == e.f32 and (c.entry.nw, c.entry.kpw) == (e.nw, e.kpw)
                    and c.entry.form == e.form and c.entry.rows in (e.rows, other)]
            assert set(both) == set(EPIS), e


# ---- part A: every instantiation, forced ------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_forced_instantiation(c, weights, tuning):
    e = c.entry
    if e.kind == "g16" and e.rows == "mz" and e.nw * e.kpw in (32, 64):
        tuning("gemm_2t", 0)            # k_gemm2t takes these by default (module docstring)
    got = run_gemm(weights, M=c.M, K=c.K, ns=c.ns, epi=c.epi, f32=c.f32, nw=e.nw, sk=c.sk, spw=c.spw)
    assert got == expected_kernel(c), (got, expected_kernel(c), UNREACHABLE_WHY.get(e.why))


# ---- part B: default dispatch (nw = 0, spw = 0) of the shapes the engine produces -------------------------------------------

def wo_split(kt, M, ns):
    """(sk, spw) as wo_split_k in csrc/engine.hip sets them for one-plane weights: 1-4 rows split K two ways when kt is even;
    5-16 rows into ranges of 64 k-tiles when that gives 2..8 of them, else four ways when kt % 4 == 0, and with two strips per
    workgroup when strips x ranges reach 512"""
    if M <= 4:
        return (2 if kt % 2 == 0 else 1), 0
    sk = 4 if kt % 4 == 0 else 1
    if kt % 64 == 0 and 2 <= kt // 64 <= 8:
        sk = kt // 64
    return sk, (2 if sk > 1 and ns * sk >= 512 and ns % 2 == 0 else 0)


def family(M):
    return "k_gemv_small<" if M <= 4 else "k_gemm16<"


@pytest.mark.parametrize("M", [2, 4, 8, 16])
@pytest.mark.parametrize("epi", EPIS, ids=[EPI_NAME[e] for e in EPIS])
@pytest.mark.parametrize("K", PART_B_IN_K)
def test_default_dispatch_of_projection_inputs(K, epi, M, weights):
    """what step_gemm sets for qkv / cross-q (SCALE_STORE, x read as fp32 tiles), o / cross-o (RESID_EMIT) and wi (SWIGLU_EMIT)
    at every K_GRANULE step of a K-compacted input width: served at once, by the tuned kernel of its row count.
    K = 256 (one granule) runs k_gemv_small<8, 1> at 1-4 rows"""
    got = run_gemm(weights, M=M, K=K, ns=PART_B_NS, epi=epi, f32=True, act_f32=1 if epi == STORE else 3)
    print(f"K {K} rows {M} {EPI_NAME[epi]}: {got}")
    assert isinstance(got, str), f"dia_gemm refused the call: {got}"
    assert not got.startswith("k_gemm<") and got.startswith(family(M)), got


# wo at 2 rows: the names the dense checkpoint (hidden 8192) and the 50 %-pruned one (4096) run today, and the eight-wave
# forms of the compacted hidden widths whose k-tile count per slice sixteen waves do not divide into 1, 2, 4 or 8
WO_PINNED = {
    (8192, 2): "k_gemv_small<16, 8, 2, false, true, true, false, 0>", (8192, 4): "k_gemv_small<16, 8, 4, false, true, true, false, 0>",
    (4096, 2): "k_gemv_small<16, 4, 2, false, true, true, false, 0>", (4096, 4): "k_gemv_small<16, 4, 4, false, true, true, false, 0>",
    (3072, 2): "k_gemv_small<8, 6, 2, false, true, true, false, 0>", (5120, 2): "k_gemv_small<8, 10, 2, false, true, true, false, 0>",
    (6144, 2): "k_gemv_small<8, 12, 2, false, true, true, false, 0>", (7168, 2): "k_gemv_small<8, 14, 2, false, true, true, false, 0>",
    (8192, 8): "k_gemm16<8, 8, true, false, true, true, true, false, false>", (8192, 16): "k_gemm16<8, 8, true, false, true, true, true, false, false>",
    (4096, 8): "k_gemm16<8, 8, false, false, true, true, false, false, false>", (4096, 16): "k_gemm16<8, 8, false, false, true, true, false, false, false>",
}


@pytest.mark.parametrize("M", [2, 4, 8, 16])
@pytest.mark.parametrize("K", PART_B_WO_K)
def test_default_dispatch_of_wo(K, M, weights):
    """wo of every hidden width compact.pad_hidden_keep can leave (multiples of 1024): RESID_EMIT with gnext, fp32 tiles, split-K
    by wo_split_k's rule — DIA_OK on the first call (the engine's sk = 1 retry would land on the generic kernel)"""
    sk, spw = wo_split(K // 32, M, PART_B_NS)
    got = run_gemm(weights, M=M, K=K, ns=PART_B_NS, epi=RESID, f32=True, sk=sk, spw=spw)
    print(f"wo hidden {K} rows {M} sk {sk} spw {spw}: {got}")
    assert isinstance(got, str), f"dia_gemm refused the call (DIA_E_ARG = {E_ARG}): {got}"
    assert not got.startswith("k_gemm<") and got.startswith(family(M)), got
    if (K, M) in WO_PINNED:
        assert got == WO_PINNED[(K, M)], got


# ---- a hidden-pruned model step ---------------------------------------------------------------------------------------------

def _wide_cfg():
    """3 decoder layers of Dia-1.6B widths (as tests/test_gpu_mxfp4_model.py::_wide_cfg)"""
    from dia_hip import config as CF
    c = CF.dia_1_6b_config()
    m = c.model
    return c.model_copy(update={
        "model": m.model_copy(update={"encoder": m.encoder.model_copy(update={"n_layer": 1}), "decoder": m.decoder.model_copy(update={"n_layer": 3})}),
        "data": c.data.model_copy(update={"text_length": 128, "audio_length": 128})})


@pytest.fixture(scope="module")
def wide_sd():
    from dia_hip.weights import synthetic_state_dict
    cfg = _wide_cfg()
    return cfg, synthetic_state_dict(cfg, seed=1234, std=0.02, device=dev())


def _step(w, cfg, B):
    """kernel names and logits of the first decode step of a seeded batch-B session"""
    from dia_hip.engine import DecodeSession
    from dia_hip.tokens import effective_text, encode_text, synthetic_text
    ids = [encode_text(effective_text(synthetic_text(32 + 16 * i, cfg)), cfg) for i in range(B)]
    s = DecodeSession(w, ids, kv_dtype="f32", max_tokens=8, seeds=list(range(B)), ignore_eos=True)
    try:
        s.prefill()
        s.time_step()
        s.sync()
        return list(s.last_kernel_names), s.logits_host().copy()
    finally:
        s.close()


@pytest.mark.parametrize("amount,hidden", [(0.30, 6144), (0.63, 3072)])
def test_hidden_pruned_model_step_stays_on_tuned_kernels(wide_sd, amount, hidden, tuning):
    """MLP hidden units pruned with pruning.structured_prune_state_dict (only the decoder's wo keeps its pruned form) and compacted
    by DeviceWeights: no launch of a step runs the generic kernel, wo runs k_gemv_small at batch 1 and k_gemm16 at batch 4.
    Reference of the logits: the same session with the knob wo_sk = 1, which takes wo's split-K away — no kernel but the generic
    one serves 96 or 192 k-tiles in one workgroup, so that is the step with every wo forced generic (asserted)."""
    from dia_hip.engine import DeviceWeights
    from dia_hip.pruning import structured_prune_state_dict
    cfg, sd = wide_sd
    pruned, _ = structured_prune_state_dict(cfg, sd, amount)
    psd = {k: (pruned[k] if k.startswith("decoder.") and k.endswith("mlp.wo.weight") else v) for k, v in sd.items()}
    del pruned
    w = DeviceWeights(cfg, psd, dev())
    assert w.compacted and all(L["wo"].kt * 32 == hidden for L in w.dec_layers)
    nl = cfg.model.decoder.n_layer
    for B in (1, 4):
        names, logits = _step(w, cfg, B)
        tuning("wo_sk", 1)
        names_g, logits_g = _step(w, cfg, B)
        tuning("wo_sk", -1)
        assert len(names) == len(names_g)
        wo = [i for i, n in enumerate(names_g) if n.startswith("k_gemm<")]
        assert len(wo) == nl, names_g                       # the forced run: every wo, and nothing else, on the generic kernel
        print(f"hidden {hidden} batch {B}: wo on {sorted(set(names[i] for i in wo))}")
        assert not [n for n in names if n.startswith("k_gemm<")], names
        assert all(names[i].startswith(family(2 * B)) for i in wo), [names[i] for i in wo]
        assert all(n == m for i, (n, m) in enumerate(zip(names, names_g)) if i not in wo)
        assert np.isfinite(logits).all() and np.abs(logits).max() > 0
        err = float(np.abs(logits - logits_g).max())
        print(f"hidden {hidden} batch {B}: logits vs wo on the generic kernel {err:.3e}")
        assert err <= 1e-3, err
