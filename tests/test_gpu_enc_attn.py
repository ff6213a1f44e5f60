"""The encoder attention kernels k_enc_kv_planes and k_attn_enc_mfma (csrc/attn.hip), through dia_enc_attn, against
tests/enc_ref.py in float64 — at the sizes where each of the 4 waves walks several 32-key granules (the online-softmax
rescale, the pbuf hand-over and the lrun carry only run beyond 128 keys; 1024 keys = 8 granules per wave is the model's
text_length), at the model's 16 heads, with the utterance numbers of a slot admission, over stale scratch planes and
non-finite padding rows, and its refusals.  Tolerances: the 2e-5 of test_enc_attn_packed_batch for randn inputs; for the
constructed softmax cases the bound is derived in the test from the float32 evaluation of the same formula."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import enc_ref as R
from dia_hip import binding as hb
from dia_hip import layout as lay

HD = 128
SENTINEL = 7.0
TOL = 2e-5                 # test_enc_attn_packed_batch's bound against float64


def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    return torch.device("cuda:0")


_tables = {}


def tables(where):
    """RoPE tables (cos, sin) of 1025 positions (text_length 1024) on "cpu" or "dev", each made once"""
    if "cpu" not in _tables:
        _tables["cpu"] = lay.rope_tables(1025, HD, 1, 10000)
    if where == "dev" and "dev" not in _tables:
        _tables["dev"] = tuple(t.to(dev()) for t in _tables["cpu"])
    return _tables[where]


def pack(lens):
    """offsets of utterances packed as whole 32-row blocks, total rows"""
    offs, tot = [], 0
    for n in lens:
        offs.append(tot); tot += (n + 31) // 32 * 32
    return offs, tot


def live_mask(offs, lens, tot):
    m = np.zeros((tot,), dtype=bool)
    for o, n in zip(offs, lens):
        m[o: o + n] = True
    return m


def enc_attn_args(qkv, H, row_b, seg_off, seg_len, kp, vp, P):
    cos, sin = tables("dev")
    a = hb.EncAttnArgs()
    a.qkv, a.ldq, a.q_off, a.k_off, a.v_off, a.heads, a.rows = hb.ptr(qkv), qkv.shape[1], 0, H * HD, 2 * H * HD, H, qkv.shape[0]
    a.row_b, a.seg_off, a.seg_len, a.cos_t, a.sin_t = hb.ptr(row_b), hb.ptr(seg_off), hb.ptr(seg_len), hb.ptr(cos), hb.ptr(sin)
    a.kp, a.vp, a.P, a.p_plane_stride, a.p_ktiles = hb.ptr(kp), hb.ptr(vp), hb.ptr(P), P[0].numel(), P.shape[2]
    return a


def launch(qkv, H, offs, lens, *, numbers=None, table=None, kp=None, vp=None):
    """One dia_enc_attn launch over the packed rows of qkv [rows, 3 * H * 128] (device).  numbers: the utterance number of
    each packed utterance (default 0..n-1); table: (seg_off, seg_len) host arrays indexed by utterance number, the entries of
    `numbers` are overwritten with offs / lens.  Returns (P raw planes, kp, vp): P starts as planes of SENTINEL, kp / vp as
    zeros unless given."""
    d, tot = qkv.device, qkv.shape[0]
    numbers = list(range(len(lens))) if numbers is None else list(numbers)
    so, sl = (np.zeros((max(numbers) + 1,), dtype=np.int32) for _ in range(2)) if table is None else (t.astype(np.int32).copy() for t in table)
    rb = np.full((tot,), -1, dtype=np.int32)
    for u, o, n in zip(numbers, offs, lens):
        assert 0 <= u < len(so) and o % 32 == 0 and o + n <= tot
        so[u], sl[u] = o, n
        rb[o: o + n] = u
    assert ((so >= 0) & (sl >= 0) & (so + sl <= tot)).all()            # every entry in range, used or not
    row_b, seg_off, seg_len = (torch.from_numpy(t).to(d) for t in (rb, so, sl))
    if kp is None:
        kp = torch.zeros(3, H, tot, HD, dtype=torch.bfloat16, device=d)
    if vp is None:
        vp = torch.zeros(3, H, tot, HD, dtype=torch.bfloat16, device=d)
    assert kp.numel() >= 3 * H * tot * HD and vp.numel() >= 3 * H * tot * HD
    P = lay.pack_planes(torch.full((tot, H * HD), SENTINEL, device=d))
    a = enc_attn_args(qkv, H, row_b, seg_off, seg_len, kp, vp, P)
    hb.check(hb.lib().dia_enc_attn(C.byref(a), None), "dia_enc_attn")
    torch.cuda.synchronize()
    return P, kp, vp


def rows_of(P, tot, H):
    """[tot, H, 128] fp32 on the host: the sum of the three output planes"""
    return lay.unpack_planes(P, tot, H * HD).reshape(tot, H, HD).cpu()


def bits(t):
    return t.contiguous().view(torch.int16)


def check_planes(qkv, H, offs, lens, kp, vp):
    """the scratch planes of a launch: K planes sum to the fp32 RoPE(k) of every live row within 1e-6, the blocked V planes
    to v exactly; padding rows are exact zeros in every plane"""
    tot = qkv.shape[0]
    cos, sin = tables("dev")
    live = torch.from_numpy(live_mask(offs, lens, tot)).to(qkv.device)
    pos = torch.zeros(tot, dtype=torch.long, device=qkv.device)
    for o, n in zip(offs, lens):
        pos[o: o + n] = torch.arange(n, device=qkv.device)
    k = qkv[:, H * HD: 2 * H * HD].reshape(tot, H, HD)
    c, s = cos[pos][:, None], sin[pos][:, None]
    want_k = torch.cat([k[..., :64] * c - k[..., 64:] * s, k[..., :64] * s + k[..., 64:] * c], dim=-1)       # fp32
    kp = kp.reshape(-1)[: 3 * H * tot * HD].view(3, H, tot, HD)
    got_k = (kp[0].float() + kp[1].float() + kp[2].float()).transpose(0, 1)                                      # [tot, H, 128]
    err_k = (got_k[live] - want_k[live]).abs().max().item()
    assert err_k <= 1e-6, err_k
    assert (kp[:, :, ~live] == 0).all()
    vp = vp.reshape(-1)[: 3 * H * tot * HD].view(3, H, tot // 32, HD, 32)
    got_v = lay.v_from_blocked(vp[0].float() + vp[1].float() + vp[2].float()).transpose(0, 1)                   # [tot, H, 128]
    v = qkv[:, 2 * H * HD: 3 * H * HD].reshape(tot, H, HD)
    assert torch.equal(got_v[live], v[live])
    for pl in range(3):
        assert (lay.v_from_blocked(vp[pl].float())[:, ~live] == 0).all()
    return err_k


def check_against_f64(qkv, H, offs, lens, P, tol=TOL):
    tot = qkv.shape[0]
    out = rows_of(P, tot, H)
    ref = R.enc_attn_ref(qkv, H, offs, lens, *tables("cpu"))
    live = torch.from_numpy(live_mask(offs, lens, tot))
    err = (out[live].double() - ref[live]).abs().max().item()
    assert err <= tol, err
    assert (out[~live] == SENTINEL).all()                       # padding rows are not written
    return err


SWEEP = [33, 1024, 1, 0, 257, 32, 129, 255, 31, 160, 128, 256, 127, 161]


def test_length_sweep():
    """every length at which the granule walk changes shape — 1, around one granule (31, 32, 33), around one granule per wave
    (127, 128, 129: the first second granule of wave 0), a partial fifth / sixth granule (160, 161), two per wave (255, 256,
    257), eight per wave (1024) and an empty utterance — packed in a non-monotone order into one launch"""
    assert sorted(SWEEP) == [0, 1, 31, 32, 33, 127, 128, 129, 160, 161, 255, 256, 257, 1024]
    d = dev()
    torch.manual_seed(21)
    H = 2
    offs, tot = pack(SWEEP)
    qkv = torch.randn(tot, 3 * H * HD, device=d)
    P, kp, vp = launch(qkv, H, offs, SWEEP)
    err = check_against_f64(qkv, H, offs, SWEEP, P)
    err_k = check_planes(qkv, H, offs, SWEEP, kp, vp)
    print(f"length sweep: max-abs err vs float64 {err:.3e}, K planes vs fp32 RoPE(k) {err_k:.3e}")


def test_model_shape_16_heads():
    """the model's 16 heads, a text at text_length and a ragged one (700 = 21 whole granules + 28 keys).  ALL 16 heads of both
    utterances are checked against float64: the reference takes well under a second at this size."""
    d = dev()
    torch.manual_seed(22)
    H, lens = 16, [1024, 700]
    offs, tot = pack(lens)
    qkv = torch.randn(tot, 3 * H * HD, device=d)
    P, kp, vp = launch(qkv, H, offs, lens)
    err = check_against_f64(qkv, H, offs, lens, P)
    err_k = check_planes(qkv, H, offs, lens, kp, vp)
    print(f"16 heads, 1024 + 700 rows: max-abs err vs float64 {err:.3e}, K planes vs fp32 RoPE(k) {err_k:.3e}")


# ---------------------------------------------------------------------------------------------------------------------
# softmax stress: scores constructed after RoPE


def stress_case(case, L):
    """q | k | v rows [ceil32(L), 384] (fp32, host) of ONE head whose scores AFTER RoPE follow a plan.  The rotated vectors are
    constructed in float64 — query i = r_i * A * e (r_i in [0.6, 1], e a fixed unit vector), key j = t_j * sqrt(128) / A * e
    + noise, so score(i, j) = r_i * t_j + noise — and rotated back by -position; the rounding of the result to fp32 IS the
    input, to the kernel and to both references alike.  |score| <= 30 and |v| <= 4 are asserted by the caller on the float64
    scores of the rounded inputs.
      rise   t rises linearly over the keys: every granule raises the running maximum (alpha < 1 every time)
      fall   t falls linearly: the maximum is set by a wave's first granule, every later granule adds exp(s - m) << 1
      spike  one key outweighs all others by e^20 and sits in the last granule (a partial one at L = 1000)
      flat   all rotated keys are the same vector: uniform softmax, the output is the mean of v (lrun sums L ones)"""
    g = torch.Generator().manual_seed(1000 * L + {"rise": 1, "fall": 2, "spike": 3, "flat": 4}[case])
    j = torch.arange(L, dtype=torch.float64)
    A = 128.0 ** 0.25
    e = torch.randn(HD, generator=g, dtype=torch.float64)
    e /= e.norm()
    r = 0.6 + 0.4 * torch.rand(L, generator=g, dtype=torch.float64)
    noise = 0.3 * torch.randn(L, HD, generator=g, dtype=torch.float64)
    if case == "rise":
        t = -26.0 + 52.0 * j / (L - 1)
    elif case == "fall":
        t = 26.0 - 52.0 * j / (L - 1)
    elif case == "spike":
        t = 8.0 * torch.rand(L, generator=g, dtype=torch.float64) - 4.0
        t[L - 5] = 26.0
    elif case == "flat":
        t, noise = torch.full((L,), 10.0, dtype=torch.float64), torch.zeros(L, HD, dtype=torch.float64)
    else:
        raise ValueError(case)
    q_rot = (r * A)[:, None] * e[None, :]
    k_rot = (t * (HD ** 0.5) / A)[:, None] * e[None, :] + noise
    cos, sin = (x[:L].double() for x in tables("cpu"))

    def unrope(x):          # the inverse rotation: RoPE(unrope(x)) == x
        x1, x2 = x[:, :64], x[:, 64:]
        return torch.cat([x1 * cos + x2 * sin, -x1 * sin + x2 * cos], dim=-1)

    v = torch.randn(L, HD, generator=g, dtype=torch.float64).clamp(-4.0, 4.0)
    rows = torch.zeros((L + 31) // 32 * 32, 3 * HD, dtype=torch.float32)
    rows[:L] = torch.cat([unrope(q_rot), unrope(k_rot), v], dim=1).float()
    return rows


def stress_scores(rows, L):
    """float64 scores [L, L] of the rounded inputs"""
    cos, sin = (x.double() for x in tables("cpu"))
    x = rows[:L].double().reshape(L, 3, 1, HD)
    q, k = R.rope_ref(x[:, 0], cos, sin)[:, 0], R.rope_ref(x[:, 1], cos, sin)[:, 0]
    return q @ k.T / (HD ** 0.5)


def stress_bound(rows, L):
    """(float64 reference, err32, bound): err32 is the max-abs error against float64 of the SAME formula evaluated in float32
    by torch on the CPU on the same inputs; the kernel gets 4 times that (another summation order, another expf), never less
    than the 2e-5 of the randn tests.  4 * err32 <= 2e-4 is asserted: inputs whose float32 evaluation is itself poor could
    otherwise be chosen to loosen the bound."""
    ref = R.enc_attn_ref(rows, 1, [0], [L], *tables("cpu"))
    r32 = R.enc_attn_ref(rows, 1, [0], [L], *tables("cpu"), dtype=torch.float32)
    err32 = (r32[:L].double() - ref[:L]).abs().max().item()
    assert 4 * err32 <= 2e-4, err32
    return ref, err32, max(TOL, 4 * err32)


def granule_max(s):
    """[L, ceil(L / 32)]: the largest score of every query row in every 32-key granule"""
    L = s.shape[0]
    pad = torch.full((L, (L + 31) // 32 * 32 - L), float("-inf"), dtype=s.dtype)
    return torch.cat([s, pad], dim=1).reshape(L, -1, 32).max(dim=-1).values


# err32 (the float32 CPU evaluation against float64) and the kernel's measured max-abs error on the MI355X, per case; every bound
# comes out as the 2e-5 floor (4 * err32 <= 1.4e-5):
STRESS = [
    # rise,  L = 1024: err32 = 3.2e-06, kernel 3.0e-06
    ("rise", 1024),
    # rise,  L = 1000: err32 = 3.5e-06, kernel 3.4e-06
    ("rise", 1000),
    # fall,  L = 1024: err32 = 3.0e-06, kernel 3.6e-06
    ("fall", 1024),
    # fall,  L = 1000: err32 = 2.9e-06, kernel 3.4e-06
    ("fall", 1000),
    # spike, L = 1024: err32 = 8.5e-07, kernel 1.1e-06
    ("spike", 1024),
    # spike, L = 1000: err32 = 1.0e-06, kernel 1.2e-06
    ("spike", 1000),
    # flat,  L = 1024: err32 = 1.1e-07, kernel 1.3e-07
    ("flat", 1024),
    # flat,  L = 1000: err32 = 1.1e-07, kernel 1.1e-07
    ("flat", 1000),
]


def check_stress_plan(case, L, rows):
    """the constructed inputs do what the case says (float64, on the host)"""
    s = stress_scores(rows, L)
    assert s.abs().max().item() <= 30.0 and rows[:, 2 * HD:].abs().max().item() <= 4.0
    gm = granule_max(s)
    if case == "rise":
        assert (gm[:, 1:] > gm[:, :-1]).all()               # every granule raises every row's running maximum
    elif case == "fall":
        assert (gm[:, 1:] < gm[:, :-1]).all()
    elif case == "spike":
        assert L - 5 >= (L - 1) // 32 * 32                   # the key sits in the last granule (8 keys wide at L = 1000)
        others = torch.cat([s[:, : L - 5], s[:, L - 4:]], dim=1)
        assert (s[:, L - 5] - others.max(dim=1).values).min().item() >= 9.0
    elif case == "flat":
        assert (s.max(dim=1).values - s.min(dim=1).values).max().item() <= 1e-5
    return s


@pytest.mark.parametrize("case,L", STRESS)
def test_softmax_stress(case, L):
    d = dev()
    rows = stress_case(case, L)
    check_stress_plan(case, L, rows)
    ref, err32, bound = stress_bound(rows, L)
    qkv = rows.to(d)
    P, _, _ = launch(qkv, 1, [0], [L])
    out = rows_of(P, qkv.shape[0], 1)
    err = (out[:L].double() - ref[:L]).abs().max().item()
    print(f"softmax stress {case} L={L}: err32 {err32:.3e}, bound {bound:.3e}, kernel max-abs err vs float64 {err:.3e}")
    assert err <= bound, (err, bound)
    assert (out[L:] == SENTINEL).all()
    if case == "flat":          # the mean of v, stated without the reference
        mean = rows[:L, 2 * HD:].double().mean(dim=0)
        assert (out[:L, 0].double() - mean[None]).abs().max().item() <= bound


# ---------------------------------------------------------------------------------------------------------------------
# packing, utterance numbers, stale state, refusals


def test_solo_equals_packed_bitwise():
    """the granule split and the merge order depend on an utterance's length only: its rows in a packed launch equal, bit for
    bit, the launch of that utterance alone at offset 0"""
    d = dev()
    torch.manual_seed(23)
    H, lens = 2, [33, 257, 1024]
    offs, tot = pack(lens)
    qkv = torch.randn(tot, 3 * H * HD, device=d)
    P, _, _ = launch(qkv, H, offs, lens)
    check_against_f64(qkv, H, offs, lens, P)
    for o, n in zip(offs, lens):
        n32 = (n + 31) // 32 * 32
        Ps, _, _ = launch(qkv[o: o + n32].contiguous(), H, [0], [n])
        assert torch.equal(bits(P[:, o // 16: (o + n32) // 16]), bits(Ps)), n


def test_slot_numbers_and_oversized_tables():
    """what a slot admission passes: three utterances carry the numbers 6, 1, 4 of 8-entry seg_off / seg_len tables — not in
    packing order — and the five entries of slots that are not in the call hold other utterances' offsets and lengths (wrong,
    but in range).  The output and the scratch planes equal, bit for bit, those of the same rows numbered 0, 1, 2."""
    d = dev()
    torch.manual_seed(24)
    H, lens = 2, [161, 1, 70]
    offs, tot = pack(lens)
    qkv = torch.randn(tot, 3 * H * HD, device=d)
    P0, kp0, vp0 = launch(qkv, H, offs, lens)
    check_against_f64(qkv, H, offs, lens, P0)
    so = np.array([offs[1], 0, offs[2], offs[0], 0, offs[2], 0, offs[1]], dtype=np.int32)
    sl = np.array([lens[2], 0, lens[1], lens[0], 0, lens[2], 0, lens[1]], dtype=np.int32)
    P1, kp1, vp1 = launch(qkv, H, offs, lens, numbers=[6, 1, 4], table=(so, sl))
    assert torch.equal(bits(P0), bits(P1))
    assert torch.equal(bits(kp0), bits(kp1)) and torch.equal(bits(vp0), bits(vp1))


def poison_padding(qkv, offs, lens):
    """NaN, +Inf and -Inf, in turn, in every row that belongs to no utterance (the tail of an utterance's last 32-row block
    and whole padding blocks alike)"""
    pad = torch.from_numpy(~live_mask(offs, lens, qkv.shape[0])).to(qkv.device)
    junk = torch.tensor([float("nan"), float("inf"), float("-inf")], device=qkv.device)
    n = int(pad.sum().item()) * qkv.shape[1]
    out = qkv.clone()
    out[pad] = junk[torch.arange(n, device=qkv.device) % 3].reshape(-1, qkv.shape[1])
    return out


def test_stale_planes_and_non_finite_padding_rows():
    """the pruned-layer sequence on one scratch: a 4-head launch, then a 2-head launch that finds the 4-head planes there;
    the scratch starts as bf16 NaN and the padding rows of qkv hold NaN / +-Inf.  Output and the planes the launch owns equal
    a run over zeroed scratch and finite padding rows, bit for bit."""
    d = dev()
    torch.manual_seed(25)
    lens = [45, 0, 129, 1, 256]
    offs, tot = pack(lens)
    qkvs = {H: torch.randn(tot, 3 * H * HD, device=d) for H in (4, 2)}
    kp = torch.full((3, 4, tot, HD), float("nan"), dtype=torch.bfloat16, device=d)
    vp = torch.full((3, 4, tot, HD), float("nan"), dtype=torch.bfloat16, device=d)
    for H in (4, 2):
        clean, ckp, cvp = launch(qkvs[H], H, offs, lens)
        check_against_f64(qkvs[H], H, offs, lens, clean)
        dirty_qkv = poison_padding(qkvs[H], offs, lens)
        assert not torch.isfinite(dirty_qkv).all() and torch.equal(dirty_qkv[offs[0]: offs[0] + 45], qkvs[H][offs[0]: offs[0] + 45])
        got, _, _ = launch(dirty_qkv, H, offs, lens, kp=kp, vp=vp)
        assert torch.equal(bits(got), bits(clean)), H
        n = 3 * H * tot * HD                                   # [3][H][rows][128]: what a launch with H heads owns
        assert torch.equal(bits(kp.reshape(-1)[:n]), bits(ckp.reshape(-1))), H
        assert torch.equal(bits(vp.reshape(-1)[:n]), bits(cvp.reshape(-1))), H


def test_refusals_launch_nothing():
    """rows not a multiple of 32, ldq not a multiple of 4, output planes narrower than heads * 128 columns: DIA_E_ARG, and
    neither the output nor the scratch planes are touched"""
    d = dev()
    torch.manual_seed(26)
    H, lens = 2, [40]
    offs, tot = pack(lens)
    qkv = torch.randn(tot, 3 * H * HD, device=d)
    rb = np.full((tot,), -1, dtype=np.int32)
    rb[:40] = 0
    row_b = torch.from_numpy(rb).to(d)
    seg_off = torch.zeros(1, dtype=torch.int32, device=d)
    seg_len = torch.full((1,), 40, dtype=torch.int32, device=d)
    kp = torch.full((3, H, tot, HD), 3.0, dtype=torch.bfloat16, device=d)
    vp = torch.full((3, H, tot, HD), 3.0, dtype=torch.bfloat16, device=d)
    P = lay.pack_planes(torch.full((tot, H * HD), SENTINEL, device=d))
    P_before = P.clone()

    def args():
        return enc_attn_args(qkv, H, row_b, seg_off, seg_len, kp, vp, P)

    bad = []
    a = args(); a.rows = tot - 16; bad.append(("rows % 32", a))
    a = args(); a.rows = 0; bad.append(("rows == 0", a))
    a = args(); a.ldq = 3 * H * HD + 2; bad.append(("ldq % 4", a))
    a = args(); a.p_ktiles = H * HD // 32 - 1; bad.append(("p_ktiles", a))
    for what, a in bad:
        assert hb.lib().dia_enc_attn(C.byref(a), None) == -1, what          # DIA_E_ARG
        assert hb.lib().dia_last_error()
    torch.cuda.synchronize()
    assert torch.equal(bits(P), bits(P_before)) and (kp == 3.0).all() and (vp == 3.0).all()
    hb.check(hb.lib().dia_enc_attn(C.byref(args()), None), "dia_enc_attn")     # the same arguments, unbroken, do launch
    torch.cuda.synchronize()
    assert not torch.equal(bits(P), bits(P_before)) and not (kp == 3.0).all()
