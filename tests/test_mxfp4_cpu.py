"""MXFP4 weight-only quantisation (dia_hip/quant.py), the stream layout (layout.tile_weight_fp4), DeviceWeights(quant="mxfp4"),
the knob and the C ABI additions, on the CPU (no GPU needed)."""
import ctypes
import os
import subprocess
import sys
import tempfile

import pytest
import torch

from dia_hip import binding as hb
from dia_hip import config as C
from dia_hip import dist as D
from dia_hip import layout as lay
from dia_hip import quant as Q
from dia_hip.pruning import _kernel_2d
from dia_hip.weights import param_shapes, synthetic_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MATS = ("qkv", "o", "cq", "co", "wi", "wo")
VALUES = torch.tensor(Q.E2M1_VALUES)
MIDPOINTS = torch.tensor(Q.E2M1_MIDPOINTS)


def _edge_blocks():
    """[32 * 6, 4]: blocks built to hit the edges, every one with a block maximum that fixes X = 1 (amax in [4, 8)) unless noted"""
    w = torch.zeros(32 * 6, 4)
    # block 0: all zero (every column)
    # block 1: one huge element, everything else tiny
    w[32:64] = 1e-6
    w[40, :] = torch.tensor([3.0e4, -1.0e3, 7.0, 2.0 ** 20])
    # block 2: values exactly on the seven midpoints (both signs), block maximum 4 -> X = 1
    w[64:71, 0], w[64:71, 1] = MIDPOINTS, -MIDPOINTS
    w[64:71, 2], w[64:71, 3] = MIDPOINTS * 1.0000001, MIDPOINTS * 0.9999999     # just beside them
    w[95, :] = 4.0
    # block 3: the same midpoints at another scale (X = 2^-7)
    w[96:128] = w[64:96] * 2.0 ** -7
    # block 4: amax / X in (6, 8)
    w[128:160] = 0.3
    w[130, :] = torch.tensor([6.01, -7.0, 7.5, -7.999])
    # block 5: amax / X in (6, 8) at X = 2^5, and elements of |w / X| <= 7 around it
    w[160:192] = 2.0 ** 5 * torch.linspace(-7.0, 7.0, 32)[:, None]
    w[161, :] = 2.0 ** 5 * 7.9
    return w


def _cases():
    gen = torch.Generator().manual_seed(4)
    return [("n512x48", torch.randn(512, 48, generator=gen) * 0.02), ("n96x20", torch.randn(96, 20, generator=gen) * 1.3),
            ("edges", _edge_blocks())]


# ---- quantiser -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,w", _cases(), ids=[c[0] for c in _cases()])
def test_quantiser(name, w):
    K, N = w.shape
    Kp = (K + 31) // 32 * 32
    codes, sc = Q.mxfp4_quantize_2d(w)
    assert codes.shape == (Kp, N) and codes.dtype == torch.uint8 and sc.shape == (Kp // 32, N) and sc.dtype == torch.uint8
    assert int(codes.max()) < 16
    wp = torch.zeros(Kp, N)
    wp[:K] = w
    b = wp.reshape(Kp // 32, 32, N)
    amax = b.abs().amax(dim=1)
    e = torch.where(amax > 0, torch.floor(torch.log2(amax.double())).to(torch.int32) - 2, torch.zeros(1, dtype=torch.int32))
    assert torch.equal(sc.to(torch.int32) - 127, e)                 # e = floor(log2 amax) - 2; zero block: e = 0
    X = torch.exp2(e.float())[:, None, :].expand_as(b)
    dq = Q.mxfp4_dequantize_2d(codes, sc)
    dqb = dq.reshape(Kp // 32, 32, N)
    err = (b - dqb).abs()
    assert (err <= 2.0 * X).all()
    near = (b / X).abs() <= 7.0
    assert (err[near] <= X[near]).all()
    assert (dqb.abs() <= 6.0 * X).all()                             # nothing exceeds +-6 X
    assert torch.equal(dq.bfloat16().float(), dq)                   # every dequantised value is a bf16 value
    # nearest: no representable magnitude is closer to the clamped |w / X| than the one chosen
    r = (b / X).abs().clamp(max=6.0)
    best = (r[..., None] - VALUES).abs().amin(dim=-1)
    assert torch.equal((r - dqb.abs() / X).abs(), best)
    rounded = Q.mxfp4_round_2d(w)
    assert rounded.shape == w.shape and torch.equal(rounded, dq[:K])
    assert Q.is_mxfp4(rounded) and not Q.is_mxfp4(w)
    c2, s2 = Q.mxfp4_quantize_2d(dq)                                # quantise(dequantise(q)) == q, bit for bit
    assert torch.equal(c2, codes) and torch.equal(s2, sc)


def test_ties_go_to_the_even_code_and_zero_blocks():
    w = _edge_blocks()
    codes, sc = Q.mxfp4_quantize_2d(w)
    assert (sc[0] == 127).all() and (codes[0:32] == 0).all()        # all-zero block: e = 0, code 0
    even_up = torch.tensor([0, 2, 2, 4, 4, 6, 6], dtype=torch.uint8)   # midpoint i lies between codes i and i + 1: the even one
    for blk, e in ((2, 0), (3, -7)):
        r = slice(32 * blk, 32 * blk + 7)
        assert (sc[blk] == 127 + e).all()
        assert torch.equal(codes[r, 0], even_up)
        assert torch.equal(codes[r, 1], torch.where(even_up > 0, even_up | 8, even_up))      # the sign bit; zero has one code
        assert torch.equal(codes[r, 2], torch.arange(1, 8, dtype=torch.uint8))               # just above: the upper code
        assert torch.equal(codes[r, 3], torch.arange(0, 7, dtype=torch.uint8))               # just below: the lower one
    # amax / X in (6, 8): clamped to 6, never to the next binade
    assert (sc[4] == 127).all() and torch.equal(codes[130] & 7, torch.full((4,), 7, dtype=torch.uint8))
    assert torch.equal(Q.mxfp4_round_2d(w)[130], torch.tensor([6.0, -6.0, 6.0, -6.0]))
    # one huge element: the rest of its block rounds to zero
    dq = Q.mxfp4_round_2d(w)
    assert (dq[32:40] == 0).all() and dq[40, 3] == 2.0 ** 20 and dq[40, 2] == 6.0 and dq[40, 1] == -768.0


def test_scale_clamp():
    w = torch.zeros(64, 2)
    w[0, 0] = 2.0 ** -120
    w[33, 1] = 3.0
    codes, sc = Q.mxfp4_quantize_2d(w)
    assert sc[0, 0].item() == 127 - 100 and sc[1, 1].item() == 127 - 1
    dq = Q.mxfp4_round_2d(w)
    assert dq[0, 0] == 0.0 and dq[33, 1] == 3.0


# ---- layout ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,N", [(512, 48), (1056, 20)])
def test_tile_weight_fp4_round_trip(K, N):
    gen = torch.Generator().manual_seed(K + N)
    w = torch.randn(K, N, generator=gen) * 0.02
    stream, kt, ns = lay.tile_weight_fp4(w)
    G = (K + 511) // 512
    assert kt == (K + 31) // 32 and ns == (N + 15) // 16
    assert lay.FP4_GROUP_BYTES == 4352
    assert stream.dtype == torch.uint8 and stream.shape == (ns, G, 4352)
    assert torch.equal(lay.untile_weight_fp4(stream, K, N), Q.mxfp4_round_2d(w))
    if K % 512 == 0:
        dense, _, _ = lay.tile_weight(w)
        assert stream.numel() * 64 == dense.numel() * 2 * 17        # 4352 / 16384 = 0.265625 of the dense tiles' bytes


def test_tile_weight_fp4_operand_order():
    """k-tile t, lane l = 16 q + c, element j = W[32 t + 8 q + j][c]: nibble j & 1 of byte 4 (t % 4) + (j >> 1) of lane l of slot
    (t % 16) / 4 behind the group's 256-byte scale block, whose byte 16 c + t % 16 is the block's E8M0 scale"""
    K, N = 1024, 32
    for j in (4, 5):
        w = torch.zeros(K, N)
        t, q, c, strip = 21, 2, 7, 1
        w[32 * t + 8 * q + j, 16 * strip + c] = -1.5                 # X = 2^-2, element -6: code 0xf
        stream, kt, ns = lay.tile_weight_fp4(w)
        g, p, i = t // 16, (t % 16) // 4, t % 4
        byte = stream[strip, g, 256 + p * 1024 + (16 * q + c) * 16 + 4 * i + (j >> 1)].item()
        assert byte == (0xf0 if j & 1 else 0x0f)
        assert stream[strip, g, c * 16 + t % 16].item() == 127 - 2
        assert int((stream[:, :, 256:] != 0).sum()) == 1 and int((stream[:, :, :256] != 127).sum()) == 1


# ---- state dict and tool -----------------------------------------------------------------------------------------------
def test_quantize_state_dict_touches_exactly_the_streamed_matrices():
    cfg = C.tiny_config()
    gen = torch.Generator().manual_seed(3)
    sd = {k: (torch.randn(shp, generator=gen) * 0.05 if not k.endswith("norm.weight") else torch.ones(shp))
          for k, shp in param_shapes(cfg).items()}
    qsd = Q.mxfp4_quantize_state_dict(cfg, sd)
    names = Q.mxfp8_names(cfg)
    assert Q.mx_names is Q.mxfp8_names
    assert set(k for k in sd if not torch.equal(qsd[k], sd[k])) == set(names)
    for k in names:
        assert qsd[k].shape == sd[k].shape and qsd[k].dtype == torch.float32 and Q.is_mxfp4(_kernel_2d(k, qsd[k])), k
    again = Q.mxfp4_quantize_state_dict(cfg, qsd)
    assert all(torch.equal(again[k], qsd[k]) for k in qsd)


def test_offline_quantize_tool_and_cli_flag(tmp_path):
    sys.path.insert(0, ROOT)
    import cli
    import offline_quantize
    cfg = C.tiny_config()
    sd = synthetic_state_dict(cfg, seed=5, std=0.02)
    src = tmp_path / "m"
    src.mkdir()
    torch.save(sd, src / "pytorch_model.bin")
    cfg.save(str(src / "config.json"))
    assert offline_quantize.main(["--model-path", str(src), "--output-dir", str(tmp_path / "q"), "--format", "mxfp4"]) == 0
    got = torch.load(tmp_path / "q" / "pytorch_model.bin", weights_only=True)
    want = Q.mxfp4_quantize_state_dict(cfg, {k: v.float() for k, v in sd.items()})
    assert all(torch.equal(got[k], want[k]) for k in want)
    assert cli.build_parser().parse_args(["hi", "--codes-output", "x.npy", "--weight-format", "mxfp4"]).weight_format == "mxfp4"


# ---- DeviceWeights(quant="mxfp4") on CPU tensors -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mid():
    cfg = C.mid_config()
    raw = synthetic_state_dict(cfg, seed=1234, std=0.02)
    return cfg, raw, Q.mxfp4_quantize_state_dict(cfg, raw)


def test_device_weights_mxfp4_streams_and_signature(mid):
    from dia_hip.engine import DeviceWeights
    cfg, raw, sd = mid
    dev = torch.device("cpu")
    w = DeviceWeights(cfg, sd, dev, quant="mxfp4")
    dense = DeviceWeights(cfg, sd, dev)
    assert w.quant == "mxfp4" and w.logits_f8 is None and dense.logits_f4 is None and dense.dec_layers[0]["wof4"] is None
    for L in w.dec_layers:
        for k in MATS:
            f4, dn = L[k + "f4"], L[k]
            assert L[k + "f8"] is None and f4.ns == dn.ns and f4.kt == dn.kt and f4.t.dtype == torch.uint8, k
            assert torch.equal(lay.untile_weight_fp4(f4.t, dn.kt * 32, dn.ns * 16), lay.untile_weight(dn.t, dn.kt * 32, dn.ns * 16)), k
            assert f4.nbytes * 64 == dn.nbytes * 17
    assert w.max_weight_rounding == 0.0
    ts, dts = w.tensors(), dense.tensors()                          # the streams lie behind everything the dense model holds
    assert len(ts) == len(dts) + 6 * len(w.dec_layers) + 1 and ts[len(dts)] is w.dec_layers[0]["qkvf4"].t and ts[-1] is w.logits_f4.t
    assert torch.equal(w.flat[: dense.flat.numel()], dense.flat)
    # what a step streams follows the knob mxfp4, not mxfp8
    full = sum(L[k + "f4"].nbytes for L in w.dec_layers for k in MATS) + w.logits_f4.nbytes
    try:
        hb.set_tuning("mxfp4", 0x7f7f)
        hb.set_tuning("mxfp8", 0)
        assert w.decode_weight_bytes(2) == w.decode_weight_bytes(16) == full
        assert w.decode_weight_bytes(17) == dense.decode_weight_bytes()
        hb.set_tuning("mxfp4", 0x0020)                              # wo alone, at most 4 rows
        saved = sum(L["wo"].nbytes - L["wof4"].nbytes for L in w.dec_layers)
        assert w.decode_weight_bytes(4) == dense.decode_weight_bytes() - saved and w.decode_weight_bytes(5) == dense.decode_weight_bytes()
    finally:
        hb.set_tuning("mxfp4", -1)
        hb.set_tuning("mxfp8", -1)
    # off / mxfp8 / mxfp4 arenas are told apart, also by an empty receiver
    f8 = DeviceWeights(cfg, Q.mxfp8_quantize_state_dict(cfg, raw), dev, quant="mxfp8")
    sigs = [tuple(D._arena_signature(x)) for x in (dense, f8, w)]
    assert len(set(sigs)) == 3 and len(set(s[3] for s in sigs)) == 3
    empty = DeviceWeights.empty_like_config(cfg, dev, quant="mxfp4")
    assert D._arena_signature(empty) == D._arena_signature(w)


def test_device_weights_mxfp4_rejections(mid):
    from dia_hip.engine import DeviceWeights
    from dia_hip.pruning import semi_structured_prune_state_dict, structured_prune_state_dict
    cfg, raw, sd = mid
    dev = torch.device("cpu")
    with pytest.raises(hb.DiaHipError, match=r"decoder\.layers\.0\.qkv is not MXFP4"):
        DeviceWeights(cfg, raw, dev, quant="mxfp4")
    with pytest.raises(hb.DiaHipError, match=r"is not MXFP4"):       # an MXFP8 checkpoint is not an MXFP4 one
        DeviceWeights(cfg, Q.mxfp8_quantize_state_dict(cfg, raw), dev, quant="mxfp4")
    with pytest.raises(hb.DiaHipError, match="weight_planes"):
        DeviceWeights(cfg, sd, dev, weight_planes=2, quant="mxfp4")
    with pytest.raises(hb.DiaHipError, match="seg"):
        DeviceWeights(cfg, sd, dev, seg="on", quant="mxfp4")
    with pytest.raises(hb.DiaHipError, match="2:4"):
        DeviceWeights(cfg, semi_structured_prune_state_dict(cfg, sd), dev, sparse="2:4", quant="mxfp4")
    spd, _ = structured_prune_state_dict(cfg, raw, 0.5)
    with pytest.raises(hb.DiaHipError, match="compacted"):
        DeviceWeights(cfg, Q.mxfp4_quantize_state_dict(cfg, spd), dev, quant="mxfp4")
    with pytest.raises(hb.DiaHipError, match="multiple of 512"):
        DeviceWeights._tile_mx("m", Q.mxfp4_round_2d(torch.randn(96, 16)), "mxfp4")
    with pytest.raises(ValueError):
        DeviceWeights(cfg, sd, dev, quant="mxfp6")


# ---- C ABI -----------------------------------------------------------------------------------------------------------
def test_abi_number_and_struct_sizes_unchanged():
    L = hb.lib()
    assert hasattr(L, "dia_mxfp4_classes") and hasattr(L, "dia_engine_set_mxfp4")
    assert hb.ABI_VERSION == 8 and L.dia_abi_version() == 8 and hb.W_MXFP4 == 4 and hb.W_MXFP8 == 2
    prog = r'''
    #include <stdio.h>
    #include "dia_hip.h"
    int main(void){ printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d\n", sizeof(dia_gemm_args), sizeof(dia_attn_args),
        sizeof(dia_embed_args), sizeof(dia_sample_args), sizeof(dia_dec_layer), sizeof(dia_engine_desc), sizeof(dia_enc_attn_args),
        sizeof(dia_dec_prefill_args), sizeof(dia_seg_args), sizeof(dia_mxfp4_layer), sizeof(dia_mxfp4_streams), DIA_W_MXFP4); return 0; }
    '''
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "s.c")
        open(c, "w").write(prog)
        exe = os.path.join(td, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        sizes = [int(v) for v in subprocess.check_output([exe]).split()]
    assert sizes[:9] == [296, 168, 120, 296, 312, 584, 112, 200, 144]      # the nine pinned structs, as before the MXFP4 stream
    assert sizes[9:] == [ctypes.sizeof(hb.Mxfp4Layer), ctypes.sizeof(hb.Mxfp4Streams), hb.W_MXFP4]
    assert L.dia_engine_set_mxfp4(None, None) == -1 and b"null engine" in L.dia_last_error()


def test_knob_mxfp4_round_trips_and_drives_the_classes():
    try:
        assert hb.get_tuning("mxfp4") == -1
        assert [hb.mxfp4_mask(r) for r in (1, 4, 5, 16, 17)] == [0x70, 0x70, 0x50, 0x50, 0]      # the initial default, 0x5070
        hb.set_tuning("mxfp4", 0x2541)
        assert hb.get_tuning("mxfp4") == 0x2541
        assert [hb.mxfp4_mask(r) for r in (1, 4, 5, 16, 17)] == [0x41, 0x41, 0x25, 0x25, 0]
        assert hb.mxfp8_mask(1) == 0x70                               # the other knob is untouched
        hb.set_tuning("mxfp4", 0)
        assert [hb.mxfp4_mask(r) for r in (1, 4, 5, 16, 17)] == [0, 0, 0, 0, 0]
        hb.set_tuning("mxfp4", 0xffff)
        assert hb.mxfp4_mask(2) == 0x7f and hb.mxfp4_mask(8) == 0x7f and hb.mxfp4_mask(0) == 0
    finally:
        hb.set_tuning("mxfp4", -1)
    assert hb.get_tuning("mxfp4") == -1


def test_dia_gemm_mxfp4_refuses_unsupported_combinations_without_a_gpu():
    L = hb.lib()
    buf = ctypes.create_string_buffer(64)                          # never dereferenced: every case is refused before a launch
    addr = ctypes.addressof(buf)

    def rc_of(**kw):
        g = hb.GemmArgs()
        g.A, g.W, g.out = addr, addr, addr
        g.a_ktiles, g.M, g.KT, g.nstrips, g.epi, g.ldo, g.act_f32, g.w_format, g.ssq_ld = 16, 4, 16, 2, hb.EPI_SCALE_STORE, 32, 3, hb.W_MXFP4, 16
        for k, v in kw.items():
            setattr(g, k, v)
        rc = L.dia_gemm(ctypes.byref(g), None)
        return rc, L.dia_last_error()
    for kw, word in ((dict(M=17), b"16 rows"), (dict(w_planes=2), b"w_planes"), (dict(w_planes=3), b"w_planes"), (dict(w_layout=1), b"w_layout"),
                     (dict(sp_blocks=addr), b"sp_blocks"), (dict(epi=hb.EPI_CROSSKV), b"CROSSKV"), (dict(cmap=addr), b"compaction"),
                     (dict(strip_map=addr), b"compaction"), (dict(act_f32=0), b"planes"), (dict(epi=hb.EPI_SWIGLU_EMIT, act_f32=1), b"planes"),
                     (dict(KT=24, a_ktiles=24), b"512"),
                     (dict(KT=32, a_ktiles=32, sk=4, sk_scratch=addr, sk_tickets=addr), b"512"), (dict(KT=256, a_ktiles=256), b"128 k-tiles")):
        rc, msg = rc_of(**kw)
        assert rc == -1 and b"MXFP4" in msg and word in msg, (kw, rc, msg)
    for fmt in (3, 5):                                             # 3 stays unassigned
        rc, msg = rc_of(w_format=fmt)
        assert rc == -1 and b"w_format" in msg
