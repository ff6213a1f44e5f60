"""The unstructured sparse weight stream: layout.tile_weight_us / untile_weight_us, DeviceWeights(sparse="unstructured"), the knob
and the C ABI additions, on the CPU (no GPU needed)."""
import ctypes
import os
import subprocess
import sys
import tempfile

import pytest
import torch

from dia_hip import binding as hb
from dia_hip import config as C
from dia_hip import layout as lay
from dia_hip.pruning import unstructured_prune_state_dict
from dia_hip.weights import synthetic_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MATS = ("qkv", "o", "cq", "co", "wi", "wo")


def crafted(K, N, R):
    """lane-tiles (8 consecutive K of a column) with 0, exactly R, R + 1 and 8 non-zeros, an all-zero k-tile, a fully dense column, a
    negative zero; with N > 16 also a strip with an empty overflow list and a strip whose whole overflow sits in one column"""
    gen = torch.Generator().manual_seed(K + N + R)
    val = (torch.randn(K, N, generator=gen) * 0.1).bfloat16().float()
    val[val == 0] = 0.5
    w = torch.zeros(K, N)
    w[0:R, 0] = val[0:R, 0]                                  # exactly R
    w[8:8 + R + 1, 0] = val[8:8 + R + 1, 0]                  # R + 1: one overflow entry
    w[16:24, 0] = val[16:24, 0]                              # 8
    w[64:96, :] = 0.0                                        # an all-zero k-tile (it is anyway)
    w[:, 5] = val[:, 5]                                      # a fully dense column: the strip's whole overflow but one entry
    w[40, 7] = -0.0                                          # a negative zero: dropped
    w[41, 7] = val[41, 7]
    if N > 16:
        w[100:103:2, 17] = val[100:103:2, 17]                # strip 1: two non-zeros per lane-tile at most -> an empty overflow list
        w[:, 37] = val[:, 37]                                # strip 2: its whole overflow sits in one column
    return w


@pytest.mark.parametrize("R", [4, 2])
@pytest.mark.parametrize("K,N", [(512, 16), (1024, 40)])
def test_round_trip_crafted(K, N, R):
    w = crafted(K, N, R)
    s, kt, ns = lay.tile_weight_us(w, R)
    assert s.dtype == torch.uint8 and s.dim() == 1 and kt == K // 32 and ns == (N + 15) // 16
    back = lay.untile_weight_us(s, K, N, R)
    assert torch.equal(back, w.bfloat16().float())
    assert not torch.signbit(back[40, 7])                    # the negative zero did not travel
    G = (kt + 15) // 16
    gb = lay.us_group_bytes(R)
    tab = s[ns * G * gb: ns * G * gb + 4 * (ns * G * 16 + 1)].reshape(-1, 4).to(torch.int64)
    tab = (tab << (8 * torch.arange(4))).sum(dim=1)
    runs = (tab[1:] - tab[:-1]).reshape(ns, G, 16)
    assert runs[0, 0, 0] == 1 + (8 - R) and runs[0, :, 5].sum() == (K // 8) * (8 - R) and runs[0, :, 7].sum() == 0
    if N > 16:
        assert runs[1].sum() == 0                            # a strip with an empty overflow list
        assert runs[2].sum() == runs[2, :, 5].sum() > 0      # a strip whose whole overflow sits in one column (37 = 32 + 5)
    assert s.numel() == lay.us_stream_bytes(ns, G, R, int(tab[-1]))


@pytest.mark.parametrize("R", [4, 2])
def test_round_trip_fully_dense_random(R):
    w = torch.randn(700, 33, generator=torch.Generator().manual_seed(R))
    w[w.bfloat16() == 0] = 1.0
    s, kt, ns = lay.tile_weight_us(w, R)
    assert torch.equal(lay.untile_weight_us(s, 700, 33, R), w.bfloat16().float())
    # everything beyond R per lane-tile of the UNPADDED matrix spills
    nz = torch.zeros(kt * 32, ns * 16, dtype=torch.bool)
    nz[:700, :33] = True
    spilled = (nz.reshape(-1, 8, ns * 16).sum(dim=1) - R).clamp(min=0).sum().item()
    assert s.numel() == lay.us_stream_bytes(ns, (kt + 15) // 16, R, spilled)


def test_stream_sizes_and_the_choice_of_rate():
    gen = torch.Generator().manual_seed(9)
    K, N = 2048, 256
    w = torch.randn(K, N, generator=gen).bfloat16().float() * (torch.rand(K, N, generator=gen) >= 0.6)
    cnt = (w != 0).reshape(K // 8, 8, N).sum(dim=1)
    sizes = {}
    for R in (4, 2):
        s, kt, ns = lay.tile_weight_us(w, R)
        spilled = int((cnt - R).clamp(min=0).sum())
        # the docstring's formula: fixed part + run table + 4 bytes per spilled value (each padded to 16) + 16
        want = ns * 4 * (1024 + 2048 * R) + (4 * (ns * 4 * 16 + 1) + 15) // 16 * 16 + (4 * spilled + 15) // 16 * 16 + 16
        assert s.numel() == want == lay.us_stream_bytes(ns, 4, R, spilled)
        sizes[R] = want
    dense = (K // 32) * (N // 16) * 1024
    assert abs(sizes[4] / dense - 0.62) < 0.01               # the issue's table: 60 % zeros at R = 4
    pick = lay.us_choose(w)
    assert pick[1] == min(sizes, key=sizes.get) and pick[4] == min(sizes.values()) and pick[5] == dense
    assert lay.us_choose(torch.randn(512, 32, generator=gen)) is None          # a dense matrix: no stream
    assert lay.us_choose(w, max_ratio=0.5) is None
    with pytest.raises(ValueError):
        lay.tile_weight_us(w, 3)


# ---- DeviceWeights(sparse="unstructured") on CPU tensors ---------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    cfg = C.mid_config()
    raw = synthetic_state_dict(cfg, seed=1234, std=0.02)
    return cfg, raw, unstructured_prune_state_dict(cfg, raw, 0.6)


def test_device_weights_unstructured_streams(tiny):
    from dia_hip.engine import DeviceWeights
    cfg, raw, sd = tiny
    dev = torch.device("cpu")
    w = DeviceWeights(cfg, sd, dev, sparse="unstructured", compact="off")
    dense = DeviceWeights(cfg, sd, dev, compact="off")
    assert w.sparse == "unstructured" and dense.logits_us is None and dense.dec_layers[0]["wous"] is None
    n = 0
    for i, L in enumerate(w.dec_layers):
        for k in MATS:
            us, dn = L[k + "us"], L[k]
            name = f"decoder.layers.{i}.{k}"
            assert w.dense_bytes[name] == dn.nbytes
            if us is None:
                assert w.us_bytes[name] == 0
                continue
            n += 1
            assert us.ns == dn.ns and us.kt == dn.kt and us.rate in (4, 2) and w.us_bytes[name] == us.nbytes < dn.nbytes
            assert torch.equal(lay.untile_weight_us(us.t, dn.kt * 32, dn.ns * 16, us.rate), lay.untile_weight(dn.t, dn.kt * 32, dn.ns * 16)), k
    assert n > 0
    assert torch.equal(w.flat[: dense.flat.numel()], dense.flat)   # the streams lie behind everything the dense model holds
    none = DeviceWeights(cfg, raw, dev, sparse="unstructured", compact="off")          # a dense checkpoint: no matrix gets a stream
    assert all(L[k + "us"] is None for L in none.dec_layers for k in MATS) and none.logits_us is None
    try:                                                     # what a step streams follows the knob usparse
        hb.set_tuning("usparse", 0)
        assert w.decode_weight_bytes(2) == dense.decode_weight_bytes(2)
        hb.set_tuning("usparse", 0x7f)
        assert w.decode_weight_bytes(2) < dense.decode_weight_bytes(2) and w.decode_weight_bytes(6) == dense.decode_weight_bytes(6)
    finally:
        hb.set_tuning("usparse", -1)


def test_device_weights_unstructured_rejections(tiny):
    from dia_hip.engine import DeviceWeights
    from dia_hip.pruning import structured_prune_state_dict
    cfg, raw, sd = tiny
    dev = torch.device("cpu")
    with pytest.raises(hb.DiaHipError, match="weight_planes"):
        DeviceWeights(cfg, sd, dev, weight_planes=2, sparse="unstructured")
    with pytest.raises(hb.DiaHipError, match="seg"):
        DeviceWeights(cfg, sd, dev, seg="on", sparse="unstructured")
    with pytest.raises(hb.DiaHipError, match="quant"):
        DeviceWeights(cfg, sd, dev, quant="mxfp8", sparse="unstructured")
    spd, _ = structured_prune_state_dict(cfg, raw, 0.5)
    with pytest.raises(hb.DiaHipError, match="compacted"):
        DeviceWeights(cfg, spd, dev, sparse="unstructured")
    with pytest.raises(hb.DiaHipError, match="multiple of 512"):
        DeviceWeights._tile_us(DeviceWeights.__new__(DeviceWeights), "m", torch.zeros(96, 16))
    with pytest.raises(hb.DiaHipError, match="every rank"):
        DeviceWeights.empty_like_config(cfg, dev, sparse="unstructured")
    with pytest.raises(ValueError):
        DeviceWeights(cfg, sd, dev, sparse="1:2")


def test_offline_prune_unstructured_output_loads(tmp_path):
    sys.path.insert(0, ROOT)
    import cli
    import offline_prune
    from dia_hip.engine import DeviceWeights
    cfg = C.mid_config()
    sd = synthetic_state_dict(cfg, seed=5, std=0.02)
    src = tmp_path / "m"
    src.mkdir()
    torch.save(sd, src / "pytorch_model.bin")
    cfg.save(str(src / "config.json"))
    assert offline_prune.main(["--model-path", str(src), "--output-dir", str(tmp_path / "p"), "--prune-mode", "unstructured",
                               "--prune-amount", "0.6"]) == 0
    got = torch.load(tmp_path / "p" / "pytorch_model.bin", weights_only=True)
    w = DeviceWeights(cfg, {k: v.float() for k, v in got.items()}, torch.device("cpu"), sparse="unstructured", compact="off")
    assert any(L[k + "us"] is not None for L in w.dec_layers for k in MATS)
    assert cli.build_parser().parse_args(["hi", "--codes-output", "x.npy", "--sparse-weights", "unstructured"]).sparse_weights == "unstructured"


# ---- C ABI -----------------------------------------------------------------------------------------------------------
def test_abi_number_and_new_struct_sizes():
    L = hb.lib()
    assert hasattr(L, "dia_usparse_classes") and hasattr(L, "dia_engine_set_usparse")
    assert hb.ABI_VERSION == 8 and L.dia_abi_version() == 8 and hb.W_USPARSE == 5
    prog = r'''
    #include <stdio.h>
    #include "dia_hip.h"
    int main(void){ printf("%zu %zu %zu %zu %zu %zu %d\n", sizeof(dia_gemm_args), sizeof(dia_dec_layer), sizeof(dia_engine_desc),
        sizeof(dia_us_mat), sizeof(dia_us_layer), sizeof(dia_us_streams), DIA_W_USPARSE); return 0; }
    '''
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "s.c")
        open(c, "w").write(prog)
        exe = os.path.join(td, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        sizes = [int(v) for v in subprocess.check_output([exe]).split()]
    assert sizes[:3] == [296, 312, 584]                      # no existing struct changed
    assert sizes[3:] == [ctypes.sizeof(hb.UsMat), ctypes.sizeof(hb.UsLayer), ctypes.sizeof(hb.UsStreams), 5] == [16, 96, 32, 5]
    assert L.dia_engine_set_usparse(None, None) == -1 and b"null engine" in L.dia_last_error()


def test_knob_usparse_round_trips_and_drives_the_classes():
    try:
        assert hb.get_tuning("usparse") == -1
        assert [hb.usparse_mask(r) for r in (0, 1, 4, 5)] == [0, 0, 0, 0]          # opt-in: nothing streams by default
        hb.set_tuning("usparse", 0x7f)
        assert hb.get_tuning("usparse") == 0x7f
        assert [hb.usparse_mask(r) for r in (0, 1, 2, 4, 5, 16)] == [0, 0x7f, 0x7f, 0x7f, 0, 0]
        hb.set_tuning("usparse", 0x130)
        assert hb.usparse_mask(2) == 0x30 and hb.usparse_mask(5) == 0
        assert hb.mxfp8_mask(1) == 0x70 and hb.mxfp4_mask(1) == 0x70               # the other knobs are untouched
    finally:
        hb.set_tuning("usparse", -1)
    assert hb.get_tuning("usparse") == -1


def test_dia_gemm_usparse_refuses_unsupported_combinations_without_a_gpu():
    L = hb.lib()
    buf = ctypes.create_string_buffer(64)                    # never dereferenced on the device: every case is refused before a launch
    addr = ctypes.addressof(buf)
    um = hb.UsMat(stream=addr, rate=4)
    uaddr = ctypes.addressof(um)

    def rc_of(**kw):
        g = hb.GemmArgs()
        g.A, g.W, g.out = addr, uaddr, addr
        g.a_ktiles, g.M, g.KT, g.nstrips, g.epi, g.ldo, g.act_f32, g.w_format, g.ssq_ld = 16, 4, 16, 2, hb.EPI_SCALE_STORE, 32, 3, hb.W_USPARSE, 16
        for k, v in kw.items():
            setattr(g, k, v)
        rc = L.dia_gemm(ctypes.byref(g), None)
        return rc, L.dia_last_error()
    for kw, word in ((dict(M=5), b"4 rows"), (dict(w_planes=2), b"w_planes"), (dict(w_planes=3), b"w_planes"), (dict(w_layout=1), b"w_layout"),
                     (dict(sp_blocks=addr), b"sp_blocks"), (dict(epi=hb.EPI_CROSSKV), b"CROSSKV"), (dict(cmap=addr), b"compaction"),
                     (dict(strip_map=addr), b"compaction"), (dict(act_f32=0), b"planes"), (dict(epi=hb.EPI_SWIGLU_EMIT, act_f32=1), b"planes"),
                     (dict(KT=24, a_ktiles=24), b"512"), (dict(W=addr), b"dia_us_mat"),
                     (dict(KT=32, a_ktiles=32, sk=4, sk_scratch=addr, sk_tickets=addr), b"512"), (dict(KT=256, a_ktiles=256), b"128 k-tiles")):
        rc, msg = rc_of(**kw)
        assert rc == -1 and b"unstructured sparse stream" in msg and word in msg, (kw, rc, msg)
    um.rate = 3
    rc, msg = rc_of()
    assert rc == -1 and b"4 or 2" in msg
    rc, msg = rc_of(w_format=3)                              # 3 stays unassigned
    assert rc == -1 and b"unknown w_format" in msg
