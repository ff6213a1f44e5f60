"""MXFP8 weight-only quantisation (dia_hip/quant.py), the stream layout (layout.tile_weight_fp8), DeviceWeights(quant="mxfp8"),
the tool and the flag, on the CPU (no GPU needed)."""
import ctypes
import os
import sys

import pytest
import torch

from dia_hip import binding as hb
from dia_hip import config as C
from dia_hip import layout as lay
from dia_hip import quant as Q
from dia_hip.pruning import _kernel_2d
from dia_hip.weights import param_shapes, synthetic_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MATS = ("qkv", "o", "cq", "co", "wi", "wo")


def _random_sd(cfg, seed=3):
    gen = torch.Generator().manual_seed(seed)
    return {k: (torch.randn(shp, generator=gen) * 0.05 if not k.endswith("norm.weight") else torch.ones(shp))
            for k, shp in param_shapes(cfg).items()}


def _matrix(K, N, std, seed):
    gen = torch.Generator().manual_seed(seed)
    w = torch.randn(K, N, generator=gen) * std
    w[0:32, 0] = 0.0                                              # an all-zero block
    w[32:64, 1] = 0.0
    w[40, 1] = 100.0 * std                                        # a one-spike block
    return w


# ---- quantiser -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("std", [1e-6, 0.02, 1.0])
def test_quantiser_elements_scales_and_error_bound(std):
    K, N = 2048, 512
    w = _matrix(K, N, std, seed=7)
    el, sc = Q.mxfp8_quantize_2d(w)
    assert el.shape == (K, N) and el.dtype == torch.uint8 and sc.shape == (K // 32, N) and sc.dtype == torch.uint8
    b = w.reshape(K // 32, 32, N)
    amax = b.abs().amax(dim=1)
    e = torch.where(amax > 0, torch.floor(torch.log2(amax.double())).to(torch.int32) - 8, torch.zeros(1, dtype=torch.int32))
    assert torch.equal(sc.to(torch.int32) - 127, e)               # e = floor(log2 amax) - 8; zero block: e = 0
    assert sc[0, 0].item() == 127 and (el[0:32, 0] == 0).all()
    X = torch.exp2(e.float())[:, None, :]
    scaled = (b / X).clamp(-448.0, 448.0)
    assert torch.equal(el.reshape(K // 32, 32, N), scaled.to(torch.float8_e4m3fn).view(torch.uint8))     # bit for bit
    dq = Q.mxfp8_dequantize_2d(el, sc)
    assert torch.isfinite(dq).all()
    assert torch.equal(dq.bfloat16().float(), dq)                 # every dequantised value is a bf16 value
    # error bound.  With E = floor(log2 amax) and X = 2^(E - 8) every |w / X| < 512.  e4m3 has 3 fraction bits, so in its top
    # binade [256, 448] the step is 32 X and round-to-nearest errs by at most 16 X = 2^-4 * 2^E; lower binades have finer steps.
    # |w / X| in (448, 512) is clamped to 448: up to 464 that is what rounding would give as well (error <= 16 X); beyond it the
    # saturation error stays below 512 X - 448 X = 64 X.
    err = (b - dq.reshape(K // 32, 32, N)).abs()
    sat = (b / X).abs() > 464.0
    assert (err[~sat] <= 16.0 * X.expand_as(err)[~sat]).all()
    assert (err[sat] < 64.0 * X.expand_as(err)[sat]).all()
    # idempotence: quantise(dequantise(q)) == q, and the predicate
    el2, sc2 = Q.mxfp8_quantize_2d(dq)
    assert torch.equal(el2, el) and torch.equal(sc2, sc)
    assert Q.is_mxfp8(dq) and not Q.is_mxfp8(w)
    rel = ((w - dq).pow(2).sum() / w.pow(2).sum()).sqrt().item()
    print(f"std {std}: relative RMS error {rel:.4f}")
    assert rel < 0.05


def test_no_nan_for_block_maxima_between_448_and_512_scales():
    """block maximum in (448 X, 512 X): torch's cast does not saturate (500 -> NaN), the quantiser clamps first"""
    assert torch.isnan(torch.tensor([500.0]).to(torch.float8_e4m3fn).float()).all()
    w = torch.full((32, 4), 0.01)
    w[3, 0], w[5, 1], w[7, 2], w[9, 3] = 449.0 / 256, -500.0 / 256, 511.0 / 256, 463.0 / 256       # E = 0, X = 2^-8
    el, sc = Q.mxfp8_quantize_2d(w)
    assert (sc == 127 - 8).all()
    dq = Q.mxfp8_dequantize_2d(el, sc)
    assert torch.isfinite(dq).all()
    assert dq[3, 0] == 448.0 / 256 and dq[5, 1] == -448.0 / 256 and dq[7, 2] == 448.0 / 256 and dq[9, 3] == 448.0 / 256
    assert Q.is_mxfp8(dq)


def test_scale_clamp_and_padding():
    w = torch.zeros(40, 2)                                        # K = 40: zero-padded to 64
    w[0, 0] = 2.0 ** -120
    w[33, 1] = 3.0
    el, sc = Q.mxfp8_quantize_2d(w)
    assert el.shape == (64, 2) and sc.shape == (2, 2)
    assert sc[0, 0].item() == 127 - 100                           # e clamped to -100: the tiny value rounds to zero
    dq = Q.mxfp8_round_2d(w)
    assert dq.shape == w.shape and dq[0, 0] == 0.0 and dq[33, 1] == 3.0


# ---- layout ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [512, 2048, 8192])
@pytest.mark.parametrize("N", [16, 3072, 9252])
def test_tile_weight_fp8_round_trip(K, N):
    gen = torch.Generator().manual_seed(K + N)
    w = torch.randn(K, N, generator=gen) * 0.02
    stream, kt, ns = lay.tile_weight_fp8(w)
    assert kt == K // 32 and ns == (N + 15) // 16
    assert stream.dtype == torch.uint8 and stream.shape == (ns, kt // 16, lay.FP8_GROUP_BYTES)
    assert torch.equal(lay.untile_weight_fp8(stream, K, N), Q.mxfp8_round_2d(w))
    dense, _, _ = lay.tile_weight(w)
    assert stream.numel() * 64 == dense.numel() * 2 * 33          # 8448 / 16384 = 0.515625 of the dense tiles' bytes


def test_tile_weight_fp8_operand_order():
    """k-tile t, lane l = 16 q + c, element j = W[32 t + 8 q + j][c]: byte 8 (t & 1) + j of lane l of slot (t % 16) / 2 behind the
    group's 256-byte scale block, whose byte 16 c + t % 16 is the block's E8M0 scale"""
    K, N = 1024, 32
    w = torch.zeros(K, N)
    t, q, j, c, strip = 21, 2, 5, 7, 1
    w[32 * t + 8 * q + j, 16 * strip + c] = 1.5
    stream, kt, ns = lay.tile_weight_fp8(w)
    g, p, h = t // 16, (t % 16) // 2, t % 2
    byte = stream[strip, g, 256 + p * 1024 + (16 * q + c) * 16 + 8 * h + j]
    scale = stream[strip, g, c * 16 + t % 16].item()
    assert scale == 127 - 8                                        # floor(log2 1.5) - 8
    assert byte.view(torch.float8_e4m3fn).float().item() * 2.0 ** (scale - 127) == 1.5
    vals = stream[:, :, 256:]
    assert int((vals != 0).sum()) == 1
    assert int((stream[:, :, :256] != 127).sum()) == 1


def test_tile_weight_fp8_pads_partial_groups():
    w = torch.randn(100, 37, generator=torch.Generator().manual_seed(1))
    stream, kt, ns = lay.tile_weight_fp8(w)
    assert (kt, ns) == (4, 3) and stream.shape == (3, 1, lay.FP8_GROUP_BYTES)
    assert torch.equal(lay.untile_weight_fp8(stream, 100, 37), Q.mxfp8_round_2d(w))


# ---- state dict, oracle, tool ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg_fn", [C.tiny_config, C.mid_config])
def test_quantize_state_dict_touches_exactly_the_streamed_matrices(cfg_fn):
    cfg = cfg_fn()
    sd = _random_sd(cfg)
    qsd = Q.mxfp8_quantize_state_dict(cfg, sd)
    names = Q.mxfp8_names(cfg)
    d = cfg.model.decoder
    assert len(names) == 8 * d.n_layer + 1 and all(n.startswith("decoder.") for n in names)
    assert not any("cross_attention.k_proj" in n or "cross_attention.v_proj" in n for n in names)
    for k in sd:
        if k in names:
            assert qsd[k].shape == sd[k].shape and qsd[k].dtype == torch.float32
            assert not torch.equal(qsd[k], sd[k]), k
            assert Q.is_mxfp8(_kernel_2d(k, qsd[k])), k
        else:
            assert torch.equal(qsd[k], sd[k]), k
    again = Q.mxfp8_quantize_state_dict(cfg, qsd)
    assert all(torch.equal(again[k], qsd[k]) for k in qsd)


def test_oracle_runs_the_quantised_state_dict():
    from oracle import dia_oracle as O
    cfg = C.tiny_config()
    sd = synthetic_state_dict(cfg, seed=1234, std=0.02)
    qsd = Q.mxfp8_quantize_state_dict(cfg, sd)
    dm = O.Dims.of(cfg)
    nz = O.exp_noise(42, 3, dm.C, dm.tgt_vocab)
    a = O.generate(sd, cfg, "[S1] hello", max_tokens=4, noise=nz, mirror=False)
    b = O.generate(qsd, cfg, "[S1] hello", max_tokens=4, noise=nz, mirror=False)
    assert len(b.logits) == len(a.logits) and all(torch.isfinite(torch.as_tensor(l)).all() for l in b.logits)
    assert any(not torch.equal(torch.as_tensor(x), torch.as_tensor(y)) for x, y in zip(a.logits, b.logits))


def test_offline_quantize_tool(tmp_path):
    sys.path.insert(0, ROOT)
    import offline_quantize
    cfg = C.tiny_config()
    sd = _random_sd(cfg, seed=5)
    src = tmp_path / "m"
    src.mkdir()
    torch.save(sd, src / "pytorch_model.bin")
    cfg.save(str(src / "config.json"))
    assert offline_quantize.main(["--model-path", str(src), "--output-dir", str(tmp_path / "q"), "--format", "mxfp8"]) == 0
    got = torch.load(tmp_path / "q" / "pytorch_model.bin", weights_only=True)
    want = Q.mxfp8_quantize_state_dict(cfg, {k: v.float() for k, v in sd.items()})
    assert all(torch.equal(got[k], want[k]) for k in want)
    assert all(Q.is_mxfp8(_kernel_2d(k, got[k])) for k in Q.mxfp8_names(cfg))
    assert (tmp_path / "q" / "config.json").exists()
    with pytest.raises(SystemExit):
        offline_quantize.main(["--model-path", str(src), "--output-dir", str(tmp_path / "r"), "--format", "fp4"])
    assert offline_quantize.main(["--model-path", str(tmp_path / "none"), "--output-dir", str(tmp_path / "r")]) == 1


# ---- DeviceWeights(quant="mxfp8"), the CLI flag and the arena broadcast (mid config, CPU tensors) ---------------------------
def _mid_f8():
    cfg = C.mid_config()
    return cfg, Q.mxfp8_quantize_state_dict(cfg, synthetic_state_dict(cfg, seed=1234, std=0.02))


def test_device_weights_mxfp8_streams():
    from dia_hip.engine import DeviceWeights
    cfg, sd = _mid_f8()
    w = DeviceWeights(cfg, sd, torch.device("cpu"), quant="mxfp8")
    dense = DeviceWeights(cfg, sd, torch.device("cpu"))
    assert w.quant == "mxfp8" and dense.quant == "off" and dense.logits_f8 is None and dense.dec_layers[0]["wof8"] is None
    for L in w.dec_layers:
        for k in MATS:
            f8, dn = L[k + "f8"], L[k]
            assert f8.ns == dn.ns and f8.kt == dn.kt and f8.t.dtype == torch.uint8, k
            K, N = dn.kt * 32, dn.ns * 16
            assert torch.equal(lay.untile_weight_fp8(f8.t, K, N), lay.untile_weight(dn.t, K, N)), k
            assert f8.nbytes * 64 == dn.nbytes * 33
    assert torch.equal(lay.untile_weight_fp8(w.logits_f8.t, w.logits.kt * 32, w.logits.ns * 16),
                       lay.untile_weight(w.logits.t, w.logits.kt * 32, w.logits.ns * 16))
    assert w.max_weight_rounding == 0.0                            # the dense tiles hold the same numbers exactly
    # the streams live in the flat arena, behind everything the dense model holds
    ts, dts = w.tensors(), dense.tensors()
    assert len(ts) == len(dts) + 6 * len(w.dec_layers) + 1
    assert all(a.shape == b.shape and a.dtype == b.dtype for a, b in zip(ts, dts))
    assert ts[len(dts)] is w.dec_layers[0]["qkvf8"].t and ts[-1] is w.logits_f8.t
    assert torch.equal(w.flat[: dense.flat.numel()], dense.flat)
    base = w.flat.data_ptr()
    assert base + dense.flat.numel() <= w.dec_layers[0]["qkvf8"].t.data_ptr() and w.logits_f8.t.data_ptr() < base + w.flat.numel()
    # what a step streams: the MXFP8 streams of the enabled launch classes up to 16 rows, the dense tiles above
    assert dense.decode_weight_bytes() == dense.decode_weight_bytes(64)
    assert w.decode_weight_bytes(16) < w.decode_weight_bytes(17) == dense.decode_weight_bytes()
    assert w.decode_weight_bytes(2) < dense.decode_weight_bytes()
    full = sum(L[k + "f8"].nbytes for L in w.dec_layers for k in MATS) + w.logits_f8.nbytes
    hb.set_tuning("mxfp8", 0x7f7f)
    try:
        assert w.decode_weight_bytes(2) == w.decode_weight_bytes(16) == full
        hb.set_tuning("mxfp8", 0x0020)                             # wo alone, at most 4 rows
        assert hb.mxfp8_mask(4) == 0x20 and hb.mxfp8_mask(5) == 0 and hb.mxfp8_mask(17) == 0
        assert w.decode_weight_bytes(16) == dense.decode_weight_bytes()
        saved = sum(L["wo"].nbytes - L["wof8"].nbytes for L in w.dec_layers)
        assert w.decode_weight_bytes(4) == dense.decode_weight_bytes() - saved
    finally:
        hb.set_tuning("mxfp8", -1)


def test_device_weights_mxfp8_rejections():
    from dia_hip.engine import DeviceWeights
    from dia_hip.pruning import semi_structured_prune_state_dict, structured_prune_state_dict
    cfg, sd = _mid_f8()
    dev = torch.device("cpu")
    with pytest.raises(hb.DiaHipError, match="weight_planes"):
        DeviceWeights(cfg, sd, dev, weight_planes=2, quant="mxfp8")
    with pytest.raises(hb.DiaHipError, match="seg"):
        DeviceWeights(cfg, sd, dev, seg="on", quant="mxfp8")
    with pytest.raises(hb.DiaHipError, match="2:4"):
        DeviceWeights(cfg, semi_structured_prune_state_dict(cfg, sd), dev, sparse="2:4", quant="mxfp8")
    raw = synthetic_state_dict(cfg, seed=1234, std=0.02)
    with pytest.raises(hb.DiaHipError, match=r"decoder\.layers\.0\.qkv is not MXFP8"):
        DeviceWeights(cfg, raw, dev, quant="mxfp8")
    bad = dict(sd)
    name = "decoder.layers.1.mlp.wo.weight"
    bad[name] = sd[name].clone()
    bad[name][5, 3] += 2.0 ** -20
    with pytest.raises(hb.DiaHipError, match=r"decoder\.layers\.1\.wo is not MXFP8"):
        DeviceWeights(cfg, bad, dev, quant="mxfp8")
    spd, _ = structured_prune_state_dict(cfg, raw, 0.5)
    with pytest.raises(hb.DiaHipError, match="compacted"):
        DeviceWeights(cfg, Q.mxfp8_quantize_state_dict(cfg, spd), dev, quant="mxfp8")
    with pytest.raises(ValueError):
        DeviceWeights(cfg, sd, dev, quant="fp4")


def test_cli_weight_format_flag(monkeypatch):
    sys.path.insert(0, ROOT)
    import cli
    from dia_hip.model import Dia
    p = cli.build_parser()
    assert p.parse_args(["hi", "--codes-output", "x.npy"]).weight_format == "bf16"
    assert p.parse_args(["hi", "--codes-output", "x.npy", "--weight-format", "mxfp8"]).weight_format == "mxfp8"
    with pytest.raises(SystemExit):
        p.parse_args(["hi", "--codes-output", "x.npy", "--weight-format", "fp4"])
    assert Dia.weight_format == "bf16"

    class Stop(Exception):
        pass

    def stop(*a, **k):
        raise Stop
    monkeypatch.setattr(Dia, "weight_format", "bf16")
    monkeypatch.setattr(Dia, "from_local", classmethod(stop), raising=False)
    monkeypatch.setattr(Dia, "from_pretrained", classmethod(stop), raising=False)
    try:
        cli.main(["hi", "--codes-output", str(os.devnull), "--weight-format", "mxfp8", "--no-dac"])
    except (Stop, Exception):
        pass
    assert Dia.weight_format == "mxfp8"


def _bcast_worker(rank, world, port, q):
    sys.path.insert(0, os.path.join(ROOT, "dia-tts-prune_amd"))
    import torch.distributed as dist
    from dia_hip import dist as D
    from dia_hip.engine import DeviceWeights
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    cfg, sd = _mid_f8()
    if rank == 0:
        w = DeviceWeights(cfg, sd, torch.device("cpu"), quant="mxfp8")
    else:
        w = DeviceWeights.empty_like_config(cfg, torch.device("cpu"), quant="mxfp8")
    D.broadcast_weights(w, src=0)
    ref = DeviceWeights(cfg, sd, torch.device("cpu"), quant="mxfp8")
    ok = torch.equal(w.flat, ref.flat) and torch.equal(w.dec_layers[2]["wif8"].t, ref.dec_layers[2]["wif8"].t)
    # a receiver without the streams has a different arena: every rank refuses
    plain = DeviceWeights.empty_like_config(cfg, torch.device("cpu")) if rank == 1 else ref
    try:
        D.broadcast_weights(plain, src=0)
        refused = False
    except ValueError:
        refused = True
    q.put((rank, ok, refused))
    dist.barrier()
    dist.destroy_process_group()


def test_gloo_world2_broadcast_of_mxfp8_weights():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 33500 + (os.getpid() % 2000)
    ps = [ctx.Process(target=_bcast_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    res = sorted(q.get(timeout=300) for _ in range(2))
    for p in ps:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert all(r[1] and r[2] for r in res), res


# ---- C ABI -----------------------------------------------------------------------------------------------------------
def test_abi_grew_at_the_tail_only():
    assert hb.ABI_VERSION == 8 and hb.W_MXFP8 == 2
    assert [f[0] for f in hb.GemmArgs._fields_][-2:] == ["w_format", "_pad2"]
    assert [f[0] for f in hb.DecLayer._fields_][-6:] == ["w_" + k + "_f8" for k in MATS]
    assert hb.EngineDesc._fields_[-1][0] == "w_logits_f8"


def test_dia_gemm_mxfp8_refuses_unsupported_combinations_without_a_gpu():
    L = hb.lib()
    buf = ctypes.create_string_buffer(64)                          # never dereferenced: every case is refused before a launch
    addr = ctypes.addressof(buf)

    def rc_of(**kw):
        g = hb.GemmArgs()
        g.A, g.W, g.out = addr, addr, addr
        g.a_ktiles, g.M, g.KT, g.nstrips, g.epi, g.ldo, g.act_f32, g.w_format, g.ssq_ld = 16, 4, 16, 2, hb.EPI_SCALE_STORE, 32, 3, hb.W_MXFP8, 16
        for k, v in kw.items():
            setattr(g, k, v)
        rc = L.dia_gemm(ctypes.byref(g), None)
        return rc, L.dia_last_error()
    for kw, word in ((dict(M=17), b"16 rows"), (dict(w_planes=2), b"w_planes"), (dict(w_planes=3), b"w_planes"), (dict(w_layout=1), b"w_layout"),
                     (dict(sp_blocks=addr), b"sp_blocks"), (dict(epi=hb.EPI_CROSSKV), b"CROSSKV"), (dict(cmap=addr), b"compaction"),
                     (dict(strip_map=addr), b"compaction"), (dict(act_f32=0), b"planes"), (dict(KT=24, a_ktiles=24), b"512"),
                     (dict(KT=32, a_ktiles=32, sk=4, sk_scratch=addr, sk_tickets=addr), b"512"), (dict(KT=256, a_ktiles=256), b"128 k-tiles")):
        rc, msg = rc_of(**kw)
        assert rc == -1 and b"MXFP8" in msg and word in msg, (kw, rc, msg)
    rc, msg = rc_of(w_format=3)
    assert rc == -1 and b"w_format" in msg
