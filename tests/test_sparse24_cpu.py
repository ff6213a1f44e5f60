"""2:4 semi-structured pruning and the sparse weight stream's layout, on the CPU (no GPU needed)."""
import os
import sys

import pytest
import torch

from dia_hip import binding as hb
from dia_hip import config as C
from dia_hip import layout as lay
from dia_hip.pruning import is_2of4, prunable_names, semi_structured_prune_state_dict
from dia_hip.weights import param_shapes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _kernel_2d(name, w):
    """[K, N] with K the contraction axis, as DeviceWeights flattens the kernel"""
    return w.reshape(-1, w.shape[-1]) if name.endswith("o_proj.weight") else w.reshape(w.shape[0], -1)


def _random_sd(cfg, seed=3):
    gen = torch.Generator().manual_seed(seed)
    return {k: (torch.randn(shp, generator=gen) * 0.05 if not k.endswith("norm.weight") else torch.ones(shp))
            for k, shp in param_shapes(cfg).items()}


@pytest.mark.parametrize("cfg_fn", [C.tiny_config, C.mid_config])
def test_pattern_idempotence_and_untouched(cfg_fn):
    cfg = cfg_fn()
    sd = _random_sd(cfg)
    psd = semi_structured_prune_state_dict(cfg, sd)
    names = prunable_names(cfg)
    for k in names:
        w2 = _kernel_2d(k, psd[k])
        assert is_2of4(w2), k
        K = w2.shape[0]
        full = (K // 4) * 4
        # exactly the 2 largest of every group survive (random data: no zeros, no ties)
        nz = (w2[:full] != 0).reshape(K // 4, 4, -1).sum(dim=1)
        assert (nz == 2).all(), k
        kept = w2[:full].reshape(K // 4, 4, -1).abs()
        orig = _kernel_2d(k, sd[k])[:full].reshape(K // 4, 4, -1).abs()
        assert torch.equal(kept.sum(dim=1), orig.topk(2, dim=1).values.sum(dim=1)), k
        assert psd[k].shape == sd[k].shape and psd[k].dtype == sd[k].dtype
    for k in sd:
        if k not in names:
            assert torch.equal(psd[k], sd[k]), k
    again = semi_structured_prune_state_dict(cfg, psd)
    assert all(torch.equal(again[k], psd[k]) for k in psd)


def test_tie_rule_keeps_lower_k():
    cfg = C.tiny_config()
    sd = _random_sd(cfg)
    name = "decoder.layers.0.mlp.wo.weight"                       # [F, D]: K = F along dim 0
    w = torch.zeros_like(sd[name])
    w[0:4, 0] = torch.tensor([1.0, 1.0, 1.0, 1.0])
    w[4:8, 0] = torch.tensor([-2.0, 2.0, 2.0, 0.5])
    w[8:12, 0] = torch.tensor([0.0, 0.0, 0.0, 3.0])
    sd[name] = w
    out = semi_structured_prune_state_dict(cfg, sd)[name]
    assert out[0:4, 0].tolist() == [1.0, 1.0, 0.0, 0.0]
    assert out[4:8, 0].tolist() == [-2.0, 2.0, 0.0, 0.0]
    assert out[8:12, 0].tolist() == [0.0, 0.0, 0.0, 3.0]


def test_is_2of4_detects_violations():
    w = torch.zeros(8, 3)
    assert is_2of4(w)
    w[0:2, 1] = 1.0
    w[5:7, 2] = 1.0
    assert is_2of4(w)
    w[3, 1] = 1.0
    assert not is_2of4(w)
    assert not is_2of4(torch.ones(6, 1))                          # trailing partial group of 2 rows is fine, the full one is not
    assert is_2of4(torch.ones(2, 1))


@pytest.mark.parametrize("K,N", [(512, 48), (100, 37), (2048, 16), (576, 5), (64, 1)])
def test_tile_weight_24_round_trip(K, N):
    gen = torch.Generator().manual_seed(K * 7 + N)
    w = torch.randn(K, N, generator=gen)
    Kp = (K + 3) // 4 * 4
    wp = torch.zeros(Kp, N)
    wp[:K] = w
    g = wp.reshape(Kp // 4, 4, N)
    keep = torch.zeros_like(g, dtype=torch.bool).scatter_(1, g.abs().topk(2, dim=1).indices, True)
    w = (g * keep).reshape(Kp, N)[:K].bfloat16().float()
    w[: min(K, 8), 0] = 0.0                                        # groups with fewer than 2 non-zeros
    stream, kt, ns = lay.tile_weight_24(w)
    G = (kt + 7) // 8
    assert kt == (K + 63) // 64 and ns == (N + 15) // 16
    assert stream.shape == (ns, G, 9, 64, 8) and stream.dtype == torch.bfloat16
    assert torch.equal(lay.untile_weight_24(stream, K, N), w)
    if K % 512 == 0 and N % 16 == 0:
        assert stream.numel() * 2 == (K * N * 2) * 9 // 16         # 0.5625 of the dense bytes


def test_tile_weight_24_operand_order():
    """lane l of sparse k-tile t: column l & 15, K = 64 t + 16 (l >> 4) + 4 g + position; value j = 2 g + s in position order;
    index word bits [2j + 1 : 2j]; dword d of the metadata block = k-tiles 2d (low half) and 2d + 1 (high half)"""
    K, N = 1024, 16
    w = torch.zeros(K, N)
    t, q, g, c = 9, 2, 3, 5
    k0 = 64 * t + 16 * q + 4 * g
    w[k0 + 1, c] = 1.5
    w[k0 + 3, c] = -2.0
    stream, kt, ns = lay.tile_weight_24(w)
    lane = 16 * q + c
    grp, slot = t // 8, t % 8
    vals = stream[0, grp, 1 + slot, lane].float()
    assert vals[2 * g].item() == 1.5 and vals[2 * g + 1].item() == -2.0
    assert vals.abs().sum().item() == 3.5
    meta = stream[0, grp, 0, lane].contiguous().view(torch.int16).view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    word = (int(meta[slot // 2]) >> (16 * (slot % 2))) & 0xFFFF
    assert (word >> (4 * g)) & 3 == 1 and (word >> (4 * g + 2)) & 3 == 3
    # the other groups of the lane: zero values at positions 0 and 1
    assert (word & 0xF) == (0 | 1 << 2)


def test_tile_weight_24_rejects_dense_groups():
    with pytest.raises(ValueError):
        lay.tile_weight_24(torch.ones(64, 16))


def test_offline_prune_2of4(tmp_path):
    sys.path.insert(0, ROOT)
    import offline_prune
    cfg = C.tiny_config()
    sd = _random_sd(cfg, seed=5)
    src = tmp_path / "m"
    src.mkdir()
    torch.save(sd, src / "pytorch_model.bin")
    cfg.save(str(src / "config.json"))
    assert offline_prune.main(["--model-path", str(src), "--output-dir", str(tmp_path / "p"), "--prune-mode", "2:4", "--prune-amount", "0.5"]) == 0
    got = torch.load(tmp_path / "p" / "pytorch_model.bin", weights_only=True)
    want = semi_structured_prune_state_dict(cfg, {k: v.float() for k, v in sd.items()})
    assert all(torch.equal(got[k], want[k]) for k in want)
    assert all(is_2of4(_kernel_2d(k, got[k])) for k in prunable_names(cfg))
    assert (tmp_path / "p" / "config.json").exists()
    assert offline_prune.main(["--model-path", str(src), "--output-dir", str(tmp_path / "q"), "--prune-mode", "2:4", "--prune-amount", "0.3"]) == 1
    assert not (tmp_path / "q" / "pytorch_model.bin").exists()


def test_gemm_args_carries_w_format():
    assert hb.ABI_VERSION == 8
    g = hb.GemmArgs()
    assert g.w_format == 0
    names = [f[0] for f in hb.GemmArgs._fields_]
    assert names[-2:] == ["w_format", "_pad2"]


# ---- DeviceWeights(sparse="2:4"), the CLI flag and the arena broadcast (mid config, CPU tensors) -----------------------------
def _mid_24():
    from dia_hip.weights import synthetic_state_dict
    cfg = C.mid_config()
    return cfg, semi_structured_prune_state_dict(cfg, synthetic_state_dict(cfg, seed=1234, std=0.02))


def test_device_weights_sparse_streams():
    from dia_hip.engine import DeviceWeights
    cfg, sd = _mid_24()
    w = DeviceWeights(cfg, sd, torch.device("cpu"), sparse="2:4")
    dense = DeviceWeights(cfg, sd, torch.device("cpu"))
    assert w.sparse == "2:4" and dense.sparse == "off" and dense.logits24 is None
    for L in w.dec_layers:
        for k in ("qkv", "o", "cq", "co", "wi", "wo"):
            sp, dn = L[k + "24"], L[k]
            assert sp.ns == dn.ns and 2 * sp.kt == dn.kt, k
            K, N = dn.kt * 32, dn.ns * 16
            assert torch.equal(lay.untile_weight_24(sp.t, K, N), lay.untile_weight(dn.t, K, N)), k
    assert torch.equal(lay.untile_weight_24(w.logits24.t, w.logits.kt * 32, w.logits.ns * 16),
                       lay.untile_weight(w.logits.t, w.logits.kt * 32, w.logits.ns * 16))
    # the streams live in the flat arena, after everything the dense model holds
    ts = w.tensors()
    assert ts[: len(dense.tensors())][-1].shape == dense.tensors()[-1].shape
    assert any(t is w.dec_layers[0]["wo24"].t for t in ts) and w.logits24.t is ts[-1]
    base = w.flat.data_ptr()
    assert base <= w.logits24.t.data_ptr() < base + w.flat.numel()
    # what a step streams: every matrix at <= 4 rows, the dense tiles above
    assert dense.decode_weight_bytes() == dense.decode_weight_bytes(64)
    assert w.decode_weight_bytes(4) < w.decode_weight_bytes(5) == dense.decode_weight_bytes()
    full = sum(L[k + "24"].nbytes for L in w.dec_layers for k in ("qkv", "o", "cq", "co", "wi", "wo")) + w.logits24.nbytes
    assert w.decode_weight_bytes(2) == full


def test_device_weights_sparse_rejections():
    from dia_hip.engine import DeviceWeights
    from dia_hip.pruning import structured_prune_state_dict
    from dia_hip.weights import synthetic_state_dict
    cfg, sd = _mid_24()
    dev = torch.device("cpu")
    with pytest.raises(hb.DiaHipError, match="weight_planes"):
        DeviceWeights(cfg, sd, dev, weight_planes=2, sparse="2:4")
    with pytest.raises(hb.DiaHipError, match="seg"):
        DeviceWeights(cfg, sd, dev, seg="on", sparse="2:4")
    dense_sd = synthetic_state_dict(cfg, seed=1234, std=0.02)
    with pytest.raises(hb.DiaHipError, match=r"decoder\.layers\.0\.qkv is not 2:4"):
        DeviceWeights(cfg, dense_sd, dev, sparse="2:4")
    bad = dict(sd)
    name = "decoder.layers.1.mlp.wo.weight"
    bad[name] = sd[name].clone()
    bad[name][0:4, 3] = 1.0
    with pytest.raises(hb.DiaHipError, match=r"decoder\.layers\.1\.wo is not 2:4"):
        DeviceWeights(cfg, bad, dev, sparse="2:4")
    spd, _ = structured_prune_state_dict(cfg, dense_sd, 0.5)
    with pytest.raises(hb.DiaHipError, match="compacted"):
        DeviceWeights(cfg, spd, dev, sparse="2:4")
    with pytest.raises(ValueError):
        DeviceWeights(cfg, sd, dev, sparse="4:8")


def test_cli_sparse_weights_flag(monkeypatch):
    sys.path.insert(0, ROOT)
    import cli
    from dia_hip.model import Dia
    p = cli.build_parser()
    assert p.parse_args(["hi", "--codes-output", "x.npy"]).sparse_weights == "off"
    assert p.parse_args(["hi", "--codes-output", "x.npy", "--sparse-weights", "2:4"]).sparse_weights == "2:4"
    with pytest.raises(SystemExit):
        p.parse_args(["hi", "--codes-output", "x.npy", "--sparse-weights", "1:2"])
    assert Dia.sparse_weights == "off"

    class Stop(Exception):
        pass

    def stop(*a, **k):
        raise Stop
    monkeypatch.setattr(Dia, "sparse_weights", "off")
    monkeypatch.setattr(Dia, "from_local", classmethod(stop), raising=False)
    monkeypatch.setattr(Dia, "from_pretrained", classmethod(stop), raising=False)
    try:
        cli.main(["hi", "--codes-output", str(os.devnull), "--sparse-weights", "2:4", "--no-dac"])
    except (Stop, Exception):
        pass
    assert Dia.sparse_weights == "2:4"


def _bcast_worker(rank, world, port, q):
    sys.path.insert(0, os.path.join(ROOT, "dia-tts-prune_amd"))
    import torch.distributed as dist
    from dia_hip import dist as D
    from dia_hip.engine import DeviceWeights
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    cfg, sd = _mid_24()
    if rank == 0:
        w = DeviceWeights(cfg, sd, torch.device("cpu"), sparse="2:4")
    else:
        w = DeviceWeights.empty_like_config(cfg, torch.device("cpu"), sparse="2:4")
    D.broadcast_weights(w, src=0)
    ref = DeviceWeights(cfg, sd, torch.device("cpu"), sparse="2:4")
    ok = torch.equal(w.flat, ref.flat) and torch.equal(w.dec_layers[2]["wi24"].t, ref.dec_layers[2]["wi24"].t)
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


def test_gloo_world2_broadcast_of_sparse_weights():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 31500 + (os.getpid() % 2000)
    ps = [ctx.Process(target=_bcast_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    res = sorted(q.get(timeout=300) for _ in range(2))
    for p in ps:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert all(r[1] and r[2] for r in res), res
