"""Two-plane bf16 weights (w_planes = 2, Dia.fp32_weights = "bf16x2") on the CPU: the layout, the device-weight builder, the
multi-rank weight broadcast and the CLI switch."""
import os
import sys

import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dia-tts-prune_amd"))
sys.path.insert(0, ROOT)


def test_tile_weight_bf16x2_round_trip_and_interleave():
    from dia_hip import layout as lay

    g = torch.Generator().manual_seed(5)
    K, N = 96, 40                                    # padded to 96 x 48: 3 activation k-tiles, 3 strips
    w = torch.randn(K, N, generator=g) * 0.05
    tiles, kt2, ns = lay.tile_weight_bf16x2(w)
    assert (kt2, ns) == (6, 3) and tuple(tiles.shape) == (3, 6, 64, 8) and tiles.dtype == torch.bfloat16
    hi, lo = lay.untile_weight_bf16x2(tiles, K, N)
    # hi + lo within 2^-17 relative of w, per element
    err = (hi.double() + lo.double() - w.double()).abs()
    assert bool((err <= w.double().abs() * 2.0 ** -17).all())
    # the hi plane is the one-plane tile set, bit for bit; even weight k-tiles hold it, odd ones the lo plane
    one, kt, _ = lay.tile_weight(w)
    assert kt2 == 2 * kt
    assert torch.equal(tiles[:, 0::2].view(torch.int16), one.view(torch.int16))
    lo_t, _, _ = lay.tile_weight((w - w.bfloat16().float()))
    assert torch.equal(tiles[:, 1::2].view(torch.int16), lo_t.view(torch.int16))
    assert torch.equal(hi, w.bfloat16().float())
    h2, l2 = lay.split2(w)
    assert torch.equal(h2.float(), hi) and torch.equal(l2.float(), lo)


def test_device_weights_two_planes_mid():
    from dia_hip import config as C
    from dia_hip.engine import DeviceWeights
    from dia_hip.weights import synthetic_state_dict

    cfg = C.mid_config()
    sd = synthetic_state_dict(cfg, seed=11, std=0.02)
    cpu = torch.device("cpu")
    w1 = DeviceWeights(cfg, sd, cpu)
    w2 = DeviceWeights(cfg, sd, cpu, weight_planes=2)
    assert w2.weight_planes == 2
    assert w2.decode_weight_bytes() == 2 * w1.decode_weight_bytes()
    assert w2.prefill_weight_bytes() == 2 * w1.prefill_weight_bytes()
    assert w2.ckv_all() is None and w1.ckv_all() is not None
    L1, L2 = w1.dec_layers[0], w2.dec_layers[0]
    for k in ("qkv", "o", "cq", "co", "wi", "wo", "ckv"):
        assert L2[k].kt == 2 * L1[k].kt and L2[k].ns == L1[k].ns
        assert torch.equal(L2[k].t[:, 0::2].view(torch.int16), L1[k].t.view(torch.int16))    # bf16-representable: hi == tiles
        assert not bool(L2[k].t[:, 1::2].float().any())                                        # ... and lo == 0
    z = DeviceWeights.empty_like_config(cfg, cpu, weight_planes=2)
    assert z.flat.numel() == w2.flat.numel()
    with pytest.raises(ValueError):
        DeviceWeights(cfg, sd, cpu, weight_planes=4)


def _worker(rank, world, port, mode, q):
    sys.path.insert(0, os.path.join(ROOT, "dia-tts-prune_amd"))
    import torch.distributed as dist
    from dia_hip import config as C
    from dia_hip import dist as D
    from dia_hip.engine import DeviceWeights
    from dia_hip.weights import synthetic_state_dict

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(2)
    cfg = C.mid_config()
    cpu = torch.device("cpu")
    g = torch.Generator().manual_seed(3)
    sd = synthetic_state_dict(cfg, seed=7, std=0.02)
    sd = {k: (v + v.abs().mean() * 2.0 ** -10 * torch.randn(v.shape, generator=g)) if v.ndim >= 2 and "embedding" not in k else v
          for k, v in sd.items()}                    # not bf16-representable: the lo plane carries data
    if rank == 0:
        w = DeviceWeights(cfg, sd, cpu, weight_planes=2)
    else:
        w = DeviceWeights.empty_like_config(cfg, cpu, weight_planes=2 if mode == "same" else 3)
    ok, raised = False, False
    try:
        D.broadcast_weights(w, src=0)
        ref = DeviceWeights(cfg, sd, cpu, weight_planes=2)
        ok = torch.equal(w.flat, ref.flat)
    except ValueError:
        raised = True
    q.put((rank, ok, raised))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("mode", ["same", "mismatch"])
def test_gloo_world2_two_plane_arena(mode):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 33500 + (os.getpid() % 2000) + (0 if mode == "same" else 7)
    ps = [ctx.Process(target=_worker, args=(r, 2, port, mode, q)) for r in range(2)]
    for p in ps:
        p.start()
    res = sorted((q.get(timeout=240) for _ in range(2)), key=lambda t: t[0])
    for p in ps:
        p.join(timeout=60)
        assert p.exitcode == 0
    if mode == "same":
        assert all(ok and not raised for _, ok, raised in res)          # the receiver's arena equals the sender's
    else:
        assert all(raised for _, _, raised in res)                      # 2-plane sender, 3-plane receiver: both ranks raise


def test_cli_fp32_weights_flag():
    import cli

    p = cli.build_parser()
    assert p.parse_args(["hi", "--codes-output", "x.npy"]).fp32_weights == "exact"
    assert p.parse_args(["hi", "--codes-output", "x.npy", "--fp32-weights", "bf16x2"]).fp32_weights == "bf16x2"
    assert p.parse_args(["hi", "--codes-output", "x.npy", "--fp32-weights", "round"]).fp32_weights == "round"
    with pytest.raises(SystemExit):
        p.parse_args(["hi", "--codes-output", "x.npy", "--fp32-weights", "fp8"])
