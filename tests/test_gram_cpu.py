"""Host side of the Gram matrices and GPTQ (dia_hip/calib.py GramStats, dia_hip/quant.py gptq_*, offline_quantize.py --gram-stats;
DESIGN.md "Gram matrices and GPTQ"): no GPU.

The GPTQ condition on the three synthetic cases is strict, not a tolerance: the calibration-set output error tr(delta^T G delta) of
GPTQ lies below round-to-nearest's (measured 0.04 .. 0.21 of it; the test prints the ratios).  The held-out ratio is printed, not
asserted: with fewer calibration rows than channels GPTQ overfits a rank-deficient Hessian."""
import os
import sys

import numpy as np
import pytest
import torch

import gram_ref as R
from dia_hip import calib as CAL
from dia_hip import config as C
from dia_hip import quant as Q
from dia_hip.calib import ActStats, GramStats
from dia_hip.pruning import _kernel_2d
from dia_hip.weights import param_shapes, synthetic_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FMTS = [("mxfp4", Q.mxfp4_round_2d, Q.is_mxfp4), ("mxfp8", Q.mxfp8_round_2d, Q.is_mxfp8)]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def random_grams(cfg, seed, rows=40, layers=None):
    """a GramStats of random correlated rows per tap"""
    rs = np.random.RandomState(seed)
    g = GramStats.zeros(cfg, layers)
    for t in g.taps():
        K = g.channels(t)
        X = (rs.randn(rows, K) @ (np.eye(K) + 0.3 * rs.randn(K, K))).astype(np.float32).astype(np.float64)
        g.packed[t] = CAL.pack_gram(X.T @ X)
        g.rows[t] = rows
    return g


# ---- packed layout -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [32, 96, 256])
def test_pack_unpack_and_tile_order(K):
    rs = np.random.RandomState(K)
    X = rs.randn(7, K)
    G = X.T @ X
    G = np.tril(G) + np.tril(G, -1).T                                     # symmetric bit for bit
    p = CAL.pack_gram(G)
    T = K // 32
    assert p.shape == (T * (T + 1) // 2, 32, 32) == (CAL.gram_tiles(K), 32, 32) and CAL.gram_channels(p.shape[0]) == K
    for ti in range(T):
        for tj in range(ti + 1):                                          # tile (ti, tj) at ti (ti + 1) / 2 + tj, row-major
            assert np.array_equal(p[ti * (ti + 1) // 2 + tj], G[32 * ti: 32 * ti + 32, 32 * tj: 32 * tj + 32])
    d = CAL.unpack_gram(p)
    assert np.array_equal(bits(d), bits(G)) and np.array_equal(bits(d), bits(d.T))
    assert np.array_equal(bits(CAL.gram_diagonal(p)), bits(np.diagonal(G).copy()))
    with pytest.raises(ValueError):
        CAL.gram_tiles(K + 8)
    with pytest.raises(ValueError):
        CAL.gram_channels(p.shape[0] + 1 if K > 32 else 2)


def test_gram_stats_taps_cover_the_mx_kernels_once():
    cfg = C.tiny_config()
    g = GramStats.zeros(cfg)
    n = cfg.model.decoder.n_layer
    assert g.taps() == CAL.gram_tap_keys(cfg) and len(g.taps()) == 6 * n + 1
    assert sorted(g.names()) == sorted(Q.mx_names(cfg))                     # the encoder and the cross-K/V projections get no Gram
    p = "decoder.layers.0."
    assert g.tap_of(p + "self_attention.q_proj.weight") == g.tap_of(p + "self_attention.v_proj.weight") == p + "qkv"
    assert g.kernels[p + "wi"] == [p + "mlp.wi_fused.weight"]
    shp = param_shapes(cfg)
    for k in g.names():
        assert g.dense(k).shape == (CAL.contraction_size(k, shp[k]),) * 2
    one = GramStats.zeros(cfg, layers=[1])
    assert one.taps() == CAL.gram_tap_keys(cfg)[6:12]
    assert GramStats.zeros(cfg, layers=(n, n + 1)).taps() == ["decoder.logits_dense"]
    for bad in ([n + 1], [-1], []):
        with pytest.raises(ValueError, match="gram_layers"):
            GramStats.zeros(cfg, layers=bad)


def test_save_load_bitwise_merge_and_act_stats(tmp_path):
    cfg = C.tiny_config()
    a, b = random_grams(cfg, 1), random_grams(cfg, 2, rows=9)
    path = str(tmp_path / "g.npz")
    a.save(path)
    with np.load(path, allow_pickle=False) as z:                           # arrays only, each tap's matrix once
        assert sorted(k for k in z.files if k.startswith("gram/")) == sorted("gram/" + t for t in a.taps())
    l = GramStats.load(path)
    assert l.taps() == a.taps() and l.rows == a.rows and l.kernels == a.kernels and l.shape_fields == a.shape_fields
    assert all(np.array_equal(bits(l.packed[t]), bits(a.packed[t])) for t in a.taps())
    # the diagonals as activation statistics
    st = a.to_act_stats()
    assert sorted(st.names()) == sorted(Q.mx_names(cfg))
    for k in st.names():
        assert np.array_equal(bits(st.sums[k]), bits(np.diagonal(a.dense(k)).copy())) and st.rows[k] == a.rows_of(k) == 40
    full = a.to_act_stats(into=ActStats.zeros(cfg))
    assert full.rows["encoder.layers.0.mlp.wo.weight"] == 0 and full.rows["decoder.logits_dense.weight"] == 40
    # merge adds matrices and counts; a tap only the other holds is taken over
    want = {t: a.packed[t] + b.packed[t] for t in a.taps()}
    m = GramStats.load(path).merge(b)
    assert all(np.array_equal(bits(m.packed[t]), bits(want[t])) and m.rows[t] == 49 for t in a.taps())
    lo, hi = random_grams(cfg, 3, layers=[0]), random_grams(cfg, 4, layers=(1, cfg.model.decoder.n_layer + 1))
    both = lo.merge(hi)
    assert sorted(both.taps()) == sorted(a.taps())
    both.check_against(cfg)
    other = GramStats(b.packed, b.rows, b.kernels, dict(b.shape_fields, dec_n_embd=1))
    with pytest.raises(ValueError, match="different shapes"):
        a.merge(other)


def test_check_against_names_the_offending_tensor():
    cfg = C.tiny_config()
    g = random_grams(cfg, 5)
    g.check_against(cfg)
    name = "decoder.layers.1.mlp.wo.weight"
    tap = g.tap_of(name)
    g.rows[tap] = 0
    with pytest.raises(ValueError, match=name.replace(".", r"\.") + " counted no row"):
        g.check_against(cfg)
    g.packed[tap] = np.zeros((1, 32, 32))
    with pytest.raises(ValueError, match=name.replace(".", r"\.") + " has 32 channels"):
        g.check_against(cfg)
    part = random_grams(cfg, 6, layers=[0])
    with pytest.raises(ValueError, match=r"nothing for decoder\.layers\.1\.self_attention\.q_proj\.weight"):
        part.check_against(cfg)
    with pytest.raises(ValueError, match="nothing for"):
        Q.gptq_quantize_state_dict(cfg, synthetic_state_dict(cfg, seed=5, std=0.02), part, "mxfp4")


# ---- GPTQ ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,N", [(64, 48), (128, 16), (72, 20), (200, 8)])
def test_diagonal_gram_is_round_to_nearest(K, N):
    """no coupling, no error to push: the scale and tie rules of the format's own quantiser, byte for byte"""
    rs = np.random.RandomState(K)
    w = torch.from_numpy((rs.randn(K, N) * np.exp(rs.randn(1, N))).astype(np.float32))
    w[5] = 0
    w[:32, 3] = 0                                                           # an all-zero block
    w[:, 1] = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 6.0] * (K // 8)) * 0.5      # ties of the e2m1 grid
    w[:, 2] = torch.tensor([17.0, 19.0, 21.0, 23.0, 1.0625, 1.1875, 448.0, 480.0] * (K // 8))  # ties of e4m3, and the clamp
    G = np.diag(np.abs(rs.randn(K)) + 0.1)
    for fmt, rnd, ok in FMTS:
        got = Q.gptq_quantize_2d(w, G, 5, fmt)
        assert got.dtype == torch.float32 and np.array_equal(got.numpy().view(np.uint32), rnd(w).numpy().view(np.uint32)), fmt
        assert ok(got)


def test_a_silent_channel_keeps_its_plain_rounding():
    K, N, M = 96, 24, 200
    rs = np.random.RandomState(4)
    X = (rs.randn(M, K) @ (np.eye(K) + 0.4 * rs.randn(K, K))).astype(np.float32).astype(np.float64)
    X[:, [7, 40]] = 0                                                       # silent in calibration
    w = torch.from_numpy((rs.randn(K, N) * 0.02).astype(np.float32))
    G = X.T @ X
    for fmt, rnd, ok in FMTS:
        got = Q.gptq_quantize_2d(w, G, M, fmt)
        assert ok(got)
        assert not torch.equal(got, rnd(w))                                 # the other channels did move
        for k in (7, 40):
            # the channel's own value rounded under the scale its block ended up with: nothing was pushed into it, nothing zeroed
            b0 = k // 32 * 32
            mixed = got.clone()
            mixed[k] = w[k]
            e_blk = Q._mx_exponent_np(got[b0: b0 + 32].double().numpy(), Q._MX_FMT[fmt][0])
            want = Q._mx_round_row_np(w[k].double().numpy(), e_blk, fmt)
            assert (got[k] != 0).any()
            assert np.array_equal(got[k].double().numpy(), want), (fmt, k)


@pytest.mark.parametrize("K,N,M", R.GPTQ_CASES)
def test_gptq_beats_round_to_nearest_on_the_calibration_rows(K, N, M):
    rs = np.random.RandomState(K + M)
    W, X, G, Gh = R.gptq_case(rs, K, N, M)
    Wt = torch.from_numpy(W)
    for fmt, rnd, ok in FMTS:
        got = Q.gptq_quantize_2d(Wt, G, M, fmt)
        assert ok(got), fmt
        e_g, e_r = Q.calibration_error(G, got - Wt), Q.calibration_error(G, rnd(Wt) - Wt)
        assert abs(e_g - R.output_error(G, (got - Wt).double().numpy())) <= 1e-9 * e_g
        h = Q.calibration_error(Gh, got - Wt) / Q.calibration_error(Gh, rnd(Wt) - Wt)
        print(f"K={K} N={N} rows={M} {fmt}: calibration-set error GPTQ / round-to-nearest {e_g / e_r:.3f}, held-out {h:.3f}")
        assert e_g < e_r, (fmt, e_g, e_r)


@pytest.mark.parametrize("K", [40, 100, 33])
def test_outputs_stay_on_the_grid_when_k_is_no_multiple_of_32(K):
    rs = np.random.RandomState(K)
    N, M = 12, 300
    X = (rs.randn(M, K) @ (np.eye(K) + 0.5 * rs.randn(K, K))).astype(np.float32).astype(np.float64)
    w = torch.from_numpy((rs.randn(K, N) * np.exp(2 * rs.randn(K, 1))).astype(np.float32))
    for fmt, rnd, ok in FMTS:
        for block in (32, 64, 128):
            got = Q.gptq_quantize_2d(w, X.T @ X, M, fmt, block=block)
            assert got.shape == (K, N) and ok(got), (fmt, block)
    with pytest.raises(ValueError, match="multiple of 32"):
        Q.gptq_quantize_2d(w, X.T @ X, M, "mxfp4", block=48)
    with pytest.raises(ValueError, match="mxfp4 or mxfp8"):
        Q.gptq_quantize_2d(w, X.T @ X, M, "int4")
    with pytest.raises(ValueError, match="no row"):
        Q.gptq_quantize_2d(w, X.T @ X, 0, "mxfp4")
    with pytest.raises(ValueError, match="channels"):
        Q.gptq_quantize_2d(w, np.eye(K + 1), 3, "mxfp4")


def test_lazy_batches_do_not_change_the_walk():
    """block = 32 and block = 128 are the same recurrence; they differ only by float64 summation order"""
    rs = np.random.RandomState(8)
    W, X, G, _ = R.gptq_case(rs, 256, 32, 400)
    Wt = torch.from_numpy(W)
    a, b = Q.gptq_quantize_2d(Wt, G, 400, "mxfp4", block=32), Q.gptq_quantize_2d(Wt, G, 400, "mxfp4", block=256)
    assert float((a != b).float().mean()) < 0.01


# ---- the tool ----------------------------------------------------------------------------------------------------------------
def test_offline_quantize_with_and_without_gram_stats(tmp_path, capsys):
    sys.path.insert(0, ROOT)
    import cli
    import offline_quantize
    cfg = C.tiny_config()
    sd = synthetic_state_dict(cfg, seed=5, std=0.02)
    src = tmp_path / "m"
    src.mkdir()
    torch.save(sd, src / "pytorch_model.bin")
    cfg.save(str(src / "config.json"))
    grams = random_grams(cfg, 7, rows=300)
    gpath = str(tmp_path / "grams.npz")
    grams.save(gpath)
    fsd = {k: v.float() for k, v in sd.items()}
    for fmt, plain, ok in (("mxfp4", Q.mxfp4_quantize_state_dict, Q.is_mxfp4), ("mxfp8", Q.mxfp8_quantize_state_dict, Q.is_mxfp8)):
        base = ["--model-path", str(src), "--format", fmt]
        assert offline_quantize.main(base + ["--output-dir", str(tmp_path / ("q" + fmt))]) == 0
        out = capsys.readouterr().out
        assert "Calibration-set" not in out and "Relative RMS error" in out
        got = torch.load(tmp_path / ("q" + fmt) / "pytorch_model.bin", weights_only=True)
        want = plain(cfg, fsd)
        assert list(got) == list(want) and all(torch.equal(got[k], want[k]) for k in want)      # without the flag: what it wrote before
        assert offline_quantize.main(base + ["--output-dir", str(tmp_path / ("g" + fmt)), "--gram-stats", gpath, "--damp", "0.02"]) == 0
        out = capsys.readouterr().out
        errs = {ln.split(",")[1].split(":")[0].strip(): float(ln.split(":")[-1]) for ln in out.splitlines() if ln.startswith("Calibration-set")}
        assert "Relative RMS error" in out and errs["GPTQ"] < errs["round-to-nearest"]
        gq = torch.load(tmp_path / ("g" + fmt) / "pytorch_model.bin", weights_only=True)
        ref = Q.gptq_quantize_state_dict(cfg, fsd, GramStats.load(gpath), fmt, damp=0.02)
        for k in want:
            assert torch.equal(gq[k], ref[k]), k
            if k in Q.mx_names(cfg):
                assert ok(_kernel_2d(k, gq[k])), k
            else:
                assert torch.equal(gq[k], fsd[k]), k
        assert any(not torch.equal(gq[k], want[k]) for k in Q.mx_names(cfg))
    bad = random_grams(cfg, 7, layers=[0])
    bad.save(str(tmp_path / "bad.npz"))
    assert offline_quantize.main(["--model-path", str(src), "--output-dir", str(tmp_path / "x"), "--gram-stats", str(tmp_path / "bad.npz")]) == 1
    assert "nothing for" in capsys.readouterr().out
    # cli.py: the flags parse, and need each other
    a = cli.build_parser().parse_args(["hi", "--calibrate-codes", "c.npy", "--stats-output", "s.npz", "--gram-output", "g.npz", "--gram-layers", "0:2"])
    assert a.gram_output == "g.npz" and a.gram_layers == "0:2"


def test_session_refuses_gram_layers_without_gram_and_unknown_modes():
    from dia_hip.engine import DecodeSession
    with pytest.raises(ValueError, match="calibrate is False, True or 'gram'"):
        DecodeSession(None, [], calibrate="hessian")
    with pytest.raises(ValueError, match="gram_layers needs"):
        DecodeSession(None, [], calibrate=True, gram_layers=[0])
    with pytest.raises(ValueError, match="teacher_tokens"):
        DecodeSession(None, [], calibrate="gram")
