"""Activation-aware pruning without a GPU: the Wanda score in the three prune modes, ActStats on disk, offline_prune.py --act-stats
end to end, and the argument refusals of dia_act_stats / dia_engine_set_calib, which return before any HIP call."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from dia_hip import binding as hb
from dia_hip import config as CF
from dia_hip import pruning as P
from dia_hip.calib import ActStats, contraction_size, decoder_tap_names, encoder_tap_names
from dia_hip.weights import param_shapes, synthetic_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tiny():
    cfg = CF.tiny_config()
    return cfg, synthetic_state_dict(cfg, seed=7, std=0.05)


def random_stats(cfg, seed):
    rs = np.random.RandomState(seed)
    st = ActStats.zeros(cfg)
    for k in st.sums:
        st.sums[k] = rs.gamma(2.0, 3.0, size=st.sums[k].shape)
        st.rows[k] = 17
    return st


def same(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


def test_taps_cover_every_prunable_name_once(tiny):
    cfg, _ = tiny
    names = [k for tap in decoder_tap_names(cfg) + encoder_tap_names(cfg) for k in tap]
    assert sorted(names) == sorted(P.prunable_names(cfg)) and len(set(names)) == len(names)
    assert len(decoder_tap_names(cfg)) == 6 * cfg.model.decoder.n_layer + 1
    shp = param_shapes(cfg)
    for k in P.prunable_names(cfg):
        assert contraction_size(k, shp[k]) == P._kernel_2d(k, torch.zeros(shp[k])).shape[0]


def test_all_ones_stats_change_nothing(tiny):
    cfg, sd = tiny
    ones = ActStats.ones(cfg)
    assert same(P.semi_structured_prune_state_dict(cfg, sd, act_stats=ones), P.semi_structured_prune_state_dict(cfg, sd))
    for dim, n in ((0, 2), (1, 1)):
        a, ka = P.structured_prune_state_dict(cfg, sd, 0.3, dim=dim, n=n, act_stats=ones)
        b, kb = P.structured_prune_state_dict(cfg, sd, 0.3, dim=dim, n=n)
        assert same(a, b) and all(np.array_equal(ka[k], kb[k]) for k in kb)
    # unstructured with statistics is per output column: restated here by magnitude alone
    got = P.unstructured_prune_state_dict(cfg, sd, 0.4, act_stats=ones)
    for k in P.prunable_names(cfg):
        w2 = P._kernel_2d(k, sd[k].float()).numpy()
        K = w2.shape[0]
        want = w2.copy()
        for col in range(w2.shape[1]):
            order = np.argsort(np.abs(w2[:, col]), kind="stable")
            want[order[: int(round(0.4 * K))], col] = 0
        assert np.array_equal(P._kernel_2d(k, got[k].float()).numpy(), want), k
    for k in sd:
        if k not in P.prunable_names(cfg):
            assert torch.equal(got[k], sd[k])


def test_stats_flip_the_survivors_of_a_group():
    w = torch.tensor([[4., 4.], [3., 3.], [2., 2.], [1., 1.], [1., -8.], [2., 7.], [3., -6.], [4., 5.]])       # [K = 8, N = 2]
    plain = P._prune_2of4_2d(w)
    assert torch.equal(plain != 0, torch.tensor([[1, 1], [1, 1], [0, 0], [0, 0], [0, 1], [0, 1], [1, 0], [1, 0]]).bool())
    rms = torch.tensor([1., 1., 4., 8., 8., 1., 1., 1.])
    got = P._prune_2of4_2d(w, rms)
    # group 0 scores (4, 3, 8, 8): rows 2 and 3 survive now; group 1 column 0 (8, 2, 3, 4): rows 4, 7; column 1 (64, 7, 6, 5): rows 4, 5
    assert torch.equal(got != 0, torch.tensor([[0, 0], [0, 0], [1, 1], [1, 1], [1, 1], [0, 1], [0, 0], [1, 0]]).bool())
    assert torch.equal(got[got != 0], w[got != 0]) and P.is_2of4(got) and P.is_2of4(plain)
    assert torch.equal(P._prune_2of4_2d(got, rms), got)                                                       # idempotent


def test_tie_rule_lower_k_stays():
    w = torch.ones(8, 3)
    rms = torch.tensor([2., 2., 2., 2., 1., 2., 2., 0.5])
    got = P._prune_2of4_2d(w, rms)
    assert torch.equal(got[:, 0] != 0, torch.tensor([1, 1, 0, 0, 0, 1, 1, 0]).bool())
    # |w| * rms ties across different weights: (2 * 1, 1 * 2, 4 * 0.5, 1 * 2) all score 2 -> rows 0 and 1 stay
    w2 = torch.tensor([[2.], [1.], [4.], [1.]])
    assert torch.equal(P._prune_2of4_2d(w2, torch.tensor([1., 2., 0.5, 2.])) != 0, torch.tensor([[1], [1], [0], [0]]).bool())


def test_unstructured_per_column_ties_go_to_the_lower_k(tiny):
    cfg, sd = tiny
    sd1 = {k: (torch.ones_like(v) if k in P.prunable_names(cfg) else v) for k, v in sd.items()}
    got = P.unstructured_prune_state_dict(cfg, sd1, 0.25, act_stats=ActStats.ones(cfg))
    for k in P.prunable_names(cfg):
        w2 = P._kernel_2d(k, got[k])
        n = int(round(0.25 * w2.shape[0]))
        assert bool((w2[:n] == 0).all()) and bool((w2[n:] == 1).all()), k


def test_pruning_with_stats_on_a_model(tiny):
    cfg, sd = tiny
    st = random_stats(cfg, 3)
    a = P.semi_structured_prune_state_dict(cfg, sd, act_stats=st)
    plain = P.semi_structured_prune_state_dict(cfg, sd)
    assert not same(a, plain)
    for k in P.prunable_names(cfg):
        w2 = P._kernel_2d(k, a[k].float())
        assert P.is_2of4(w2) and abs(float((w2 == 0).float().mean()) - 0.5) < 1e-6
        # the survivors are the two largest |w| * rms of their group
        K, N = w2.shape
        sc = (P._kernel_2d(k, sd[k].float()).abs() * torch.from_numpy(st.rms(k)).float()[:, None]).reshape(K // 4, 4, N)
        kept = (w2 != 0).reshape(K // 4, 4, N)
        lo_kept = torch.where(kept, sc, torch.full_like(sc, float("inf"))).min(dim=1).values
        hi_drop = torch.where(kept, torch.full_like(sc, -1.0), sc).max(dim=1).values
        assert bool((lo_kept >= hi_drop).all()), k
    assert same(P.semi_structured_prune_state_dict(cfg, a, act_stats=st), a)                                  # idempotent
    s1, kept1 = P.structured_prune_state_dict(cfg, sd, 0.5, dim=0, n=2, act_stats=st)
    s0, kept0 = P.structured_prune_state_dict(cfg, sd, 0.5, dim=0, n=2)
    assert any(not np.array_equal(kept1[k], kept0[k]) for k in kept0)
    k = "decoder.layers.0.mlp.wo.weight"                                    # dim 0 is the contraction axis here: slice norm * rms
    norm = torch.norm(sd[k].float(), dim=1) * torch.from_numpy(st.rms(k)).float()
    want = np.sort(torch.topk(norm, k=len(kept1[k])).indices.numpy())
    assert np.array_equal(kept1[k], want)


def test_act_stats_round_trip_merge_and_refusals(tiny, tmp_path):
    cfg, sd = tiny
    a, b = random_stats(cfg, 1), random_stats(cfg, 2)
    path = str(tmp_path / "stats.npz")
    a.save(path)
    with np.load(path, allow_pickle=False) as z:                            # arrays and integers only
        assert all(z[k].dtype in (np.float64, np.int64) for k in z.files)
    c = ActStats.load(path)
    assert c.shape_fields == a.shape_fields and c.rows == a.rows and all(np.array_equal(c.sums[k], a.sums[k]) for k in a.sums)
    k0 = P.prunable_names(cfg)[0]
    want = a.sums[k0] + b.sums[k0]
    c.merge(b)
    assert np.array_equal(c.sums[k0], want) and c.rows[k0] == 34
    assert np.allclose(c.rms(k0), np.sqrt(want / 34), rtol=0, atol=0)
    c.check_against(cfg)
    with pytest.raises(ValueError, match="mid|shapes"):
        c.merge(ActStats.zeros(CF.mid_config()))
    short = ActStats.load(path)
    victim = "decoder.layers.1.mlp.wo.weight"
    short.sums[victim] = short.sums[victim][:-1]
    with pytest.raises(ValueError, match=victim.replace(".", r"\.")):
        P.semi_structured_prune_state_dict(cfg, sd, act_stats=short)
    missing = ActStats.load(path)
    del missing.sums[victim], missing.rows[victim]
    with pytest.raises(ValueError, match=victim.replace(".", r"\.")):
        P.unstructured_prune_state_dict(cfg, sd, 0.5, act_stats=missing)
    with pytest.raises(ValueError, match="no row"):
        P.structured_prune_state_dict(cfg, sd, 0.5, act_stats=ActStats.zeros(cfg))


def test_offline_prune_with_act_stats_end_to_end(tiny, tmp_path):
    cfg, sd = tiny
    src, out = tmp_path / "model", tmp_path / "pruned"
    src.mkdir()
    torch.save(dict(sd), src / "pytorch_model.bin")
    cfg.save(str(src / "config.json"))
    st = random_stats(cfg, 9)
    st.save(str(tmp_path / "stats.npz"))
    tool = os.path.join(ROOT, "offline_prune.py")
    base = [sys.executable, tool, "--model-path", str(src), "--prune-mode", "2:4", "--prune-amount", "0.5"]
    r = subprocess.run(base + ["--output-dir", str(out), "--act-stats", str(tmp_path / "stats.npz")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    got = torch.load(out / "pytorch_model.bin")
    assert same(got, dict(P.semi_structured_prune_state_dict(cfg, sd, act_stats=st)))
    # without the flag: what the function gives without statistics
    r = subprocess.run(base + ["--output-dir", str(tmp_path / "plain")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert same(torch.load(tmp_path / "plain" / "pytorch_model.bin"), dict(P.semi_structured_prune_state_dict(cfg, sd)))
    # statistics of another model: refused, the tensor named, nothing written
    ActStats.ones(CF.mid_config()).save(str(tmp_path / "other.npz"))
    r = subprocess.run(base + ["--output-dir", str(tmp_path / "bad"), "--act-stats", str(tmp_path / "other.npz")], capture_output=True, text=True)
    assert r.returncode == 1 and "encoder.layers.0.self_attention.q_proj.weight" in r.stdout
    assert not (tmp_path / "bad" / "pytorch_model.bin").exists()
    h = subprocess.run([sys.executable, tool, "--help"], capture_output=True, text=True).stdout
    assert "--act-stats" in h and "COLUMN" in h


# ------------------------------------------------------------------------------------------------ C ABI refusals, no device
def good_args(keep):
    x = np.zeros(16 * 64, dtype=np.float32)
    acc = np.zeros(64, dtype=np.float64)
    cnt = np.zeros(2, dtype=np.int64)
    ssq = np.zeros(4 * 16, dtype=np.float32)
    cur = np.zeros(8, dtype=np.int32)
    keep.extend([x, acc, cnt, ssq, cur])
    a = hb.ActStatsArgs()
    a.x, a.ktiles, a.M, a.rows_pad, a.act_f32 = x.ctypes.data, 2, 4, 16, 1
    a.ssq_in, a.ssq_in_n, a.ssq_ld, a.inv_d, a.eps = ssq.ctypes.data, 4, 16, 1 / 64, 1e-5
    a.rows_per_slot, a.cur, a.T = 2, cur.ctypes.data, 8
    a.acc, a.counter = acc.ctypes.data, cnt.ctypes.data
    return a


@pytest.mark.parametrize("field,value,word", [
    ("x", None, b"null plane"), ("acc", None, b"null acc"), ("counter", None, b"null counter"), ("ktiles", 0, b"ktiles <= 0"),
    ("ktiles", -3, b"ktiles <= 0"), ("ktiles_used", 3, b"ktiles_used"), ("M", 0, b"M <= 0"), ("M", 17, b"beyond the plane"),
    ("rows_pad", 12, b"rows_pad"), ("ssq_in_n", 0, b"ssq_in without"), ("ssq_ld", 3, b"ssq_ld"), ("cur", None, b"without cur"),
    ("rows_per_slot", 1, b"rows_per_slot"), ("T", 0, b"without T"), ("act_f32", 0, b"plane_stride"),
])
def test_act_stats_refusals_without_a_device(field, value, word):
    L = hb.lib()
    keep = []
    a = good_args(keep)
    setattr(a, field, value)
    assert L.dia_act_stats(C.byref(a), None) == -1, field
    msg = L.dia_last_error()
    assert msg.startswith(b"dia_act_stats: ") and word in msg, msg
    assert L.dia_act_stats(None, None) == -1
    assert not keep[1].any() and not keep[2].any()                          # nothing was written


def test_set_calib_refusals_without_a_device():
    L = hb.lib()
    ca = hb.CalibArgs()
    assert L.dia_engine_set_calib(None, C.byref(ca)) == -1 and b"null engine" in L.dia_last_error()
    assert L.dia_engine_set_calib(None, None) == -1
