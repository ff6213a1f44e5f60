"""Host side of the per-request (unmerged) LoRA adapters: a hand-written PEFT directory parsed into the AdapterBank's tables on a
CPU device — module-path mapping, name segment, rank / alpha patterns, fan_in_fan_out, the flattened A / B against
merge_lora_state_dict's delta — the refusals, and the CLI's argument surface.  No GPU, no library load before the last tests."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from dia_hip import config as C
from dia_hip.lora import MAX_RANK, AdapterBank, merge_lora_state_dict
from dia_hip.weights import synthetic_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def write_adapter(tmp_path, name, tensors, r=4, alpha=8, **extra):
    d = tmp_path / name
    d.mkdir(exist_ok=True)
    json.dump(dict(r=r, lora_alpha=alpha, target_modules=["q_proj", "v_proj"], **extra), open(d / "adapter_config.json", "w"))
    torch.save(tensors, d / "adapter_model.bin")
    return str(d)


def pair(sd, path, r, gen, prefix="base_model.model.", seg=""):
    """lora_A [r, in] / lora_B [out, r] of the right shapes for `path` (the kernel is [in, out...])"""
    w = sd[path + ".weight"]
    n_in = w.shape[0]
    n_out = w.numel() // n_in
    A, B = torch.randn(r, n_in, generator=gen), torch.randn(n_out, r, generator=gen)
    return {f"{prefix}{path}.lora_A{seg}.weight": A, f"{prefix}{path}.lora_B{seg}.weight": B}


@pytest.fixture(scope="module")
def tiny():
    cfg = C.tiny_config()
    return cfg, synthetic_state_dict(cfg, seed=1, std=0.05)


SITES = {
    "encoder.layers.1.self_attention.q_proj": ("enc", 1, "q"),
    "encoder.layers.0.self_attention.k_proj": ("enc", 0, "k"),
    "encoder.layers.0.self_attention.v_proj": ("enc", 0, "v"),
    "decoder.layers.0.self_attention.q_proj": ("self", 0, "q"),
    "decoder.layers.1.self_attention.k_proj": ("self", 1, "k"),
    "decoder.layers.1.self_attention.v_proj": ("self", 1, "v"),
    "decoder.layers.1.cross_attention.q_proj": ("cross", 1, "q"),
    "decoder.layers.0.cross_attention.k_proj": ("cross", 0, "k"),
    "decoder.layers.0.cross_attention.v_proj": ("cross", 0, "v"),
}


def test_module_paths_and_delta(tiny, tmp_path):
    """every supported site, with and without the .default segment and the base_model.model. prefix, rank_pattern and
    alpha_pattern on one module: the bank's A / B reproduce merge_lora_state_dict's delta"""
    cfg, sd = tiny
    gen = torch.Generator().manual_seed(0)
    tensors = {}
    for i, path in enumerate(SITES):
        r = 6 if path.endswith("layers.1.self_attention.k_proj") else 4
        tensors.update(pair(sd, path, r, gen, prefix="" if i % 3 == 0 else "base_model.model.", seg=".default" if i % 2 else ""))
    ad = write_adapter(tmp_path, "all", tensors, r=4, alpha=8, rank_pattern={"layers.1.self_attention.k_proj": 6},
                       alpha_pattern={"decoder.layers.1.self_attention.k_proj": 3.0})
    bank = AdapterBank(cfg, "cpu")
    assert bank.add("voice", ad) == 0 and bank.names == ["voice"] and len(bank) == 1
    assert bank.index_of("voice") == 0 and bank.index_of(None) == -1 and bank.index_of(0) == 0
    with pytest.raises(ValueError):
        bank.index_of("nobody")
    host = bank.host[0]
    assert set(host) == set(SITES.values())
    for path, mod in SITES.items():
        assert bank.module_of(path) == mod
    k6 = host[("self", 1, "k")]
    assert k6["rank"] == 6 and k6["scale"] == 3.0 / 6 and host[("enc", 1, "q")]["rank"] == 4 and host[("enc", 1, "q")]["scale"] == 2.0
    assert bank.max_rank(("self", 1, "k")) == 6 and bank.max_rank(("self", 0, "k")) == 0      # a module the adapter lacks: rank 0
    merged = merge_lora_state_dict(sd, ad)
    for path, mod in SITES.items():
        w = sd[path + ".weight"]
        n_in, n_out = bank.shape_of(mod)
        assert (n_in, n_out) == (w.shape[0], w.numel() // w.shape[0])
        h = host[mod]
        assert h["A"].dtype == torch.float32 and tuple(h["A"].shape) == (h["rank"], n_in) and tuple(h["B"].shape) == (h["rank"], n_out)
        assert h["A"].is_contiguous() and h["B"].is_contiguous()
        delta = h["scale"] * (h["A"].double().t() @ h["B"].double())               # [in, out]: what the kernels add, as a matrix
        want = (merged[path + ".weight"].double() - w.double()).reshape(n_in, n_out)
        # merge adds the fp32 delta to the fp32 kernel: one rounding of the sum and the fp32 product's own, both relative to 2^-24
        tol = 2.0 ** -22 * (w.abs().max().double() + delta.abs().max())
        assert float((delta - want).abs().max()) <= float(tol), path


def test_fan_in_fan_out(tiny, tmp_path):
    """fan_in_fan_out: merge adds scale * B @ A untransposed (square kernels only) — the bank's A / B change roles"""
    cfg, sd = tiny
    path = "decoder.layers.0.self_attention.q_proj"                # tiny: 96 -> 4 heads x 16 = 64: not square
    w = sd[path + ".weight"]
    assert w.shape[0] != w.numel() // w.shape[0]
    gen = torch.Generator().manual_seed(1)
    bank = AdapterBank(cfg, "cpu")
    with pytest.raises(RuntimeError, match="do not fit"):
        bank.add("x", write_adapter(tmp_path, "fifo_bad", pair(sd, path, 4, gen), fan_in_fan_out=True))
    js = C.config_to_json_dict(cfg)
    js["model"]["encoder"]["n_embd"] = 64                           # encoder q_proj 64 -> 4 x 16: square
    cfg2 = C.config_from_json_dict(js)
    sd2 = synthetic_state_dict(cfg2, seed=2, std=0.05)
    p2 = "encoder.layers.0.self_attention.q_proj"
    ad = write_adapter(tmp_path, "fifo", pair(sd2, p2, 4, gen), fan_in_fan_out=True)
    bank2 = AdapterBank(cfg2, "cpu")
    bank2.add("f", ad)
    h = bank2.host[0][("enc", 0, "q")]
    delta = h["scale"] * (h["A"].double().t() @ h["B"].double())
    w2 = sd2[p2 + ".weight"]
    want = (merge_lora_state_dict(sd2, ad)[p2 + ".weight"].double() - w2.double()).reshape(64, 64)
    assert float((delta - want).abs().max()) <= float(2.0 ** -22 * (w2.abs().max().double() + delta.abs().max()))
    plain = write_adapter(tmp_path, "plain", pair(sd2, p2, 4, torch.Generator().manual_seed(1)))
    bank2.add("p", plain)
    assert not torch.equal(bank2.host[1][("enc", 0, "q")]["A"], h["A"])


def test_refusals(tiny, tmp_path):
    cfg, sd = tiny
    gen = torch.Generator().manual_seed(2)
    bank = AdapterBank(cfg, "cpu")
    for bad in ("decoder.layers.1.cross_attention.o_proj", "decoder.layers.0.mlp.wi_fused", "encoder.layers.0.mlp.wo", "decoder.logits_dense"):
        w = sd[bad + ".weight"]
        t = {f"{bad}.lora_A.weight": torch.randn(4, 8, generator=gen), f"{bad}.lora_B.weight": torch.randn(8, 4, generator=gen)}
        with pytest.raises(RuntimeError) as ei:
            bank.add("bad", write_adapter(tmp_path, "bad", t))
        assert bad in str(ei.value) and "adapter_path=" in str(ei.value)
    # the first unsupported module is the one named
    good, bad = "decoder.layers.0.self_attention.q_proj", "decoder.layers.0.self_attention.o_proj"
    t = dict(pair(sd, good, 4, gen), **pair(sd, bad, 4, gen))
    with pytest.raises(RuntimeError, match=r"self_attention\.o_proj"):
        bank.add("mixed", write_adapter(tmp_path, "mixed", t))
    with pytest.raises(RuntimeError, match="rank 65"):
        bank.add("wide", write_adapter(tmp_path, "wide", pair(sd, good, MAX_RANK + 1, gen), r=MAX_RANK + 1))
    bank.add("r64", write_adapter(tmp_path, "r64", pair(sd, good, MAX_RANK, gen), r=MAX_RANK))
    with pytest.raises(RuntimeError, match="not a module of this model"):
        bank.add("nope", write_adapter(tmp_path, "nope", {"decoder.layers.9.self_attention.q_proj.lora_A.weight": torch.zeros(4, 96),
                                                         "decoder.layers.9.self_attention.q_proj.lora_B.weight": torch.zeros(64, 4)}))
    with pytest.raises(RuntimeError, match="not a module of this model"):
        bank.add("nope2", write_adapter(tmp_path, "nope2", {"nope.lora_A.weight": torch.zeros(4, 96), "nope.lora_B.weight": torch.zeros(64, 4)}))
    with pytest.raises(RuntimeError, match="does not match adapter_config"):
        bank.add("r", write_adapter(tmp_path, "r", pair(sd, good, 4, gen), r=8))
    with pytest.raises(RuntimeError, match="do not fit"):
        bank.add("s", write_adapter(tmp_path, "s", {f"{good}.lora_A.weight": torch.zeros(4, 95), f"{good}.lora_B.weight": torch.zeros(64, 4)}))
    with pytest.raises(ValueError, match="already in the bank"):
        bank.add("r64", write_adapter(tmp_path, "again", pair(sd, good, 4, gen)))
    assert bank.names == ["r64"]                                    # nothing half-added


def test_bank_is_fixed_once_a_session_took_it(tiny, tmp_path):
    """freeze() is what a session calls on the bank it is handed: the tables are uploaded (here: to the CPU device) and add() raises"""
    cfg, sd = tiny
    gen = torch.Generator().manual_seed(3)
    bank = AdapterBank(cfg, "cpu")
    with pytest.raises(RuntimeError, match="empty"):
        bank.freeze()
    q, v = "decoder.layers.0.self_attention.q_proj", "decoder.layers.1.cross_attention.v_proj"
    bank.add("a", write_adapter(tmp_path, "a", pair(sd, q, 4, gen)))
    bank.add("b", write_adapter(tmp_path, "b", dict(pair(sd, q, 2, gen), **pair(sd, v, 3, gen)), r=2, rank_pattern={"v_proj": 3}))
    bank.freeze()
    with pytest.raises(RuntimeError, match="fixed once a session"):
        bank.add("c", write_adapter(tmp_path, "c", pair(sd, q, 4, gen)))
    # the uploaded tables: [module][adapter] rank / scale, pointers into ONE arena at 16-byte aligned offsets
    iq, iv = bank.modules.index(("self", 0, "q")), bank.modules.index(("cross", 1, "v"))
    assert bank.rank[iq].tolist() == [4, 2] and bank.rank[iv].tolist() == [0, 3]
    assert bank.scale[iq].tolist() == [2.0, 4.0] and int(bank.ptr_a[iv, 0]) == 0 and int(bank.ptr_b[iv, 0]) == 0
    base, n = bank.arena.data_ptr(), bank.arena.numel()
    for t in (bank.ptr_a, bank.ptr_b):
        for p in t[t != 0].tolist():
            assert (p - base) % 16 == 0 and 0 <= (p - base) // 4 < n
    off = (int(bank.ptr_b[iv, 1]) - base) // 4
    hB = bank.host[1][("cross", 1, "v")]["B"]
    assert torch.equal(bank.arena[off: off + hB.numel()].reshape(hB.shape), hB)


def test_cli_adapter_flags(capsys):
    sys.path.insert(0, ROOT)
    import cli

    p = cli.build_parser()
    a = p.parse_args(["hi", "--codes-output", "x.npy", "--adapter", "anna=/a", "--adapter", "ben=/b", "--use-adapter", "ben"])
    assert a.adapter == ["anna=/a", "ben=/b"] and a.use_adapter == "ben"
    assert cli.parse_adapter_flags(p, a) == {"anna": "/a", "ben": "/b"} and cli.used_adapters(a) == ["ben"]
    a = p.parse_args(["hi", "--codes-output", "x.npy", "--slots", "2", "--adapter", "anna=/a", "--use-adapter", "anna,,anna"])
    assert cli.parse_adapter_flags(p, a) == {"anna": "/a"} and cli.used_adapters(a) == ["anna", None, "anna"]
    assert cli.used_adapters(p.parse_args(["hi"])) is None
    for argv, msg in ((["hi", "--codes-output", "x.npy", "--adapter", "a=/a", "--adapter-path", "/m"], "cannot be combined"),
                      (["hi", "--codes-output", "x.npy", "--use-adapter", "a", "--adapter-path", "/m"], "cannot be combined"),
                      (["hi", "--codes-output", "x.npy", "--adapter", "a"], "NAME=DIR"),
                      (["hi", "--codes-output", "x.npy", "--adapter", "a=/a", "--use-adapter", "b"], "not among"),
                      (["hi", "--codes-output", "x.npy", "--adapter", "a=/a", "--use-adapter", "a,a"], "only with --slots")):
        with pytest.raises(SystemExit):
            cli.main(argv)
        assert msg in capsys.readouterr().err, argv


def test_plan_adapters():
    from dia_hip.callers import _plan_adapters
    assert _plan_adapters(None, 3) is None and _plan_adapters("a", 2) == ["a", "a"] and _plan_adapters(["a"], 2) == ["a", "a"]
    assert _plan_adapters(["a", None], 2) == ["a", None]
    with pytest.raises(ValueError):
        _plan_adapters(["a", "b"], 3)


def test_kernel_entry_points_refuse_bad_arguments():
    """the argument checks that never launch (the library loads without a GPU)"""
    import ctypes

    from dia_hip import binding as hb

    L = hb.lib()
    assert L.dia_lora_apply(ctypes.byref(hb.LoraArgs()), None) == -1 and b"dia_lora_apply" in L.dia_last_error()
    assert L.dia_lora_crosskv(ctypes.byref(hb.LoraCrossKvArgs()), None) == -1 and b"dia_lora_crosskv" in L.dia_last_error()
    assert L.dia_engine_set_lora(None, None) == -1 and b"null engine" in L.dia_last_error()


def test_lora_structs_match_the_header():
    """size and every field offset of the new ctypes mirrors against include/dia_hip.h, through the system compiler (the check
    tests/test_abi.py makes for the older structs' sizes)"""
    import ctypes
    import subprocess
    import tempfile

    from dia_hip import binding as hb

    pairs = [("dia_lora_seg", hb.LoraSeg), ("dia_lora_args", hb.LoraArgs), ("dia_lora_crosskv_args", hb.LoraCrossKvArgs),
             ("dia_lora_layer", hb.LoraLayer), ("dia_lora_step", hb.LoraStep)]
    lines = []
    for cname, t in pairs:
        lines.append(f'printf("%zu", sizeof({cname}));')
        lines += [f'printf(" %zu", offsetof({cname}, {f[0]}));' for f in t._fields_]
        lines.append('printf("\\n");')
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "dia_hip.h"\nint main(void){\n' + "\n".join(lines) + "\nreturn 0; }\n"
    with tempfile.TemporaryDirectory() as td:
        c, exe = os.path.join(td, "s.c"), os.path.join(td, "s")
        open(c, "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [[int(v) for v in ln.split()] for ln in subprocess.check_output([exe]).decode().splitlines()]
    for (cname, t), row in zip(pairs, got):
        assert row == [ctypes.sizeof(t)] + [getattr(t, f[0]).offset for f in t._fields_], cname
    assert hb.LORA_MAX_RANK == 64 and hb.LORA_MAX_SEGS == 3
