"""Teacher-forced scoring, the parts that need no GPU: dia_score_args on the C side against its ctypes mirror, the forced rows and the
valid positions (dia_hip/score.py) against the oracle's delayed prefill, the summary against a direct NumPy computation, and the
argument errors of the kernel entry point, the engine hook, the session, Dia.score's host work and the command line."""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from dia_hip import binding as hb
from dia_hip import config as C
from dia_hip import score as S
from oracle import dia_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_score_args_layout_matches_header():
    names = [f[0] for f in hb.ScoreArgs._fields_]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "dia_hip.h"\nint main(void){ printf("%zu", sizeof(dia_score_args));\n'
    prog += "".join(f'printf(" %zu", offsetof(dia_score_args, {n}));\n' for n in names) + "return 0; }\n"
    with tempfile.TemporaryDirectory() as td:
        c, exe = os.path.join(td, "s.c"), os.path.join(td, "s")
        open(c, "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(v) for v in subprocess.check_output([exe]).split()]
    assert got == [ctypes.sizeof(hb.ScoreArgs)] + [getattr(hb.ScoreArgs, n).offset for n in names]
    assert names == ["logits", "ld_logits", "B", "T", "C", "V", "cfg_scale", "cfg_scales", "eos", "pad", "bos", "_pad0",
                     "tokens", "cur", "first_step", "fsm", "out"]
    assert hb.ABI_VERSION == 8 and "dia_score" in hb.EXPORTS and "dia_engine_set_score" in hb.EXPORTS


def test_score_refusals_without_gpu():
    L = hb.lib()
    buf = ctypes.create_string_buffer(64)            # never dereferenced: every case is refused before a launch
    addr = ctypes.addressof(buf)

    def args(**kw):
        a = hb.ScoreArgs()
        a.logits = a.tokens = a.cur = a.out = addr
        a.ld_logits, a.B, a.T, a.C, a.V = 9 * 1028 + 12, 1, 8, 9, 1028
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    assert L.dia_score(None, None) == -1
    for kw, word in ((dict(C=13), b"channels"), (dict(V=1089), b"vocabulary"), (dict(out=None), b"null"), (dict(logits=None), b"null"),
                     (dict(tokens=None), b"null"), (dict(cur=None), b"null"), (dict(C=0), b"channels"), (dict(V=0), b"vocabulary"),
                     (dict(B=0), b"empty"), (dict(ld_logits=9 * 1028 - 1), b"ld_logits")):
        assert L.dia_score(ctypes.byref(args(**kw)), None) == -1, kw
        assert word in L.dia_last_error(), (kw, L.dia_last_error())
    assert L.dia_engine_set_score(None, ctypes.byref(args())) == -1
    assert L.dia_engine_set_score(None, None) == -1


@pytest.mark.parametrize("T", [1, 5, 40])
def test_teacher_rows_and_valid_mask(T):
    cfg = C.tiny_config()
    dm = O.Dims.of(cfg)
    assert dm.C == 9
    codes = np.random.RandomState(T).randint(0, 1024, size=(T, dm.C)).astype(np.int32)
    rows = S.teacher_rows(cfg, codes)
    want, step = O.delayed_prefill(dm, codes)
    assert rows.dtype == np.int32 and np.array_equal(rows, want) and rows.shape == (1 + T + max(dm.delay), dm.C)
    assert np.array_equal(S.teacher_rows(cfg, rows), rows)                  # a delayed buffer: taken as is
    assert np.array_equal(S.teacher_rows(cfg, codes[None]), rows)           # [1, T, C]
    m = S.valid_mask(rows, 1, dm)
    assert m.shape == rows.shape and int(m.sum()) == T * dm.C
    assert not m[(rows == dm.pad) | (rows == dm.bos)].any()
    for c, d in enumerate(dm.delay):                                        # channel c's frames sit at rows 1 + d .. T + d
        assert np.array_equal(np.nonzero(m[:, c])[0], np.arange(1 + d, 1 + d + T))
    assert np.array_equal(S.valid_mask(rows, 1, cfg.data), m)               # cfg.data names the same ids
    # rows below first_step never count
    fs = min(3, rows.shape[0])
    assert np.array_equal(S.valid_mask(rows, fs, dm), m & (np.arange(rows.shape[0]) >= fs)[:, None])
    # batched, one first_step per utterance
    mb = S.valid_mask(np.stack([rows, rows]), [1, fs], dm)
    assert np.array_equal(mb[0], m) and np.array_equal(mb[1], S.valid_mask(rows, fs, dm))


def test_valid_mask_eos_counts_on_channel_zero_only():
    dm = O.Dims.of(C.tiny_config())
    rows = np.full((4, dm.C), dm.eos, dtype=np.int32)
    rows[0] = dm.bos
    rows[3] = -1                                                            # the fill behind a buffer
    m = S.valid_mask(rows, 1, dm)
    assert m[1:3, 0].all() and int(m.sum()) == 2
    rows[2, 1] = dm.tgt_vocab                                               # outside the vocabulary
    rows[2, 2] = dm.eos - 1
    m = S.valid_mask(rows, 1, dm)
    assert not m[2, 1] and m[2, 2] and int(m.sum()) == 3


def test_teacher_rows_with_prompt():
    cfg = C.tiny_config()
    dm = O.Dims.of(cfg)
    rs = np.random.RandomState(7)
    prompt, codes = rs.randint(0, 1024, size=(3, dm.C)), rs.randint(0, 1024, size=(6, dm.C))
    rows = S.teacher_rows(cfg, codes, prompt=prompt)
    assert np.array_equal(rows, O.delayed_prefill(dm, np.concatenate([prompt, codes]))[0])
    assert S.check_prompt_rows(cfg, rows, prompt) == 4
    assert S.check_prompt_rows(cfg, rows[:12], prompt) == 4                 # a cut delayed buffer keeps its prompt rows
    with pytest.raises(ValueError, match="do not start"):
        S.check_prompt_rows(cfg, S.teacher_rows(cfg, codes), prompt)
    with pytest.raises(ValueError, match="nothing to score"):
        S.check_prompt_rows(cfg, rows[:4], prompt)


def test_summarise_against_numpy():
    rs = np.random.RandomState(1)
    rows, Cn = 23, 9
    sc = -np.abs(rs.normal(size=(rows, Cn, 3))).astype(np.float32) * 4
    sc[..., 2] = np.abs(sc[..., 2])
    valid = rs.rand(rows, Cn) < 0.6
    valid[:, 8] = False                                                     # a channel with nothing valid
    sc[~valid] = np.nan                                                     # what the device leaves at positions it never scored ...
    sc[0, 8, 1] = -np.inf                                                   # ... and at a masked target: both ignored where invalid
    r = S.summarise(sc, valid)
    assert r.n_valid == int(valid.sum())
    v64 = sc.astype(np.float64)
    assert r.nll_cond == pytest.approx(-v64[..., 0][valid].mean(), rel=1e-12)
    assert r.nll_cfg == pytest.approx(-v64[..., 1][valid].mean(), rel=1e-12)
    assert r.mean_entropy_cfg == pytest.approx(v64[..., 2][valid].mean(), rel=1e-12)
    assert r.perplexity_cfg == pytest.approx(np.exp(-v64[..., 1][valid].mean()), rel=1e-12)
    for c in range(Cn):
        if valid[:, c].any():
            assert r.nll_cond_per_channel[c] == pytest.approx(-v64[:, c, 0][valid[:, c]].mean(), rel=1e-12)
            assert r.nll_cfg_per_channel[c] == pytest.approx(-v64[:, c, 1][valid[:, c]].mean(), rel=1e-12)
        else:
            assert np.isnan(r.nll_cond_per_channel[c]) and np.isnan(r.nll_cfg_per_channel[c])
    assert np.isfinite([r.nll_cond, r.nll_cfg, r.mean_entropy_cfg, r.perplexity_cfg]).all()
    assert r.lp_cfg.shape == (rows, Cn) and np.array_equal(r.valid, valid)
    import json
    assert json.loads(json.dumps(r.summary()))["n_valid"] == r.n_valid


def test_summarise_propagates_a_valid_zero_probability():
    sc = np.full((3, 2, 3), -1.0, dtype=np.float32)
    valid = np.ones((3, 2), dtype=bool)
    sc[1, 1, 1] = -np.inf                                                   # a VALID target the guided distribution excludes
    r = S.summarise(sc, valid)
    assert r.nll_cfg == np.inf and r.perplexity_cfg == np.inf and r.nll_cfg_per_channel[1] == np.inf
    assert r.nll_cond == 1.0 and r.nll_cfg_per_channel[0] == 1.0
    sc[0, 0, 0] = np.nan                                                    # a valid position no step scored
    assert np.isnan(S.summarise(sc, valid).nll_cond)
    with pytest.raises(ValueError):
        S.summarise(sc, valid[:2])


def test_wrong_codes_shape():
    cfg = C.tiny_config()
    for bad in (np.zeros((5, 8), np.int32), np.zeros((5,), np.int32), np.zeros((2, 5, 9), np.int32), np.zeros((0, 9), np.int32)):
        with pytest.raises(ValueError, match="Unexpected codes shape"):
            S.teacher_rows(cfg, bad)
    with pytest.raises(ValueError, match="integers"):
        S.teacher_rows(cfg, np.zeros((5, 9), np.float32))


def test_score_without_teacher_tokens_is_refused():
    """the check comes before anything touches a device"""
    from dia_hip.engine import DecodeSession
    with pytest.raises(ValueError, match="teacher_tokens"):
        DecodeSession(None, [np.zeros(4, np.int32)], score=True)
    with pytest.raises(ValueError, match="teacher_tokens"):
        DecodeSession(None, [np.zeros(4, np.int32)], score=True, teacher_tokens=[np.zeros((4, 9), np.int32)], _slotted=True)


def test_cli_score_codes_needs_a_model_path(tmp_path, capsys):
    sys.path.insert(0, ROOT)
    import cli
    f = tmp_path / "codes.npy"
    np.save(f, np.zeros((4, 9), np.int32))
    with pytest.raises(SystemExit) as e:
        cli.main(["[S1] Hello.", "--score-codes", str(f)])
    assert e.value.code == 2 and "--model-path" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cli.main(["[S1] Hello.", "--score-output", str(tmp_path / "o.npz"), "--codes-output", str(tmp_path / "c.npy")])
    assert "--score-codes" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cli.main(["[S1] Hello.", "--score-codes", str(f), "--model-path", str(tmp_path), "--codes-output", str(tmp_path / "c.npy")])
    assert "generates nothing" in capsys.readouterr().err
