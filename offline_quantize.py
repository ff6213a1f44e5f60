#!/usr/bin/env python3
"""Offline weight-only quantisation of a Dia checkpoint: ``--format mxfp8`` (``mxfp4``: the same with e2m1 elements, for
``--weight-format mxfp4`` / ``quant="mxfp4"``, a quarter of the bytes) rounds every DenseGeneral kernel a decode step
streams (decoder q/k/v, o, cross-q, cross-o, wi, wo and the logits head) to OCP MXFP8 — e4m3 elements with one power-of-two
scale per 32 consecutive K of a column (dia_hip/quant.py) — and writes the DEQUANTISED values back as an ordinary
``pytorch_model.bin`` + ``config.json``.  Every such value is exactly a bf16 value, so the checkpoint runs anywhere a Dia
checkpoint runs; ``cli.py --weight-format mxfp8`` / ``DeviceWeights(quant="mxfp8")`` additionally stream it at half the bytes.

This is an offline CPU tool (fp32 tensor arithmetic on the checkpoint, no model execution), in the style of offline_prune.py.
"""

from __future__ import annotations

import argparse
import os
import sys
from pathlib import Path

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "dia-tts-prune_amd"))


def main(argv=None) -> int:
    p = argparse.ArgumentParser(description="Quantise a Dia checkpoint on the CPU and write it back with the rounded weights baked in.")
    p.add_argument("--model-path", type=str, required=True, help="directory of the model: config.json plus its checkpoint")
    p.add_argument("--output-dir", type=str, required=True, help="where pytorch_model.bin and config.json of the quantised model go")
    p.add_argument("--format", type=str, default="mxfp8", choices=["mxfp8", "mxfp4"],
                   help="mxfp8 = e4m3 elements, mxfp4 = e2m1 elements; an E8M0 scale per 32 K of a column")
    p.add_argument("--gram-stats", type=str, default=None, metavar="FILE.npz",
                   help="Gram matrices of the decode step's GEMM inputs (cli.py --calibrate-codes ... --gram-output): quantise by GPTQ, pushing "
                        "every element's rounding error into the weights behind it, instead of rounding to nearest")
    p.add_argument("--damp", type=float, default=0.01, help="with --gram-stats: the share of the Hessian's mean diagonal added to its diagonal")
    a = p.parse_args(argv)

    from dia_hip import weights as W
    from dia_hip.pruning import _kernel_2d
    from dia_hip.quant import calibration_error, gptq_quantize_state_dict, mxfp4_quantize_state_dict, mxfp8_names, mxfp8_quantize_state_dict

    out = Path(a.output_dir)
    out.mkdir(parents=True, exist_ok=True)
    print(f"Loading model from {a.model_path}...")
    try:
        cfg_path, ckpt = W.find_checkpoint_in_dir(a.model_path)
        cfg = W.read_hub_config(cfg_path)
        sd = {k: v.float() for k, v in W.load_state_dict_file(ckpt).items()}
        missing, _ = W.check_state_dict(cfg, sd)
        if missing:
            raise RuntimeError(f"Missing keys in checkpoint: {missing}")
    except Exception as e:
        print(f"Error loading model: {e}")
        return 1
    print(f"\nQuantising to {a.format}...")
    qsd = (mxfp4_quantize_state_dict if a.format == "mxfp4" else mxfp8_quantize_state_dict)(cfg, sd)
    if a.gram_stats:
        from dia_hip.calib import GramStats
        try:
            grams = GramStats.load(a.gram_stats)
            grams.check_against(cfg)
        except Exception as e:
            print(f"Error loading Gram matrices: {e}")
            return 1
        rtn = qsd
        print(f"GPTQ against {a.gram_stats} (damp {a.damp})...")
        qsd = gptq_quantize_state_dict(cfg, sd, grams, a.format, damp=a.damp)
        err = {"round-to-nearest": 0.0, "GPTQ": 0.0}
        for k in mxfp8_names(cfg):                     # sum over the kernels of tr(delta^T G delta), the output error on the calibration rows
            G, w = grams.dense(k), _kernel_2d(k, sd[k])
            err["round-to-nearest"] += calibration_error(G, _kernel_2d(k, rtn[k]) - w)
            err["GPTQ"] += calibration_error(G, _kernel_2d(k, qsd[k]) - w)
        for kind, v in err.items():
            print(f"Calibration-set output error, {kind}: {v:.6e}")
        print(f"GPTQ / round-to-nearest: {err['GPTQ'] / max(err['round-to-nearest'], 1e-300):.4f}")
    num = sum(float((_kernel_2d(k, qsd[k]) - _kernel_2d(k, sd[k])).pow(2).sum()) for k in mxfp8_names(cfg))
    den = sum(float(sd[k].pow(2).sum()) for k in mxfp8_names(cfg))
    print(f"Relative RMS error of the quantised kernels: {(num / max(den, 1e-30)) ** 0.5:.4f}")
    print(f"\nSaving quantised model to {a.output_dir}...")
    torch.save(dict(qsd), out / "pytorch_model.bin")
    cfg.save(str(out / "config.json"))
    print("Offline quantisation finished successfully.")
    return 0


if __name__ == "__main__":
    sys.exit(main())
