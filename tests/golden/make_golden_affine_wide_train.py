#!/usr/bin/env python3
"""Generates the training fixtures of the wide RealNVP coupling layers (tests/golden/grad_affine_wide_<name>.npz) by running the REAL
reference (normflows 1.7.3, PyTorch CPU) under autograd, as make_golden_circ_coupled_train.py does.  Run where the reference is
importable (NF_REFERENCE_DIR names its checkout when it is not installed); the GPU box has no reference:
    python tests/golden/make_golden_affine_wide_train.py

Per case of tests/affine_wide_cases.py: the weights and x (130 rows) of the existing affine_wide_<name>.npz, cotangents cz (130, d) and
cl (130,) drawn from torch.Generator().manual_seed(case seed + 2), loss = sum(z * cz) + sum(ld * cl) through layer.forward(x) (key
prefix `fwd`) and layer.inverse(x) (`inv`), in float32 (`f32`) and float64 (`f64`): z, ld, gx, and of every parameter gradient a strided
sample (every 37th element of the flattened tensor) plus its sum and absolute sum.  No weights: they are in the existing files.

The generator asserts that the reference's own float32 leg is within 1e-4 of scale (max|a - b| / max(1, max|b|)) of its float64 leg
for every stored quantity and every full parameter gradient -- a larger gap means a row sits on a ReLU kink, and no implementation
could be held to a bar on it."""
import os
import sys

import numpy as np
import torch

if os.environ.get("NF_REFERENCE_DIR"):
    sys.path.insert(0, os.environ["NF_REFERENCE_DIR"])
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import normflows as nf  # noqa: E402
import affine_wide_cases as cases  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
torch.set_num_threads(4)
STRIDE = 37


def scale_err(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max()) / max(1.0, float(b.abs().max()))


def main():
    overall = 0.0
    for name, case in cases.CASES.items():
        g = dict(np.load(os.path.join(OUT, "affine_wide_%s.npz" % name)))
        sd = {k[4:].replace("__", "."): torch.from_numpy(v) for k, v in g.items() if k.startswith("sd__")}
        x = torch.from_numpy(g["x"])
        gen = torch.Generator().manual_seed(case["seed"] + 2)
        cz = torch.randn(cases.ROWS, case["d"], generator=gen)
        cl = torch.randn(cases.ROWS, generator=gen)
        out, full = {"cz": cz, "cl": cl}, {}
        for dt, leg in ((torch.float32, "f32"), (torch.float64, "f64")):
            layer = cases.build(nf, name)
            layer.load_state_dict(sd)
            layer = layer.to(dt)
            for d in ("fwd", "inv"):
                layer.zero_grad(set_to_none=True)
                xx = x.to(dt).clone().requires_grad_(True)
                z, ld = (layer.forward if d == "fwd" else layer.inverse)(xx)
                ((z * cz.to(dt)).sum() + (ld * cl.to(dt)).sum()).backward()
                out.update({"z_%s_%s" % (d, leg): z.detach(), "ld_%s_%s" % (d, leg): ld.detach(), "gx_%s_%s" % (d, leg): xx.grad})
                for k, p_ in layer.named_parameters():
                    gflat = (torch.zeros_like(p_) if p_.grad is None else p_.grad).reshape(-1)
                    key = k.replace(".", "__")
                    out["g_%s_%s__%s" % (d, leg, key)] = gflat[::STRIDE].clone()
                    out["chk_%s_%s__%s" % (d, leg, key)] = torch.tensor([float(gflat.double().sum()), float(gflat.double().abs().sum())],
                                                                       dtype=torch.float64)
                    full["%s_%s__%s" % (d, leg, key)] = gflat.detach().clone()
        worst = max(scale_err(out[k], out[k.replace("_f32", "_f64")]) for k in list(out) if "_f32" in k and not k.startswith("chk_"))
        worst = max([worst] + [scale_err(full[k], full[k.replace("_f32__", "_f64__")]) for k in full if "_f32__" in k])
        overall = max(overall, worst)
        print("%s: worst float32-vs-float64 %.2e of scale" % (name, worst))
        assert worst <= 1e-4, "a row sits on a ReLU kink"
        arrays = {k: v.detach().cpu().numpy() for k, v in out.items()}
        arrays["stride"] = np.array(STRIDE)
        path = os.path.join(OUT, "grad_affine_wide_%s.npz" % name)
        np.savez_compressed(path, **arrays)
        kb = os.path.getsize(path) / 1024
        assert kb < 1024, (path, kb)
        print("  wrote %s %.1f KB" % (os.path.basename(path), kb))
    print("worst over all cases: %.2e" % overall)


if __name__ == "__main__":
    main()
