#!/usr/bin/env python3
"""Generates the fixtures of the one-launch wide RealNVP coupling layer (tests/golden/affine_wide_<name>.npz) by running the REAL
reference (normflows 1.7.3, PyTorch CPU), as the other make_golden_*.py scripts do.  Run where the reference is importable
(NF_REFERENCE_DIR names its checkout when it is not installed); the GPU box has no reference:
    python tests/golden/make_golden_affine_wide.py

Per case of tests/affine_wide_cases.py: the layer (MaskedAffineFlow, affine/coupling.py:174-229, or AffineCouplingBlock, :232-267,
over nets/mlp.py:5-58) default-initialised under the case's seed; the rows of its last Linear that give the scale parameter are then
multiplied by one factor so that max |s| over the fixture's rows is 2 (the transform is far from the identity; the median |s| is
printed).  Each file holds the float32 state dict (`sd__*`, the mask buffer included), x (130 rows, N(0, 1)), and y_fwd / ld_fwd,
y_inv / ld_inv of layer.forward(x) and layer.inverse(x) in float32, plus the same float32 parameters evaluated in float64
(`*_f64`: the reference's own float32 error)."""
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
S_MAX = 2.0


def scale_param(layer, case, x):
    """The scale parameter the layer computes on x: s(b x) of a masked flow, param[:, 1::2] of a block."""
    if case["kind"] == "masked":
        return layer.s(layer.b * x)
    z1 = layer.flows[0](x)[0][0]
    return layer.flows[1].param_map(z1)[:, 1::2]


def main():
    for name, case in cases.CASES.items():
        layer = cases.build(nf, name)
        x = torch.randn(cases.ROWS, case["d"], generator=torch.Generator().manual_seed(case["seed"] + 1))
        med = 0.0
        with torch.no_grad():
            so = cases.scale_outputs(layer, case)
            if so is not None:
                lin, rows = so
                f = S_MAX / float(scale_param(layer, case, x).abs().max())
                lin.weight[rows] *= f
                lin.bias[rows] *= f
                s = scale_param(layer, case, x).abs()
                assert abs(float(s.max()) - S_MAX) < 1e-3
                med = float(s.median())
            out = {"x": x}
            out.update({"sd__" + k.replace(".", "__"): v.clone() for k, v in layer.state_dict().items()})
            for leg, dt in (("", torch.float32), ("_f64", torch.float64)):
                m = layer.to(dt)
                for dname, fn in (("fwd", m.forward), ("inv", m.inverse)):
                    y, ld = fn(x.to(dt))
                    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(ld).all())
                    out["y_%s%s" % (dname, leg)], out["ld_%s%s" % (dname, leg)] = y, ld
        path = os.path.join(OUT, "affine_wide_%s.npz" % name)
        np.savez_compressed(path, **{k: v.detach().cpu().numpy() for k, v in out.items()})
        print("%s: median |s| %.3f, max |y_fwd| %.2f, max |y_inv| %.2f, max |ld| %.2f, %.1f KB"
              % (name, med, float(out["y_fwd"].abs().max()), float(out["y_inv"].abs().max()), float(out["ld_fwd"].abs().max()),
                 os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
