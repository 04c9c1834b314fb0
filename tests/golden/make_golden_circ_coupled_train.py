#!/usr/bin/env python3
"""Generates the training fixtures of the circular NSF coupling layer (CircularCoupledRationalQuadraticSpline, wrapper.py:88-185) by
running the REAL reference (normflows 1.7.3, PyTorch CPU) under autograd, like make_golden_ar_ft_train.py: loss = sum(z * cz) +
sum(ld * cl) through layer.inverse(x) (the density direction; key prefix `inv`) and, for the first case, through layer.forward(x) as well
(the sampling direction; `fwd`): float32 and float64 legs of z, ld, gx, and of every parameter gradient a strided sample (every 37th
element of the flattened tensor) plus its sum and absolute sum.  In addition the STATE DICT, x, cz, cl and `outside`.

    python tests/golden/make_golden_circ_coupled_train.py <path of the reference checkout>

Every parameter is perturbed by N(0, sigma^2) (init_identity=False); inputs are uniform within 0.98 x bound.  In the first case rows
0-3 carry one coordinate each 0.5 outside its interval -- an identity and a transform coordinate of either tails type, listed in
`outside` as (row, column): list tails leave output, log-det and every gradient of such a coordinate 0 (utils/splines.py:48-57).

The generator asserts (change the seed if one fails): no coordinate within 1e-3 of +-bound; the outputs at `outside` are exactly 0; and
the reference's own float32 leg is within 1e-4 of scale (max|a - b| / max(1, max|b|)) of its float64 leg for every stored quantity -- a
larger gap means a row sits on a ReLU or bin kink, and no implementation could be held to a bar on it.

A committed file stays below 1 MiB: the weights of a fixture that would not fit go to part files <name>__w1.npz, ...
(tests/circ_coupled_train_cases.load_case puts them together again)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.abspath(sys.argv[1]))
import normflows as nf  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
torch.set_num_threads(4)
STRIDE = 37
PART_BYTES = 900 * 1024


def bound_d7():
    b = torch.tensor([2.0 + 0.1 * i for i in range(7)], dtype=torch.float32)
    b[[0, 2, 3, 6]] = float(np.pi)
    return b


# (name, constructor, D, B, seed, sigma, directions, outside positions)
CASES = (
    ("grad_circ_cpl_d7_h40", lambda: nf.flows.CircularCoupledRationalQuadraticSpline(
        7, 2, 40, ind_circ=[0, 2, 3, 6], num_bins=8, tail_bound=bound_d7(), init_identity=False),
     7, 70, 5111, 0.2, ("inv", "fwd"), ((0, 0), (1, 4), (2, 3), (3, 1))),
    ("grad_circ_cpl_d21_h260", lambda: nf.flows.CircularCoupledRationalQuadraticSpline(
        21, 1, 260, ind_circ=[1, 2, 8, 17, 20], num_bins=8, tail_bound=float(np.pi), reverse_mask=True, init_identity=False),
     21, 130, 5102, 0.08, ("inv",), ()),
    ("grad_circ_cpl_d6_k5", lambda: nf.flows.CircularCoupledRationalQuadraticSpline(
        6, 2, 24, ind_circ=[1, 3, 4], num_bins=5, tail_bound=2.5, init_identity=False),
     6, 70, 5103, 0.2, ("inv",), ()),
)


def build(make, seed, sigma, dt):
    torch.manual_seed(seed)
    layer = make()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for p in layer.parameters():
            p.add_(sigma * torch.randn(p.shape, generator=g, dtype=p.dtype))
    return layer.to(dt)


def full_bound(layer, D):
    """The (D,) bound of every column, put together from the two halves."""
    p = layer.prqct
    tb = torch.zeros(D)
    for idx, b in ((p.transform_features, p.tail_bound), (p.identity_features, p.unconditional_transform.tail_bound)):
        tb[idx] = b.float() if torch.is_tensor(b) else torch.full((len(idx),), float(b))
    return tb


def scale_err(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max()) / max(1.0, float(b.abs().max()))


def compute(make, D, B, seed, sigma, directions, outside):
    """(stored arrays, state dict, worst float32-vs-float64 gap of scale) of one case."""
    out, full = {}, {}
    for dt, leg in ((torch.float32, "f32"), (torch.float64, "f64")):
        layer = build(make, seed, sigma, dt)
        g = torch.Generator().manual_seed(seed + 2)
        tb = full_bound(layer, D)
        x = (2 * torch.rand(B, D, generator=g) - 1) * tb * 0.98
        for k, (r, c) in enumerate(outside):
            x[r, c] = (tb[c] + 0.5) * (1.0 if k % 2 == 0 else -1.0)
        assert float((x.abs() - tb).abs().min()) > 1e-3, "a coordinate within 1e-3 of +-bound: change the seed"
        cz = torch.randn(B, D, generator=g)
        cl = torch.randn(B, generator=g)
        for d in directions:
            layer.zero_grad(set_to_none=True)
            xx = x.to(dt).clone().requires_grad_(True)
            z, ld = (layer.inverse if d == "inv" else layer.forward)(xx)
            ((z * cz.to(dt)).sum() + (ld * cl.to(dt)).sum()).backward()
            for r, c in outside:
                assert float(z.detach()[r, c]) == 0.0, "list tails: 0 outside the interval"
            out.update({"z_%s_%s" % (d, leg): z.detach(), "ld_%s_%s" % (d, leg): ld.detach(), "gx_%s_%s" % (d, leg): xx.grad})
            for k, p_ in layer.named_parameters():
                gflat = p_.grad.reshape(-1)
                key = k.replace(".", "__")
                out["g_%s_%s__%s" % (d, leg, key)] = gflat[::STRIDE].clone()
                out["chk_%s_%s__%s" % (d, leg, key)] = torch.tensor([float(gflat.double().sum()), float(gflat.double().abs().sum())],
                                                                   dtype=torch.float64)
                full["%s_%s__%s" % (d, leg, key)] = gflat.detach().clone()
        if dt == torch.float32:
            out.update(x=x, cz=cz, cl=cl)
            sd = layer.state_dict()
    worst = max(scale_err(out[k], out[k.replace("_f32", "_f64")]) for k in list(out) if "_f32" in k and not k.startswith("chk_"))
    worst = max([worst] + [scale_err(full[k], full[k.replace("_f32__", "_f64__")]) for k in full if "_f32__" in k])
    return out, sd, worst


def main():
    for name, make, D, B, seed, sigma, directions, outside in CASES:
        out, sd, worst = compute(make, D, B, seed, sigma, directions, outside)
        print("%s: worst float32-vs-float64 %.2e of scale" % (name, worst))
        assert worst <= 1e-4, "a row sits on a ReLU or bin kink: change the seed"
        arrays = {k: v.detach().cpu().numpy() for k, v in out.items()}
        arrays["stride"] = np.array(STRIDE)
        arrays["outside"] = np.asarray(outside, dtype=np.int64).reshape(-1, 2)
        parts, weights = [], []
        for k, v in sd.items():
            a = v.detach().cpu().numpy()
            key = "sd__" + k.replace(".", "__")
            if a.nbytes > 64 * 1024:
                weights.append((key, a))
            else:
                arrays[key] = a
        cur, size = {}, 0
        total = sum(a.nbytes for _, a in weights)
        if total <= PART_BYTES // 2:
            arrays.update(dict(weights))
        else:
            for key, a in weights:
                if size + a.nbytes > PART_BYTES and cur:
                    parts.append(cur)
                    cur, size = {}, 0
                cur[key] = a
                size += a.nbytes
            parts.append(cur)
        paths = [(os.path.join(OUT, name + ".npz"), arrays)]
        paths += [(os.path.join(OUT, "%s__w%d.npz" % (name, i + 1)), p) for i, p in enumerate(parts)]
        for path, arr in paths:
            np.savez_compressed(path, **arr)
            kb = os.path.getsize(path) / 1024
            assert kb < 1024, (path, kb)
            print("  wrote %s %.1f KB" % (os.path.basename(path), kb))


if __name__ == "__main__":
    main()
