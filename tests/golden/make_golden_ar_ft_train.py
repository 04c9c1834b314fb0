#!/usr/bin/env python3
"""Generates the training fixtures of the degree-order AR-NSF path (autograd.MadeFtFn) by running the REAL reference (normflows 1.7.3,
PyTorch CPU) under autograd, like gen_made_train in make_golden.py: loss = sum(z * cz) + sum(ld * cl) through layer.inverse(x) (the
density direction: ONE MADE pass), float32 and float64 legs of z, ld, gx, and of every parameter gradient a strided sample (every
37th element of the flattened tensor) plus its sum and absolute sum.  In addition the STATE DICT: masks and degrees are buffers, so the
permutation travels with it.

    python tests/golden/make_golden_ar_ft_train.py <path of the reference checkout>

Layers: CircularAutoregressiveRationalQuadraticSpline (wrapper.py:247-311) with a tensor bound / a scalar bound at 512 hidden slots,
and AutoregressiveRationalQuadraticSpline(permute_mask=True) (:186-244: no periodic feed, inputs beyond the bound).

The generator asserts (change the seed if either fails): the degree permutation is not the identity, and the reference's own float32
leg is within 1e-4 of scale (max|a - b| / max(1, max|b|)) of its float64 leg for every stored quantity -- a larger gap means a row sits
on a ReLU or bin kink, and no implementation could be held to a bar on it.

A committed file stays below 1 MiB: the masks are stored as bytes, and the weights of a fixture that would not fit go to part files
<name>__w1.npz, ... (tests/ar_ft_train_cases.load_case puts them together again)."""
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


def bound_d21():
    b = torch.tensor([2.0 + 0.1 * i for i in range(21)], dtype=torch.float32)
    b[[0, 3, 4, 9, 20]] = float(np.pi)
    return b


CASES = (
    ("grad_circ_ar_perm_d21_h40", lambda: nf.flows.CircularAutoregressiveRationalQuadraticSpline(
        21, 2, 40, ind_circ=[0, 3, 4, 9, 20], num_bins=8, tail_bound=bound_d21(), permute_mask=True, init_identity=False),
     21, 25, 70, 4101, 0.2, "bound"),
    ("grad_circ_ar_perm_d40_h260", lambda: nf.flows.CircularAutoregressiveRationalQuadraticSpline(
        40, 1, 260, ind_circ=[1, 2, 17, 39], num_bins=5, tail_bound=3.0, permute_mask=True, init_identity=False),
     40, 16, 130, 4102, 0.08, "bound"),
    ("grad_ar_perm_lin_d12_h24", lambda: nf.flows.AutoregressiveRationalQuadraticSpline(
        12, 2, 24, num_bins=8, tail_bound=3.0, permute_mask=True, init_identity=False),
     12, 23, 70, 4103, 0.2, "randn"),
)


def build(make, seed, sigma, dt):
    torch.manual_seed(seed)
    layer = make()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for p in layer.parameters():
            p.add_(sigma * torch.randn(p.shape, generator=g, dtype=p.dtype))
    return layer.to(dt)


def scale_err(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max()) / max(1.0, float(b.abs().max()))


def main():
    for name, make, D, mult, B, seed, sigma, rule in CASES:
        out, full = {}, {}
        for dt, leg in ((torch.float32, "f32"), (torch.float64, "f64")):
            layer = build(make, seed, sigma, dt)
            deg = layer.mprqat.autoregressive_net.final_layer.degrees[::mult]
            assert not torch.equal(deg, torch.arange(1, D + 1)), "the seed must give a non-identity degree permutation"
            g = torch.Generator().manual_seed(seed + 2)
            if rule == "bound":
                tb = layer.mprqat.tail_bound
                tb = tb.float() if torch.is_tensor(tb) else torch.full((D,), float(tb))
                x = (2 * torch.rand(B, D, generator=g) - 1) * tb * 0.98
            else:
                x = 1.3 * torch.randn(B, D, generator=g)
            cz = torch.randn(B, D, generator=g)
            cl = torch.randn(B, generator=g)
            xx = x.to(dt).clone().requires_grad_(True)
            z, ld = layer.inverse(xx)
            ((z * cz.to(dt)).sum() + (ld * cl.to(dt)).sum()).backward()
            out.update({"z_" + leg: z.detach(), "ld_" + leg: ld.detach(), "gx_" + leg: xx.grad})
            for k, p_ in layer.named_parameters():
                gflat = p_.grad.reshape(-1)
                key = k.replace(".", "__")
                out["g_%s__%s" % (leg, key)] = gflat[::STRIDE].clone()
                out["chk_%s__%s" % (leg, key)] = torch.tensor([float(gflat.double().sum()), float(gflat.double().abs().sum())],
                                                              dtype=torch.float64)
                full["%s__%s" % (leg, key)] = gflat.detach().clone()
            if dt == torch.float32:
                out.update(x=x, cz=cz, cl=cl)
                sd = layer.state_dict()
                if rule == "randn":
                    assert int((x.abs() > 3.0).sum()) > 0, "some entries must lie beyond the bound"
        worst = max(scale_err(out[k], out[k.replace("_f32", "_f64")]) for k in list(out) if "_f32" in k and not k.startswith("chk_"))
        worst = max([worst] + [scale_err(full[k], full[k.replace("f32__", "f64__")]) for k in full if k.startswith("f32__")])
        print("%s: degrees %s..., worst float32-vs-float64 %.2e of scale" % (name, deg[:6].tolist(), worst))
        assert worst <= 1e-4, "a row sits on a ReLU or bin kink: change the seed"
        arrays = {k: v.detach().cpu().numpy() for k, v in out.items()}
        arrays["stride"] = np.array(STRIDE)
        parts, weights = [], []
        for k, v in sd.items():
            a = v.detach().cpu().numpy()
            key = "sd__" + k.replace(".", "__")
            if k.endswith(".mask"):
                assert set(np.unique(a).tolist()) <= {0.0, 1.0}
                arrays[key] = a.astype(np.uint8)                      # (bytes: they compress to nothing; load_state_dict casts back)
            elif a.nbytes > 64 * 1024:
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
