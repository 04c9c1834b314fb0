#!/usr/bin/env python3
"""Generates the Planar / Radial fixtures (flows/planar.py:8-81, flows/radial.py:8-46) by running the REAL reference (normflows
1.7.3, PyTorch CPU) under autograd, like the other make_golden_*.py:

    python tests/golden/make_golden_rank1.py <path of the reference checkout>

Per case of tests/rank1_cases.py one file rank1_<case>.npz with
  * seed and sd0__*: the state dict of the seeded construction (torch.manual_seed(seed), then the constructors in order);
  * sd__*: the state dict the results belong to: every parameter perturbed, p += 0.3 randn, except Radial's beta, which keeps its
    initialisation range so that the layers stay well away from singular;
  * x, cz, cl, and per direction (`fwd`; `inv` where every layer is leaky) for loss = sum(z * cz) + sum(log_det * cl):
    z_<dir>, ld_<dir>, gx_<dir>, g_<dir>__<parameter> as float32 legs and float64 legs (`*_f64`).
radial_d2_k8: row 0 of x is the first layer's z_0, so r = 0 there.

For every case with a leaky layer the generator asserts, in the float64 leg, min |lin| >= 1e-3 over all leaky layers, rows and
directions -- the derivative jumps at lin = 0, and a row on the kink would make two correct float32 evaluations disagree -- and
moves to the next seed until it holds.

rank1_planar_edges.npz: the two single layers of rank1_cases.edge_layers (parameters written in, not drawn), keys prefixed
`tanh__` / `leaky__` (leaky also with an inv leg).  The tanh layer's float32 leg holds what the reference computes there:
cosh(95) overflows, its sech^2 is 1 / inf = 0 and the derivative of that is 0 * inf = NaN, which the batch sums carry into every
parameter gradient; the float64 leg is finite."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.abspath(sys.argv[1]))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import normflows as nf  # noqa: E402
import rank1_cases as cases  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
torch.set_num_threads(4)


def min_abs_lin(flows, x, inverse):
    """Smallest |w . z + b| any leaky layer sees on the way of x through `flows` (inf without one)."""
    lo = float("inf")
    with torch.no_grad():
        for f in (reversed(flows) if inverse else flows):
            if isinstance(f, nf.flows.Planar) and f.act == "leaky_relu":
                lin = torch.sum(f.w * x, list(range(1, f.w.dim()))) + f.b
                lo = min(lo, float(lin.abs().min()))
            x = (f.inverse(x) if inverse else f(x))[0]
    return lo


def legs(flows, x, cz, cl, dirs, out, prefix=""):
    for dt, leg in ((torch.float32, ""), (torch.float64, "_f64")):
        fl = torch.nn.ModuleList(flows).to(dt)
        for dname in dirs:
            fl.zero_grad(set_to_none=True)
            xx = x.to(dt).clone().requires_grad_(True)
            z, ld = cases.run(list(fl), xx, dname == "inv")
            ((z * cz.to(dt)).sum() + (ld * cl.to(dt)).sum()).backward()
            out.update({"%sz_%s%s" % (prefix, dname, leg): z.detach(), "%sld_%s%s" % (prefix, dname, leg): ld.detach(),
                        "%sgx_%s%s" % (prefix, dname, leg): xx.grad.clone()})
            for k, p_ in fl.named_parameters():
                out["%sg_%s%s__%s" % (prefix, dname, leg, k.replace(".", "__"))] = p_.grad.detach().clone()
    torch.nn.ModuleList(flows).to(torch.float32)


def save(name, out):
    path = os.path.join(OUT, "rank1_%s.npz" % name)
    np.savez_compressed(path, **{k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in out.items()})
    print("wrote %s %.1f KB" % (os.path.basename(path), os.path.getsize(path) / 1024))


def case(name):
    codes, shape, rows = cases.CASES[name]
    dirs = cases.directions(name)
    seed = cases.SEEDS[name]
    while True:
        m = cases.model(nf, name, seed=seed)
        sd0 = {k: v.clone() for k, v in m.state_dict().items()}
        g = torch.Generator().manual_seed(seed + 1)
        with torch.no_grad():
            for k, p in m.named_parameters():
                if not k.endswith(".beta"):
                    p.add_(0.3 * torch.randn(p.shape, generator=g))
        x = torch.randn((rows,) + tuple(shape), generator=g) * 1.2
        if name == "radial_d2_k8":
            x[0] = m.flows[0].z_0.detach()[0]
        cz, cl = torch.randn(x.shape, generator=g), torch.randn(rows, generator=g)
        flows64 = list(torch.nn.ModuleList(list(m.flows)).double())
        lo = min(min_abs_lin(flows64, x.double(), d == "inv") for d in dirs)
        torch.nn.ModuleList(list(m.flows)).float()
        if lo >= 1e-3:
            break
        print("%s: seed %d puts a row within %.2e of a leaky kink: next seed" % (name, seed, lo))
        seed += 1
    out = {"seed": seed, "x": x, "cz": cz, "cl": cl}
    out.update({"sd0__" + k.replace(".", "__"): v for k, v in sd0.items()})
    out.update({"sd__" + k.replace(".", "__"): v.clone() for k, v in m.state_dict().items()})
    legs(list(m.flows), x, cz, cl, dirs, out)
    print("%s: seed %d, min |lin| at a leaky layer %.3e, max |ld| %.2f" % (name, seed, lo, float(out["ld_fwd_f64"].abs().max())))
    save(name, out)


def edges():
    out = {}
    g = torch.Generator().manual_seed(9300)
    for key, (layer, x) in cases.edge_layers(nf).items():
        cz, cl = torch.randn(x.shape, generator=g), torch.randn(x.shape[0], generator=g)
        out.update({key + "__x": x, key + "__cz": cz, key + "__cl": cl})
        legs([layer], x, cz, cl, ("fwd", "inv") if key == "leaky" else ("fwd",), out, prefix=key + "__")
    save("planar_edges", out)


if __name__ == "__main__":
    for name in cases.CASES:
        case(name)
    edges()
