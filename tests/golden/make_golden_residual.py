#!/usr/bin/env python3
"""Generates the Residual-flow fixtures (flows/residual.py:12-437, nets/lipschitz.py, utils/optim.py) by running the REAL reference
(normflows 1.7.3, PyTorch CPU), like the other make_golden_*.py:

    python tests/golden/make_golden_residual.py <path of the reference checkout>

Per stack of tests/residual_cases.py one file residual_<case>.npz with
  * seed and sd0__*: the state dict of the seeded construction (torch.manual_seed(seed), then the constructors in order);
  * sd__*: the state dict the results belong to (residual_cases.at_the_cap: weights and biases times 3, ActNorm perturbed, 50 power
    iterations), buffers u, v, scale included;
  * x, and as float32 legs and float64 legs (`*_f64`):
      CHAIN cases:    z, ld_layers (layers in execution order, rows), ld (their sum) in the density direction, and log_prob;
      SAMPLING cases: the same in the fixed-point direction, and iters: the further fixed-point steps of every Residual layer in
                      execution order (residual.py:135-141's i).
For every layer of a SAMPLING case the generator asserts that the largest squared-step ratio (x - x_prev)^2 / (atol + |y| rtol) is
below 0.5 at the stopping iteration and above 2 at the one before, and moves to the next seed until both hold: two correct float32
evaluations then stop at the same iteration.

residual_lipschitz.npz: one LipschitzMLP after update_lipschitz(net, 5) from the seeded state, after compute_weight by tolerance
(n_iterations None, atol = rtol = 1e-3, one layer), and compute_one_iter's value: u, v, scale of every layer.

Per ESTIMATORS case one file residual_est_<case>.npz: a single training-mode layer on a stochastic branch, np.random.seed(seed) and
torch.manual_seed(seed) right before the call: z, ld, gx and g__<parameter> (parameters the loss does not reach are absent) for loss
= sum(z cz) + sum(ld cl) in the density direction, the buffers last_n_samples / last_firmom / last_secmom afterwards; float32 and
`_f64` legs."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.abspath(sys.argv[1]))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import normflows as nf  # noqa: E402
import residual_cases as cases  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
torch.set_num_threads(4)


LIMIT = 700 * 1024      # bytes of arrays per file: no fixture file comes near 1 MiB


def save(name, out):
    """residual_<name>.npz; a state dict too large for one file (the 16-layer example model) is spread over residual_<name>_sd<i>.npz
    (tests/residual_cases.load merges them), and that case keeps no sd0__ copy."""
    arrays = {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in out.items()}
    files = {"": {}}
    if sum(a.nbytes for a in arrays.values()) > LIMIT:
        arrays = {k: a for k, a in arrays.items() if not k.startswith("sd0__")}
        part, size = 0, 0
        for k in [k for k in arrays if k.startswith("sd__")]:
            a = arrays.pop(k)
            if size + a.nbytes > LIMIT:
                part, size = part + 1, 0
            files.setdefault("_sd%d" % part, {})[k] = a
            size += a.nbytes
    files[""] = arrays
    for suffix, content in files.items():
        if content:
            path = os.path.join(OUT, "residual_%s%s.npz" % (name, suffix))
            np.savez_compressed(path, **content)
            print("wrote %s %.1f KB" % (os.path.basename(path), os.path.getsize(path) / 1024))


def sd(prefix, m):
    return {prefix + k.replace(".", "__"): v.clone() for k, v in m.state_dict().items()}


def step_ratios(block, y, atol=1e-5, rtol=1e-5):
    """Largest squared-step ratio after every update of the fixed-point iteration of `block` on y (index = residual.py's i)."""
    out = []
    with torch.no_grad():
        x, x_prev = y - block.nnet(y), y
        tol = atol + y.abs() * rtol
        while True:
            r = (x - x_prev) ** 2 / tol
            out.append(float(r.max()))
            if torch.all(r < 1) or len(out) > 1001:
                return out
            x, x_prev = y - block.nnet(x), x


def stack_case(name, sampling):
    rows = cases.STACKS[name][3]
    seed = cases.SEEDS[name]
    while True:
        m = cases.stack(nf, name, seed=seed)
        sd0 = sd("sd0__", m)
        g = torch.Generator().manual_seed(seed + 1)
        cases.at_the_cap(nf, m, g)
        x = torch.randn(rows, 2, generator=g) * 1.5
        out = {"seed": seed, "x": x}
        out.update(sd0)
        out.update(sd("sd__", m))
        density_inverse = cases.density_is_inverse(name)
        inverse = density_inverse != sampling          # the pass of the model that is this case's direction
        ok = True
        for dt, leg in ((torch.float32, ""), (torch.float64, "_f64")):
            m.to(dt)
            with torch.no_grad():
                xx = x.to(dt)
                if sampling:
                    iters, cur = [], xx
                    for f in (reversed(m.flows) if inverse else m.flows):
                        if isinstance(f, nf.flows.Residual):
                            r = step_ratios(f.iresblock, cur)
                            iters.append(len(r) - 1)
                            if leg == "" and not (len(r) >= 2 and r[-1] < 0.5 and r[-2] > 2):
                                ok = False
                            if leg == "":
                                print("  %s: layer stops after %d further steps, ratios %.3g / %.3g" % (name, len(r) - 1, r[-1], r[-2] if len(r) > 1 else float("nan")))
                        cur = (f.inverse(cur) if inverse else f(cur))[0].detach()
                    out["iters" + leg] = np.asarray(iters)
                z, lds = cases.walk(list(m.flows), xx, inverse)
                out["z" + leg], out["ld_layers" + leg] = z, torch.stack(lds)
                out["ld" + leg] = torch.stack(lds).sum(0)
                if not sampling:
                    # (the reference's log_prob keeps a float32 accumulator whatever the model's dtype)
                    out["log_prob" + leg] = m.log_prob(xx).detach() if density_inverse else torch.zeros(0)
        m.to(torch.float32)
        if ok:
            break
        print("%s: seed %d leaves a layer too close to the stop threshold: next seed" % (name, seed))
        seed += 1
    per_layer = out["ld_layers_f64"].abs()
    print("%s: seed %d, |log det| per Residual layer %.3f .. %.3f, f32 - f64 sum %.2e"
          % (name, seed, float(per_layer.max(1).values.min()), float(per_layer.max()), float((out["ld"].double() - out["ld_f64"]).abs().max())))
    save(name, out)


def lipschitz_case():
    seed = 9700
    torch.manual_seed(seed)
    net = nf.nets.LipschitzMLP([2, 40, 24, 2], init_zeros=True, lipschitz_const=cases.LIPSCHITZ)
    out = {"seed": seed}
    out.update(sd("sd0__", net))
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(3.0)
    nf.utils.update_lipschitz(net, 5)
    out.update(sd("after5__", net))
    out["one_iter"] = np.asarray([float(net.net[2 * i + 1].compute_one_iter()) for i in range(3)])
    with torch.no_grad():
        w = net.net[3].compute_weight(update=True, n_iterations=None, atol=1e-3, rtol=1e-3)
    out["tol_weight"] = w.detach().clone()
    out.update(sd("tol__", net))
    x = torch.randn(9, 2, generator=torch.Generator().manual_seed(seed + 1))
    out["x"] = x
    with torch.no_grad():
        out["y"] = net(x)
    out.update(sd("end__", net))        # (the forward pass wrote every layer's scale)
    save("lipschitz", out)


def estimator_case(name):
    d = cases.ESTIMATORS[name][0]
    seed = cases.EST_SEEDS[name]
    f = cases.estimator_layer(nf, name, seed=seed)
    out = {"seed": seed}
    out.update(sd("sd0__", f))
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for mod in f.modules():
            if isinstance(mod, nf.nets.InducedNormLinear):
                mod.weight.mul_(2.0)
    nf.utils.update_lipschitz(f, 50)
    out.update(sd("sd__", f))
    x = torch.randn(cases.EST_ROWS, d, generator=g)
    cz, cl = torch.randn(x.shape, generator=g), torch.randn(x.shape[0], generator=g)
    out.update({"x": x, "cz": cz, "cl": cl})
    for dt, leg in ((torch.float32, ""), (torch.float64, "_f64")):
        f.to(dt)
        f.zero_grad(set_to_none=True)
        xx = x.to(dt).clone().requires_grad_(True)
        np.random.seed(seed)
        torch.manual_seed(seed)
        z, ld = f.inverse(xx)
        ((z * cz.to(dt)).sum() + (ld * cl.to(dt)).sum()).backward()
        out.update({"z" + leg: z.detach(), "ld" + leg: ld.detach(), "gx" + leg: xx.grad.clone()})
        for k, p in f.named_parameters():
            if p.grad is not None:
                out["g%s__%s" % (leg, k.replace(".", "__"))] = p.grad.detach().clone()
        for b in ("last_n_samples", "last_firmom", "last_secmom"):
            out[b + leg] = getattr(f.iresblock, b).detach().clone()
    f.to(torch.float32)
    print("%s: n = %s, |ld| max %.3f" % (name, out["last_n_samples"].tolist(), float(out["ld_f64"].abs().max())))
    save("est_" + name, out)


if __name__ == "__main__":
    for name in cases.CHAIN:
        stack_case(name, False)
    for name in cases.SAMPLING:
        stack_case(name, True)
    lipschitz_case()
    for name in cases.ESTIMATORS:
        estimator_case(name)
