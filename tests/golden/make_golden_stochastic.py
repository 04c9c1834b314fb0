#!/usr/bin/env python3
"""Generates the stochastic-layer fixtures (flows/stochastic.py, distributions/mh_proposal.py, distributions/linear_interpolation.py,
sampling/hais.py) by running the REAL reference (normflows 1.7.3, PyTorch CPU) under autograd, like the other make_golden_*.py:

    python tests/golden/make_golden_stochastic.py <path of the reference checkout>

Per case of tests/stochastic_cases.py one file stochastic_<case>.npz with
  * z, cz, c: the input and the cotangents of z_out and log_det; seed: the layer runs under torch.manual_seed(seed);
  * per leg (float32: no suffix; float64: `_f64`): eps, u = the random numbers the layer drew (replayed in its order), z_out,
    log_det, accept (hmc: (rows); mh: (steps, rows)), margin = |log u - log prob| per row in float64, gz = d loss / d z and, for hmc,
    g__log_step_size, g__log_mass with loss = sum(z_out * cz) + sum(log_det * c);
  * sd__*: the layer's state dict (float32).
stochastic_hais.npz: betas, step_size, log_mass, num_leapfrog, seed, and per leg prior_eps, eps (layers, rows, 2), u (layers, rows),
margin (layers, rows), samples, log_weights of HAIS(...).sample(rows) from a DiagGaussian(2) prior to TwoModes(2, 0.1).

The generator asserts that every value is finite, that the replayed decisions are the reference's, and that every row of every case
has a margin of at least stochastic_cases.MIN_MARGIN: no decision can then flip between CPUs."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.abspath(sys.argv[1]))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import normflows as nf  # noqa: E402
import stochastic_cases as cases  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
torch.set_num_threads(4)
SEED0 = 9100


class NS:
    """The reference's classes by name, wherever it defines them."""

    def __getattr__(self, name):
        for mod in (nf.flows.stochastic, nf.distributions.mh_proposal, nf.distributions.linear_interpolation, nf.distributions.target,
                    nf.distributions.prior, nf.distributions.base):
            if hasattr(mod, name):
                return getattr(mod, name)
        raise AttributeError(name)


def save(name, out):
    path = os.path.join(OUT, "stochastic_%s.npz" % name)
    np.savez_compressed(path, **{k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in out.items()})
    print("wrote %s %.1f KB" % (os.path.basename(path), os.path.getsize(path) / 1024))


def finite(out):
    for k, v in out.items():
        if torch.is_tensor(v) and v.dtype.is_floating_point and not k.startswith("margin"):
            assert torch.isfinite(v).all(), k


def layer_margins(name, layer, z, eps, u):
    c = cases.CASES[name]
    if c["layer"] == "hmc":
        return cases.margins("hmc", layer.target, z, eps, u, c["steps"], lss=layer.log_step_size.detach(), lm=layer.log_mass.detach(),
                             clip=c["clip"])
    return cases.margins("mh", layer.target, z, eps, u, c["steps"], scale=layer.proposal.scale.detach().double())


def case(i, name, seed):
    c = cases.CASES[name]
    z, cz, cc = cases.rows(name, 9000 + i)
    out = {"z": z, "cz": cz, "c": cc, "seed": seed}
    for dt, leg in ((torch.float32, ""), (torch.float64, "_f64")):
        layer = cases.build_layer(NS(), name, dt)
        zz = z.to(dt).clone().requires_grad_(True)
        torch.manual_seed(seed)
        z_out, log_det = layer(zz)
        ((z_out * cz.to(dt)).sum() + (log_det * cc.to(dt)).sum()).backward()
        eps, u = cases.draw(name, seed, dt)
        margin, accept = layer_margins(name, layer, z.to(dt), eps, u)
        if c["layer"] == "hmc":     # the replayed decisions are the reference's
            assert torch.equal(accept, (z_out.detach() != zz.detach()).any(1)), (name, leg)
        out.update({"eps" + leg: eps, "u" + leg: u, "z_out" + leg: z_out.detach(), "log_det" + leg: log_det.detach(),
                    "accept" + leg: accept, "margin" + leg: margin, "gz" + leg: zz.grad.clone()})
        if c["layer"] == "hmc":
            out.update({"g__log_step_size" + leg: layer.log_step_size.grad.clone(), "g__log_mass" + leg: layer.log_mass.grad.clone()})
    layer = cases.build_layer(NS(), name, torch.float32)
    out.update({"sd__" + k.replace(".", "__"): v.clone() for k, v in layer.state_dict().items()})
    finite(out)
    worst = min(float(out["margin"].min()), float(out["margin_f64"].min()))
    print("%s seed %d: accepted %.2f / %.2f, min margin %.2e, f32 vs f64 z_out %.2e" % (
        name, seed, float(out["accept"].double().mean()), float(out["accept_f64"].double().mean()), worst,
        float((out["z_out"].double() - out["z_out_f64"]).abs().max())))
    return out, worst


def hais(seed):
    n = cases.HAIS_ROWS
    out = {"betas": torch.tensor(cases.HAIS_BETAS), "step_size": torch.tensor([0.08, 0.06]), "log_mass": torch.tensor(cases.LM),
           "num_leapfrog": 3, "seed": seed}
    for dt, leg in ((torch.float32, ""), (torch.float64, "_f64")):
        prior = cases.set_gauss(nf.distributions.DiagGaussian(2, trainable=False).to(dt), dt)
        target = nf.distributions.TwoModes(2.0, 0.1)
        h = nf.HAIS(out["betas"].to(dt), prior, target, out["num_leapfrog"], out["step_size"].to(dt), out["log_mass"].to(dt))
        torch.manual_seed(seed)
        samples, log_weights = h.sample(n)
        # the same chain layer by layer, replaying each layer's draws for the margins
        torch.manual_seed(seed)
        prior_eps = torch.randn(n, 2, dtype=dt)
        torch.manual_seed(seed)
        s, _ = prior.forward(n)
        eps_all, u_all, margins = [], [], []
        for layer in h.layers:
            before = torch.get_rng_state()
            s2, _ = layer.forward(s)
            after = torch.get_rng_state()
            torch.set_rng_state(before)
            eps, u = torch.randn(n, 2, dtype=dt), torch.rand(n, dtype=dt)
            assert torch.equal(torch.get_rng_state(), after)
            m, acc = cases.margins("hmc", layer.target, s.detach(), eps, u, layer.steps, lss=layer.log_step_size.detach(),
                                   lm=layer.log_mass.detach())
            assert torch.equal(acc, (s2.detach() != s.detach()).any(1))
            eps_all.append(eps), u_all.append(u), margins.append(m)
            s = s2.detach()
        assert torch.equal(s, samples.detach())
        out.update({"prior_eps" + leg: prior_eps, "eps" + leg: torch.stack(eps_all), "u" + leg: torch.stack(u_all),
                    "margin" + leg: torch.stack(margins), "samples" + leg: samples.detach(), "log_weights" + leg: log_weights.detach()})
    finite(out)
    worst = min(float(out["margin"].min()), float(out["margin_f64"].min()))
    print("hais seed %d: min margin %.2e" % (seed, worst))
    return out, worst


def first_seed(make, start):
    """The first seed from `start` on whose every row has the margin (the seeds are chosen, then fixed in the fixture)."""
    for seed in range(start, start + 200):
        out, worst = make(seed)
        if worst >= cases.MIN_MARGIN:
            return out
    raise AssertionError("no seed with every margin >= %g" % cases.MIN_MARGIN)


if __name__ == "__main__":
    for i, name in enumerate(cases.CASES):
        save(name, first_seed(lambda seed: case(i, name, seed), SEED0 + 1000 * i))
    save("hais", first_seed(hais, SEED0 + 50000))
