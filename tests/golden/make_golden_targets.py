#!/usr/bin/env python3
"""Generates the target / prior / mixture fixtures (distributions/target.py, prior.py, base.py:573-659) by running the REAL
reference (normflows 1.7.3, PyTorch CPU) under autograd, like the other make_golden_*.py:

    python tests/golden/make_golden_targets.py <path of the reference checkout>

Per 2-D case of tests/target_cases.py one file targets_<case>.npz with
  * cls, args: the constructor; z (256, 2): the eight edge rows, then 2.5 * randn; c (256): the cotangent;
  * lp, gz = d sum(lp * c) / d z as float32 legs and float64 legs (`*_f64`);
  * sd__*: the state dict, for the modules;
  * for the cases of target_cases.SAMPLED: sample_seed and sample = sample(64) under torch.manual_seed(sample_seed).
Per mixture case targets_gmm_<case>.npz: loc0, scale0, weights0 (the constructor's arguments), sd__* (the state dict, float64 as
constructed), z (200, d), c, and lp, gz, g__loc, g__log_scale, g__weight_scores in both legs (the float32 leg on the module after
.float()), plus sample_seed, sample_z, sample_lp = forward(64) of the float64 module under torch.manual_seed(sample_seed).

The generator asserts that every value and gradient is finite in both precisions."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.abspath(sys.argv[1]))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import normflows as nf  # noqa: E402
import target_cases as cases  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
torch.set_num_threads(4)


class NS:
    """The reference's classes by name, wherever its __init__ exports them."""

    def __getattr__(self, name):
        for mod in (nf.distributions.target, nf.distributions.prior, nf.distributions.base):
            if hasattr(mod, name):
                return getattr(mod, name)
        raise AttributeError(name)


def save(name, out):
    path = os.path.join(OUT, "targets_%s.npz" % name)
    np.savez_compressed(path, **{k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in out.items()})
    print("wrote %s %.1f KB" % (os.path.basename(path), os.path.getsize(path) / 1024))


def finite(out):
    for k, v in out.items():
        if torch.is_tensor(v) and v.dtype.is_floating_point:
            assert torch.isfinite(v).all(), k


def case_2d(i, name):
    cls, args = cases.CASES_2D[name]
    z, c = cases.rows_2d(7100 + i)
    out = {"cls": cls, "args": np.asarray(args, dtype=np.float64), "z": z, "c": c}
    for dt, leg in ((torch.float32, ""), (torch.float64, "_f64")):
        p = cases.build_2d(NS(), name)
        if isinstance(p, torch.nn.Module):
            p = p.to(dt)
        zz = z.to(dt).clone().requires_grad_(True)
        lp = p.log_prob(zz)
        (lp * c.to(dt)).sum().backward()
        out.update({"lp" + leg: lp.detach(), "gz" + leg: zz.grad.clone()})
    p = cases.build_2d(NS(), name)
    if isinstance(p, torch.nn.Module):
        out.update({"sd__" + k.replace(".", "__"): v.clone() for k, v in p.state_dict().items()})
    if name in cases.SAMPLED:
        seed = 7300 + i
        torch.manual_seed(seed)
        out.update({"sample_seed": seed, "sample": p.sample(cases.N_SAMPLES)})
    finite(out)
    print("%s: max |lp| %.3e, f32 vs f64: lp %.2e (rel), gz %.2e of scale" % (
        name, float(out["lp_f64"].abs().max()),
        float(((out["lp"].double() - out["lp_f64"]).abs() / out["lp_f64"].abs().clamp(min=1)).max()),
        float((out["gz"].double() - out["gz_f64"]).abs().max() / out["gz_f64"].abs().max())))
    save(name, out)


def case_gmm(i, name):
    M, d = cases.GMM[name]
    loc, scale, weights = cases.gmm_args(name, 7500 + i)
    z, c = cases.rows_gmm(name, 7600 + i)
    out = {"loc0": loc, "scale0": scale, "weights0": weights, "z": z, "c": c}
    m = nf.distributions.GaussianMixture(M, d, loc=loc, scale=scale, weights=weights)
    out.update({"sd__" + k: v.clone() for k, v in m.state_dict().items()})
    for dt, leg in ((torch.float32, ""), (torch.float64, "_f64")):
        m = nf.distributions.GaussianMixture(M, d, loc=loc, scale=scale, weights=weights).to(dt)
        zz = z.to(dt).clone().requires_grad_(True)
        lp = m.log_prob(zz)
        (lp * c.to(dt)).sum().backward()
        out.update({"lp" + leg: lp.detach(), "gz" + leg: zz.grad.clone()})
        out.update({"g__%s%s" % (k, leg): p.grad.clone() for k, p in m.named_parameters()})
    m = nf.distributions.GaussianMixture(M, d, loc=loc, scale=scale, weights=weights)
    seed = 7700 + i
    torch.manual_seed(seed)
    with torch.no_grad():
        sz, slp = m(cases.N_SAMPLES)
    out.update({"sample_seed": seed, "sample_z": sz, "sample_lp": slp})
    finite(out)
    print("gmm_%s: max |lp| %.3e, f32 vs f64: lp %.2e (rel), loc %.2e, log_scale %.2e of scale" % (
        name, float(out["lp_f64"].abs().max()),
        float(((out["lp"].double() - out["lp_f64"]).abs() / out["lp_f64"].abs().clamp(min=1)).max()),
        float((out["g__loc"].double() - out["g__loc_f64"]).abs().max() / out["g__loc_f64"].abs().max()),
        float((out["g__log_scale"].double() - out["g__log_scale_f64"]).abs().max() / out["g__log_scale_f64"].abs().max())))
    save("gmm_" + name, out)


if __name__ == "__main__":
    for i, name in enumerate(cases.CASES_2D):
        case_2d(i, name)
    for i, name in enumerate(cases.GMM):
        case_gmm(i, name)
