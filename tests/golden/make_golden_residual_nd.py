#!/usr/bin/env python3
"""Generates the d-dimensional Residual-flow fixtures (flows/residual.py:118-228, :355-365, nets/lipschitz.py) by running the REAL
reference (normflows 1.7.3, PyTorch CPU), like the other make_golden_*.py:

    python tests/golden/make_golden_residual_nd.py <path of the reference checkout>

Per stack of tests/residual_nd_cases.py one file residual_nd_<case>.npz with
  * seed, sd__*: the state dict the results belong to (residual_cases.at_the_cap's recipe), buffers u, v, scale included, and x;
  * per Residual layer in draw (= execution) order after np.random.seed(seed); torch.manual_seed(seed): n (the drawn truncation
    samples, one row per layer), terms (max(n) + 20), coef (layers, max terms; coef[i, k - 1] = coeff_fn(k), zero-padded) and vareps
    (layers, rows, d): what the reference's sample function returned and what it handed to basic_logdet_estimator;
  * z, ld_layers (layers in execution order, rows), ld (their sum) and, where the density direction is the model's inverse,
    log_prob; as float32 legs and float64 legs (`*_f64`).  The float64 leg runs on the float32 leg's draws (the recorded vareps cast
    to float64), so the two legs differ by rounding alone;
  * ld_floor: the largest |ld_f32 - ld_f64| over ld_layers and ld, the reference's own float32 error on the case;
  * SAMPLING cases: iters, the further fixed-point steps of every Residual layer in execution order (residual.py:135-141's i).
For every layer of a SAMPLING case the generator asserts that the largest squared-step ratio (x - x_prev)^2 / (atol + |y| rtol) is
below 0.5 at the stopping iteration and above 2 at the one before, and moves to the next seed until both hold: two correct float32
evaluations then stop at the same iteration."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.abspath(sys.argv[1]))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import normflows as nf  # noqa: E402
import normflows.flows.residual as ref_residual  # noqa: E402
import residual_nd_cases as cases  # noqa: E402
from make_golden_residual import LIMIT, sd, step_ratios  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
torch.set_num_threads(4)


class Recorder:
    """Records, and on replay substitutes, what the reference draws: wraps the module-level sample functions and
    basic_logdet_estimator of normflows.flows.residual."""

    def __init__(self):
        self.n, self.terms, self.coef, self.vareps = [], [], [], []
        self.replay = None
        self._saved = {}

    def __enter__(self):
        for name in ("geometric_sample", "poisson_sample", "basic_logdet_estimator"):
            self._saved[name] = getattr(ref_residual, name)

        def sample(fn):
            def wrapped(p, n_samples):
                n = fn(p, n_samples)
                self.n.append(np.asarray(n))
                return n
            return wrapped

        def estimator(g, x, n_power_series, vareps, coeff_fn, training):
            if self.replay is not None:
                vareps = self.replay.pop(0).to(vareps)
            self.terms.append(int(n_power_series))
            self.coef.append([float(coeff_fn(k)) for k in range(1, int(n_power_series) + 1)])
            self.vareps.append(vareps.detach().clone())
            return self._saved["basic_logdet_estimator"](g, x, n_power_series, vareps, coeff_fn, training)

        ref_residual.geometric_sample = sample(self._saved["geometric_sample"])
        ref_residual.poisson_sample = sample(self._saved["poisson_sample"])
        ref_residual.basic_logdet_estimator = estimator
        return self

    def __exit__(self, *exc):
        for name, fn in self._saved.items():
            setattr(ref_residual, name, fn)


def stack_case(name, sampling):
    channels, _, _, rows, _ = cases.STACKS[name]
    d = channels[0]
    seed = cases.SEEDS[name]
    while True:
        m = cases.stack(nf, name, seed=seed)
        g = torch.Generator().manual_seed(seed + 1)
        cases.at_the_cap(nf, m, g)
        x = torch.randn(rows, d, generator=g) * 1.5
        out = {"seed": seed, "x": x}
        out.update(sd("sd__", m))
        density_inverse = cases.density_is_inverse(name)
        inverse = density_inverse != sampling          # the pass of the model that is this case's direction
        ok = True
        first = None
        for dt, leg in ((torch.float32, ""), (torch.float64, "_f64")):
            m.to(dt)
            xx = x.to(dt)
            with Recorder() as rec:
                if first is not None:
                    rec.replay = [v.clone() for v in first.vareps]
                np.random.seed(seed)
                torch.manual_seed(seed)
                iters, lds, cur = [], [], xx
                for f in (reversed(m.flows) if inverse else m.flows):
                    if sampling and isinstance(f, nf.flows.Residual):
                        r = step_ratios(f.iresblock, cur)
                        iters.append(len(r) - 1)
                        if leg == "" and not (len(r) >= 2 and r[-1] < 0.5 and r[-2] > 2):
                            ok = False
                        if leg == "":
                            print("  %s: layer stops after %d further steps, ratios %.3g / %.3g"
                                  % (name, len(r) - 1, r[-1], r[-2] if len(r) > 1 else float("nan")))
                    with torch.no_grad():
                        cur, l = f.inverse(cur) if inverse else f(cur)
                    lds.append(l.detach() * torch.ones(rows, dtype=dt))
                    cur = cur.detach()
                out["z" + leg], out["ld_layers" + leg] = cur, torch.stack(lds)
                out["ld" + leg] = torch.stack(lds).sum(0)
                if sampling:
                    out["iters" + leg] = np.asarray(iters)
                elif density_inverse:
                    if first is not None:
                        rec.replay = [v.clone() for v in first.vareps]
                    np.random.seed(seed)
                    torch.manual_seed(seed)
                    with torch.no_grad():
                        out["log_prob" + leg] = m.log_prob(xx).detach()
                else:
                    out["log_prob" + leg] = torch.zeros(0)
            if first is None:
                first = rec
                nres = len(rec.terms) // (1 if sampling or not density_inverse else 2)
                width = max(rec.terms[:nres])
                out["n"] = np.stack(rec.n[:nres])
                out["terms"] = np.asarray(rec.terms[:nres])
                out["coef"] = np.asarray([c + [0.0] * (width - len(c)) for c in rec.coef[:nres]], dtype=np.float64)
                out["vareps"] = torch.stack(rec.vareps[:nres])
            else:
                assert rec.terms == first.terms and all(np.array_equal(a, b) for a, b in zip(rec.n, first.n)), "the legs drew differently"
        m.to(torch.float32)
        if ok:
            break
        print("%s: seed %d leaves a layer too close to the stop threshold: next seed" % (name, seed))
        seed += 1
    floor = max(float((out["ld_layers"].double() - out["ld_layers_f64"]).abs().max()),
                float((out["ld"].double() - out["ld_f64"]).abs().max()))
    out["ld_floor"] = np.float64(floor)
    print("%s: seed %d, terms %s, |log det| max %.3f, ld_floor %.2e" % (name, seed, out["terms"].tolist(), float(out["ld_f64"].abs().max()), floor))
    arrays = {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in out.items()}
    assert sum(a.nbytes for a in arrays.values()) <= LIMIT, name
    path = os.path.join(OUT, "residual_nd_%s.npz" % name)
    np.savez_compressed(path, **arrays)
    print("wrote %s %.1f KB" % (os.path.basename(path), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    for name in cases.DENSITY:
        stack_case(name, False)
    for name in cases.SAMPLING:
        stack_case(name, True)
