#!/usr/bin/env python3
"""Generates the Residual-flow TRAINING fixtures by running the REAL reference (normflows 1.7.3, PyTorch CPU), like
make_golden_residual.py:

    python tests/golden/make_golden_residual_train.py <path of the reference checkout>

Per case of tests/residual_train_cases.py one file residual_train_<case>.npz with seed, sd__* (the state dict the results belong
to, buffers included), x, cz, cl and, as float32 legs and float64 legs (`*_f64`), under np.random.seed(seed) and
torch.manual_seed(seed) right before the call: z, ld, gx and g__<parameter> (parameters the loss does not reach are absent) for loss
= sum(z cz) + sum(ld cl) in the density direction, and the buffers last_n_samples / last_firmom / last_secmom afterwards.  The
stack case: loss = forward_kld(x) and the gradient of every parameter.  Where a file would pass LIMIT the float64
parameter-gradient legs are dropped (there is no sd0__ copy in these files)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.abspath(sys.argv[1]))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import normflows as nf  # noqa: E402
import residual_train_cases as tc  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
torch.set_num_threads(4)
LIMIT = 700 * 1024      # bytes of arrays per file: no fixture file comes near 1 MiB


def save(name, out):
    arrays = {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in out.items()}
    if sum(a.nbytes for a in arrays.values()) > LIMIT:
        arrays = {k: a for k, a in arrays.items() if not k.startswith("g_f64__")}
    assert sum(a.nbytes for a in arrays.values()) <= LIMIT, name
    path = os.path.join(OUT, "residual_train_%s.npz" % name)
    np.savez_compressed(path, **arrays)
    print("wrote %s %.1f KB" % (os.path.basename(path), os.path.getsize(path) / 1024))


def sd(m):
    return {"sd__" + k.replace(".", "__"): v.clone() for k, v in m.state_dict().items()}


def layer_case(name):
    seed = tc.SEEDS[name]
    m = tc.layer(nf, name, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    tc.prepare(nf, m, name, g)
    f = m.flows[0]
    out = {"seed": seed}
    out.update(sd(f))
    x = torch.randn(tc.ROWS, 2, generator=g) * 1.5
    cz, cl = torch.randn(x.shape, generator=g), torch.randn(x.shape[0], generator=g)
    out.update({"x": x, "cz": cz, "cl": cl})
    for dt, leg in ((torch.float32, ""), (torch.float64, "_f64")):
        f.to(dt)
        f.zero_grad(set_to_none=True)
        xx = x.to(dt).clone().requires_grad_(True)
        np.random.seed(seed)
        torch.manual_seed(seed)
        z, ld = tc.density(f, xx)
        ((z * cz.to(dt)).sum() + (ld * cl.to(dt)).sum()).backward()
        out.update({"z" + leg: z.detach(), "ld" + leg: ld.detach(), "gx" + leg: xx.grad.clone()})
        for k, p in f.named_parameters():
            if p.grad is not None:
                out["g%s__%s" % (leg, k.replace(".", "__"))] = p.grad.detach().clone()
        for b in ("last_n_samples", "last_firmom", "last_secmom"):
            out[b + leg] = getattr(f.iresblock, b).detach().clone()
    f.to(torch.float32)
    scales = [float(mod.scale) for mod in f.modules() if type(mod).__name__ == "InducedNormLinear"]
    print("%s: n = %s, |ld| max %.3f, sigma %s" % (name, out["last_n_samples"].tolist(), float(out["ld_f64"].abs().max()),
                                                   ["%.3f" % s for s in scales]))
    save(name, out)


def stack_case():
    name = tc.STACK
    seed = tc.SEEDS[name]
    m = tc.stack(nf, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    tc.prepare(nf, m, name, g)
    out = {"seed": seed}
    out.update(sd(m))
    x = torch.randn(tc.ROWS, 2, generator=g) * 1.5
    out["x"] = x
    for dt, leg in ((torch.float32, ""), (torch.float64, "_f64")):
        m.to(dt)
        m.zero_grad(set_to_none=True)
        np.random.seed(seed)
        torch.manual_seed(seed)
        loss = m.forward_kld(x.to(dt))
        loss.backward()
        out["loss" + leg] = loss.detach()
        for k, p in m.named_parameters():
            if p.grad is not None:
                out["g%s__%s" % (leg, k.replace(".", "__"))] = p.grad.detach().clone()
    m.to(torch.float32)
    print("%s: loss %.6f" % (name, float(out["loss_f64"])))
    save(name, out)


if __name__ == "__main__":
    for name in tc.LAYERS:
        layer_case(name)
    stack_case()
