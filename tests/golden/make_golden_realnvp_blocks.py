#!/usr/bin/env python3
"""Generates the training fixtures of AffineCouplingBlock(nets.MLP) + Permute stacks (affine/coupling.py:117-171, :232-267,
flows/reshape.py:30-34, 59-64, flows/mixing.py:32-54, nets/mlp.py:5-58) by running the REAL reference (normflows 1.7.3, PyTorch CPU)
under autograd, like make_golden_realnvp_train.py, with the same keys:

    python tests/golden/make_golden_realnvp_blocks.py <path of the reference checkout>

Per case of tests/realnvp_block_cases.py one file grad_realnvp_block_<case>.npz with
  * x, cz, cl and the state dict (`sd__*`: the shuffle permutations and data_dep_init_done included; an ActNorm is initialised by
    one no_grad pass first);
  * loss = sum(z * cz) + sum(log_det * cl) through NormalizingFlow.forward_and_log_det (`fwd`) and inverse_and_log_det (`inv`):
    z_<dir>, ld_<dir>, gx_<dir> and g_<dir>__<parameter>, as float32 legs and float64 legs (`*_f64`);
  * loss / g__<parameter>: forward_kld(x) and its gradients (float32), loss_f64.
Every parameter is perturbed AFTER the ActNorm initialisation (the init_zeros last layers included); the last linear of every MLP by
its own sigma, so that the scale parameters stay around |s| <= 2.

The generator asserts, in the float64 leg, that no hidden pre-activation of any row lies within 1e-4 of 0: a row on a LeakyReLU kink
makes a gradient comparison meaningless.  Change the seed if it fails."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.abspath(sys.argv[1]))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import normflows as nf  # noqa: E402
import realnvp_block_cases as cases  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
torch.set_num_threads(4)
SEEDS = {"readme_d2": 7201, "d5_maps": 7211, "d16": 7221, "d3_inv": 7230}
SIGMA = {"readme_d2": (0.5, 0.1), "d5_maps": (0.3, 0.08), "d16": (0.3, 0.08), "d3_inv": (0.5, 0.2)}   # (every parameter, an MLP's last linear)


def build(name, x, dt):
    torch.manual_seed(SEEDS[name])
    m = cases.model(nf, name)
    with torch.no_grad():
        m.inverse_and_log_det(x)            # ActNorm's data-dependent initialisation
    g = torch.Generator().manual_seed(SEEDS[name] + 1)
    last = set()
    for mod in m.modules():
        if isinstance(mod, nf.nets.MLP):
            lin = [l for l in mod.net if isinstance(l, torch.nn.Linear)][-1]
            last |= {id(lin.weight), id(lin.bias)}
    with torch.no_grad():
        for p in m.parameters():
            p.add_(SIGMA[name][1 if id(p) in last else 0] * torch.randn(p.shape, generator=g, dtype=p.dtype))
    return m.to(dt)


def main():
    for name, rows in cases.CASES.items():
        case(name, rows)


def case(name, rows):
    d = cases.build(nf, name)[1]
    g = torch.Generator().manual_seed(SEEDS[name] + 2)
    x = torch.randn(rows, d, generator=g) * 1.2
    cz, cl = torch.randn(rows, d, generator=g), torch.randn(rows, generator=g)
    out = {"x": x, "cz": cz, "cl": cl}
    for dt, leg in ((torch.float32, ""), (torch.float64, "_f64")):
        m = build(name, x, dt)
        pre = []
        hooks = [mod.register_forward_pre_hook(lambda _m, inp: pre.append(float(inp[0].detach().abs().min())))
                 for mod in m.modules() if isinstance(mod, torch.nn.LeakyReLU)]
        for dname, fn in (("fwd", m.forward_and_log_det), ("inv", m.inverse_and_log_det)):
            m.zero_grad(set_to_none=True)
            xx = x.to(dt).clone().requires_grad_(True)
            z, ld = fn(xx)
            ((z * cz.to(dt)).sum() + (ld * cl.to(dt)).sum()).backward()
            out.update({"z_%s%s" % (dname, leg): z.detach(), "ld_%s%s" % (dname, leg): ld.detach(),
                        "gx_%s%s" % (dname, leg): xx.grad.clone()})
            for k, p_ in m.named_parameters():
                out["g_%s%s__%s" % (dname, leg, k.replace(".", "__"))] = p_.grad.detach().clone()
        if dt == torch.float64:
            assert pre and min(pre) > 1e-4, "%s: a hidden pre-activation within 1e-4 of 0 (%.2e): change the seed" % (name, min(pre))
            print("%s: smallest |hidden pre-activation| %.3e, max |ld| %.2f, max |z| %.2f / %.2f"
                  % (name, min(pre), float(out["ld_fwd_f64"].abs().max()), float(out["z_fwd_f64"].abs().max()),
                     float(out["z_inv_f64"].abs().max())))
        for h in hooks:
            h.remove()
        m.zero_grad(set_to_none=True)
        loss = m.forward_kld(x.to(dt))
        loss.backward()
        if dt == torch.float32:
            out["loss"] = loss.detach()
            out.update({"g__" + k.replace(".", "__"): p_.grad.detach().clone() for k, p_ in m.named_parameters()})
            out.update({"sd__" + k.replace(".", "__"): v for k, v in m.state_dict().items()})
        else:
            out["loss_f64"] = loss.detach()
    path = os.path.join(OUT, "grad_realnvp_block_%s.npz" % name)
    np.savez_compressed(path, **{k: v.detach().cpu().numpy() for k, v in out.items()})
    print("wrote %s %.1f KB" % (os.path.basename(path), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
