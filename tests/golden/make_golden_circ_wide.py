#!/usr/bin/env python3
"""Generates the fixtures of the one-launch CIRCULAR NSF coupling layer (tests/golden/circ_wide_*.npz, uniform_gaussian.npz,
circ_model_nsf.npz) by running the REAL reference (normflows 1.7.3, PyTorch CPU), as make_golden.py does for the other layers.  Run
where the reference is importable (NF_REFERENCE_DIR names its checkout when it is not installed); the GPU box has no reference:
    python tests/golden/make_golden_circ_wide.py

circ_wide_{a..g}: CircularCoupledRationalQuadraticSpline (wrapper.py:88-185), K = 8 (f: 4 bins, g: 16 bins -- four features / one
feature per lane-half of the kernel's final layer instead of two), default init with init_identity=False plus an
N(0, 0.3^2) perturbation of the final layer (the splines are not the identity).  Each file holds the float32 state dict, the inputs
(uniform inside every feature's interval; rows 0-3 carry one coordinate each 0.5 OUTSIDE its interval: list tails give output 0 and
log-det 0 there, utils/splines.py:31-32, 48-57; `outside` lists the (row, column) pairs), and outputs / log-dets of both directions
in float32 and float64 (the same float32 parameter values evaluated in float64: the reference's own float32 error).  No coordinate lies within 1e-3 of +-bound (the output
jumps there); the spline is C1 at the interior knots, so nothing else is excluded.  Layer (c)'s state dict lives in
circ_wide_c_state.npz (a committed file stays below 1 MiB).
uniform_gaussian: UniformGaussian (distributions/base.py:198-270) state dict shapes, points and their log_prob.
circ_model_nsf: NormalizingFlow(UniformGaussian(6, [1, 3, 4], scale), 3 x [circular coupling of shape (a) with alternating
reverse_mask, PeriodicShift]): state dict, points drawn from the model and their log_prob."""
import os
import sys

import numpy as np
import torch

if os.environ.get("NF_REFERENCE_DIR"):
    sys.path.insert(0, os.environ["NF_REFERENCE_DIR"])
import normflows as nf  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
torch.set_num_threads(4)

K = 8
TB_A = [3.0, np.pi, 2.0, np.pi, 3.5, 1.5]
# name: (D, blocks, hidden, ind_circ, tail_bound, reverse_mask, rows, seed)
LAYERS = {
    "a": (6, 1, 32, [1, 3, 4], TB_A, False, 70, 101),
    "b": (6, 1, 32, [1, 3, 4], TB_A, True, 70, 102),
    "c": (66, 2, 160, list(range(0, 66, 3)), 3.0, False, 130, 103),
    "d": (16, 2, 64, [], 3.0, False, 40, 104),
    "e": (16, 2, 64, list(range(16)), float(np.pi), False, 40, 105),
    "f": (22, 1, 48, list(range(0, 22, 3)), 2.5, False, 40, 106),
    "g": (22, 1, 48, list(range(0, 22, 3)), 2.5, True, 40, 107),
}
BINS = {"f": 4, "g": 16}      # the others: K


def bound_of(tb):
    return torch.tensor(tb, dtype=torch.float32) if isinstance(tb, list) else tb


def build(name):
    D, NB, H, ind_circ, tb, rev, rows, seed = LAYERS[name]
    torch.manual_seed(seed)
    layer = nf.flows.CircularCoupledRationalQuadraticSpline(D, NB, H, ind_circ=ind_circ, num_bins=BINS.get(name, K),
                                                            tail_bound=bound_of(tb), reverse_mask=rev, init_identity=False)
    g = torch.Generator().manual_seed(seed + 1000)
    fin = layer.prqct.transform_net.final_layer
    with torch.no_grad():
        for p in (fin.weight, fin.bias):
            p.add_(0.3 * torch.randn(p.shape, generator=g, dtype=p.dtype))
    return layer


def outside_coordinates(name):
    """Four (row, column) pairs: an identity and a transform coordinate of either tails type where the layer has them."""
    D, _, _, ind_circ, _, rev, _, _ = LAYERS[name]
    ident = [c for c in range(D) if (c % 2 == 0) != rev]      # create_alternating_binary_mask: mask 0 = identity
    trans = [c for c in range(D) if c not in ident]
    picks = []
    for half in (ident, trans):
        lin = [c for c in half if c not in ind_circ]
        circ = [c for c in half if c in ind_circ]
        picks.append((lin or circ)[-1])
        picks.append((circ or lin)[0])
    return [(r, c) for r, c in enumerate(picks)]


def inputs(name):
    D, _, _, _, tb, _, rows, seed = LAYERS[name]
    bound = bound_of(tb) if isinstance(tb, list) else torch.full((D,), tb)
    g = torch.Generator().manual_seed(seed + 2000)
    x = (torch.rand(rows, D, generator=g) * 2 - 1) * bound * 0.995
    out = outside_coordinates(name)
    for i, (r, c) in enumerate(out):
        x[r, c] = (bound[c] + 0.5) * (1.0 if i % 2 == 0 else -1.0)
    assert float(((x.abs() - bound).abs()).min()) > 1e-3, "a coordinate within 1e-3 of its bound"
    return x, np.array(out, dtype=np.int64)


def save(name, out):
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **{k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in out.items()})
    print("wrote %s %.1f KB" % (os.path.basename(path), os.path.getsize(path) / 1024))


def sd(module):
    return {"sd__" + k.replace(".", "__"): v for k, v in module.state_dict().items()}


def layer_fixture(name):
    layer = build(name)
    mask = layer.prqct.identity_features
    assert torch.equal(mask, torch.arange(1 if LAYERS[name][5] else 0, LAYERS[name][0], 2)), "identity features = mask 0 entries"
    x, out = inputs(name)
    with torch.no_grad():
        zf, ldf = layer.forward(x)                    # sampling direction (prqct.inverse)
        zi, ldi = layer.inverse(x)                    # density direction (prqct.forward)
        l64 = build(name).double()
        zf64, ldf64 = l64.forward(x.double())
        zi64, ldi64 = l64.inverse(x.double())
    for r, c in out:
        assert float(zf[r, c]) == 0.0 and float(zi[r, c]) == 0.0
    print("%s: float32 vs float64  sampling x %.2e ld %.2e   density x %.2e ld %.2e" % (
        name, float((zf.double() - zf64).abs().max()), float((ldf.double() - ldf64).abs().max()),
        float((zi.double() - zi64).abs().max()), float((ldi.double() - ldi64).abs().max())))
    res = dict(x=x, outside=out, z_fwd=zf, ld_fwd=ldf, z_inv=zi, ld_inv=ldi, z_fwd_f64=zf64, ld_fwd_f64=ldf64, z_inv_f64=zi64,
               ld_inv_f64=ldi64)
    if LAYERS[name][0] * LAYERS[name][2] > 4096:      # (c): weights and vectors in two files, each within the size limit of a committed file
        save("circ_wide_" + name + "_state", sd(layer))
    else:
        res.update(sd(layer))
    save("circ_wide_" + name, res)


MODEL_SCALE = [0.5, 2 * np.pi, 0.5, 2 * np.pi, 7.0, 0.4]      # uniform width = 2 bound on the circular entries, Gaussian std elsewhere


def model():
    torch.manual_seed(111)
    tb = bound_of(TB_A)
    flows = []
    for i in range(3):
        flows.append(nf.flows.CircularCoupledRationalQuadraticSpline(6, 1, 32, ind_circ=[1, 3, 4], num_bins=K, tail_bound=tb,
                                                                     reverse_mask=bool(i % 2), init_identity=False))
        flows.append(nf.flows.PeriodicShift([1, 3, 4], bound=tb[[1, 3, 4]], shift=torch.tensor([0.7, -1.1, 2.0])))
    g = torch.Generator().manual_seed(112)
    with torch.no_grad():
        for f in flows[::2]:
            fin = f.prqct.transform_net.final_layer
            for p in (fin.weight, fin.bias):
                p.add_(0.3 * torch.randn(p.shape, generator=g, dtype=p.dtype))
    q0 = nf.distributions.UniformGaussian(6, [1, 3, 4], torch.tensor(MODEL_SCALE, dtype=torch.float32))
    return nf.NormalizingFlow(q0, flows)


def main():
    only = sys.argv[1:]                               # layer names: write those fixtures alone (seeds are per layer)
    for name in only or LAYERS:
        layer_fixture(name)
    if only:
        return
    q0 = nf.distributions.UniformGaussian(6, [1, 3, 4], torch.tensor(MODEL_SCALE, dtype=torch.float32))
    torch.manual_seed(113)
    z = q0.sample(33)
    res = dict(z=z, log_prob=q0.log_prob(z))
    res.update(sd(q0))
    save("uniform_gaussian", res)
    m = model()
    torch.manual_seed(114)
    with torch.no_grad():
        x, _ = m.sample(64)
        lp = m.log_prob(x)
        lp64 = model().double().log_prob(x.double())
    tb = bound_of(TB_A)
    print("model: rows with a coordinate outside its interval: %d   float32 vs float64 log_prob %.2e"
          % (int((x.abs() > tb).any(1).sum()), float((lp.double() - lp64).abs().max())))
    res = dict(x=x, log_prob=lp, log_prob_f64=lp64)
    res.update(sd(m))
    save("circ_model_nsf", res)


if __name__ == "__main__":
    main()
