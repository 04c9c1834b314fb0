"""The models of the d-dimensional Residual-flow fixtures (tests/golden/residual_nd_*.npz), built from whichever package is handed
in: the reference (tests/golden/make_golden_residual_nd.py) or normflows_amd (the tests) -- same constructors in the same order,
same state dict.  Evaluation mode, exact_trace off: the log-det is Hutchinson's power series with max(n) + 20 terms.

A case is (channels of the LipschitzMLP, number of Residual layers, ActNorm after every Residual?, rows, Residual keyword arguments).
DENSITY: the density direction (x -> x + g(x) in every Residual).  SAMPLING: the fixed-point direction."""
import os

import numpy as np
import torch

import residual_cases

GOLDEN = residual_cases.GOLDEN
LIPSCHITZ = residual_cases.LIPSCHITZ
ROWS = 24

DENSITY = {
    "d3_h16_k1": ([3, 16, 3], 1, False, ROWS, {}),                                    # the smallest d, odd, hp 32
    "d5_h40x24_k2": ([5, 40, 24, 5], 2, True, ROWS, {}),                              # hp 64, uneven widths, affine records
    "d17_h128x3_k1": ([17, 128, 128, 128, 17], 1, False, ROWS, {}),                   # three hidden layers, d % 4 != 0, d > 16
    "d64_h128x2_k1": ([64, 128, 128, 64], 1, False, ROWS, {}),                        # the largest d
    "d8_h32_k3_poisson": ([8, 32, 8], 3, False, ROWS, {"n_dist": "poisson", "n_samples": 3, "reverse": False}),
}
SAMPLING = {
    "sample_d3_h16_k1": ([3, 16, 3], 1, False, ROWS, {}),
    "sample_d8_h64_k2": ([8, 64, 8], 2, False, ROWS, {}),
}
STACKS = dict(DENSITY, **SAMPLING)
SEEDS = {name: 9900 + 10 * i for i, name in enumerate(STACKS)}

at_the_cap = residual_cases.at_the_cap
walk = residual_cases.walk


def dim(name):
    return STACKS[name][0][0]


def stack(nf, name, seed=None):
    """NormalizingFlow of stack `name` in evaluation mode; with `seed` the construction is seeded."""
    channels, n, actnorm, _, kw = STACKS[name]
    if seed is not None:
        torch.manual_seed(seed)
    flows = []
    for _ in range(n):
        net = nf.nets.LipschitzMLP(channels, init_zeros=False, lipschitz_const=LIPSCHITZ)
        flows.append(nf.flows.Residual(net, reduce_memory=True, **kw))
        if actnorm:
            flows.append(nf.flows.ActNorm(channels[0]))
    return nf.NormalizingFlow(nf.distributions.DiagGaussian(channels[0], trainable=False), flows).eval()


def density_is_inverse(name):
    return STACKS[name][4].get("reverse", True)


def load(name):
    return dict(np.load(os.path.join(GOLDEN, "residual_nd_%s.npz" % name)))


def draws(g):
    """[(terms, [coef(1) .. coef(terms)], vareps (B, d))] of a fixture's Residual layers in draw (= execution) order."""
    out = []
    for i, t in enumerate(g["terms"].tolist()):
        out.append((int(t), [float(c) for c in g["coef"][i, :t]], g["vareps"][i]))
    return out


def ld_bar(g, tol):
    """The log-det bar of a fixture: `tol` (conftest.ld_tol), with 4 x the fixture's recorded ld_floor -- the reference's own
    |float32 - float64| on the case -- as the absolute part where that floor exceeds a quarter of the bar's."""
    tol = dict(tol)
    floor = float(g["ld_floor"])
    if floor > tol["atol"] / 4:
        tol["atol"] = 4 * floor
    return tol
