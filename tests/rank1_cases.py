"""The models of the Planar / Radial fixtures (tests/golden/rank1_*.npz), built from whichever package is handed in: the reference
(tests/golden/make_golden_rank1.py) or normflows_amd (the tests) -- same constructors in the same order, same state dict.

A case is (layer codes, shape, rows): P = Planar tanh, L = Planar leaky_relu, R = Radial.  `inv` legs exist where every layer is
leaky.  `planar_edges` is not in this table: single layers with written-in parameters (edge_layers)."""
import math

import torch

MIXED = "PRLRPR"
CASES = {
    "planar_tanh_d2_k16": ("P" * 16, (2,), 300),      # lane = row, ragged last tile
    "planar_leaky_d3_k4": ("L" * 4, (3,), 70),        # forward and inverse legs
    "radial_d2_k8": ("R" * 8, (2,), 300),             # row 0 = the first layer's z_0: r = 0
    "mixed_d16_k6": (MIXED, (16,), 70),               # the last lane = row size
    "mixed_d17_k6": (MIXED, (17,), 70),               # the first 16-lanes-per-row size, ragged group tail
    "planar_d40_k16": ("P" * 16, (40,), 70),          # the VAE latent
    "mixed_d128_k4": ("PRLR", (128,), 35),            # the maximum, 8 elements per lane
    "planar_shape_1x4x4": ("PP", (1, 4, 4), 70),      # z of shape (B, 1, 4, 4): the flattening
}
SEEDS = {name: 9100 + 10 * i for i, name in enumerate(CASES)}


def directions(name):
    return ("fwd", "inv") if set(CASES[name][0]) == {"L"} else ("fwd",)


def layers(nf, codes, shape):
    out = []
    for c in codes:
        out.append(nf.flows.Radial(shape) if c == "R" else nf.flows.Planar(shape, act="tanh" if c == "P" else "leaky_relu"))
    return out


def model(nf, name, seed=None):
    """NormalizingFlow of case `name`; with `seed` the construction is seeded (torch.manual_seed(seed), then the constructors in
    order)."""
    codes, shape, _ = CASES[name]
    if seed is not None:
        torch.manual_seed(seed)
    flows = layers(nf, codes, shape)
    return nf.NormalizingFlow(nf.distributions.DiagGaussian(math.prod(shape), trainable=False), flows)


def run(flows, x, inverse=False):
    """(z, summed log-det) of the layers' own methods in order, in the layers' precision (the reference's NormalizingFlow keeps a
    float32 accumulator whatever the dtype)."""
    ld = 0
    for f in (reversed(flows) if inverse else flows):
        x, l = f.inverse(x) if inverse else f(x)
        ld = ld + l
    return x, ld


# ---- planar_edges: single layers, parameters written in ---------------------------------------------------------------------------
EDGE_LIN = (0.0, 15.0, -15.0, 50.0, -50.0, 95.0, -95.0)


def edge_layers(nf, dtype=torch.float32):
    """{"tanh": (layer, x), "leaky": (layer, x)}.  tanh: w = (1, 0), b = 0, rows with lin = EDGE_LIN exactly: sech^2 underflows at
    |lin| = 50 and float32 cosh overflows at 95.  leaky: b = 0 and row 0 = 0, so lin == 0 exactly (the slope-1 side); the other rows
    have |lin| >= 0.25.  The values are float32 and cast afterwards: the float64 leg runs on the float32 parameters and inputs, like
    every other fixture."""
    u = torch.tensor([[0.5, -0.3]])
    tanh = nf.flows.Planar((2,), act="tanh", u=u.clone(), w=torch.tensor([[1.0, 0.0]]), b=torch.zeros(1))
    xt = torch.tensor([[v, 0.25 * i - 0.5] for i, v in enumerate(EDGE_LIN)])
    leaky = nf.flows.Planar((2,), act="leaky_relu", u=u.clone(), w=torch.tensor([[0.5, -1.0]]), b=torch.zeros(1))
    xl = torch.tensor([[0.0, 0.0], [0.5, 0.0], [0.0, 0.5], [-1.5, 0.25], [2.0, 0.5]])
    return {"tanh": (tanh.to(dtype), xt.to(dtype)), "leaky": (leaky.to(dtype), xl.to(dtype))}
