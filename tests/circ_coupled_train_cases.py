"""Shared by tests/test_host_circ_coupled_train.py and tests/test_gpu_circ_coupled_train.py: the three reference training fixtures of
tests/golden/make_golden_circ_coupled_train.py (a fixture whose weights would pass 1 MiB is stored in parts) and the layers they
belong to."""
import glob
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# name -> the directions the fixture holds (inv = layer.inverse: density; fwd = layer.forward: sampling)
FIXTURES = {"grad_circ_cpl_d7_h40": ("inv", "fwd"), "grad_circ_cpl_d21_h260": ("inv",), "grad_circ_cpl_d6_k5": ("inv",)}


def load_case(name):
    g = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    for part in sorted(glob.glob(os.path.join(GOLDEN, name + "__w*.npz"))):
        g.update(np.load(part))
    return g


def make_layer(nfa, name, g):
    """The project's layer of fixture `name` with the reference's state."""
    C = nfa.flows.CircularCoupledRationalQuadraticSpline
    if name == "grad_circ_cpl_d7_h40":
        tb = torch.zeros(7)
        tb[torch.from_numpy(g["sd__prqct__transform_features"])] = torch.from_numpy(g["sd__prqct__tail_bound"])
        tb[torch.from_numpy(g["sd__prqct__identity_features"])] = torch.from_numpy(g["sd__prqct__unconditional_transform__tail_bound"])
        layer = C(7, 2, 40, ind_circ=[0, 2, 3, 6], num_bins=8, tail_bound=tb, init_identity=False)
    elif name == "grad_circ_cpl_d21_h260":
        layer = C(21, 1, 260, ind_circ=[1, 2, 8, 17, 20], num_bins=8, tail_bound=float(np.pi), reverse_mask=True, init_identity=False)
    else:
        layer = C(6, 2, 24, ind_circ=[1, 3, 4], num_bins=5, tail_bound=2.5, init_identity=False)
    sd = {k[4:].replace("__", "."): torch.from_numpy(np.asarray(v)) for k, v in g.items() if k.startswith("sd__")}
    layer.load_state_dict(sd, strict=True)
    return layer
