"""Shared by tests/test_host_arnsf_train_ft.py and tests/test_gpu_arnsf_train_ft.py: the three reference training fixtures of
tests/golden/make_golden_ar_ft_train.py (a fixture whose weights would pass 1 MiB is stored in parts) and the layers they belong to."""
import glob
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ("grad_circ_ar_perm_d21_h40", "grad_circ_ar_perm_d40_h260", "grad_ar_perm_lin_d12_h24")


def load_case(name):
    g = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    for part in sorted(glob.glob(os.path.join(GOLDEN, name + "__w*.npz"))):
        g.update(np.load(part))
    return g


def make_layer(nfa, name, g):
    """The project's layer of fixture `name` with the reference's state (masks, degrees and the permutation with it)."""
    F = nfa.flows
    if name == "grad_circ_ar_perm_d21_h40":
        layer = F.CircularAutoregressiveRationalQuadraticSpline(21, 2, 40, ind_circ=[0, 3, 4, 9, 20], num_bins=8,
                                                                tail_bound=torch.from_numpy(g["sd__mprqat__tail_bound"]),
                                                                permute_mask=True, init_identity=False)
    elif name == "grad_circ_ar_perm_d40_h260":
        layer = F.CircularAutoregressiveRationalQuadraticSpline(40, 1, 260, ind_circ=[1, 2, 17, 39], num_bins=5, tail_bound=3.0,
                                                                permute_mask=True, init_identity=False)
    else:
        layer = F.AutoregressiveRationalQuadraticSpline(12, 2, 24, num_bins=8, tail_bound=3.0, permute_mask=True, init_identity=False)
    sd = {k[4:].replace("__", "."): torch.from_numpy(np.asarray(v)) for k, v in g.items() if k.startswith("sd__")}
    sd = {k: (v.float() if k.endswith(".mask") else v) for k, v in sd.items()}
    layer.load_state_dict(sd, strict=True)
    return layer
