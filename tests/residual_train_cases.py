"""The cases of the Residual-flow TRAINING fixtures (tests/golden/residual_train_*.npz), built from whichever package is handed in:
the reference (tests/golden/make_golden_residual_train.py) or normflows_amd (the tests).

LAYERS: single layers in the density direction with loss = sum(z cz) + sum(ld cl), 70 rows (ragged in every tile size of the
kernels), built by residual_cases.at_the_cap unless `cap` is False: name -> (channels, Residual keyword arguments, training mode?,
cap?).  STACK: 3 x [Residual, ActNorm] in training mode through NormalizingFlow.forward_kld."""
import os

import numpy as np
import torch

import residual_cases as cases

GOLDEN = cases.GOLDEN
ROWS = 70

LAYERS = {
    "brute_h32": ([2, 32, 2], {"brute_force": True}, True, True),              # no hidden product
    "eval_h128x2": ([2, 128, 128, 2], {}, False, True),                        # evaluation mode with gradients
    "neumann_h128x2": ([2, 128, 128, 2], {}, True, True),                      # the default: Neumann, memory-saving
    "basic_h40x24": ([2, 40, 24, 2], {"reduce_memory": False}, True, True),    # padded widths, Hutchinson with a graph
    "neumann_h128x3": ([2, 128, 128, 128, 2], {}, True, True),                 # deepest: the LDS budget
    "exact_h64": ([2, 64, 2], {"exact_trace": True}, True, True),
    "poisson3_h32": ([2, 32, 2], {"n_dist": "poisson", "n_samples": 3}, True, True),
    "fwd_h32": ([2, 32, 2], {"reverse": False}, True, True),                   # the other density direction
    "slack_h32": ([2, 32, 2], {}, True, False),                                # weights not scaled up: the clamp is inactive
}
STACK = "stack_h32_k3"
SEEDS = {name: 9900 + 10 * i for i, name in enumerate(list(LAYERS) + [STACK])}


def layer(nf, name, seed=None):
    """The Residual layer of case `name` inside a one-layer NormalizingFlow (at_the_cap walks a model)."""
    channels, kw, training, _ = LAYERS[name]
    if seed is not None:
        torch.manual_seed(seed)
    f = nf.flows.Residual(nf.nets.LipschitzMLP(channels, init_zeros=False, lipschitz_const=cases.LIPSCHITZ), **kw)
    m = nf.NormalizingFlow(nf.distributions.DiagGaussian(2, trainable=False), [f])
    return m.train() if training else m.eval()


def stack(nf, seed=None):
    if seed is not None:
        torch.manual_seed(seed)
    flows = []
    for _ in range(3):
        flows.append(nf.flows.Residual(nf.nets.LipschitzMLP([2, 32, 2], init_zeros=False, lipschitz_const=cases.LIPSCHITZ)))
        flows.append(nf.flows.ActNorm(2))
    return nf.NormalizingFlow(nf.distributions.DiagGaussian(2, trainable=False), flows).train()


def prepare(nf, m, name, generator):
    """The state the results belong to: at_the_cap, or for a `cap` False case 50 power iterations alone."""
    if name == STACK or LAYERS[name][3]:
        cases.at_the_cap(nf, m, generator)
    else:
        nf.utils.update_lipschitz(m, 50)


def density(f, x):
    """(z, log_det) of a Residual layer in its density direction."""
    return f.inverse(x) if f.reverse else f(x)


def load(name):
    return dict(np.load(os.path.join(GOLDEN, "residual_train_%s.npz" % name)))


def state(g):
    return {k[len("sd__"):].replace("__", "."): torch.from_numpy(v) for k, v in g.items() if k.startswith("sd__")}
