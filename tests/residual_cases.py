"""The models of the Residual-flow fixtures (tests/golden/residual_*.npz), built from whichever package is handed in: the reference
(tests/golden/make_golden_residual.py) or normflows_amd (the tests) -- same constructors in the same order, same state dict.

CHAIN: eval-mode stacks in the density direction (x -> x + g(x) in every Residual).  A case is (channels of the LipschitzMLP, number
of Residual layers, ActNorm after every Residual?, rows, Residual keyword arguments, training mode?).
SAMPLING: the fixed-point direction of the same kind of stack.
ESTIMATORS: single training-mode layers on the stochastic branches (CPU only), keyword arguments and post-construction switches."""
import glob
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LIPSCHITZ = 0.9         # the constant of the residual-flow examples

CHAIN = {
    "h32_k4": ([2, 32, 2], 4, True, 70, {}, False),                       # one hidden layer, ragged tile
    "h128x2_k16": ([2, 128, 128, 2], 16, True, 300, {}, False),           # the example model, several tiles
    "h128x3_k3": ([2, 128, 128, 128, 2], 3, True, 70, {}, False),         # maximum depth
    "h40x24_k2": ([2, 40, 24, 2], 2, True, 70, {}, False),                # padded widths
    "fwd_h32_k3": ([2, 32, 2], 3, True, 70, {"reverse": False}, False),   # the other density direction
    "bare_h64_k3": ([2, 64, 2], 3, False, 70, {}, False),                 # Residuals with no ActNorm between them
    "brute_train_h32_k2": ([2, 32, 2], 2, True, 70, {"brute_force": True}, True),   # the training-mode brute-force branch
}
SAMPLING = {
    "sample_h32_k1": ([2, 32, 2], 1, False, 70, {}, False),
    "sample_h32_k4": ([2, 32, 2], 4, True, 70, {}, False),
}
STACKS = dict(CHAIN, **SAMPLING)
SEEDS = {name: 9500 + 10 * i for i, name in enumerate(STACKS)}

# name -> (d, channels, Residual kwargs, iResBlock attributes set after construction)
ESTIMATORS = {
    "basic_geometric": (2, [2, 16, 16, 2], {"reduce_memory": False}, {}),
    "neumann_memsave_geometric": (2, [2, 16, 16, 2], {"reduce_memory": True}, {}),
    "neumann_plain_geometric": (2, [2, 16, 16, 2], {"reduce_memory": True}, {"grad_in_forward": False}),
    "basic_memsave_geometric": (2, [2, 16, 16, 2], {"reduce_memory": True}, {"neumann_grad": False}),
    "basic_poisson": (2, [2, 16, 16, 2], {"reduce_memory": False, "n_dist": "poisson"}, {}),
    "neumann_memsave_poisson": (2, [2, 16, 16, 2], {"reduce_memory": True, "n_dist": "poisson", "n_samples": 3}, {}),
    "series5_basic": (2, [2, 16, 16, 2], {"reduce_memory": False, "n_power_series": 5}, {}),
    "series5_memsave": (2, [2, 16, 16, 2], {"reduce_memory": True, "n_power_series": 5}, {}),
    "exact_trace_geometric": (2, [2, 16, 16, 2], {"reduce_memory": False, "exact_trace": True}, {}),
    "exact_trace_poisson": (3, [3, 16, 3], {"reduce_memory": True, "exact_trace": True, "n_dist": "poisson"}, {}),
    "d4_memsave_geometric": (4, [4, 128, 128, 4], {"reduce_memory": True, "n_dist": "geometric"}, {}),
    "d5_basic_poisson": (5, [5, 128, 128, 5], {"reduce_memory": False, "n_dist": "poisson"}, {}),
}
EST_SEEDS = {name: 9800 + 10 * i for i, name in enumerate(ESTIMATORS)}
EST_ROWS = 12


def stack(nf, name, seed=None):
    """NormalizingFlow of stack `name`; with `seed` the construction is seeded (torch.manual_seed(seed), then the constructors in
    order)."""
    channels, n, actnorm, _, kw, training = STACKS[name]
    if seed is not None:
        torch.manual_seed(seed)
    flows = []
    for _ in range(n):
        net = nf.nets.LipschitzMLP(channels, init_zeros=False, lipschitz_const=LIPSCHITZ)
        flows.append(nf.flows.Residual(net, reduce_memory=True, **kw))
        if actnorm:
            flows.append(nf.flows.ActNorm(2))
    m = nf.NormalizingFlow(nf.distributions.DiagGaussian(2, trainable=False), flows)
    return m.train() if training else m.eval()


def at_the_cap(nf, m, generator):
    """The fixtures' recipe: weights and biases of every network times 3 (so that every layer sits at the Lipschitz cap), the
    ActNorm parameters perturbed and marked initialised, then 50 power iterations."""
    with torch.no_grad():
        for mod in m.modules():
            if type(mod).__name__ == "InducedNormLinear":
                mod.weight.mul_(3.0)
                mod.bias.mul_(3.0)
            elif type(mod).__name__ == "ActNorm":
                mod.s.add_(0.3 * torch.randn(mod.s.shape, generator=generator))
                mod.t.add_(0.3 * torch.randn(mod.t.shape, generator=generator))
                mod.data_dep_init_done.fill_(1.0)
    nf.utils.update_lipschitz(m, 50)


def density_is_inverse(name):
    return STACKS[name][4].get("reverse", True)


def walk(flows, x, inverse):
    """(z, [log_det of every layer in execution order]) through the layers' own methods."""
    lds = []
    for f in (reversed(flows) if inverse else flows):
        x, l = f.inverse(x) if inverse else f(x)
        lds.append(l.detach() * torch.ones(x.shape[0], dtype=x.dtype, device=x.device))
        x = x.detach()
    return x, lds


def estimator_layer(nf, name, seed=None):
    d, channels, kw, attrs = ESTIMATORS[name]
    if seed is not None:
        torch.manual_seed(seed)
    net = nf.nets.LipschitzMLP(channels, init_zeros=False, lipschitz_const=LIPSCHITZ)
    f = nf.flows.Residual(net, **kw)
    for k, v in attrs.items():
        setattr(f.iresblock, k, v)
    return f.train()


def load(name):
    """The arrays of fixture residual_<name>.npz, with the state-dict parts residual_<name>_sd<i>.npz of a large model merged in."""
    out = dict(np.load(os.path.join(GOLDEN, "residual_%s.npz" % name)))
    for part in sorted(glob.glob(os.path.join(GOLDEN, "residual_%s_sd[0-9]*.npz" % name))):
        out.update(np.load(part))
    return out
