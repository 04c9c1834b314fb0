"""The layers of tests/golden/circ_wide_{a..g}.npz (tests/golden/make_golden_circ_wide.py) rebuilt from their stored state, shared by the
CPU and the GPU tests of the one-launch circular NSF coupling layer.  Test infrastructure."""
import os

import numpy as np
import torch

from conftest import GOLDEN, golden_state, load_golden

K = 8
TB_A = [3.0, np.pi, 2.0, np.pi, 3.5, 1.5]
# name: (D, blocks, hidden, ind_circ, tail_bound, reverse_mask)
LAYERS = {
    "a": (6, 1, 32, [1, 3, 4], TB_A, False),
    "b": (6, 1, 32, [1, 3, 4], TB_A, True),
    "c": (66, 2, 160, list(range(0, 66, 3)), 3.0, False),
    "d": (16, 2, 64, [], 3.0, False),
    "e": (16, 2, 64, list(range(16)), float(np.pi), False),
    "f": (22, 1, 48, list(range(0, 22, 3)), 2.5, False),
    "g": (22, 1, 48, list(range(0, 22, 3)), 2.5, True),
}
BINS = {"f": 4, "g": 16}      # the others: K
MODEL_SCALE = [0.5, 2 * np.pi, 0.5, 2 * np.pi, 7.0, 0.4]

_cache = {}


def golden(name):
    """The fixture of layer `name` (vectors and state; layer (c) keeps its state in a second file).  Loaded once, never modified."""
    if name not in _cache:
        g = load_golden("circ_wide_" + name)
        if os.path.exists(os.path.join(GOLDEN, "circ_wide_%s_state.npz" % name)):
            g.update(load_golden("circ_wide_%s_state" % name))
        _cache[name] = g
    return _cache[name]


def _tensors(state):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in state.items()}


def bound_of(tb):
    return torch.tensor(tb, dtype=torch.float32) if isinstance(tb, list) else tb


def bins(name):
    return BINS.get(name, K)


def layer(nfa, name):
    D, NB, H, ind_circ, tb, rev = LAYERS[name]
    lay = nfa.flows.CircularCoupledRationalQuadraticSpline(D, NB, H, ind_circ=ind_circ, num_bins=bins(name), tail_bound=bound_of(tb),
                                                           reverse_mask=rev, init_identity=False)
    lay.load_state_dict(_tensors(golden_state(golden(name))), strict=True)
    return lay.eval()


def model(nfa):
    """UniformGaussian(6, [1, 3, 4], scale) + 3 x [circular coupling of shape (a) with alternating reverse_mask, PeriodicShift] with the
    state of tests/golden/circ_model_nsf.npz; (model, fixture)."""
    g = load_golden("circ_model_nsf")
    tb = bound_of(TB_A)
    flows = []
    for i in range(3):
        flows.append(nfa.flows.CircularCoupledRationalQuadraticSpline(6, 1, 32, ind_circ=[1, 3, 4], num_bins=K, tail_bound=tb,
                                                                      reverse_mask=bool(i % 2), init_identity=False))
        flows.append(nfa.flows.PeriodicShift([1, 3, 4], bound=tb[[1, 3, 4]], shift=torch.tensor([0.7, -1.1, 2.0])))
    q0 = nfa.distributions.UniformGaussian(6, [1, 3, 4], torch.tensor(MODEL_SCALE, dtype=torch.float32))
    m = nfa.NormalizingFlow(q0, flows)
    m.load_state_dict(_tensors(golden_state(g)), strict=True)
    return m.eval(), g


DECLINED = ("context", "non_alternating_mask", "five_bins", "tanh_preprocessing", "no_unconditional_transform")
DECLINED_CONTEXT = 3


def declined_layer(nfa, what):
    """A D = 8 circular coupling layer outside nf_nsf_wide_ft's structure in the one respect `what` names (the packer returns None,
    the route keeps the layer-wise path); the "context" layer takes a (B, DECLINED_CONTEXT) context."""
    from torch import nn
    mk = lambda **kw: nfa.flows.CircularCoupledRationalQuadraticSpline(8, 2, 32, [1, 4], init_identity=False, **kw).eval()
    torch.manual_seed(3)
    if what == "context":
        return mk(num_context_channels=DECLINED_CONTEXT)
    if what == "non_alternating_mask":
        return mk(mask=torch.tensor([0, 0, 0, 0, 1, 1, 1, 1]))
    if what == "five_bins":
        return mk(num_bins=5)
    lay = mk()
    if what == "tanh_preprocessing":
        lay.prqct.transform_net.preprocessing = nfa.nets.PeriodicFeaturesElementwise(4, [2], 1.0, activation=nn.Tanh())
    else:
        assert what == "no_unconditional_transform"
        lay.prqct.unconditional_transform = None
    return lay


def _by_value(module):
    """Parameters set by formula: the same on every machine, no random generator involved."""
    with torch.no_grad():
        for i, p in enumerate(module.parameters()):
            p.copy_((((torch.arange(p.numel()) * 37 + 11 * i) % 101 - 50).double() / 128).reshape(p.shape).to(p.dtype))   # exact
    return module


def ar_pack_cases(nfa):
    """{name: transform} of the autoregressive spline layers whose per-feature packs (flows/maf_pack.pack_made(..., rows=True,
    features=...)) tests/golden/arnsf_ft_pack_parent.npz records as the packer wrote them before its table helper was factored out."""
    g = load_golden("circ_ar_perm_tb")
    fix = nfa.flows.CircularAutoregressiveRationalQuadraticSpline(7, 2, 24, ind_circ=[0, 2, 5], num_bins=6, permute_mask=True,
                                                                  tail_bound=torch.from_numpy(g["sd__mprqat__tail_bound"]),
                                                                  init_identity=False)
    fix.load_state_dict(_tensors(golden_state(g)), strict=True)
    circ = _by_value(nfa.flows.CircularAutoregressiveRationalQuadraticSpline(5, 2, 12, ind_circ=[0, 3], num_bins=4, tail_bound=2.5,
                                                                             permute_mask=False, init_identity=False))
    lin = _by_value(nfa.flows.AutoregressiveRationalQuadraticSpline(9, 2, 40, num_bins=4, tail_bound=2.5, permute_mask=False,
                                                                    init_identity=False))
    return {"fixture_perm_tensor_bound": fix.mprqat, "circular_scalar_bound": circ.mprqat, "linear_tails": lin.mprqat}
