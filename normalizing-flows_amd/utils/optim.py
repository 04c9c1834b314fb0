"""Training-loop helpers (normflows/utils/optim.py:4-31)."""
from ..nets import InducedNormLinear


def set_requires_grad(module, flag):
    """Sets requires_grad of every parameter of `module`."""
    for p in module.parameters():
        p.requires_grad = flag


def clear_grad(model):
    """Drops every parameter's gradient (None, not zeros)."""
    for p in model.parameters():
        p.grad = None


def update_lipschitz(model, n_iterations):
    """`n_iterations` power-iteration steps on the u / v buffers of every InducedNormLinear below `model`: once per training step of
    a residual flow.  The buffers change in place and with them the effective weights -- no parameter is touched."""
    for m in model.modules():
        if isinstance(m, InducedNormLinear):
            m.compute_weight(update=True, n_iterations=n_iterations)
