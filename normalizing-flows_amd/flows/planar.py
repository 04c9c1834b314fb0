"""Planar flow, f(z) = z + u h(w . z + b) (arXiv 1505.05770), with the interface of normflows/flows/planar.py:8-81: constructor
signature, parameter names and shapes (`u`, `w`: (1, *shape); `b`: (1)), state_dict keys, the order of the seeded draws (u, then w)
and the errors.

A CUDA float32 input of at most 128 elements per row runs on the rank-1 chain kernels (csrc/rank1_chain.hip, flows/rank1_pack.py),
alone or inside a run of Planar / Radial layers that core.run_chain hands to ONE launch.  Everything else -- CPU tensors, float64,
more than 128 elements, a non-contiguous input, config.higher_order_gradients(), config.rank1_chain off, a subclass -- takes
`_torch_forward` / `_torch_inverse`: the reference's arithmetic in torch operations, differentiable to any order."""
import math

import torch
from torch import nn

from .base import Flow

SLOPE = 0.2                       # negative slope of the "leaky_relu" nonlinearity (planar.py:47)
ACTS = ("tanh", "leaky_relu")     # record kinds 0 and 1 of the kernels


def _uniform_parameter(shape, lim):
    p = nn.Parameter(torch.empty(shape)[None])
    nn.init.uniform_(p, -lim, lim)
    return p


class Planar(Flow):
    def __init__(self, shape, act="tanh", u=None, w=None, b=None):
        super().__init__()
        n = math.prod(shape) if not isinstance(shape, int) else shape
        self.u = nn.Parameter(u) if u is not None else _uniform_parameter(shape, math.sqrt(2.0))
        self.w = nn.Parameter(w) if w is not None else _uniform_parameter(shape, math.sqrt(2.0 / n))
        self.b = nn.Parameter(b if b is not None else torch.zeros(1))
        if act not in ACTS:
            raise NotImplementedError("Nonlinearity is not implemented.")
        self.act = act
        self.h = torch.tanh if act == "tanh" else nn.LeakyReLU(negative_slope=SLOPE)

    def _feature_dims(self):
        return list(range(1, self.w.dim()))

    def _u_hat(self):
        """u moved along w so that w . u_hat > -1, the condition for invertibility (planar.py:54-56)."""
        wu = (self.w * self.u).sum()
        return self.u + (torch.log(1 + torch.exp(wu)) - 1 - wu) * self.w / (self.w ** 2).sum()

    def _slope_at(self, lin):
        """h' of the leaky nonlinearity: the reference's (x < 0) rule, so 0 is on the slope-1 side."""
        return (lin < 0) * (self.h.negative_slope - 1.0) + 1.0

    def _torch_forward(self, z):
        lin = (self.w * z).sum(self._feature_dims(), keepdim=True) + self.b
        u_hat = self._u_hat()
        flat = lin.reshape(-1)
        dh = 1 / torch.cosh(flat) ** 2 if self.act == "tanh" else self._slope_at(flat)
        return z + u_hat * self.h(lin), torch.log(torch.abs(1 + (self.w * u_hat).sum() * dh))

    def _torch_inverse(self, z):
        if self.act != "leaky_relu":
            raise NotImplementedError("This flow has no algebraic inverse.")
        lin = (self.w * z).sum(self._feature_dims()) + self.b
        per_row = [-1] + (self.u.dim() - 1) * [1]
        u_eff = self._slope_at(lin).reshape(*per_row) * self._u_hat()       # the slope of the active branch, absorbed into u
        inner = (self.w * u_eff).sum(self._feature_dims())
        return z - u_eff * (lin / (1 + inner)).reshape(*per_row), -torch.log(torch.abs(1 + inner))

    def forward(self, z):
        from . import rank1_pack
        if type(self) is Planar and rank1_pack.eligible([self], z, False):
            return rank1_pack.run([self], z, False, None, None)
        return self._torch_forward(z)

    def inverse(self, z):
        from . import rank1_pack
        if type(self) is Planar and self.act == "leaky_relu" and rank1_pack.eligible([self], z, True):
            return rank1_pack.run([self], z, True, None, None)
        return self._torch_inverse(z)
