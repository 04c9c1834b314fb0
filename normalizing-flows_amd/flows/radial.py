"""Radial flow, f(z) = z + beta h(alpha, r) (z - z_0) (arXiv 1505.05770), with the interface of normflows/flows/radial.py:8-46:
constructor signature, parameters `beta`, `alpha` (1) and `z_0` (1, *shape), the buffer `d`, state_dict keys and the order of the
seeded draws (beta, alpha, z_0); there is no inverse.  Routes as flows/planar.py: the rank-1 chain kernels for CUDA float32 inputs
of at most 128 elements per row, `_torch_forward` (the reference's arithmetic) for everything else."""
import math

import torch
from torch import nn

from .base import Flow


class Radial(Flow):
    def __init__(self, shape, z_0=None):
        super().__init__()
        n = math.prod(shape) if not isinstance(shape, int) else shape
        self.d_cpu = torch.prod(torch.tensor(shape))
        self.register_buffer("d", self.d_cpu)
        self.beta = nn.Parameter(torch.empty(1))
        nn.init.uniform_(self.beta, -1.0 / n - 1.0, 1.0 / n - 1.0)
        self.alpha = nn.Parameter(torch.empty(1))
        nn.init.uniform_(self.alpha, -1.0 / n, 1.0 / n)
        self.z_0 = nn.Parameter(z_0 if z_0 is not None else torch.randn(shape)[None])

    def _torch_forward(self, z):
        a = torch.abs(self.alpha)
        beta = torch.log(1 + torch.exp(self.beta)) - a           # beta' >= -|alpha|: the condition for invertibility
        dz = z - self.z_0
        r = torch.linalg.vector_norm(dz, dim=list(range(1, self.z_0.dim())), keepdim=True)
        h = beta / (a + r)
        dh_r = -beta * r / (a + r) ** 2                            # r h'(r)
        log_det = (self.d - 1) * torch.log(1 + h) + torch.log(1 + h + dh_r)
        return z + h * dz, log_det.reshape(-1)

    def forward(self, z):
        from . import rank1_pack
        if type(self) is Radial and rank1_pack.eligible([self], z, False):
            return rank1_pack.run([self], z, False, None, None)
        return self._torch_forward(z)
