"""Cases of the stochastic-layer fixtures (flows/stochastic.py, sampling/hais.py), shared by tests/golden/make_golden_stochastic.py
and the tests.

CASES: name -> settings.  `layer` is "hmc" or "mh"; `target` names an entry of TARGETS.  The 2-D cases have ROWS rows: the first
KINK rows lie on TwoModes' kinks (z0 = 0, the origin), the next third near the ring of radius 2 where the transitions are accepted
often, the rest 1.5 * randn.  "mvn4" is the reference's own unit-test setting (MultivariateNormal in 4-D, 3 steps, batch 3).
`clip` cases carry a max_abs_grad small enough to bind on most rows.

The helpers below are written against a namespace `ns` with the classes as attributes, so the generator builds the reference's
objects and the tests this package's from one description.  TorchDiagGaussian stands in for DiagGaussian on the CPU (this
package's runs on the device only): the reference's formulas and its one draw per forward."""
import numpy as np
import torch
from torch import nn

ROWS = 64
KINK_ROWS = [(0.0, 0.0), (0.0, 1.9), (0.0, -2.1), (-0.0, 0.5)]
LSS = (-2.6, -2.9)           # log_step_size / log_mass of the 2-D cases: two different entries each
LM = (0.1, -0.2)
HAIS_BETAS = (1.0, 0.75, 0.5, 0.25, 0.0)     # n = 4: three layers, alpha = 0.25, 0.5, 0.75 in the order they are built
HAIS_ROWS = 48

TARGETS = {
    "mvn4": ("MultivariateNormal", ()),
    "two_modes": ("TwoModes", (2.0, 0.1)),
    "two_moons": ("TwoMoons", ()),
    "circ_gmm_8": ("CircularGaussianMixture", (8,)),
    "interp": ("LinearInterpolation", ("two_modes", "gauss2", 0.3)),
}

CASES = {
    "hmc_mvn4": dict(layer="hmc", target="mvn4", steps=3, d=4, rows=3, lss=(-2.0,) * 4, lm=(0.0,) * 4, clip=None),
    "mh_mvn4": dict(layer="mh", target="mvn4", steps=3, d=4, rows=3, scale=0.1),
    "hmc_two_modes": dict(layer="hmc", target="two_modes", steps=3, d=2, rows=ROWS, lss=LSS, lm=LM, clip=None),
    "hmc_two_modes_clip": dict(layer="hmc", target="two_modes", steps=3, d=2, rows=ROWS, lss=LSS, lm=LM, clip=4.0),
    "hmc_two_moons": dict(layer="hmc", target="two_moons", steps=2, d=2, rows=ROWS, lss=LSS, lm=LM, clip=None),
    "hmc_circ_gmm_8": dict(layer="hmc", target="circ_gmm_8", steps=4, d=2, rows=ROWS, lss=(-2.0, -2.2), lm=LM, clip=None),
    "hmc_interp": dict(layer="hmc", target="interp", steps=3, d=2, rows=ROWS, lss=LSS, lm=LM, clip=None),
    "mh_two_modes": dict(layer="mh", target="two_modes", steps=4, d=2, rows=ROWS, scale=0.05),
    "mh_two_moons": dict(layer="mh", target="two_moons", steps=3, d=2, rows=ROWS, scale=(0.05, 0.08)),
    "mh_circ_gmm_8": dict(layer="mh", target="circ_gmm_8", steps=4, d=2, rows=ROWS, scale=0.2),
    "mh_interp": dict(layer="mh", target="interp", steps=4, d=2, rows=ROWS, scale=0.1),
}
MIN_MARGIN = 1e-3            # |log u - log prob| of every row (float64): no decision can flip between CPUs


class TorchDiagGaussian(nn.Module):
    """distributions.DiagGaussian(shape, trainable=False) in torch statements (normflows/distributions/base.py:52-103)."""

    def __init__(self, shape):
        super().__init__()
        self.shape = (shape,) if isinstance(shape, int) else tuple(shape)
        self.d = int(np.prod(self.shape))
        self.register_buffer("loc", torch.zeros(1, *self.shape))
        self.register_buffer("log_scale", torch.zeros(1, *self.shape))
        self.temperature = None

    def forward(self, num_samples=1, context=None):
        eps = torch.randn((num_samples,) + self.shape, dtype=self.loc.dtype, device=self.loc.device)
        z = self.loc + torch.exp(self.log_scale) * eps
        log_p = -0.5 * self.d * np.log(2 * np.pi) - torch.sum(self.log_scale + 0.5 * torch.pow(eps, 2), 1)
        return z, log_p

    def log_prob(self, z, context=None):
        return -0.5 * self.d * np.log(2 * np.pi) - torch.sum(self.log_scale + 0.5 * torch.pow((z - self.loc) / torch.exp(self.log_scale), 2), 1)


GAUSS_LOC, GAUSS_LOG_SCALE = (0.3, -0.2), (0.2, 0.4)


def set_gauss(g, dtype):
    """The Gaussian of the interpolation and HAIS cases: a loc and a log_scale that differ per dimension."""
    with torch.no_grad():
        g.loc.copy_(torch.tensor([GAUSS_LOC], dtype=dtype))
        g.log_scale.copy_(torch.tensor([GAUSS_LOG_SCALE], dtype=dtype))
    return g


def build_target(ns, name, dtype, gauss=None):
    """The target `name` from the namespace `ns`, in `dtype`.  gauss: the class of the 2-D Gaussian (default ns.DiagGaussian with
    trainable=False)."""
    cls, args = TARGETS[name]
    if cls == "MultivariateNormal":
        return torch.distributions.MultivariateNormal(torch.zeros(4, dtype=dtype), torch.eye(4, dtype=dtype))
    if cls == "LinearInterpolation":
        g = (gauss(2) if gauss is not None else ns.DiagGaussian(2, trainable=False)).to(dtype)
        return ns.LinearInterpolation(build_target(ns, args[0], dtype), set_gauss(g, dtype), args[2])
    t = getattr(ns, cls)(*args)
    return t.to(dtype) if isinstance(t, nn.Module) else t


def build_layer(ns, name, dtype, gauss=None):
    c = CASES[name]
    target = build_target(ns, c["target"], dtype, gauss)
    if c["layer"] == "hmc":
        layer = ns.HamiltonianMonteCarlo(target, c["steps"], torch.tensor(c["lss"], dtype=dtype), torch.tensor(c["lm"], dtype=dtype),
                                         c["clip"])
    else:
        layer = ns.MetropolisHastings(target, ns.DiagGaussianProposal((c["d"],), c["scale"]), c["steps"])
        layer.proposal.to(dtype)
    return layer


def rows(name, seed):
    """(z (rows, d), cz (rows, d), c (rows)): the input and the cotangents of z_out and log_det, float32."""
    c = CASES[name]
    g = torch.Generator().manual_seed(seed)
    n, d = c["rows"], c["d"]
    z = 1.5 * torch.randn(n, d, generator=g)
    if d == 2 and n >= 3 * len(KINK_ROWS):
        k, m = len(KINK_ROWS), n // 3
        phi = 6.2831853 * torch.rand(m, generator=g)
        z[k:k + m] = 2.0 * torch.stack([torch.cos(phi), torch.sin(phi)], 1) + 0.1 * torch.randn(m, 2, generator=g)
        z[:k] = torch.tensor(KINK_ROWS)
    return z, torch.randn(n, d, generator=g), torch.randn(n, generator=g)


def draw(name, seed, dtype):
    """The random numbers a layer of case `name` draws under torch.manual_seed(seed), in its order: (eps, u).  hmc: eps (rows, d),
    u (rows); mh: eps (steps, rows, d), u (steps, rows)."""
    c = CASES[name]
    torch.manual_seed(seed)
    if c["layer"] == "hmc":
        eps = torch.randn(c["rows"], c["d"], dtype=dtype)
        return eps, torch.rand(c["rows"], dtype=dtype)
    eps, u = [], []
    for _ in range(c["steps"]):
        eps.append(torch.randn(c["rows"], c["d"], dtype=dtype))
        u.append(torch.rand(c["rows"], dtype=dtype))
    return torch.stack(eps), torch.stack(u)


def margins(layer_kind, target, z, eps, u, steps, lss=None, lm=None, clip=None, scale=None):
    """|log u - log prob| per row in float64 (the minimum over the steps for mh; inf where exp(.) >= 1 accepts whatever u is), and
    the decisions: a float64 restatement of the two transitions on explicit noise, for any target with a differentiable log_prob."""
    z, eps, u = z.double(), eps.double(), u.double()

    def grad(x):
        x = x.detach().requires_grad_()
        lp = target.log_prob(x)
        g = torch.autograd.grad(lp.sum(), x)[0]
        return torch.clamp(g, min=-clip, max=clip) if clip else g

    with torch.no_grad():
        if layer_kind == "hmc":
            s, m = torch.exp(lss.double()), torch.exp(lm.double())
            p = eps * torch.sqrt(m)
            zn, pn = z.clone(), p.clone()
            for _ in range(steps):
                with torch.enable_grad():
                    g = grad(zn)
                ph = pn + 0.5 * s * g
                zn = zn + s * ph / m
                with torch.enable_grad():
                    g = grad(zn)
                pn = ph + 0.5 * s * g
            lr = target.log_prob(zn) - target.log_prob(z) - 0.5 * (pn ** 2 / m).sum(1) + 0.5 * (p ** 2 / m).sum(1)
            return (torch.log(u) - lr).abs(), torch.log(u) < lr
        sc = torch.as_tensor(scale, dtype=torch.float64)
        margin = torch.full((len(z),), float("inf"), dtype=torch.float64)
        accepts = []
        lp = target.log_prob(z)
        for i in range(steps):
            z_ = eps[i] * sc + z
            lp_ = target.log_prob(z_)
            lr = lp_ - lp
            acc = torch.log(u[i]) <= torch.clamp(lr, max=0.0)
            margin = torch.minimum(margin, torch.where(lr >= 0, margin, (torch.log(u[i]) - lr).abs()))
            z = torch.where(acc.unsqueeze(1), z_, z)
            lp = torch.where(acc, lp_, lp)
            accepts.append(acc)
        return margin, torch.stack(accepts)
