"""Stochastic flow layers (normflows/flows/stochastic.py): MetropolisHastings and HamiltonianMonteCarlo, the MCMC layers of a
stochastic normalizing flow (arXiv 2002.06707) and of HAIS.

Every layer keeps a torch-formula route (`_transition_torch`) that does the reference's arithmetic op for op and makes its random
draws in its order; it serves every target, shape, dtype and device.  On contiguous float32 CUDA (B, 2) batches against the
closed-form 2-D densities, a 2-D DiagGaussian or a LinearInterpolation of two of them, one transition is ONE launch
(stochastic_route.py, csrc/hmc2d.hip) behind config.stochastic_kernels: torch draws the random numbers in front of the launch, in
the same order, so both routes consume the same numbers of a seeded generator.

One deliberate difference from the reference: `HamiltonianMonteCarlo.gradlogP` evaluates inside `torch.enable_grad()`, so a layer
also runs under `torch.no_grad()` (the reference raises there: its torch.autograd.grad finds no graph)."""
import torch

from .base import Flow
from .. import stochastic_route as _route


class MetropolisHastings(Flow):
    """`steps` Metropolis-Hastings steps towards `target` with `proposal` (stochastic.py:6-51).  Per step the proposal draws its
    `randn`, then the layer draws `rand(num_samples)`; a step is accepted on `w <= clamp(exp(.), max=1)` (a NaN rejects).  The
    log-det is the sum of log p(z) - log p(z') over the accepted steps.  `inverse` is `forward`."""

    def __init__(self, target, proposal, steps):
        super().__init__()
        self.target = target
        self.proposal = proposal
        self.steps = steps

    def forward(self, z):
        if _route.mh_eligible(self, z):
            num_samples = len(z)
            eps = torch.empty((self.steps, num_samples, 2), dtype=z.dtype, device=z.device)
            u = torch.empty((self.steps, num_samples), dtype=z.dtype, device=z.device)
            for i in range(self.steps):        # the reference's order: the proposal's randn, then rand(num_samples)
                torch.randn((num_samples, 2), out=eps[i])
                torch.rand(num_samples, out=u[i])
            return _route.mh_transition(self, z, eps, u)
        return self._transition_torch(z)

    def _transition(self, z, eps, u):
        """forward on explicit random numbers: eps (steps, B, ...) the proposal's standard-normal noise, u (steps, B) the uniforms.
        The proposal is a DiagGaussianProposal (or anything with its `_propose`)."""
        if _route.mh_eligible(self, z):
            return _route.mh_transition(self, z, eps.contiguous(), u.contiguous())
        return self._transition_torch(z, eps, u)

    def _transition_torch(self, z, eps=None, u=None):
        num_samples = len(z)
        log_det = torch.zeros(num_samples, dtype=z.dtype, device=z.device)
        log_p = self.target.log_prob(z)
        for i in range(self.steps):
            z_, log_p_diff = self.proposal(z) if eps is None else self.proposal._propose(z, eps[i])
            log_p_ = self.target.log_prob(z_)
            w = torch.rand(num_samples, dtype=z.dtype, device=z.device) if u is None else u[i]
            log_w_accept = log_p_ - log_p + log_p_diff
            w_accept = torch.clamp(torch.exp(log_w_accept), max=1)
            accept = w <= w_accept
            z = torch.where(accept.unsqueeze(1), z_, z)
            log_det_ = log_p - log_p_
            log_det = torch.where(accept, log_det + log_det_, log_det)
            log_p = torch.where(accept, log_p_, log_p)
        return z, log_det

    def inverse(self, z):
        return self.forward(z)


class HamiltonianMonteCarlo(Flow):
    """One HMC transition towards `target` with `steps` leapfrog steps (stochastic.py:54-108).  Parameters `log_step_size` and
    `log_mass` (shape (dim)); `max_abs_grad` clips the gradient that drives the dynamics (None or 0: no clipping).  Draws
    `randn_like(z)` first and `rand_like(probabilities)` after the trajectory; accepts on `uniforms < probabilities` (a NaN
    rejects).  The log-det is log p(z) - log p(z_out).  `inverse` is `forward`.

    `gradlogP` detaches its argument and builds no graph: to autograd the force is a constant.  Unlike the reference it evaluates
    inside `torch.enable_grad()`, so the layer also runs under `torch.no_grad()`."""

    def __init__(self, target, steps, log_step_size, log_mass, max_abs_grad=None):
        super().__init__()
        self.target = target
        self.steps = steps
        self.register_parameter("log_step_size", torch.nn.Parameter(log_step_size))
        self.register_parameter("log_mass", torch.nn.Parameter(log_mass))
        self.max_abs_grad = max_abs_grad

    def forward(self, z):
        eps = torch.randn_like(z)
        if _route.hmc_eligible(self, z):
            return _route.hmc_transition(self, z, eps, torch.rand(len(z), dtype=z.dtype, device=z.device))
        return self._transition_torch(z, eps)

    def _transition(self, z, eps, u):
        """forward on explicit random numbers: eps like z (standard-normal noise of the momentum), u (B) the uniforms."""
        if _route.hmc_eligible(self, z):
            return _route.hmc_transition(self, z, eps.contiguous(), u.contiguous())
        return self._transition_torch(z, eps, u)

    def _transition_torch(self, z, eps, u=None):
        # Draw momentum
        p = eps * torch.exp(0.5 * self.log_mass)

        # leapfrog
        z_new = z.clone()
        p_new = p.clone()
        step_size = torch.exp(self.log_step_size)
        for i in range(self.steps):
            p_half = p_new - (step_size / 2.0) * -self.gradlogP(z_new)
            z_new = z_new + step_size * (p_half / torch.exp(self.log_mass))
            p_new = p_half - (step_size / 2.0) * -self.gradlogP(z_new)

        # Metropolis Hastings correction
        probabilities = torch.exp(
            self.target.log_prob(z_new)
            - self.target.log_prob(z)
            - 0.5 * torch.sum(p_new ** 2 / torch.exp(self.log_mass), 1)
            + 0.5 * torch.sum(p ** 2 / torch.exp(self.log_mass), 1)
        )
        uniforms = torch.rand_like(probabilities) if u is None else u
        mask = uniforms < probabilities
        z_out = torch.where(mask.unsqueeze(1), z_new, z)

        return z_out, self.target.log_prob(z) - self.target.log_prob(z_out)

    def inverse(self, z):
        return self.forward(z)

    def gradlogP(self, z):
        with torch.enable_grad():
            z_ = z.detach().requires_grad_()
            logp = self.target.log_prob(z_)
            grad = torch.autograd.grad(logp, z_, grad_outputs=torch.ones_like(logp))[0]
        if self.max_abs_grad:
            grad = torch.clamp(grad, max=self.max_abs_grad, min=-self.max_abs_grad)
        return grad
