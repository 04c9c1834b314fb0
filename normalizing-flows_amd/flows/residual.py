"""Residual flow, f(x) = x + g(x) with a Lipschitz-bounded g (arXiv 1906.02735), with the interface of
normflows/flows/residual.py:12-437: constructor signatures, the `iresblock` with its parameters (`geom_p` as a logit, `lamb`), its
`nnet` and its buffers (`last_n_samples`, `last_firmom`, `last_secmom`), every log-det estimator, and the order of the random draws
(first np.random.geometric / np.random.poisson of size n_samples, then ONE torch.randn_like(x)): a seeded run reproduces the
reference's numbers.

The deterministic part -- 2-D inputs with `brute_force or not training`: the exact 2 x 2 Jacobian determinant -- runs on the HIP
kernels of csrc/lipmlp.hip for a CUDA float32 input when no gradient is needed (flows/lipmlp_pack.py has the conditions): the density
direction as one launch per layer, or per run of layers inside core.run_chain; the fixed-point direction as one launch and one
read-back per iteration.  With config.residual_train on, a density-direction pass of such a layer that DOES need a gradient, or a
training-mode pass on a stochastic estimator, runs on the training kernels of csrc/lipmlp_train.hip (one forward and one backward
launch; lipmlp_pack.train_eligible).  With config.residual_nd on, an evaluation-mode layer with exact_trace off on (B, d) rows,
3 <= d <= 64, runs Hutchinson's power series on the kernels of csrc/lipmlp_nd.hip (flows/lipmlp_nd_pack.py has the conditions and
the order of the draws).  Everything else takes the torch formulas below: training at d > 2, exact_trace, d > 64.

One deliberate difference from the reference: under torch.no_grad() the outputs are detached and the caller's tensor is left alone
(the reference leaks a graph out of its enable_grad block and flips requires_grad on the caller's input)."""
import math

import numpy as np
import torch
from torch import nn

from .. import config as _config
from .base import Flow


class Residual(Flow):
    """Invertible residual block.  reverse=True: x + g(x) is the INVERSE pass (density direction = inverse), the fixed-point
    iteration the forward pass; reverse=False the other way round.  reduce_memory: Neumann-series gradient estimator with the
    backward pass precomputed in the forward pass."""

    def __init__(self, net, reverse=True, reduce_memory=True, geom_p=0.5, lamb=2.0, n_power_series=None, exact_trace=False,
                 brute_force=False, n_samples=1, n_exact_terms=2, n_dist="geometric"):
        super().__init__()
        self.reverse = reverse
        self.iresblock = iResBlock(net, n_samples=n_samples, n_exact_terms=n_exact_terms, neumann_grad=reduce_memory,
                                   grad_in_forward=reduce_memory, exact_trace=exact_trace, geom_p=geom_p, lamb=lamb,
                                   n_power_series=n_power_series, brute_force=brute_force, n_dist=n_dist)

    def _torch_pass(self, z, density, truncation=None):
        """(z', log_det) by the torch formulas: density=True is x + g(x), False the fixed-point iteration.  truncation: what
        iResBlock._truncation() returned when a route has drawn it already and then declined the call."""
        z, log_det = self.iresblock.forward(z, 0, truncation) if density else self.iresblock.inverse(z, 0)
        return z, -log_det.view(-1)

    def _pass(self, z, density):
        from . import lipmlp_pack
        if lipmlp_pack.train_eligible(self, z, density):
            out, drawn = lipmlp_pack.run_train(self, z)
            if out is not None:
                return out
            return self._torch_pass(z, density, drawn)      # more than 32 series terms drawn: the formulas, with that draw
        if type(self) is Residual and lipmlp_pack.eligible([self], z, sampling=not density):
            if density:
                return lipmlp_pack.run_density([self], z, None, None)
            return lipmlp_pack.run_sampling(self, z)
        if _config.residual_nd:         # (B, d) rows, 3 <= d <= 64, at inference: csrc/lipmlp_nd.hip
            from . import lipmlp_nd_pack
            if lipmlp_nd_pack.eligible([self], z, sampling=not density):
                if density:
                    return lipmlp_nd_pack.run_density([self], z, None, None)
                return lipmlp_nd_pack.run_sampling(self, z)
        return self._torch_pass(z, density)

    def _density_nd(self, z, vareps, terms, coefs):
        """The density direction on the d-dimensional kernels with the noise and the truncation handed in (nothing is drawn):
        vareps (B, d), terms series terms with the weights coefs[k - 1] = coef(k).  For tests and fixtures: one seed gives CPU and
        GPU generators different numbers.  Raises where flows/lipmlp_nd_pack.eligible declines."""
        from . import lipmlp_nd_pack
        if not lipmlp_nd_pack.eligible([self], z):
            raise NotImplementedError("Residual._density_nd: config.residual_nd is off or the d-dimensional kernels do not take this call")
        return lipmlp_nd_pack.run_density_noise([self], z, vareps.reshape((1,) + tuple(z.shape)), [terms], [coefs])

    def forward(self, z):
        return self._pass(z, not self.reverse)

    def inverse(self, z):
        return self._pass(z, bool(self.reverse))


class iResBlock(nn.Module):
    """x + nnet(x) and the estimators of log|det(I + J)|, J the Jacobian of nnet.
      * brute force (2-D inputs; `brute_force` or evaluation mode): the determinant itself;
      * otherwise the power series sum_k (-1)^(k+1) tr(J^k) / k, truncated at n_power_series (biased) or at a random length with
        reweighted terms (unbiased, "Russian roulette"; geometric or Poisson), with the exact trace or Hutchinson's estimator
        v^T J^k v; `neumann_grad` estimates the gradient's own series instead, `grad_in_forward` precomputes the backward pass."""

    def __init__(self, nnet, geom_p=0.5, lamb=2.0, n_power_series=None, exact_trace=False, brute_force=False, n_samples=1,
                 n_exact_terms=2, n_dist="geometric", neumann_grad=True, grad_in_forward=False):
        super().__init__()
        self.nnet = nnet
        self.n_dist = n_dist
        self.geom_p = nn.Parameter(torch.tensor(np.log(geom_p) - np.log(1.0 - geom_p)))
        self.lamb = nn.Parameter(torch.tensor(lamb))
        self.n_samples = n_samples
        self.n_power_series = n_power_series
        self.exact_trace = exact_trace
        self.brute_force = brute_force
        self.n_exact_terms = n_exact_terms
        self.grad_in_forward = grad_in_forward
        self.neumann_grad = neumann_grad
        self.register_buffer("last_n_samples", torch.zeros(self.n_samples))
        self.register_buffer("last_firmom", torch.zeros(1))
        self.register_buffer("last_secmom", torch.zeros(1))

    def forward(self, x, logpx=None, truncation=None):
        if logpx is None:
            return x + self.nnet(x)
        g, logdetgrad = self._logdetgrad(x, truncation)
        return x + g, logpx - logdetgrad

    def inverse(self, y, logpy=None):
        x = self._inverse_fixed_point(y)
        if logpy is None:
            return x
        return x, logpy + self._logdetgrad(x)[1]

    def _inverse_fixed_point(self, y, atol=1e-5, rtol=1e-5, count=None):
        """x with x + nnet(x) = y by x <- y - nnet(x) from x = y, until every element's squared step is below atol + |y| rtol (all
        rows at once), at most 1001 further steps.  `count`: a list that receives the number of further steps."""
        x, x_prev = y - self.nnet(y), y
        tol = atol + y.abs() * rtol
        i = 0
        while not torch.all((x - x_prev) ** 2 / tol < 1):
            x, x_prev = y - self.nnet(x), x
            i += 1
            if i > 1000:
                break
        if count is not None:
            count.append(i)
        return x

    def _truncation(self):
        """(number of series terms, coefficient function k -> weight of term k, the drawn n or None)."""
        if self.training and self.n_power_series is not None:
            return self.n_power_series, (lambda k: 1.0), None
        if self.n_dist == "geometric":
            p = torch.sigmoid(self.geom_p).item()
            draw, tail = (lambda m: geometric_sample(p, m)), (lambda k, offset: geometric_1mcdf(p, k, offset))
        elif self.n_dist == "poisson":
            lamb = self.lamb.item()
            draw, tail = (lambda m: poisson_sample(lamb, m)), (lambda k, offset: poisson_1mcdf(lamb, k, offset))
        exact = self.n_exact_terms if self.training else 20
        n = draw(self.n_samples)

        def coeff(k):       # 1 / P(N >= k) times the fraction of draws that reach term k
            return 1 / tail(k, exact) * sum(n >= k - exact) / len(n)

        return max(n) + exact, coeff, n

    def _logdetgrad(self, x, truncation=None):
        """(g(x), log|det d(x + g(x)) / dx|) as a (B, 1) column.  truncation: a _truncation() result drawn by the caller."""
        keep_graph = torch.is_grad_enabled()
        with torch.enable_grad():
            g, logdetgrad = self._logdetgrad_impl(x if keep_graph else x.detach(), truncation)
        if not keep_graph:
            g, logdetgrad = g.detach(), logdetgrad.detach()
        return g, logdetgrad

    def _logdetgrad_impl(self, x, truncation=None):
        if (self.brute_force or not self.training) and x.ndimension() == 2 and x.shape[1] == 2:
            x = _differentiable(x)
            g = self.nnet(x)
            jac = batch_jacobian(g, x)
            det = (jac[:, 0, 0] + 1) * (jac[:, 1, 1] + 1) - jac[:, 0, 1] * jac[:, 1, 0]
            return g, torch.log(torch.abs(det)).view(-1, 1)

        n_terms, coeff, drawn = self._truncation() if truncation is None else truncation
        if not self.exact_trace:
            vareps = torch.randn_like(x)
            estimator = neumann_logdet_estimator if self.training and self.neumann_grad else basic_logdet_estimator
            if self.training and self.grad_in_forward:
                g, logdetgrad = mem_eff_wrapper(estimator, self.nnet, x, n_terms, vareps, coeff, self.training)
            else:
                x = _differentiable(x)
                g = self.nnet(x)
                logdetgrad = estimator(g, x, n_terms, vareps, coeff, self.training)
        else:
            x = _differentiable(x)
            g = self.nnet(x)
            jac = batch_jacobian(g, x)
            logdetgrad = batch_trace(jac)
            jac_k = jac
            for k in range(2, n_terms + 1):
                jac_k = torch.bmm(jac, jac_k)
                logdetgrad = logdetgrad + (-1) ** (k + 1) / k * coeff(k) * batch_trace(jac_k)

        if self.training and self.n_power_series is None:
            self.last_n_samples.copy_(torch.tensor(drawn).to(self.last_n_samples))
            est = logdetgrad.detach()
            self.last_firmom.copy_(torch.mean(est).to(self.last_firmom))
            self.last_secmom.copy_(torch.mean(est ** 2).to(self.last_secmom))
        return g, logdetgrad.view(-1, 1)

    def extra_repr(self):
        return "dist={}, n_samples={}, n_power_series={}, neumann_grad={}, exact_trace={}, brute_force={}".format(
            self.n_dist, self.n_samples, self.n_power_series, self.neumann_grad, self.exact_trace, self.brute_force)


def _differentiable(x):
    """x as a tensor autograd can differentiate with respect to: x itself when it already takes part in a graph, else a view of the
    same values that does (the caller's tensor keeps its flag)."""
    return x if x.requires_grad else x.detach().requires_grad_(True)


def batch_jacobian(g, x):
    """(B, dg, dx): row d is the gradient of sum_b g[b, d], one autograd pass per output."""
    rows = [torch.autograd.grad(g[:, d].sum(), x, create_graph=True)[0].view(x.shape[0], 1, x.shape[1]) for d in range(g.shape[1])]
    return torch.cat(rows, 1)


def batch_trace(M):
    return M.view(M.shape[0], -1)[:, ::M.shape[1] + 1].sum(1)


def basic_logdet_estimator(g, x, n_power_series, vareps, coeff_fn, training):
    """sum_k (-1)^(k+1) / k coeff(k) v^T J^k v."""
    vjp = vareps
    logdetgrad = torch.tensor(0.0).to(x)
    for k in range(1, n_power_series + 1):
        vjp = torch.autograd.grad(g, x, vjp, create_graph=training, retain_graph=True)[0]
        tr = (vjp.view(x.shape[0], -1) * vareps.view(x.shape[0], -1)).sum(1)
        logdetgrad = logdetgrad + (-1) ** (k + 1) / k * coeff_fn(k) * tr
    return logdetgrad


def neumann_logdet_estimator(g, x, n_power_series, vareps, coeff_fn, training):
    """v^T (sum_k (-1)^k coeff(k) J^k) J v: the value estimates the GRADIENT's series; only the last product carries a graph."""
    vjp = neumann = vareps
    with torch.no_grad():
        for k in range(1, n_power_series + 1):
            vjp = torch.autograd.grad(g, x, vjp, retain_graph=True)[0]
            neumann = neumann + (-1) ** k * coeff_fn(k) * vjp
    vjp_jac = torch.autograd.grad(g, x, neumann, create_graph=training)[0]
    return (vjp_jac.view(x.shape[0], -1) * vareps.view(x.shape[0], -1)).sum(1)


def safe_detach(tensor):
    return tensor.detach().requires_grad_(tensor.requires_grad)


class MemoryEfficientLogDetEstimator(torch.autograd.Function):
    """The estimator with its backward pass done in the forward pass: the graph of the power series is freed at once and only the
    gradients of sum(logdetgrad) with respect to x and the parameters are kept.  The backward scales them by the FIRST element of
    the log-det's cotangent (a loss weights every row's log-det alike), like the reference."""

    @staticmethod
    def forward(ctx, estimator_fn, gnet, x, n_power_series, vareps, coeff_fn, training, *g_params):
        ctx.training = training
        with torch.enable_grad():
            x = x.detach().requires_grad_(True)
            g = gnet(x)
            ctx.g, ctx.x = g, x
            logdetgrad = estimator_fn(g, x, n_power_series, vareps, coeff_fn, training)
            if training:
                grad_x, *grad_params = torch.autograd.grad(logdetgrad.sum(), (x,) + g_params, retain_graph=True, allow_unused=True)
                if grad_x is None:
                    grad_x = torch.zeros_like(x)
                ctx.save_for_backward(grad_x, *g_params, *grad_params)
        return safe_detach(g), safe_detach(logdetgrad)

    @staticmethod
    def backward(ctx, grad_g, grad_logdetgrad):
        if not ctx.training:
            raise ValueError("Provide training=True if using backward.")
        with torch.enable_grad():
            grad_x, *rest = ctx.saved_tensors
            g_params, grad_params = rest[:len(rest) // 2], rest[len(rest) // 2:]
            dg_x, *dg_params = torch.autograd.grad(ctx.g, [ctx.x] + g_params, grad_g, allow_unused=True)
        dL = grad_logdetgrad[0].detach()
        with torch.no_grad():
            grad_x.mul_(dL)
            grad_params = [gp.mul_(dL) if gp is not None else None for gp in grad_params]
            grad_x.add_(dg_x)
            grad_params = tuple(dg.add_(dj) if dj is not None else dg for dg, dj in zip(dg_params, grad_params))
        return (None, None, grad_x, None, None, None, None) + grad_params


def mem_eff_wrapper(estimator_fn, gnet, x, n_power_series, vareps, coeff_fn, training):
    if not isinstance(gnet, nn.Module):
        raise ValueError("g is required to be an instance of nn.Module.")
    return MemoryEfficientLogDetEstimator.apply(estimator_fn, gnet, x, n_power_series, vareps, coeff_fn, training,
                                                *list(gnet.parameters()))


def geometric_sample(p, n_samples):
    return np.random.geometric(p, n_samples)


def geometric_1mcdf(p, k, offset):
    """P(N >= k - offset) of the geometric distribution; 1 for the always-included terms k <= offset."""
    if k <= offset:
        return 1.0
    return (1 - p) ** max(k - offset - 1, 0)


def poisson_sample(lamb, n_samples):
    return np.random.poisson(lamb, n_samples)


def poisson_1mcdf(lamb, k, offset):
    """P(N >= k - offset) of the Poisson distribution; 1 for k <= offset."""
    if k <= offset:
        return 1.0
    k = k - offset
    total = 1.0
    for i in range(1, k):
        total += lamb ** i / math.factorial(i)
    return 1 - np.exp(-lamb) * total
