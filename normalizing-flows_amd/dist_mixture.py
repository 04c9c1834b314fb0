"""GaussianMixture and Uniform base distributions (normflows/distributions/base.py:573-659, :158-195).

GaussianMixture.log_prob keeps a torch-formula route (`_log_prob_torch`) that does the reference's arithmetic op for op: CPU,
float64 (the dtype of the parameters as constructed, as in the reference, until the user casts the module), non-contiguous inputs,
shapes beyond the kernels' limits, subclasses, config.higher_order_gradients() and config.target_density turned off.  Otherwise it
is one launch of nf_gmm_log_prob, and under autograd autograd.GmmLogProbFn (csrc/gmm.hip).

The kernels read ONE record, R = [loc (M, d) | log_scale (M, d) | log_softmax(weight_scores) (M)], built here with differentiable
torch operations: under no_grad it is cached against the parameters' versions (_keys.pcached); under autograd it is rebuilt from
the live parameters, the backward returns gR, and torch's autograd carries that to the leaves -- the softmax's backward stays in
torch.  Sampling is the reference's torch statements in the reference's draw order (multinomial, then randn)."""
import numpy as np
import torch
from torch import nn

from . import _keys
from . import config as _config
from .distributions import BaseDistribution

DMAX, MMAX, MDMAX = 128, 64, 4096     # nf_gmm_log_prob: 32 KB of LDS for loc and the inverse scales


def shape_ok(M, d):
    """The limits of nf_gmm_log_prob on (n_modes, dim)."""
    return 1 <= d <= DMAX and 1 <= M <= MMAX and M * d <= MDMAX


def record(loc, log_scale, weight_scores):
    """R (2 M d + M) of the mixture parameters (1, M, d), (1, M, d), (1, M); differentiable in all three."""
    return torch.cat([loc.reshape(-1), log_scale.reshape(-1), torch.log_softmax(weight_scores, 1).reshape(-1)])


class GaussianMixture(BaseDistribution):
    """Mixture of Gaussians with diagonal covariance (base.py:573-659).  loc, log_scale (1, M, d) and weight_scores (1, M) are
    parameters (trainable) or buffers, float64 as constructed."""

    def __init__(self, n_modes, dim, loc=None, scale=None, weights=None, trainable=True):
        super().__init__()
        self.n_modes = n_modes
        self.dim = dim
        if loc is None:
            loc = np.random.randn(self.n_modes, self.dim)
        loc = np.array(loc)[None, ...]
        if scale is None:
            scale = np.ones((self.n_modes, self.dim))
        scale = np.array(scale)[None, ...]
        if weights is None:
            weights = np.ones(self.n_modes)
        weights = np.array(weights)[None, ...]
        weights /= weights.sum(1)
        if trainable:
            self.loc = nn.Parameter(torch.tensor(1.0 * loc))
            self.log_scale = nn.Parameter(torch.tensor(np.log(1.0 * scale)))
            self.weight_scores = nn.Parameter(torch.tensor(np.log(1.0 * weights)))
        else:
            self.register_buffer("loc", torch.tensor(1.0 * loc))
            self.register_buffer("log_scale", torch.tensor(np.log(1.0 * scale)))
            self.register_buffer("weight_scores", torch.tensor(np.log(1.0 * weights)))

    def _triple(self):
        return (self.loc, self.log_scale, self.weight_scores)

    def _eligible(self, z):
        """True when the kernels take log_prob(z): the switch on and not inside config.higher_order_gradients(), this exact class,
        z a contiguous float32 CUDA (B, dim) matrix, float32 parameters of the constructor's shapes on its device, dim <= 128,
        n_modes <= 64, n_modes x dim <= 4096."""
        M, d = self.n_modes, self.dim
        if not (_config.target_density and not _config.torch_elementwise and type(self) is GaussianMixture and torch.is_tensor(z)
                and z.is_cuda and z.dtype == torch.float32 and z.dim() == 2 and z.shape[1] == d and z.is_contiguous()):
            return False
        if not shape_ok(M, d):
            return False
        shapes = ((1, M, d), (1, M, d), (1, M))
        return all(p.dtype == torch.float32 and p.device == z.device and tuple(p.shape) == s for p, s in zip(self._triple(), shapes))

    def _want(self):
        """Which sections of the record's gradient anybody needs: bit 0 loc, 1 log_scale, 2 weight_scores."""
        if not torch.is_grad_enabled():
            return 0
        return sum(1 << i for i, p in enumerate(self._triple()) if p.requires_grad)

    def _record_nograd(self):
        def build():
            with torch.no_grad():
                return record(*self._triple()).contiguous()
        ps = list(self._triple())
        return _keys.pcached(self, "_record_cache", ps, (str(ps[0].device),), build)

    def _log_prob_kernel(self, z, out=None, acc=None):
        from . import ops
        want = self._want()
        if want or (torch.is_grad_enabled() and z.requires_grad):
            from .autograd import GmmLogProbFn
            R = record(*self._triple()) if want else self._record_nograd()
            lp = GmmLogProbFn.apply(z, R, self.n_modes, want)
            if out is None:
                return lp
            return out.add_(lp) if acc > 0 else out.sub_(lp)
        return ops.gmm_log_prob(z, self._record_nograd(), self.n_modes, out=out, acc=acc)

    def _log_prob_torch(self, z):
        weights = torch.softmax(self.weight_scores, 1)
        eps = (z[:, None, :] - self.loc) / torch.exp(self.log_scale)
        log_p = (-0.5 * self.dim * np.log(2 * np.pi) + torch.log(weights)
                 - 0.5 * torch.sum(torch.pow(eps, 2), 2) - torch.sum(self.log_scale, 2))
        return torch.logsumexp(log_p, 1)

    def log_prob(self, z):
        if self._eligible(z):
            return self._log_prob_kernel(z)
        return self._log_prob_torch(z)

    def _log_prob_acc(self, z, log_q, acc=+1):
        """log_q (+|-)= log_prob(z): fused into the kernel's store where nothing needs a gradient (NormalizingFlow._log_prob_impl)."""
        if self._eligible(z) and log_q.dtype == torch.float32 and log_q.is_contiguous() and log_q.device == z.device:
            self._log_prob_kernel(z, out=log_q, acc=acc)
            return log_q
        lp = self.log_prob(z)
        if acc > 0:
            log_q += lp
        else:
            log_q -= lp
        return log_q

    def forward(self, num_samples=1):
        weights = torch.softmax(self.weight_scores, 1)
        mode = torch.multinomial(weights[0, :], num_samples, replacement=True)
        mode_1h = nn.functional.one_hot(mode, self.n_modes)
        mode_1h = mode_1h[..., None]
        eps_ = torch.randn(num_samples, self.dim, dtype=self.loc.dtype, device=self.loc.device)
        scale_sample = torch.sum(torch.exp(self.log_scale) * mode_1h, 1)
        loc_sample = torch.sum(self.loc * mode_1h, 1)
        z = eps_ * scale_sample + loc_sample
        return z, self.log_prob(z)


class Uniform(BaseDistribution):
    """Multivariate uniform distribution on [low, high]^shape (base.py:158-195).  Torch formulas."""

    def __init__(self, shape, low=-1.0, high=1.0):
        super().__init__()
        if isinstance(shape, int):
            shape = (shape,)
        if isinstance(shape, list):
            shape = tuple(shape)
        self.shape = shape
        self.d = np.prod(shape)
        self.low = torch.tensor(low)
        self.high = torch.tensor(high)
        self.log_prob_val = -self.d * np.log(self.high - self.low)

    def forward(self, num_samples=1, context=None):
        eps = torch.rand((num_samples,) + self.shape, dtype=self.low.dtype, device=self.low.device)
        z = self.low + (self.high - self.low) * eps
        log_p = self.log_prob_val * torch.ones(num_samples, device=self.low.device)
        return z, log_p

    def log_prob(self, z, context=None):
        log_p = self.log_prob_val * torch.ones(z.shape[0], device=z.device)
        out_range = torch.logical_or(z < self.low, z > self.high)
        ind_inf = torch.any(torch.reshape(out_range, (z.shape[0], -1)), dim=-1)
        log_p[ind_inf] = -np.inf
        return log_p
