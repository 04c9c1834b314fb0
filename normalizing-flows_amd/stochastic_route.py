"""The route of the stochastic flow layers onto nf_hmc2d / nf_mh2d (csrc/hmc2d.hip): how a target becomes the one or two terms of a
launch, and the host-side predicates that decide whether the kernel is taken.

A term is (weight, kind, n, record, a0, a1): kind / n / record as dist_route.record gives them for the eight closed-form 2-D
classes, or kind GAUSS for a 2-D DiagGaussian whose `loc` / `log_scale` the kernel reads in device memory (a0, a1; a0 is
CircularGaussianMixture's `scale` buffer for kind 6).  A LinearInterpolation contributes its two terms with the weights alpha and
1 - alpha, read on the HOST: a Python number or a CPU tensor.  A device `alpha` keeps the formulas, so the route never reads a
device value back (no host synchronisation; capturable into a graph).  The route evaluates the densities itself: it does not
depend on config.target_density."""
import numbers

import torch

from . import config as _config
from . import dist_route

GAUSS = 7


def _same_device(t, device):
    return t.device == device


def gauss_ok(loc_dtype, log_scale_dtype, shape, temperature, needs_grad):
    """The DiagGaussian side of the predicate, on plain properties: shape (2,), float32 tensors, no temperature, and no tensor that
    autograd would have to reach (the kernel route carries no gradient into target parameters)."""
    return bool(tuple(shape) == (2,) and loc_dtype == torch.float32 and log_scale_dtype == torch.float32 and temperature is None
                and not needs_grad)


def _term(obj, device):
    """(kind, n, record, a0, a1) of one plain target on `device`, or None when the kernels do not take it."""
    from .distributions import DiagGaussian
    rec = dist_route.record(obj)
    if rec is not None:
        kind, n, r = rec
        if not dist_route.modes_ok(kind, n):
            return None
        a0 = None
        if kind == dist_route.CIRC_GMM:
            s = obj.scale
            if not (s.dtype == torch.float32 and _same_device(s, device) and s.numel() == 1):
                return None
            a0 = s.detach().reshape(1)
        return (kind, n, tuple(r), a0, None)
    if type(obj) is DiagGaussian:
        loc, ls = obj.loc, obj.log_scale
        needs = torch.is_grad_enabled() and (loc.requires_grad or ls.requires_grad)
        if not (gauss_ok(loc.dtype, ls.dtype, obj.shape, obj.temperature, needs) and _same_device(loc, device)
                and _same_device(ls, device) and loc.numel() == 2 and ls.numel() == 2):
            return None
        return (GAUSS, 0, (), loc.detach().reshape(2), ls.detach().reshape(2))
    return None


def alpha_ok(alpha):
    """LinearInterpolation's weight can be read on the host: a Python number, or a one-element CPU tensor."""
    if torch.is_tensor(alpha):
        return alpha.device.type == "cpu" and alpha.numel() == 1 and not alpha.requires_grad
    return isinstance(alpha, numbers.Real)


def target_terms(target, device):
    """[(weight, kind, n, record, a0, a1)] of a target -- one term, or the two of a LinearInterpolation (exact type) -- or None."""
    from .dist_mh import LinearInterpolation
    if type(target) is LinearInterpolation:
        if not alpha_ok(target.alpha):
            return None
        t1, t2 = _term(target.dist1, device), _term(target.dist2, device)
        if t1 is None or t2 is None or (t1[0] == dist_route.CIRC_GMM and t2[0] == dist_route.CIRC_GMM):
            return None
        # the formula's own arithmetic: alpha and 1 - alpha in alpha's precision
        return [(float(target.alpha),) + t1, (float(1 - target.alpha),) + t2]
    t = _term(target, device)
    return None if t is None else [(1.0,) + t]


def _common(z):
    return bool(_config.stochastic_kernels and not _config.torch_elementwise and torch.is_tensor(z)
                and dist_route.input_ok(z.is_cuda, z.dtype, tuple(z.shape), z.is_contiguous()))


def _param_ok(p, device):
    return torch.is_tensor(p) and p.dtype == torch.float32 and p.numel() == 2 and p.device == device and p.is_contiguous()


def clip_of(max_abs_grad):
    """The kernel's clipping bound (0.0 = none) of a layer's max_abs_grad, or None when only the formulas serve it."""
    if not isinstance(max_abs_grad, (type(None), numbers.Real)):
        return None
    if not max_abs_grad:            # None and 0: the reference tests `if self.max_abs_grad`
        return 0.0
    return float(max_abs_grad) if max_abs_grad > 0 else None


def hmc_eligible(layer, z):
    """True when nf_hmc2d takes layer.forward(z): the switch on and not inside config.higher_order_gradients(), the layer EXACTLY a
    HamiltonianMonteCarlo, z a contiguous float32 CUDA (B, 2) matrix, float32 two-element parameters on its device, and a target
    that target_terms takes."""
    from .flows.stochastic import HamiltonianMonteCarlo
    if not (_common(z) and type(layer) is HamiltonianMonteCarlo and isinstance(layer.steps, int) and layer.steps >= 0
            and _param_ok(layer.log_step_size, z.device) and _param_ok(layer.log_mass, z.device)
            and clip_of(layer.max_abs_grad) is not None):
        return False
    return target_terms(layer.target, z.device) is not None


def mh_eligible(layer, z):
    """True when nf_mh2d takes layer.forward(z): as hmc_eligible, with an exact-type DiagGaussianProposal of shape (2,) whose float32
    `scale` buffer of one or two elements lives on z's device."""
    from .flows.stochastic import MetropolisHastings
    from .dist_mh import DiagGaussianProposal
    if not (_common(z) and type(layer) is MetropolisHastings and isinstance(layer.steps, int) and layer.steps >= 0
            and type(layer.proposal) is DiagGaussianProposal and tuple(layer.proposal.shape) == (2,)):
        return False
    s = layer.proposal.scale
    if not (s.dtype == torch.float32 and s.device == z.device and s.numel() in (1, 2) and s.is_contiguous()):
        return False
    return target_terms(layer.target, z.device) is not None


def hmc_transition(layer, z, eps, u):
    """layer's transition on the kernel (hmc_eligible holds) for given noise: (z_out, log_det); one launch, and under autograd one
    backward launch plus the fixed-order reduction when log_step_size / log_mass want a gradient."""
    from . import ops
    terms = target_terms(layer.target, z.device)
    lss, lm = layer.log_step_size, layer.log_mass
    clip = clip_of(layer.max_abs_grad)
    if torch.is_grad_enabled() and (z.requires_grad or lss.requires_grad or lm.requires_grad):
        from .autograd import Hmc2dFn
        return Hmc2dFn.apply(z, lss, lm, eps, u, terms, layer.steps, clip)
    z_out, log_det, _, _ = ops.hmc2d(z, eps, u, lss.detach(), lm.detach(), terms, layer.steps, clip)
    return z_out, log_det


def mh_transition(layer, z, eps, u):
    """layer's `steps` steps on the kernel (mh_eligible holds) for given noise (steps, B, 2) and uniforms (steps, B)."""
    from . import ops
    terms = target_terms(layer.target, z.device)
    scale = layer.proposal.scale.detach().reshape(-1)
    if torch.is_grad_enabled() and z.requires_grad:
        from .autograd import Mh2dFn
        return Mh2dFn.apply(z, scale, eps, u, terms, layer.steps)
    z_out, log_det, _ = ops.mh2d(z, eps, u, scale, terms, layer.steps)
    return z_out, log_det
