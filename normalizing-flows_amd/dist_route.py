"""The route of the closed-form 2-D targets and priors onto nf_density2d (csrc/density2d.hip): the kind codes, the parameter records
and the host-side predicate that decides whether the kernel is taken.

A record is read from the instance's attributes at CALL time (an attribute changed after construction is seen by the next call) and
is a tuple of Python floats, computed in double precision and rounded to float32 once, on its way into the kernel's argument.  The
table is in include/nf_mi355x.h.  CircularGaussianMixture's `scale` is a buffer on the device: the kernel reads it there, so the
route never reads a device value back (no host synchronisation; capturable into a graph)."""
import math

import torch

from . import config as _config

TWO_MODES, SINUSOIDAL, SIN_GAP, SIN_SPLIT, SMILEY, RINGS, CIRC_GMM = range(7)
MAX_MODES = 256        # CircularGaussianMixture: the centres live in LDS
MAX_RINGS = 1 << 16


def _two_modes(loc, scale):
    return (loc, 1.0 / (2 * scale), abs(loc), 1.0 / (3 * scale), 2.0 / (3 * scale) ** 2)


def _sinusoidal(o):
    return (2 * math.pi / o.period, 1.0 / o.scale, (20 * o.scale) ** -4.0)


def _records():
    from . import dist_prior as P
    from . import dist_target as T
    return {
        T.TwoMoons: lambda o: (TWO_MODES, 0, (2.0, 1.0 / 0.2, 2.0, 1.0 / 0.3, 2.0 / 0.09)),
        P.TwoModes: lambda o: (TWO_MODES, 0, _two_modes(float(o.loc), float(o.scale))),
        P.Sinusoidal: lambda o: (SINUSOIDAL, 0, _sinusoidal(o)),
        P.Sinusoidal_gap: lambda o: (SIN_GAP, 0, _sinusoidal(o) + (2.0 / o.scale ** 2, o.w2_amp, o.w2_mu, o.w2_scale)),
        P.Sinusoidal_split: lambda o: (SIN_SPLIT, 0, _sinusoidal(o) + (2.0 / o.scale ** 2, o.w3_amp, o.w3_mu, o.w3_scale)),
        P.Smiley: lambda o: (SMILEY, 0, (o.loc, 1.0 / (2 * o.scale), 0.8, 1.2)),
        T.RingMixture: lambda o: (RINGS, int(o.n_rings), (2.0 / o.n_rings, 1.0 / (2 * o.scale ** 2))),
        T.CircularGaussianMixture: lambda o: (CIRC_GMM, int(o.n_modes), (2 * math.pi / o.n_modes, 2 * math.pi)),
    }


_table = None


def record(obj):
    """(kind, n, rec) of an instance of one of the eight classes (exact type), or None for anything else."""
    global _table
    if _table is None:
        _table = _records()
    build = _table.get(type(obj))
    return None if build is None else build(obj)


def input_ok(is_cuda, dtype, shape, contiguous):
    """The input side of the predicate, on plain properties (no tensor needed): a contiguous float32 CUDA (B, 2) matrix."""
    return bool(is_cuda and dtype == torch.float32 and len(shape) == 2 and shape[1] == 2 and contiguous)


def modes_ok(kind, n):
    """The record side: at most 65 536 rings, at most 256 modes (CircularGaussianMixture's centres live in LDS), at least one."""
    return 1 <= n <= MAX_RINGS if kind == RINGS else (1 <= n <= MAX_MODES if kind == CIRC_GMM else True)


def eligible(obj, z):
    """True when nf_density2d takes obj.log_prob(z): the switch on and not inside config.higher_order_gradients() (the Function is
    once-differentiable), obj of one of the eight classes EXACTLY (a subclass may have changed the formula), z a contiguous float32
    CUDA (B, 2) matrix, at most 256 modes / 65 536 rings, and CircularGaussianMixture's `scale` a float32 buffer on z's device."""
    if not (_config.target_density and not _config.torch_elementwise and torch.is_tensor(z)
            and input_ok(z.is_cuda, z.dtype, tuple(z.shape), z.is_contiguous())):
        return False
    rec = record(obj)
    if rec is None or not modes_ok(rec[0], rec[1]):
        return False
    if rec[0] == CIRC_GMM:
        s = obj.scale
        return s.dtype == torch.float32 and s.device == z.device and s.numel() == 1
    return True


def log_prob(obj, z):
    """obj.log_prob(z) on the kernel (eligible(obj, z) holds): one launch; under autograd the same launch also writes d lp / d z."""
    from . import ops
    kind, n, rec = record(obj)
    dscale = obj.scale.detach().reshape(1) if kind == CIRC_GMM else None
    if torch.is_grad_enabled() and z.requires_grad:
        from .autograd import Density2dFn
        return Density2dFn.apply(z, kind, n, rec, dscale)
    return ops.density2d(z, kind, n, rec, dscale)[0]
