"""Tensor-level wrappers: one Python function per C-ABI entry point of include/nf_mi355x.h.

Each wrapper validates devices/dtypes, allocates outputs with torch.empty on the input's device and
enqueues exactly one kernel on torch's current HIP stream.  No arithmetic happens in Python.
"""
import ctypes as C
import math

import torch

from . import _lib as L
from ._lib import ptr, ptr_any


def _ld_buffer(logdet, acc, B, like, want=True):
    """The log-det convention of the wrappers, (tensor, acc): no `logdet` given -> a new (B) tensor that the kernel overwrites
    (LD_WRITE); given without `acc` -> the kernel adds to it (LD_ADD).  want=False: nothing is allocated for a missing `logdet`."""
    if logdet is None and want:
        return torch.empty(B, dtype=like.dtype, device=like.device), L.LD_WRITE
    return logdet, L.LD_ADD if acc is None else acc


def _a16(t, vec=True):
    """The tensor itself when its data pointer is 16-byte aligned (None stays None), otherwise a copy in a fresh allocation, which is.
    Every entry point that refuses a misaligned pointer (the "Pointer alignment" table of INTEGRATION.md) gets its row operands through
    this: a contiguous view that starts 4, 8 or 12 bytes into its storage -- a slice of a flat buffer, rows [i:] of a batch with
    D % 4 != 0 -- is copied once instead of reaching a kernel that moves its rows as 16-byte vectors.  An integer test otherwise.
    vec=False: the shape at hand takes the entry point's element-wise kernel, which reads the tensor where it is."""
    if t is None or not vec or t.data_ptr() % 16 == 0:
        return t
    return torch.empty(t.shape, dtype=t.dtype, device=t.device).copy_(t)


def _ld_acc(logdet, acc):
    """actnorm / inv1x1_conv: the per-sample `logdet` is optional and never allocated; LD_ADD when it is given without `acc`."""
    return (L.LD_ADD if logdet is not None and acc is None else acc) or 0


def rqs_spline(x, w, h, d, inverse=False, tails="linear", tail_bound=1.0, left=0.0, right=1.0, bottom=0.0, top=1.0,
               min_bin_width=1e-3, min_bin_height=1e-3, min_derivative=1e-3, wh_div=1.0):
    """utils/splines.py:16-97 / :100-219.  x (...,), w/h (..., K), d (..., K-1|K|K+1); last-dim strided views of one
    parameter block are accepted (row stride taken from .stride(-2))."""
    L.require_device(x, w, h, d)
    K = w.shape[-1]
    for name, a in (("widths", w), ("heights", h), ("derivatives", d)):
        if not L.leading_shape_ok(x.shape, a.shape):
            raise ValueError("rqs_spline: %s %s do not belong to inputs %s (one parameter row per element)" % (name, tuple(a.shape), tuple(x.shape)))
    if h.shape[-1] != K or not L.rqs_derivative_ok(K, d.shape[-1]):
        raise ValueError("rqs_spline: %d widths, %d heights, %d derivatives per element (K, K, K-1 | K | K+1 expected)" % (K, h.shape[-1], d.shape[-1]))
    xs = x.contiguous().view(-1)
    N = xs.numel()

    def rows(a):
        a2 = a.reshape(N, a.shape[-1]) if N > 0 else a.reshape(0, a.shape[-1])
        if a2.stride(-1) != 1:
            a2 = a2.contiguous()
        return a2

    w2, h2, d2 = rows(w), rows(h), rows(d)
    y = torch.empty_like(xs)
    lad = torch.empty_like(xs)
    L.call("nf_rqs_spline", ptr_any(xs), ptr_any(w2), w2.stride(0) if N else K, ptr_any(h2), h2.stride(0) if N else K,
           ptr_any(d2), d2.stride(0) if N else 1, ptr_any(y), ptr_any(lad), N, K, L.TAILS[tails], tail_bound, left, right, bottom,
           top, min_bin_width, min_bin_height, min_derivative, wh_div, int(inverse), L.dtype_code(x), L.stream())
    from . import config
    if config.debug_checks and N > 0:      # device-side flags, read back only in debug mode (config.set_debug_checks)
        flags = torch.zeros(1, dtype=torch.int32, device=x.device)
        L.call("nf_rqs_spline_check", ptr_any(xs), ptr_any(y), N, L.TAILS[tails], tail_bound, left, right, bottom, top,
               int(inverse), L.dtype_code(x), ptr_any(flags), L.stream())
        f = int(flags.item())
        if f & 1:
            raise RuntimeError("rational_quadratic_spline: input outside the domain with tails=None (the reference's gather fails on "
                               "bin index -1 / K, utils/splines.py:154-160)")
        if f & 2:
            raise AssertionError("rational_quadratic_spline: negative discriminant in the inverse direction (utils/splines.py:181)")
    return y.view(x.shape), lad.view(x.shape)


def _tails_args(x, tails, tail_bound, tails_t, bound_t, tails_i, bound_i):
    """What tells nf_rqs_coupling[_bwd] from its per-feature variant: (name suffix, tails code, scalar bound, the variant's trailing
    tensors [tails_t, bound_t, tails_i, bound_i] as int32 / x.dtype on x's device)."""
    if not (tails == "feature" or bound_t is not None or bound_i is not None):
        return "", L.TAILS[tails], tail_bound, []
    fix = lambda t, dtype: None if t is None else t.to(device=x.device, dtype=dtype).contiguous()   # noqa: E731
    code = 3 if tails == "feature" else L.TAILS[tails]
    scalar_bound = float(tail_bound) if not torch.is_tensor(tail_bound) else 1.0
    return "_ft", code, scalar_bound, [fix(tails_t, torch.int32), fix(bound_t, x.dtype), fix(tails_i, torch.int32), fix(bound_i, x.dtype)]


def _rqs_coupling_counts(entry, B, D, K, code, cond, uw, uh, ud, identity_idx, transform_idx, y=None, logdet=None):
    """Element counts of nf_rqs_coupling[_ft|_bwd]: cond (B, nT, M) with M = 2 K + derivatives, the batch-shared rows (nI, K | K | M - 2 K)."""
    nI, nT = identity_idx.numel(), transform_idx.numel()
    nd = L.rqs_derivative_count(K, code)
    L.check_count(entry, "cond", cond, B * nT * (2 * K + nd), "B * nT * (2 K + %d)" % nd)
    L.check_count(entry, "unnormalized_widths", uw, nI * K, "nI * K")
    L.check_count(entry, "unnormalized_heights", uh, nI * K, "nI * K")
    L.check_count(entry, "unnormalized_derivatives", ud, nI * nd, "nI * %d" % nd)
    L.check_count(entry, "y", y, B * D, "B * D")
    L.check_count(entry, "logdet", logdet, B, "B")


def rqs_coupling(x, cond, uw, uh, ud, identity_idx, transform_idx, K, mode, y=None, logdet=None, acc=None,
                 tails="linear", tail_bound=3.0, min_bin_width=1e-3, min_bin_height=1e-3, min_derivative=1e-3,
                 wh_div=1.0, tails_t=None, bound_t=None, tails_i=None, bound_i=None):
    """nsf/coupling.py:71-128 given the conditioner output `cond` (B, nT*M) or (B, nT, M).  tails="feature" with
    int32 tensors tails_t / tails_i (1 linear, 2 circular) and / or per-feature bound tensors bound_t / bound_i select
    the per-feature variant (nf_rqs_coupling_ft, utils/splines.py:48-66)."""
    # (tails_* / bound_*: converted to int32 / x.dtype by _tails_args)
    L.require_device(x, cond, uw, uh, ud, y, logdet, also=(identity_idx, transform_idx, tails_t, bound_t, tails_i, bound_i))
    B, D = x.shape
    x = x.contiguous()
    cond = None if cond is None else cond.contiguous()
    if y is None:
        y = torch.empty_like(x)
    logdet, acc = _ld_buffer(logdet, acc, B, x)
    ft, code, bound, feat = _tails_args(x, tails, tail_bound, tails_t, bound_t, tails_i, bound_i)
    _rqs_coupling_counts("rqs_coupling", B, D, K, code, cond, uw, uh, ud, identity_idx, transform_idx, y, logdet)
    L.call("nf_rqs_coupling" + ft, ptr(x), ptr(y), ptr(logdet), ptr(cond), ptr(uw), ptr(uh), ptr(ud), ptr(identity_idx),
           identity_idx.numel(), ptr(transform_idx), transform_idx.numel(), B, D, K, code, bound, min_bin_width, min_bin_height,
           min_derivative, wh_div, mode, acc, L.dtype_code(x), *map(ptr, feat), L.stream())
    return y, logdet


def lu_linear_permute(x, perm, lower_entries, upper_entries, unconstrained_upper_diag, bias, direction, eps=1e-3,
                      logdet=None, acc=None):
    """mixing.py:535-563.  direction 0 = density (LULinearPermute.inverse), 1 = sample (.forward)."""
    L.require_device(x, perm, lower_entries, upper_entries, unconstrained_upper_diag, bias, logdet)
    B, D = x.shape
    if perm.dtype != torch.int64:
        raise TypeError("lu_linear_permute: perm is %s, the kernel reads int64" % perm.dtype)
    for name, a, n in (("perm", perm, D), ("unconstrained_upper_diag", unconstrained_upper_diag, D), ("bias", bias, D),
                       ("lower_entries", lower_entries, L.tri_count(D)), ("upper_entries", upper_entries, L.tri_count(D)),
                       ("logdet", logdet, B)):
        L.check_count("lu_linear_permute", name, a, n, "D = %d: D | D (D - 1) / 2; logdet: B" % D)
    x = x.contiguous()
    y = torch.empty_like(x)
    logdet, acc = _ld_buffer(logdet, acc, B, x)
    L.call("nf_lu_linear_permute", ptr(x), ptr(y), ptr(logdet), ptr(perm.contiguous()), _cptr(lower_entries), _cptr(upper_entries),
           _cptr(unconstrained_upper_diag), _cptr(bias), B, D, eps, direction, acc, L.dtype_code(x), L.stream())
    return y, logdet


def _mask_rows(z, b):
    """(B, elements per sample, the mask b broadcast to one sample's shape and flattened) of masked_affine[_bwd]."""
    B = z.shape[0]
    inner = z[0].numel() if B else int(math.prod(z.shape[1:]))
    bb = b.to(z.dtype)
    if bb.numel() != inner:
        bb = bb.expand((1,) + tuple(z.shape[1:]))
    return B, inner, bb.contiguous().view(-1)


def _masked_affine_counts(entry, B, inner, bb, s, t, gy=None, logdet=None):
    L.check_count(entry, "b", bb, inner, "elements of one sample")
    for name, a in (("s", s), ("t", t), ("gy", gy)):
        L.check_count(entry, name, a, B * inner, "B * inner = %d * %d: the shape of z" % (B, inner))
    L.check_count(entry, "logdet", logdet, B, "B")


def masked_affine(z, b, s, t, direction, logdet=None, acc=None):
    """affine/coupling.py:209-229.  b broadcastable to z.shape[1:]; s, t same shape as z or None."""
    L.require_device(z, s, t, logdet, also=(b,))      # (b: converted to z.dtype by _mask_rows)
    z = z.contiguous()
    B, inner, bb = _mask_rows(z, b)
    _masked_affine_counts("masked_affine", B, inner, bb, s, t, logdet=logdet)
    vec = z.dtype == torch.float32 and inner <= 256 and inner % 4 == 0     # (the four-elements-per-lane kernel)
    z, bb = _a16(z, vec), _a16(bb, vec)
    y = torch.empty_like(z)
    logdet, acc = _ld_buffer(logdet, acc, B, z)
    s = None if s is None else _a16(s.contiguous(), vec)
    t = None if t is None else _a16(t.contiguous(), vec)
    L.call("nf_masked_affine", ptr(z), ptr(bb), ptr(s), ptr(t), ptr(y), ptr(logdet), B, inner, direction, acc, L.dtype_code(z),
           L.stream())
    return y, logdet


def _affine_coupling_counts(entry, B, Cc, c1, HW, scale_map, param, param_bias=None, gy=None, logdet=None):
    P = L.coupling_param_channels(Cc, c1, scale_map)
    L.check_count(entry, "param", param, B * P * HW, "B * P * HW = %d * %d * %d, P from C = %d, c1 = %d, scale_map = %r" % (B, P, HW, Cc, c1, scale_map))
    L.check_count(entry, "param_bias", param_bias, P, "P")
    L.check_count(entry, "gy", gy, B * Cc * HW, "B * C * HW")
    L.check_count(entry, "logdet", logdet, B, "B")


def affine_coupling(z, param, c1, flip, scale_map, direction, logdet=None, acc=None, param_bias=None):
    """affine/coupling.py:117-171 + channel Split/Merge.  z (B, C, *spatial), param (B, P, *spatial); param_bias (P)
    is added to param inside the kernel (bias of a bias-free last convolution)."""
    L.require_device(z, param, param_bias, logdet)
    z = z.contiguous()
    param = param.contiguous()
    B, Cc = z.shape[:2]
    HW = int(math.prod(z.shape[2:])) if z.dim() > 2 else 1
    _affine_coupling_counts("affine_coupling", B, Cc, c1, HW, scale_map, param, param_bias, logdet=logdet)
    y = torch.empty_like(z)
    logdet, acc = _ld_buffer(logdet, acc, B, z)
    L.call("nf_affine_coupling_pb", ptr(z), ptr(param), _cptr(param_bias), ptr(y), ptr(logdet), B, Cc, c1, int(flip), HW,
           L.SCALE[scale_map], direction, acc, L.dtype_code(z), L.stream())
    return y, logdet


def _actnorm_counts(entry, B, Cc, s, t, gy=None, n_gy=0, logdet=None):
    L.check_count(entry, "s", s, Cc, "C: one per channel")
    L.check_count(entry, "t", t, Cc, "C: one per channel")
    L.check_count(entry, "gy", gy, n_gy, "B * C * HW")
    L.check_count(entry, "logdet", logdet, B, "B")


def actnorm(z, s, t, direction, logdet=None, acc=None, want_scalar=True):
    """affine/coupling.py:38-54 with s, t of C elements (shape (1,C,1,..,1) flattened)."""
    L.require_device(z, s, t, logdet)
    z = z.contiguous()
    B, Cc = z.shape[:2]
    HW = int(math.prod(z.shape[2:])) if z.dim() > 2 else 1
    _actnorm_counts("actnorm", B, Cc, s, t, logdet=logdet)
    y = torch.empty_like(z)
    lds = torch.empty((), dtype=z.dtype, device=z.device) if want_scalar else None
    L.call("nf_actnorm", ptr(z), ptr(s.contiguous().view(-1)), ptr(t.contiguous().view(-1)), ptr(y), ptr(lds), ptr(logdet), B, Cc,
           HW, direction, _ld_acc(logdet, acc), L.dtype_code(z), L.stream())
    return y, lds


def actnorm_stats(z):
    L.require_device(z)
    z = z.contiguous()
    B, Cc = z.shape[:2]
    HW = int(math.prod(z.shape[2:])) if z.dim() > 2 else 1
    mean = torch.empty(Cc, dtype=z.dtype, device=z.device)
    std = torch.empty(Cc, dtype=z.dtype, device=z.device)
    L.call("nf_actnorm_stats", ptr(z), ptr(mean), ptr(std), B, Cc, HW, L.dtype_code(z), L.stream())
    return mean, std


def actnorm_init(mean, std, s_out, t_out, direction):
    L.require_device(mean, std, s_out, t_out)
    Cc = mean.numel()
    for name, a in (("std", std), ("s_out", s_out), ("t_out", t_out)):
        L.check_count("actnorm_init", name, a, Cc, "C = mean.numel()")
    if not (s_out.is_contiguous() and t_out.is_contiguous()):
        raise ValueError("actnorm_init: s_out / t_out are written in place: contiguous tensors")
    mean, std = mean.contiguous(), std.contiguous()
    L.call("nf_actnorm_init", ptr(mean), ptr(std), ptr(s_out), ptr(t_out), mean.numel(), direction, L.dtype_code(mean),
           L.stream())


def inv1x1_assemble(P, Lm, U, sign_S, log_S, inverse):
    L.require_device(P, Lm, U, sign_S, log_S)
    Cc = Lm.shape[0]
    W = torch.empty((Cc, Cc), dtype=Lm.dtype, device=Lm.device)
    ldu = torch.empty((), dtype=Lm.dtype, device=Lm.device)
    L.call("nf_inv1x1_assemble", ptr(P.contiguous()), ptr(Lm.contiguous()), ptr(U.contiguous()), ptr(sign_S.contiguous()),
           ptr(log_S.contiguous()), ptr(W), ptr(ldu), Cc, int(inverse), L.dtype_code(Lm), L.stream())
    return W, ldu


def inv1x1_lu_grads(P, Lm, U, sign_S, log_S, gW, gl):
    """(gL, gU, g_log_S) of Invertible1x1Conv's LU parametrisation in the density direction (nf_inv1x1_lu_grads)."""
    L.require_device(P, Lm, U, sign_S, log_S, gW, gl)
    Cc = Lm.shape[0]
    gL, gU, gs = torch.empty_like(Lm), torch.empty_like(U), torch.empty_like(log_S)
    L.call("nf_inv1x1_lu_grads", ptr(P.contiguous()), ptr(Lm.contiguous()), ptr(U.contiguous()), ptr(sign_S.contiguous()),
           ptr(log_S.contiguous()), ptr(gW.contiguous()), _cptr(gl), ptr(gL), ptr(gU), ptr(gs), Cc, L.dtype_code(Lm), L.stream())
    return gL, gU, gs


def _scratch(name, device, *args):
    """A float32 scratch buffer of the size the query `name` gives for `args` (at least one element)."""
    return torch.empty(max(L.query(name, *args), 1), dtype=torch.float32, device=device)


def _cptr(t):
    """Device pointer of an optional tensor, made contiguous first (NULL for None)."""
    return ptr(None if t is None else t.contiguous())


def _ptr_array(tensors):
    """A ctypes array of device pointers (NULL for None) for the *_multi entry points; the tensors must stay alive through the call."""
    arr = (C.c_void_p * len(tensors))()
    for i, t in enumerate(tensors):
        arr[i] = None if t is None else t.data_ptr()
    return arr


def ld_fold_multi(ld, terms, negate):
    """nf_ld_fold_multi: ld (B) float32 updated IN PLACE with the (B) terms in order (negate[i]: subtracted)."""
    L.require_device(ld, *terms, dtype=torch.float32)
    if ld.dtype != torch.float32 or not ld.is_contiguous() or any(t.dtype != torch.float32 or t.shape != ld.shape for t in terms):
        raise NotImplementedError("ld_fold_multi: contiguous float32 vectors of one length")
    terms = [t.contiguous() for t in terms]
    neg = (C.c_int * len(terms))(*[1 if x else 0 for x in negate])
    L.call("nf_ld_fold_multi", ptr(ld), _ptr_array(terms), neg, len(terms), ld.numel(), L.stream())
    return ld


def inv1x1_assemble_multi(layers):
    """nf_inv1x1_assemble_multi: [(W, per-pixel log|det|)] for `layers` = [(P, L, U, sign_S, log_S)] of ONE size, float32, density
    direction -- one launch per 32 layers."""
    n = len(layers)
    Cc = layers[0][1].shape[0]
    for tup in layers:
        L.require_device(*tup, dtype=torch.float32)
        if tup[1].shape != (Cc, Cc) or tup[1].dtype != torch.float32:
            raise NotImplementedError("inv1x1_assemble_multi: float32 layers of one size")
    dev = layers[0][1].device
    cols = [[t.contiguous() for t in tup] for tup in layers]
    W = torch.empty(n, Cc, Cc, dtype=torch.float32, device=dev)
    ld = torch.empty(n, dtype=torch.float32, device=dev)
    Ws, lds = list(W.unbind(0)), list(ld.unbind(0))
    arrs = [_ptr_array([c[k] for c in cols]) for k in range(5)]
    L.call("nf_inv1x1_assemble_multi", *arrs, _ptr_array(Ws), _ptr_array(lds), n, Cc, L.stream())
    return list(zip(Ws, lds))


def inv1x1_lu_grads_multi(layers, gWs, gls):
    """nf_inv1x1_lu_grads_multi: [(gL, gU, g_log_S)] for `layers` = [(P, L, U, sign_S, log_S)] of one size with cotangents gWs[i]
    (C x C) and gls[i] (0-dim or None)."""
    n = len(layers)
    Cc = layers[0][1].shape[0]
    dev = layers[0][1].device
    cols = [[t.contiguous() for t in tup] for tup in layers]
    gWs = [g.contiguous() for g in gWs]
    gls = [None if g is None else g.contiguous() for g in gls]
    L.require_device(*gWs, *gls, *[t for c in cols for t in c], dtype=torch.float32)
    gL = torch.empty(n, Cc, Cc, dtype=torch.float32, device=dev)
    gU = torch.empty(n, Cc, Cc, dtype=torch.float32, device=dev)
    gs = torch.empty(n, Cc, dtype=torch.float32, device=dev)
    gLs, gUs, gss = list(gL.unbind(0)), list(gU.unbind(0)), list(gs.unbind(0))
    arrs = [_ptr_array([c[k] for c in cols]) for k in range(5)]
    L.call("nf_inv1x1_lu_grads_multi", *arrs, _ptr_array(gWs), _ptr_array(gls), _ptr_array(gLs), _ptr_array(gUs), _ptr_array(gss),
           n, Cc, L.stream())
    return list(zip(gLs, gUs, gss))


def _inv1x1_counts(entry, B, Cc, W, bias=None, logdet_unit=None, logdet=None):
    L.check_count(entry, "W", W, Cc * Cc, "C x C")
    L.check_count(entry, "bias", bias, Cc, "C")
    L.check_count(entry, "logdet_unit", logdet_unit, 1, "one value: log|det W| per pixel")
    L.check_count(entry, "logdet", logdet, B, "B")


def inv1x1_conv(z, W, logdet_unit, logdet=None, acc=None, want_scalar=True, bias=None):
    L.require_device(z, W, logdet_unit, bias, logdet)
    z = z.contiguous()
    B, Cc = z.shape[:2]
    HW = int(math.prod(z.shape[2:]))
    _inv1x1_counts("inv1x1_conv", B, Cc, W, bias, logdet_unit, logdet)
    y = torch.empty_like(z)
    lds = torch.empty((), dtype=z.dtype, device=z.device) if want_scalar else None
    L.call("nf_inv1x1_conv_affine", ptr(z), ptr(W.contiguous()), _cptr(bias), ptr(logdet_unit), ptr(y), ptr(lds), ptr(logdet), B,
           Cc, HW, _ld_acc(logdet, acc), L.dtype_code(z), L.stream())
    return y, lds


def inv1x1_conv_t(z, W):
    """y = W^T z per pixel (nf_inv1x1_conv_t): the 1x1 convolution's input gradient without a transposed copy of W."""
    L.require_device(z, W)
    z = z.contiguous()
    B, Cc = z.shape[:2]
    HW = int(math.prod(z.shape[2:]))
    _inv1x1_counts("inv1x1_conv_t", B, Cc, W)
    y = torch.empty_like(z)
    L.call("nf_inv1x1_conv_t", ptr(z), ptr(W.contiguous()), ptr(y), B, Cc, HW, L.dtype_code(z), L.stream())
    return y


# ---- backward of the affine family (csrc/affine_bwd.hip): closed-form vector-Jacobian products ------------------------
def masked_affine_bwd(z, b, s, t, gy, gld, direction):
    """(gz, gs, gt) of nf_masked_affine for cotangents gy (like z) and gld (B) -- coupling.py:209-229 under autograd."""
    L.require_device(z, s, t, gy, gld, also=(b,))     # (b: converted to z.dtype by _mask_rows)
    z, gy = z.contiguous(), gy.contiguous()
    B, inner, bb = _mask_rows(z, b)
    _masked_affine_counts("masked_affine_bwd", B, inner, bb, s, t, gy=gy, logdet=gld)
    gz = torch.empty_like(z)
    gs = None if s is None else torch.empty_like(z)
    gt = None if t is None else torch.empty_like(z)
    L.call("nf_masked_affine_bwd", ptr(z), ptr(bb), _cptr(s), _cptr(t), ptr(gy), _cptr(gld), ptr(gz), ptr(gs), ptr(gt), B, inner,
           direction, L.dtype_code(z), L.stream())
    return gz, gs, gt


def affine_coupling_bwd(z, param, gy, gld, c1, flip, scale_map, direction):
    """(gz, gparam) of nf_affine_coupling -- coupling.py:117-171 with the channel split / merge under autograd."""
    L.require_device(z, param, gy, gld)
    z, param, gy = z.contiguous(), param.contiguous(), gy.contiguous()
    B, Cc = z.shape[:2]
    HW = int(math.prod(z.shape[2:])) if z.dim() > 2 else 1
    _affine_coupling_counts("affine_coupling_bwd", B, Cc, c1, HW, scale_map, param, gy=gy, logdet=gld)
    gz, gp = torch.empty_like(z), torch.empty_like(param)
    L.call("nf_affine_coupling_bwd", ptr(z), ptr(param), ptr(gy), _cptr(gld), ptr(gz), ptr(gp), B, Cc, c1, int(flip), HW,
           L.SCALE[scale_map], direction, L.dtype_code(z), L.stream())
    return gz, gp


def actnorm_bwd(z, s, t, gy, gld, direction):
    """(gz, gs (C), gt (C)) of nf_actnorm with the log-det returned per sample -- coupling.py:38-54 under autograd."""
    L.require_device(z, s, t, gy, gld)
    z, gy = z.contiguous(), gy.contiguous()
    B, Cc = z.shape[:2]
    HW = int(math.prod(z.shape[2:])) if z.dim() > 2 else 1
    _actnorm_counts("actnorm_bwd", B, Cc, s, t, gy=gy, n_gy=z.numel(), logdet=gld)
    vec = z.dtype == torch.float32 and HW % 4 == 0
    z, gy = _a16(z, vec), _a16(gy, vec)
    gz = torch.empty_like(z)
    gs = torch.empty(Cc, dtype=z.dtype, device=z.device)
    gt = torch.empty(Cc, dtype=z.dtype, device=z.device)
    if B == 0:
        return gz, gs.zero_(), gt.zero_()
    scratch = torch.empty(L.query("nf_actnorm_bwd_scratch_doubles", B, Cc), dtype=torch.float64, device=z.device)
    L.call("nf_actnorm_bwd", ptr(z), ptr(s.contiguous().view(-1)), ptr(t.contiguous().view(-1)), ptr(gy), _cptr(gld), ptr(gz),
           ptr(gs), ptr(gt), ptr(scratch), B, Cc, HW, direction, L.dtype_code(z), L.stream())
    return gz, gs, gt


def rows_matvec(x, W):
    """y_b = W x_b for every row of x (B, D) float32, D <= 128 (nf_rows_matvec, csrc/rows_matvec.hip)."""
    L.require_device(x, dtype=torch.float32, also=(W,))      # (W: converted to float32 below)
    if x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] > 128:
        raise NotImplementedError("rows_matvec: (B, D <= 128) float32")
    x = _a16(x.contiguous(), x.shape[1] in (64, 128))
    y = torch.empty_like(x)
    L.call("nf_rows_matvec", ptr(x), ptr(W.to(torch.float32).contiguous()), ptr(y), x.shape[0], x.shape[1], L.stream())
    return y


def rows_block(x, M1, c1, M2, c2, trans=False, mask1=None, mask2=None, relu=True):
    """(out1, out2) of nf_rows_block: out1 = mask1(M1 pre(x) + c1), out2 = x + mask2(M2 pre(out1) + c2); (B, H <= 128)
    float32.  trans: M1 / M2 are used transposed (the block's backward); relu: pre = ReLU on both products."""
    L.require_device(x, M1, c1, M2, c2, mask1, mask2, dtype=torch.float32)
    x = _a16(x.contiguous())
    B, H = x.shape
    if x.dtype != torch.float32 or H > 128 or H % 4:
        raise NotImplementedError("rows_block: (B, H <= 128, H % 4 == 0) float32")
    M1, M2 = M1.contiguous(), M2.contiguous()
    assert tuple(M1.shape) == (H, H) and tuple(M2.shape) == (H, H)
    out1, out2 = torch.empty_like(x), torch.empty_like(x)
    c = lambda t: None if t is None else _a16(t.contiguous())   # noqa: E731
    L.call("nf_rows_block", ptr(x), H, ptr(M1), H, int(trans), ptr(c(c1)), ptr(c(mask1)), H, ptr(out1), H, ptr(M2), H, int(trans),
           ptr(c(c2)), ptr(c(mask2)), H, ptr(out2), H, B, H, int(relu), int(relu), L.stream())
    return out1, out2


def lu_compose(perm, lower_entries, upper_entries, unconstrained_upper_diag, bias, eps=1e-3):
    """LULinearPermute as dense matrices (nf_lu_compose): (Wd, Ws, bias_d, bias_s, log|det| (1-element)) views of one
    buffer; float32, D <= 64."""
    L.require_device(perm, lower_entries, upper_entries, unconstrained_upper_diag, bias, dtype=torch.float32)
    D = bias.numel()
    out = torch.empty(2 * D * D + 2 * D + 1, dtype=torch.float32, device=bias.device)
    L.call("nf_lu_compose", ptr(perm), ptr(lower_entries.contiguous()), ptr(upper_entries.contiguous()),
           ptr(unconstrained_upper_diag.contiguous()), ptr(bias.contiguous()), eps, ptr(out), D, L.stream())
    N = D * D
    return out[:N].view(D, D), out[N:2 * N].view(D, D), out[2 * N:2 * N + D], out[2 * N + D:2 * N + 2 * D], out[2 * N + 2 * D:]


def lu_factors(perm, lower_entries, upper_entries, unconstrained_upper_diag, eps=1e-3):
    """(L, U, Up, diag, log|det| (1-element), L^T, Up^T) of LULinearPermute's factors in one launch (nf_lu_factors); float32."""
    L.require_device(perm, lower_entries, upper_entries, unconstrained_upper_diag, dtype=torch.float32)
    D = unconstrained_upper_diag.numel()
    out = torch.empty(5 * D * D + D + 1, dtype=torch.float32, device=unconstrained_upper_diag.device)
    L.call("nf_lu_factors", ptr(perm), ptr(lower_entries.contiguous()), ptr(upper_entries.contiguous()),
           ptr(unconstrained_upper_diag.contiguous()), eps, ptr(out), D, L.stream())
    return lu_factors_views(out, D)


def lu_factors_views(out, D):
    """The seven views (L, U, Up, diag, log|det|, L^T, Up^T) of a (5 D^2 + D + 1) factor buffer written by nf_lu_factors[_multi]."""
    N = D * D
    e = 3 * N + D + 1
    return (out[:N].view(D, D), out[N:2 * N].view(D, D), out[2 * N:3 * N].view(D, D), out[3 * N:3 * N + D], out[3 * N + D:e],
            out[e:e + N].view(D, D), out[e + N:e + 2 * N].view(D, D))


def lu_factors_multi(table, n_layers, eps, D):
    """nf_lu_factors for n_layers layers in one launch; table: (n_layers x 5) int64 device pointers (perm, lower, upper, udiag, out)."""
    L.require_device(table, dtype=torch.float32)
    L.call("nf_lu_factors_multi", ptr(table), n_layers, eps, D, L.stream())


def rqs_fused_pack_all_multi(table, n_layers, num_blocks, tail_bound=3.0, min_bin_width=1e-3, min_bin_height=1e-3,
                             min_derivative=1e-3):
    """nf_rqs_fused_pack_all for n_layers layers in one launch; table: (n_layers x (11 + 4 num_blocks)) int64 device pointers."""
    L.require_device(table, dtype=torch.float32)
    L.call("nf_rqs_fused_pack_all_multi", ptr(table), n_layers, 128, num_blocks, 8, tail_bound, min_bin_width, min_bin_height,
           min_derivative, L.stream())


def lu_param_grads(gL, gU, gld, unconstrained_upper_diag, n_tri, eps=1e-3, sign=1.0, perm=None, out=None):
    """(g_lower, g_upper, g_udiag) from the dense factor gradients (nf_lu_param_grads); float32.  gld: the (B) log-det
    cotangent (summed inside the launch) or None; perm: gU's columns are read through it (gU = (gu^T x)[:, perm]);
    out: (g_lower, g_upper, g_udiag) destinations written in place (contiguous float32) instead of new tensors."""
    L.require_device(gL, gU, gld, unconstrained_upper_diag, perm, dtype=torch.float32)
    if gld is not None:
        gld = gld.contiguous()
    D = unconstrained_upper_diag.numel()
    dev = gL.device
    if out is not None:
        g_lower, g_upper, g_udiag = out
        if (g_lower.numel() != n_tri or g_upper.numel() != n_tri or g_udiag.numel() != D
                or any(t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev for t in out)):
            raise ValueError("lu_param_grads: out = contiguous float32 (n_tri), (n_tri), (D) tensors on the inputs' device")
    else:
        g_lower = torch.empty(n_tri, dtype=torch.float32, device=dev)
        g_upper = torch.empty(n_tri, dtype=torch.float32, device=dev)
        g_udiag = torch.empty(D, dtype=torch.float32, device=dev)
    L.call("nf_lu_param_grads", ptr(gL.contiguous()), ptr(gU.contiguous()), ptr(perm), ptr(gld),
           0 if gld is None else gld.numel(), ptr(unconstrained_upper_diag.contiguous()), eps, sign, ptr(g_lower), ptr(g_upper),
           ptr(g_udiag), D, L.stream())
    return g_lower, g_upper, g_udiag


def rows_matvec_affine(x, W, bias, ld_const=None, ld_sign=1.0, logdet=None, acc=None):
    """y_b = W x_b + bias and logdet[b] (acc) ld_sign * ld_const (nf_rows_matvec_affine); (B, D <= 128) float32."""
    L.require_device(x, W, bias, ld_const, logdet, dtype=torch.float32)
    x = _a16(x.contiguous(), x.shape[1] in (64, 128))
    B, D = x.shape
    y = torch.empty_like(x)
    logdet, acc = _ld_buffer(logdet, acc, B, x, want=ld_const is not None)
    L.call("nf_rows_matvec_affine", ptr(x), ptr(W), ptr(bias), ptr(y), ptr(logdet if ld_const is not None else None),
           ptr(ld_const), ld_sign, acc, B, D, L.stream())
    return y, logdet


def rows_matvec2(x, W1, W2, bias=None, ld_const=None, ld_sign=1.0, logdet=None, acc=None, want_u=True):
    """(u, y, logdet): u_b = W1 x_b, y_b = W2 u_b + bias in one launch (nf_rows_matvec2); (B, D <= 64) float32."""
    L.require_device(x, W1, W2, bias, ld_const, logdet, dtype=torch.float32)
    x = _a16(x.contiguous(), x.shape[1] == 64)
    B, D = x.shape
    u = torch.empty_like(x) if want_u else None
    y = torch.empty_like(x)
    logdet, acc = _ld_buffer(logdet, acc, B, x, want=ld_const is not None)
    L.call("nf_rows_matvec2", ptr(x), ptr(W1.contiguous()), ptr(W2.contiguous()), ptr(bias), ptr(u), ptr(y),
           ptr(logdet if ld_const is not None else None), ptr(ld_const), ld_sign, acc, B, D, L.stream())
    return u, y, logdet


def inv1x1_wgrad(z, gy, gld):
    """(gW (C, C), g log|det|-per-pixel (0-dim)) of the per-pixel product y = W z (mixing.py:106-133): gW = sum over
    pixels of gy z^T, partial sums per group of images added in a fixed order."""
    L.require_device(z, gy, gld)
    z, gy = z.contiguous(), gy.contiguous()
    B, Cc = z.shape[:2]
    HW = int(math.prod(z.shape[2:])) if z.dim() > 2 else 1
    n = L.query("nf_inv1x1_wgrad_scratch_elems", B, Cc)
    if n < 0:
        raise NotImplementedError("inv1x1_wgrad: C <= 64")
    scratch = torch.empty(n, dtype=z.dtype, device=z.device)
    gW = torch.empty(Cc, Cc, dtype=z.dtype, device=z.device)
    gl = torch.empty((), dtype=z.dtype, device=z.device)
    L.call("nf_inv1x1_wgrad", ptr(z), ptr(gy), _cptr(gld), ptr(gW), ptr(gl), ptr(scratch), B, Cc, HW, L.dtype_code(z), L.stream())
    return gW, gl


def diag_gaussian_log_prob(z, loc, log_scale, log_scale_shift=0.0, out=None, acc=None):
    """distributions/base.py:94-103."""
    L.require_device(z, loc, log_scale, out)
    z = z.contiguous()
    B = z.shape[0]
    d = int(math.prod(z.shape[1:]))
    for name, a, n in (("loc", loc, d), ("log_scale", log_scale, d), ("out", out, B)):
        L.check_count("diag_gaussian_log_prob", name, a, n, "d = %d elements per sample of z %s; out: B" % (d, tuple(z.shape)))
    vec = z.dtype == torch.float32 and d <= 256 and d % 4 == 0      # (the four-elements-per-lane kernel)
    z = _a16(z, vec)
    out, acc = _ld_buffer(out, acc, B, z)
    L.call("nf_diag_gaussian_log_prob", ptr(z), ptr(_a16(loc.contiguous(), vec).view(-1)), ptr(_a16(log_scale.contiguous(), vec).view(-1)),
           log_scale_shift, ptr(out), B, d, acc, L.dtype_code(z), L.stream())
    return out


def squeeze(z, direction):
    """flows/reshape.py:116-128.  direction 0 = Squeeze.forward, 1 = Squeeze.inverse."""
    L.require_device(z)
    z = z.contiguous()
    B, Cc, H, W = z.shape
    shape = (B, Cc // 4, 2 * H, 2 * W) if direction == 0 else (B, 4 * Cc, H // 2, W // 2)
    y = torch.empty(shape, dtype=z.dtype, device=z.device)
    L.call("nf_squeeze", ptr(z), ptr(y), B, Cc, H, W, direction, L.dtype_code(z), L.stream())
    return y


# ---- fused NSF coupling layer (conditioner on MFMA + spline epilogue) ------------------------------------------
def rqs_fused_supported(nI, nT, hidden, num_blocks, K):
    return L.query("nf_rqs_fused_pack_size", nI, nT, hidden, num_blocks, K) > 0


def rqs_fused_pack(w_init, b_init, w_blocks, b_blocks, w_final, b_final, uw, uh, ud, K, tail_bound, min_bin_width,
                   min_bin_height, min_derivative):
    """Re-lay-out one layer's weights in MFMA operand order (nf_rqs_fused_pack).  Returns the packed device blob."""
    L.require_device(w_init, b_init, w_final, b_final, uw, uh, ud, *w_blocks, *b_blocks, dtype=torch.float32)
    hidden, nI = w_init.shape
    nT = uw.shape[0]
    nb = len(w_blocks) // 2
    size = L.query("nf_rqs_fused_pack_size", nI, nT, hidden, nb, K)
    if size <= 0:
        raise NotImplementedError("nf_rqs_fused: shape not supported")
    blob = torch.empty(size // 4, dtype=torch.float32, device=w_init.device)
    keep = [t.contiguous() for t in (w_init, b_init, w_final, b_final, uw, uh, ud)]
    wb = [t.contiguous() for t in w_blocks]
    bb = [t.contiguous() for t in b_blocks]
    wp, bp = _ptr_array(wb), _ptr_array(bb)
    L.call("nf_rqs_fused_pack", ptr(blob), ptr(keep[0]), ptr(keep[1]), wp, bp, ptr(keep[2]), ptr(keep[3]), ptr(keep[4]),
           ptr(keep[5]), ptr(keep[6]), nI, nT, hidden, nb, K, tail_bound, min_bin_width, min_bin_height, min_derivative,
           L.stream())
    return blob


def rqs_fused_pack_lu(blob, num_blocks, perm, lower_entries, upper_entries, unconstrained_upper_diag, bias, eps=1e-3, K=8):
    """Add the layer's LULinearPermute (composed dense 64 x 64 matrices, both directions) to a packed blob of K bins."""
    L.require_device(blob, perm, lower_entries, upper_entries, unconstrained_upper_diag, bias, dtype=torch.float32)
    D = bias.numel()
    L.call("nf_rqs_fused_pack_lu", ptr(blob), num_blocks, ptr(perm), ptr(lower_entries.contiguous()),
           ptr(upper_entries.contiguous()), ptr(unconstrained_upper_diag.contiguous()), ptr(bias.contiguous()), D, eps, K,
           L.stream())
    return blob


def _rqs_fused_launch(name, x, blobs, parities, hidden, num_blocks, K, direction, logdet, acc, limits, fuse_lu, live_d=None,
                      padded_rows=False):
    """The shared body of rqs_fused[_x3][_chain], `name` the entry point: one layer (blobs a tensor, parities its mask parity) or a chain
    (lists of both, in processing order); padded_rows: rows must have 64 columns, of which live_d are in use."""
    chain = not torch.is_tensor(blobs)
    L.require_device(x, *(blobs if chain else [blobs]), dtype=torch.float32)
    if x.dtype != torch.float32:
        raise TypeError("%s is fp32 only" % name)
    x = _a16(x.contiguous())
    B, D = x.shape
    y = torch.empty_like(x)
    logdet, acc = _ld_buffer(logdet, acc, B, x)
    if padded_rows and D != 64:
        raise ValueError("%s: rows of 64 columns (narrower layers: padded by the caller, live_d = columns in use)" % name)
    if chain:
        layers = (_ptr_array(blobs), (C.c_int * len(blobs))(*[int(v) for v in parities]), len(blobs))
    else:
        layers = (ptr(blobs), parities)
    L.call(name, ptr(x), ptr(y), ptr(logdet), *layers, int(fuse_lu), B, D if live_d is None else live_d, hidden, num_blocks, K,
           *limits, direction, acc, L.stream())
    return y, logdet


def rqs_fused(x, blob, mask_parity, hidden, num_blocks, K, direction, logdet=None, acc=None, tail_bound=3.0,
              min_bin_width=1e-3, min_bin_height=1e-3, min_derivative=1e-3, fuse_lu=False, live_d=None):
    """One launch for a whole CoupledRationalQuadraticSpline layer (+ its LULinearPermute when fuse_lu).
    direction 0 = density, 1 = sample."""
    return _rqs_fused_launch("nf_rqs_fused", x, blob, mask_parity, hidden, num_blocks, K, direction, logdet, acc,
                             (tail_bound, min_bin_width, min_bin_height, min_derivative), fuse_lu, live_d, padded_rows=True)


def rqs_coupling_bwd(x, grad_y, grad_logdet, cond, uw, uh, ud, identity_idx, transform_idx, K, mode, tails="linear",
                     tail_bound=3.0, min_bin_width=1e-3, min_bin_height=1e-3, min_derivative=1e-3, wh_div=1.0,
                     tails_t=None, bound_t=None, tails_i=None, bound_i=None, ft_wave=False):
    """Vector-Jacobian product of rqs_coupling (nf_rqs_coupling_bwd[_ft]).  Returns (gx, gcond, guw, guh, gud).
    ft_wave: the caller's consent (config.nsf_circular_train, passed by the circular coupling layer only) to the wave-private kernel
    for list tails with conditioner rows, 8 bins, float32 (rqs_coupling_bwd_ft_wave); a tile beyond its LDS stays here."""
    if ft_wave and tails == "feature" and K == 8 and x.dtype == torch.float32 and cond is not None:
        out = rqs_coupling_bwd_ft_wave(x, grad_y, grad_logdet, cond, uw, uh, ud, identity_idx, transform_idx, K, mode, tail_bound,
                                       min_bin_width, min_bin_height, min_derivative, wh_div, tails_t, bound_t, tails_i, bound_i)
        if out is not None:
            return out
    # (tails_* / bound_*: converted to int32 / x.dtype by _tails_args)
    L.require_device(x, grad_y, grad_logdet, cond, uw, uh, ud, also=(identity_idx, transform_idx, tails_t, bound_t, tails_i, bound_i))
    B, D = x.shape
    x, grad_y, grad_logdet = x.contiguous(), grad_y.contiguous(), grad_logdet.contiguous()
    cond = None if cond is None else cond.contiguous()
    # density mode owns (writes) every column of gx; the two sampling modes own one half and leave the rest zero
    gx = torch.empty_like(x) if mode == L.RQS_DENSITY else torch.zeros_like(x)
    gcond = torch.empty_like(cond) if cond is not None else None
    guw = torch.zeros_like(uw) if uw is not None else None
    guh = torch.zeros_like(uh) if uh is not None else None
    gud = torch.zeros_like(ud) if ud is not None else None
    ft, code, bound, feat = _tails_args(x, tails, tail_bound, tails_t, bound_t, tails_i, bound_i)
    _rqs_coupling_counts("rqs_coupling_bwd", B, D, K, code, cond, uw, uh, ud, identity_idx, transform_idx, grad_y, grad_logdet)
    L.call("nf_rqs_coupling_bwd" + ft, ptr(x), ptr(grad_y), ptr(grad_logdet), ptr(cond), ptr(uw), ptr(uh), ptr(ud),
           ptr(identity_idx), identity_idx.numel(), ptr(transform_idx), transform_idx.numel(), B, D, K, code, bound,
           min_bin_width, min_bin_height, min_derivative, wh_div, mode, ptr(gx), ptr(gcond), ptr(guw), ptr(guh), ptr(gud),
           L.dtype_code(x), *map(ptr, feat), L.stream())
    return gx, gcond, guw, guh, gud


_FT_WAVE_FITS = {}


def _ft_wave_fits(nI, nT):
    """Whether nf_rqs_coupling_bwd_ft_wave's tile of this split fits the LDS (asked once per split)."""
    key = (nI, nT)
    if key not in _FT_WAVE_FITS:
        _FT_WAVE_FITS[key] = L.query("nf_rqs_coupling_bwd_ft_wave_fits", nI, nT) == 1
    return _FT_WAVE_FITS[key]


def rqs_coupling_bwd_ft_wave(x, grad_y, grad_logdet, cond, uw, uh, ud, identity_idx, transform_idx, K, mode, tail_bound=3.0,
                             min_bin_width=1e-3, min_bin_height=1e-3, min_derivative=1e-3, wh_div=1.0, tails_t=None, bound_t=None,
                             tails_i=None, bound_i=None):
    """rqs_coupling_bwd for list tails (cond rows of 3 K + 1 floats), 8 bins, float32, on wave-private tiles
    (nf_rqs_coupling_bwd_ft_wave, csrc/rqs_bwd_ft.hip): (gx, gcond, guw, guh, gud), or None when the kernel declines the shape (its
    tile does not fit the LDS) -- nothing was allocated or launched then.  gx and gcond are deterministic, the batch-shared parameters' gradients
    come through fp32 atomics."""
    # (tails_* / bound_*: converted to int32 / x.dtype by _tails_args)
    L.require_device(x, grad_y, grad_logdet, cond, uw, uh, ud, also=(identity_idx, transform_idx, tails_t, bound_t, tails_i, bound_i))
    B, D = x.shape
    _rqs_coupling_counts("rqs_coupling_bwd_ft_wave", B, D, K, 3, cond, uw, uh, ud, identity_idx, transform_idx, grad_y, grad_logdet)
    if not _ft_wave_fits(identity_idx.numel(), transform_idx.numel()):      # (decided before anything is allocated)
        return None
    x, grad_y, grad_logdet = x.contiguous(), grad_y.contiguous(), grad_logdet.contiguous()
    cond = None if cond is None else cond.contiguous()
    gx = torch.empty_like(x) if mode == L.RQS_DENSITY else torch.zeros_like(x)
    gcond = torch.empty_like(cond) if cond is not None else None
    guw = torch.zeros_like(uw) if uw is not None else None
    guh = torch.zeros_like(uh) if uh is not None else None
    gud = torch.zeros_like(ud) if ud is not None else None
    _, code, bound, feat = _tails_args(x, "feature", tail_bound, tails_t, bound_t, tails_i, bound_i)
    rc = L.call_rc(
        "nf_rqs_coupling_bwd_ft_wave", ptr(x), ptr(grad_y), ptr(grad_logdet), ptr(cond), ptr(uw), ptr(uh), ptr(ud), ptr(identity_idx), identity_idx.numel(),
        ptr(transform_idx), transform_idx.numel(), B, D, K, code, bound, min_bin_width, min_bin_height, min_derivative, wh_div, mode,
        ptr(gx), ptr(gcond), ptr(guw), ptr(guh), ptr(gud), L.dtype_code(x), *map(ptr, feat), L.stream())
    if rc == L.ENOTSUP:
        return None
    L.check(rc, "nf_rqs_coupling_bwd_ft_wave")
    return gx, gcond, guw, guh, gud


# ---- training forward of the fused layer's last stage (csrc/rqs_fused.hip, TRAIN variant) ------------------------------
def rqs_fused_train_blob(num_blocks, device):
    """Empty packed-blob buffer of the fused layer (filled by rqs_fused_pack_final)."""
    size = L.query("nf_rqs_fused_pack_size", 32, 32, 128, num_blocks, 8)
    if size <= 0:
        raise NotImplementedError("nf_rqs_fused: shape not supported")
    return torch.zeros(size // 4, dtype=torch.float32, device=device)


def rqs_fused_pack_final(blob, w_final, b_final, uw, uh, ud, num_blocks, tail_bound=3.0, min_bin_width=1e-3,
                         min_bin_height=1e-3, min_derivative=1e-3):
    L.require_device(blob, w_final, b_final, uw, uh, ud, dtype=torch.float32)
    L.call("nf_rqs_fused_pack_final", ptr(blob), ptr(w_final.contiguous()), ptr(b_final.contiguous()), ptr(uw.contiguous()),
           ptr(uh.contiguous()), ptr(ud.contiguous()), 128, num_blocks, 8, tail_bound, min_bin_width, min_bin_height,
           min_derivative, L.stream())
    return blob


def _train_fwd(name, x, second, blob, mask_parity, num_blocks, limits, logdet, acc, with_acts=True):
    """The shared body of the three training forwards: allocates y, logdet (by the wrappers' convention), cond24 and, with_acts, the
    (2 num_blocks + 1, B, 128) activations; `second`: the tensor the entry point takes after x (h2 / xlu), if any.
    Returns (y, logdet, cond24, acts)."""
    B = x.shape[0]
    y = torch.empty_like(x)
    ld, acc = _ld_buffer(logdet, acc, B, x)
    cond = torch.empty(B, 32, 24, dtype=x.dtype, device=x.device)
    acts = torch.empty(2 * num_blocks + 1, B, 128, dtype=x.dtype, device=x.device) if with_acts else None
    L.call(name, ptr(x), *([] if second is None else [ptr(second)]), ptr(y), ptr(ld), ptr(cond),
           *([ptr(acts)] if with_acts else []), ptr(blob), mask_parity, B, 64, 128, num_blocks, 8, *limits, acc, L.stream())
    return y, ld, cond, acts


def rqs_fused_train_fwd(x, h2, blob, mask_parity, num_blocks, tail_bound=3.0, min_bin_width=1e-3, min_bin_height=1e-3,
                        min_derivative=1e-3, logdet=None, acc=None):
    """(y, logdet, cond24) of nf_rqs_fused_train_fwd: final Linear + density-direction coupling transform in one launch;
    cond24 (B, 32, 24) is the conditioner output kept for rqs_coupling_bwd_p24.  logdet given: folded into it per acc."""
    L.require_device(x, h2, blob)
    return _train_fwd("nf_rqs_fused_train_fwd", _a16(x.contiguous()), _a16(h2.contiguous()), blob, mask_parity, num_blocks,
                      (tail_bound, min_bin_width, min_bin_height, min_derivative), logdet, acc, with_acts=False)[:3]


def rqs_fused_pack_all(blob, w_init, b_init, w_blocks, b_blocks, w_final, b_final, uw, uh, ud, tail_bound=3.0, min_bin_width=1e-3,
                       min_bin_height=1e-3, min_derivative=1e-3, wfull=None, wpad=None, identity_idx=None):
    """The whole layer's blob (no LU) in one launch (nf_rqs_fused_pack_all); hidden 128, 8 bins."""
    L.require_device(blob, w_init, b_init, w_final, b_final, uw, uh, ud, wfull, wpad, identity_idx, *w_blocks, *b_blocks, dtype=torch.float32)
    n = len(w_blocks)
    wp, bp = _ptr_array(w_blocks), _ptr_array(b_blocks)
    L.call("nf_rqs_fused_pack_all", ptr(blob), ptr(w_init), ptr(b_init), wp, bp, ptr(w_final), ptr(b_final), ptr(uw), ptr(uh),
           ptr(ud), 128, n // 2, 8, tail_bound, min_bin_width, min_bin_height, min_derivative, ptr(wfull), ptr(wpad),
           ptr(identity_idx), L.stream())
    return blob


def rqs_fused_train_full_fwd(x, blob, mask_parity, num_blocks, tail_bound=3.0, min_bin_width=1e-3, min_bin_height=1e-3,
                             min_derivative=1e-3, logdet=None, acc=None):
    """(y, logdet, cond24, acts) of nf_rqs_fused_train_full_fwd: the whole conditioner + coupling transform in one launch;
    acts (2 num_blocks + 1, B, 128) = h0, then (t, h) per residual block."""
    L.require_device(x, blob)
    return _train_fwd("nf_rqs_fused_train_full_fwd", _a16(x.contiguous()), None, blob, mask_parity, num_blocks,
                      (tail_bound, min_bin_width, min_bin_height, min_derivative), logdet, acc)


def _spline_grad_views(alloc, uw, uh, ud):
    """(guw, guh, gud) shaped like the batch-shared spline parameters, as views of ONE buffer from `alloc` (torch.zeros / torch.empty)."""
    nw, nh = uw.numel(), uh.numel()
    gz = alloc(nw + nh + ud.numel(), dtype=uw.dtype, device=uw.device)
    return gz[:nw].view_as(uw), gz[nw:nw + nh].view_as(uh), gz[nw + nh:].view_as(ud)


def rqs_coupling_bwd_p24(x, grad_y, grad_logdet, cond24, uw, uh, ud, identity_idx, transform_idx, tail_bound=3.0,
                         min_bin_width=1e-3, min_bin_height=1e-3, min_derivative=1e-3, wh_div=1.0):
    """rqs_coupling_bwd (density direction) on the 24-float rows of rqs_fused_train_fwd.  Returns (gx, gcond24, guw, guh, gud)."""
    L.require_device(x, grad_y, grad_logdet, cond24, uw, uh, ud, identity_idx, transform_idx, dtype=torch.float32)
    B, D = x.shape
    x, grad_y, grad_logdet = x.contiguous(), grad_y.contiguous(), grad_logdet.contiguous()
    cond24 = _a16(cond24.contiguous())      # (the parameter rows are refused when misaligned; x / grad_y only choose the kernel)
    gx = torch.empty_like(x)
    gcond = torch.empty_like(cond24)
    guw, guh, gud = _spline_grad_views(torch.zeros, uw, uh, ud)     # one zero fill for the three atomically-accumulated outputs
    L.call("nf_rqs_coupling_bwd_p24", ptr(x), ptr(grad_y), ptr(grad_logdet), ptr(cond24), ptr(uw), ptr(uh), ptr(ud),
           ptr(identity_idx), identity_idx.numel(), ptr(transform_idx), transform_idx.numel(), B, D, tail_bound, min_bin_width,
           min_bin_height, min_derivative, wh_div, ptr(gx), ptr(gcond), ptr(guw), ptr(guh), ptr(gud), L.stream())
    return gx, gcond, guw, guh, gud


def final_bwd(x, grad_y, grad_logdet, cond24, w_t, blob, uw, uh, ud, mask_parity, num_blocks, tail_bound=3.0, min_bin_width=1e-3,
              min_bin_height=1e-3, min_derivative=1e-3):
    """(gx, gcond24, gh, guw, guh, gud) of nf_final_bwd + nf_final_bwd_reduce: the coupling transform's backward and the final
    Linear's input gradient in one pass over the rows; the batch-shared parameters' gradients by a fixed-order reduction."""
    L.require_device(x, grad_y, grad_logdet, cond24, w_t, blob, uw, uh, ud, dtype=torch.float32)
    B = x.shape[0]
    x, grad_y, grad_logdet = _a16(x.contiguous()), _a16(grad_y.contiguous()), grad_logdet.contiguous()
    cond24, w_t = _a16(cond24.contiguous()), _a16(w_t.contiguous())
    gx = torch.empty_like(x)
    gcond = torch.empty_like(cond24)
    gh = torch.empty(B, 128, dtype=x.dtype, device=x.device)
    nparts = L.query("nf_final_bwd_partials", B)
    part = torch.empty(max(nparts, 1) * 768, dtype=x.dtype, device=x.device)
    guw, guh, gud = _spline_grad_views(torch.empty, uw, uh, ud)
    kw = (tail_bound, min_bin_width, min_bin_height, min_derivative)
    L.call("nf_final_bwd", ptr(x), ptr(grad_y), ptr(grad_logdet), ptr(cond24), ptr(w_t), ptr(blob), ptr(gx), ptr(gcond), ptr(gh),
           ptr(part), mask_parity, B, 64, 128, num_blocks, 8, *kw, L.stream())
    L.call("nf_final_bwd_reduce", ptr(part), nparts, ptr(uw.contiguous()), ptr(uh.contiguous()), ptr(ud.contiguous()), ptr(guw),
           ptr(guh), ptr(gud), 8, *kw, L.stream())
    return gx, gcond, gh, guw, guh, gud


def _train_bwd_operands(who, B, num_blocks, w_blocks, dest, more_keys, device):
    """What coupling_train_bwd and pair_train_bwd (`who`) prepare alike: the gradient destinations `dest` validated (more_keys: the
    pair's LU destinations), then (scratch, the contiguous block weights -- to be kept alive through the call --, their pointer array,
    the pointer array of dest["blocks"])."""
    n = L.query("nf_%s_scratch_floats" % who, B, num_blocks)
    if n <= 0:
        raise NotImplementedError("%s: batch a multiple of 64, 1 <= num_blocks <= 5" % who)
    tensors = [dest[k] for k in ("w0", "b0", "wf", "bf", "uw", "uh", "ud") + tuple(more_keys)] + list(dest["blocks"])
    if len(w_blocks) != 2 * num_blocks or len(dest["blocks"]) != 4 * num_blocks:
        raise ValueError("%s: 2 weights and 4 gradient destinations per residual block" % who)
    L.require_device(*tensors, dtype=torch.float32)
    if any(t.dtype != torch.float32 or not t.is_contiguous() for t in tensors):
        raise ValueError("%s: gradient destinations must be contiguous float32" % who)
    scratch = torch.empty(n, dtype=torch.float32, device=device)
    wb = [w.contiguous() for w in w_blocks]
    return scratch, wb, _ptr_array(wb), _ptr_array(dest["blocks"])


def pair_train_bwd(x_in, xlu, grad_y, grad_logdet, cond24, acts, w_t, blob, wfull_t, w_blocks, uw, uh, ud, col_map, n_cols, mask_parity,
                   num_blocks, Wd, Lm, Um, perm, udiag, lu_eps, dest, tail_bound=3.0, min_bin_width=1e-3, min_bin_height=1e-3,
                   min_derivative=1e-3, side=None):
    """The whole backward of a [CoupledRQS, LULinearPermute] pair in one C-ABI call (nf_pair_train_bwd: seven launches).  dest: as
    coupling_train_bwd plus lower, upper, udiag, lbias (the LU's gradient destinations).  Returns the pair's input gradient.
    side (a torch.cuda.Stream): the last two launches -- the reduction of the partial tiles and the LU's factor gradients, which only
    produce parameter gradients -- go to that stream, forked from the current one by an event (nf_pair_train_bwd_head / _tail): they
    run under whatever the current stream does next.  The CALLER joins (`current_stream().wait_stream(side)`) before a gradient in
    `dest` is read; the scratch and the tensors the tail reads are kept from reuse through record_stream."""
    L.require_device(x_in, xlu, grad_y, grad_logdet, cond24, acts, w_t, blob, wfull_t, uw, uh, ud, col_map, Wd, Lm, Um, perm, udiag,
                     *w_blocks, dtype=torch.float32)
    B = x_in.shape[0]
    x_in, xlu, grad_y, grad_logdet = _a16(x_in.contiguous()), _a16(xlu.contiguous()), _a16(grad_y.contiguous()), grad_logdet.contiguous()
    cond24, acts, w_t, wfull_t = (_a16(t.contiguous()) for t in (cond24, acts, w_t, wfull_t))
    scratch, wb, wp, gp = _train_bwd_operands("pair_train_bwd", B, num_blocks, w_blocks, dest, ("lower", "upper", "udiag", "lbias"),
                                              x_in.device)
    gx = torch.empty_like(x_in)
    uw_, uh_, ud_, Lm_, Um_, udiag_ = uw.contiguous(), uh.contiguous(), ud.contiguous(), Lm.contiguous(), Um.contiguous(), udiag.contiguous()
    args = (ptr(x_in), ptr(xlu), ptr(grad_y), ptr(grad_logdet), ptr(cond24), ptr(acts), ptr(w_t), ptr(blob), ptr(wfull_t), wp, ptr(uw_),
            ptr(uh_), ptr(ud_), ptr(col_map), int(n_cols), ptr(Wd), ptr(Lm_), ptr(Um_), ptr(perm), ptr(udiag_), lu_eps, ptr(gx),
            ptr(dest["lower"]), ptr(dest["upper"]), ptr(dest["udiag"]), ptr(dest["lbias"]), ptr(dest["w0"]), ptr(dest["b0"]),
            ptr(dest["wf"]), ptr(dest["bf"]), ptr(dest["uw"]), ptr(dest["uh"]), ptr(dest["ud"]), gp, ptr(scratch), mask_parity, B, 64, 128,
            num_blocks, 8, tail_bound, min_bin_width, min_bin_height, min_derivative)
    if side is None:
        L.call("nf_pair_train_bwd", *args, L.stream())
        return gx
    tail = C.create_string_buffer(2048)                       # NF_PAIR_TAIL_BYTES
    L.call("nf_pair_train_bwd_head", *args, tail, L.stream())
    cur = torch.cuda.current_stream()
    side.wait_stream(cur)                                     # fork: an event recorded here, behind the five launches
    L.call("nf_pair_train_bwd_tail", tail, C.c_void_p(side.cuda_stream))
    # what the side stream reads or writes must not go back to the allocator (or be rewritten on the current stream) before it is done
    # (parameters, the prepacked factors and the flat gradient buffer outlive the step; the caller's join comes before they change)
    for t in (scratch, grad_logdet):
        t.record_stream(side)
    return gx


def lu_pack_train_multi(table, n_layers, num_blocks, eps, D=64):
    """The LU stage of n training blobs + the composed matrices for the backward in one launch (nf_lu_pack_train_multi)."""
    L.require_device(table, dtype=torch.float32)
    L.call("nf_lu_pack_train_multi", ptr(table), n_layers, num_blocks, D, eps, L.stream())


def rqs_fused_train_pair_fwd(x, blob, mask_parity, num_blocks, tail_bound=3.0, min_bin_width=1e-3, min_bin_height=1e-3,
                             min_derivative=1e-3, logdet=None, acc=None):
    """(xlu, y, logdet, cond24, acts) of nf_rqs_fused_train_pair_fwd: LULinearPermute.inverse + the whole coupling layer in one
    launch; xlu (B, 64) = the LU's output (the coupling's input), the rest as rqs_fused_train_full_fwd."""
    L.require_device(x, blob)
    x = _a16(x.contiguous())
    xlu = torch.empty_like(x)
    return (xlu,) + _train_fwd("nf_rqs_fused_train_pair_fwd", x, xlu, blob, mask_parity, num_blocks,
                               (tail_bound, min_bin_width, min_bin_height, min_derivative), logdet, acc)


def lu_bwd_composed(g, x, Wd, db_out=None):
    """(gx, dWd, db) of the composed LULinearPermute's backward, D = 64 (nf_lu_bwd_composed): gx = g Wd, dWd = g^T x, db = colsum(g)."""
    L.require_device(g, x, Wd, db_out, dtype=torch.float32)
    g, x, Wd = _a16(g.contiguous()), _a16(x.contiguous()), Wd.contiguous()
    B, D = g.shape
    n = L.query("nf_lu_bwd_composed_scratch_floats", B)
    if n <= 0 or D != 64 or g.dtype != torch.float32:
        raise NotImplementedError("lu_bwd_composed: float32, D = 64, batch a multiple of 64")
    scratch = torch.empty(n, dtype=torch.float32, device=g.device)
    dWd = torch.empty(D, D, dtype=torch.float32, device=g.device)
    if db_out is None:
        db_out = torch.empty(D, dtype=torch.float32, device=g.device)
    elif db_out.numel() != D or db_out.dtype != torch.float32 or not db_out.is_contiguous():
        raise ValueError("lu_bwd_composed: db_out = a contiguous float32 (D) tensor")
    gx = torch.empty_like(g)
    L.call("nf_lu_bwd_composed", ptr(g), ptr(x), ptr(Wd), ptr(gx), ptr(dWd), ptr(db_out), ptr(scratch), B, D, L.stream())
    return gx, dWd, db_out


def lu_param_grads_composed(dWd, Lm, Um, perm, gld, unconstrained_upper_diag, n_tri, eps=1e-3, out=None):
    """(g_lower, g_upper, g_udiag) from the composed matrix's gradient (nf_lu_param_grads_composed); out: destinations."""
    L.require_device(dWd, Lm, Um, perm, gld, unconstrained_upper_diag, dtype=torch.float32)
    D = unconstrained_upper_diag.numel()
    dev = dWd.device
    if gld is not None:
        gld = gld.contiguous()
    if out is not None:
        g_lower, g_upper, g_udiag = out
        if (g_lower.numel() != n_tri or g_upper.numel() != n_tri or g_udiag.numel() != D
                or any(t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev for t in out)):
            raise ValueError("lu_param_grads_composed: out = contiguous float32 (n_tri), (n_tri), (D) tensors")
    else:
        g_lower = torch.empty(n_tri, dtype=torch.float32, device=dev)
        g_upper = torch.empty(n_tri, dtype=torch.float32, device=dev)
        g_udiag = torch.empty(D, dtype=torch.float32, device=dev)
    L.call("nf_lu_param_grads_composed", ptr(dWd.contiguous()), ptr(Lm.contiguous()), ptr(Um.contiguous()), ptr(perm), ptr(gld),
           0 if gld is None else gld.numel(), ptr(unconstrained_upper_diag.contiguous()), eps, ptr(g_lower), ptr(g_upper),
           ptr(g_udiag), D, L.stream())
    return g_lower, g_upper, g_udiag


def coupling_train_bwd(x, grad_y, grad_logdet, cond24, acts, w_t, blob, wfull_t, w_blocks, uw, uh, ud, col_map, n_cols, mask_parity,
                       num_blocks, dest, tail_bound=3.0, min_bin_width=1e-3, min_bin_height=1e-3, min_derivative=1e-3):
    """The whole backward of a benchmark-shaped coupling layer in one C-ABI call (nf_coupling_train_bwd): four passes over the rows
    and ONE reduction launch.  w_blocks: [W1, W2] per residual block; dest: the gradient destinations, written in place --
    dict(w0, b0, wf, bf, uw, uh, ud, blocks=[gW1, gb1, gW2, gb2 per block]) of contiguous float32 tensors of the parameters'
    shapes (any addresses: fresh tensors or views of one flat gradient buffer).  Returns grad_x."""
    L.require_device(x, grad_y, grad_logdet, cond24, acts, w_t, blob, wfull_t, uw, uh, ud, col_map, *w_blocks, dtype=torch.float32)
    B = x.shape[0]
    x, grad_y, grad_logdet = _a16(x.contiguous()), _a16(grad_y.contiguous()), grad_logdet.contiguous()
    cond24, acts, w_t, wfull_t = (_a16(t.contiguous()) for t in (cond24, acts, w_t, wfull_t))
    scratch, wb, wp, gp = _train_bwd_operands("coupling_train_bwd", B, num_blocks, w_blocks, dest, (), x.device)
    gx = torch.empty_like(x)
    L.call("nf_coupling_train_bwd", ptr(x), ptr(grad_y), ptr(grad_logdet), ptr(cond24), ptr(acts), ptr(w_t), ptr(blob),
           ptr(wfull_t), wp, ptr(uw.contiguous()), ptr(uh.contiguous()), ptr(ud.contiguous()), ptr(col_map), int(n_cols), ptr(gx),
           ptr(dest["w0"]), ptr(dest["b0"]), ptr(dest["wf"]), ptr(dest["bf"]), ptr(dest["uw"]), ptr(dest["uh"]), ptr(dest["ud"]),
           gp, ptr(scratch), mask_parity, B, 64, 128, num_blocks, 8, tail_bound, min_bin_width, min_bin_height, min_derivative,
           L.stream())
    return gx


# ---- bf16x3 (error-compensated split-bf16 MFMA) variant of the fused layer ----------------------------------------
def rqs_fused_x3_pack(f32_blob, num_blocks, has_lu, nI=32, nT=32, hidden=128, K=8):
    """Derive the split-bf16 weight blob from an rqs_fused_pack blob of the same layer (nf_rqs_fused_x3_pack)."""
    L.require_device(f32_blob, dtype=torch.float32)
    size = L.query("nf_rqs_fused_x3_pack_size", nI, nT, hidden, num_blocks, K)
    if size <= 0:
        raise NotImplementedError("nf_rqs_fused_x3: shape not supported")
    blob = torch.zeros((size + 3) // 4, dtype=torch.float32, device=f32_blob.device)
    L.call("nf_rqs_fused_x3_pack", ptr(blob), ptr(f32_blob), num_blocks, int(has_lu), L.stream())
    return blob


def rqs_fused_x3(x, blob, mask_parity, hidden, num_blocks, K, direction, logdet=None, acc=None, tail_bound=3.0,
                 min_bin_width=1e-3, min_bin_height=1e-3, min_derivative=1e-3, fuse_lu=False):
    return _rqs_fused_launch("nf_rqs_fused_x3", x, blob, mask_parity, hidden, num_blocks, K, direction, logdet, acc,
                             (tail_bound, min_bin_width, min_bin_height, min_derivative), fuse_lu)


def maf_affine(x, params, direction, logdet=None, acc=None, want_logdet=True):
    """affine/autoregressive.py:98-128.  params (B, D*2) or (B, D, 2).  direction 0 = forward, 1 = inverse."""
    L.require_device(x, params)
    x = x.contiguous()
    params = params.contiguous()
    B, D = x.shape
    y = torch.empty_like(x)
    logdet, acc = _ld_buffer(logdet, acc, B, x, want=want_logdet)
    L.call("nf_maf_affine", ptr(x), ptr(params), ptr(y), ptr(logdet), B, D, direction, acc or 0, L.dtype_code(x), L.stream())
    return y, logdet


def conv3x3_gather(x, flip=False, ld=None):
    """col (B H W, 9 C) of an NCHW float32 tensor: col[r][tap C + c] = x[b][c][y + dy][x + dx] (nf_conv3x3_gather); flip negates the
    offsets.  ld: row length of the returned buffer (>= 9 C; rows rounded up to 64: the layout the MADE training kernels' weight
    gradients read directly) -- columns beyond 9 C are not written, rows beyond B H W are zero."""
    L.require_device(x, dtype=torch.float32)
    if x.dtype != torch.float32 or x.dim() != 4:
        raise NotImplementedError("conv3x3_gather: (B, C, H, W) float32")
    B, C, H, W = x.shape
    if x.stride()[1:] != (H * W, W, 1) or x.stride(0) < C * H * W:       # (a channel split is read in place through its batch stride)
        x = x.contiguous()
    R = B * H * W
    if ld is None:
        col = torch.empty(R, 9 * C, dtype=x.dtype, device=x.device)
    else:
        Rp = (R + 63) // 64 * 64
        col = (torch.empty if Rp == R else torch.zeros)(Rp, ld, dtype=x.dtype, device=x.device)
    L.call("nf_conv3x3_gather", ptr_any(x), ptr(col), B, C, H, W, col.shape[1], 1 if flip else 0,
           x.stride(0) if B > 1 else C * H * W, L.stream())
    return col


def conv3x3_gather_sum(P, bias, shape, flip=False):
    """(B, C, H, W) from per-pixel tap products P (B H W, 9 C): out[b][c][y][x] = bias[c] + sum_tap P[(b, y + dy, x + dx)][tap C + c]
    (nf_conv3x3_gather_sum); flip negates the offsets."""
    L.require_device(P, bias, dtype=torch.float32)
    B, C, H, W = shape
    P = P.contiguous()
    if P.dtype != torch.float32 or P.dim() != 2 or P.shape[0] < B * H * W or P.shape[1] < 9 * C:
        raise ValueError("conv3x3_gather_sum: P must be (>= B H W, >= 9 C) float32")
    out = torch.empty(B, C, H, W, dtype=P.dtype, device=P.device)
    L.call("nf_conv3x3_gather_sum", ptr(P), _cptr(bias), ptr(out), B, C, H, W, P.shape[1], 1 if flip else 0, L.stream())
    return out


def channel_sum(g):
    """(C) = g (B, C, H, W).sum((0, 2, 3)) in one launch with a fixed summation order (nf_channel_sum)."""
    L.require_device(g, dtype=torch.float32)
    g = g.contiguous()
    if g.dtype != torch.float32 or g.dim() != 4:
        raise ValueError("channel_sum: a float32 (B, C, H, W) tensor")
    B, C, H, W = g.shape
    g = _a16(g, (H * W) % 4 == 0)
    out = torch.empty(C, dtype=g.dtype, device=g.device)
    L.call("nf_channel_sum", ptr(g), ptr(out), B, C, H * W, L.stream())
    return out


def maf_affine_bwd(x, params, gy, gld, direction):
    """Backward of maf_affine (nf_maf_affine_bwd): (g_x (B, D), g_params shaped like params); gy / gld may be None."""
    L.require_device(x, params)
    x = x.contiguous()
    params = params.contiguous()
    B, D = x.shape
    gx = torch.empty_like(x)
    gparams = torch.empty_like(params)
    gy = None if gy is None else gy.contiguous()
    gld = None if gld is None else gld.contiguous()
    L.call("nf_maf_affine_bwd", ptr(x), ptr(params), ptr(gy), ptr(gld), ptr(gx), ptr(gparams), B, D, direction, L.dtype_code(x),
           L.stream())
    return gx, gparams


def maf_implicit_sweep(x, params, gx, gld, gxm, v, gp, changed):
    """nf_maf_implicit_sweep: v, gp updated in place; `changed` (int32 scalar tensor) set when v moved."""
    L.require_device(x, params, gx, gld, gxm, v, gp, changed)
    B, D = x.shape
    L.call("nf_maf_implicit_sweep", ptr(x), ptr(params), ptr(gx), ptr(gld), ptr(gxm), ptr(v), ptr(gp), ptr(changed), B, D,
           L.dtype_code(x), L.stream())


def rqs_fused_chain(x, blobs, parities, hidden, num_blocks, K, direction, logdet=None, acc=None, tail_bound=3.0,
                    min_bin_width=1e-3, min_bin_height=1e-3, min_derivative=1e-3, fuse_lu=True, live_d=None):
    """Up to 64 fused layers of identical shape in ONE persistent launch (nf_rqs_fused_chain).  `blobs` / `parities`
    are in processing order."""
    return _rqs_fused_launch("nf_rqs_fused_chain", x, blobs, parities, hidden, num_blocks, K, direction, logdet,
                             acc, (tail_bound, min_bin_width, min_bin_height, min_derivative), fuse_lu, live_d, padded_rows=True)


def rqs_fused_x3_chain(x, blobs, parities, hidden, num_blocks, K, direction, logdet=None, acc=None, tail_bound=3.0,
                       min_bin_width=1e-3, min_bin_height=1e-3, min_derivative=1e-3, fuse_lu=True, live_d=None):
    """Up to 64 fused layers of identical shape on the split-bf16 matrix path in ONE persistent launch
    (nf_rqs_fused_x3_chain).  `blobs` (rqs_fused_x3_pack) / `parities` are in processing order."""
    return _rqs_fused_launch("nf_rqs_fused_x3_chain", x, blobs, parities, hidden, num_blocks, K, direction,
                             logdet, acc, (tail_bound, min_bin_width, min_bin_height, min_derivative), fuse_lu)


def nsf_wide_tables(uw, uh, ud, K, tail_bound, min_bin_width=1e-3, min_bin_height=1e-3, min_derivative=1e-3):
    """Knot tables (n_identity, 3 (K + 1)) of the batch-shared spline for nf_nsf_wide (nsf/coupling.py:170-259)."""
    L.require_device(uw, uh, ud, dtype=torch.float32)
    tabs = torch.empty(uw.shape[0], 3 * (K + 1), dtype=torch.float32, device=uw.device)
    L.call("nf_nsf_wide_tables", ptr(uw.contiguous()), ptr(uh.contiguous()), ptr(ud.contiguous()), ptr(tabs), uw.shape[0], K,
           float(tail_bound), min_bin_width, min_bin_height, min_derivative, L.stream())
    return tabs


def nsf_wide(x, blob, table, tabs, hidden_padded, direction, tail_bound, min_bin_width=1e-3, min_bin_height=1e-3,
             min_derivative=1e-3, logdet=None, acc=None, lu_logdet=None, K=8):
    """CoupledRationalQuadraticSpline beyond the benchmark kernel's shapes as one launch (nf_nsf_wide_k); blob / table from
    flows/nsf_wide_pack.pack_nsf_wide, tabs from nsf_wide_tables (both for K bins: 4 | 8 | 16); lu_logdet: device scalar of the
    LULinearPermute packed with it."""
    L.require_device(x, blob, table, tabs, lu_logdet, dtype=torch.float32)
    if x.dtype != torch.float32:
        raise NotImplementedError("nsf_wide: float32 only")
    B, D = x.shape
    x = _a16(x.contiguous(), D % 4 == 0)
    y = torch.empty_like(x)
    logdet, acc = _ld_buffer(logdet, acc, B, x)
    L.call("nf_nsf_wide_k", ptr(x), ptr(y), ptr(logdet), ptr(blob), ptr(table), ptr(tabs), ptr(lu_logdet), B, D, hidden_padded,
           int(K), direction, acc, float(tail_bound), min_bin_width, min_bin_height, min_derivative, L.stream())
    return y, logdet


def _context_rows(context):
    """(context, its row stride) as the conditional kernels read a (B, C) context: the row stride is passed as it is when the inner
    stride is 1 (0 for context.expand(B, C)), otherwise the context is made contiguous."""
    B, C_ = context.shape
    if context.stride(1) != 1 and C_ > 1:
        context = context.contiguous()
    return context, context.stride(0) if B > 1 else C_


def nsf_wide_ctx(x, context, blob, table, tabs, hidden_padded, direction, tail_bound, min_bin_width=1e-3, min_bin_height=1e-3,
                 min_derivative=1e-3, logdet=None, acc=None, K=8, table_host=None):
    """The conditional CoupledRationalQuadraticSpline as one launch (nf_nsf_wide_ctx); blob / table from
    flows/nsf_ctx_pack.pack_nsf_ctx (table_host: its host copy, checked against the context's width), tabs from nsf_wide_tables.
    context (B, C) float32: a row stride is passed as it is when the inner stride is 1 (0 for context.expand(B, C)), otherwise the
    context is made contiguous."""
    L.require_device(x, context, blob, table, tabs, dtype=torch.float32)
    if x.dtype != torch.float32:
        raise NotImplementedError("nsf_wide_ctx: float32 only")
    B, D = x.shape
    if context.dim() != 2 or context.shape[0] != B or context.dtype != torch.float32:
        raise ValueError("nsf_wide_ctx: context must be (%d, C) float32, got %s %s" % (B, tuple(context.shape), context.dtype))
    C_ = context.shape[1]
    if table_host is not None and (int(table_host[25]) != C_ or int(table_host[26]) != (C_ + 31) // 32 * 32):
        raise ValueError("nsf_wide_ctx: the pack is for %d context features, the context has %d" % (int(table_host[25]), C_))
    context, ldc = _context_rows(context)
    x = _a16(x.contiguous(), D % 4 == 0)
    y = torch.empty_like(x)
    logdet, acc = _ld_buffer(logdet, acc, B, x)
    L.call("nf_nsf_wide_ctx", ptr(x), ptr_any(context), ptr(y), ptr(logdet), ptr(blob), ptr(table), ptr(tabs), B, ldc, D, C_,
           hidden_padded, int(K), direction, acc, float(tail_bound), min_bin_width, min_bin_height, min_derivative, L.stream())
    return y, logdet


def nsf_wide_tables_ft(uw, uh, ud, tails_i, bound_i, K, min_bin_width=1e-3, min_bin_height=1e-3, min_derivative=1e-3):
    """Knot tables (n_identity, 3 (K + 1)) of the batch-shared spline under list tails for nf_nsf_wide_ft: derivatives
    (n_identity, K + 1), tails_i int32 / bound_i float32 (n_identity,) per identity feature (utils/splines.py:48-66)."""
    L.require_device(uw, uh, ud, tails_i, bound_i, dtype=torch.float32)
    nI = uw.shape[0]
    if tuple(ud.shape) != (nI, K + 1) or tails_i.numel() != nI or bound_i.numel() != nI:
        raise ValueError("nsf_wide_tables_ft: derivatives (%d, %d), tails_i and bound_i (%d,) expected" % (nI, K + 1, nI))
    tabs = torch.empty(nI, 3 * (K + 1), dtype=torch.float32, device=uw.device)
    L.call("nf_nsf_wide_tables_ft", ptr(uw.contiguous()), ptr(uh.contiguous()), ptr(ud.contiguous()), ptr(tails_i), ptr(bound_i),
           ptr(tabs), nI, K, min_bin_width, min_bin_height, min_derivative, L.stream())
    return tabs


def nsf_wide_ft(x, blob, table, ftable, tabs, hidden_padded, direction, min_bin_width=1e-3, min_bin_height=1e-3, min_derivative=1e-3,
                logdet=None, acc=None, K=8):
    """CircularCoupledRationalQuadraticSpline as one launch (nf_nsf_wide_ft); blob / table / ftable from
    flows/nsf_circ_pack.pack_nsf_circ (ftable (8, Dp): tails, bounds and periodic features by tile position), tabs from
    nsf_wide_tables_ft."""
    L.require_device(x, blob, table, ftable, tabs, dtype=torch.float32)
    if x.dtype != torch.float32:
        raise NotImplementedError("nsf_wide_ft: float32 only")
    B, D = x.shape
    x = _a16(x.contiguous(), D % 4 == 0)
    y = torch.empty_like(x)
    logdet, acc = _ld_buffer(logdet, acc, B, x)
    L.call("nf_nsf_wide_ft", ptr(x), ptr(y), ptr(logdet), ptr(blob), ptr(table), ptr(ftable), ptr(tabs), B, D, hidden_padded, int(K),
           direction, acc, min_bin_width, min_bin_height, min_derivative, L.stream())
    return y, logdet


def resnet_ctx_forward_train(x, context, blob, table, st):
    """The GLU-gated ResidualNet under autograd (nf_resnet_ctx_forward_train): (out (B, O), save) -- save holds what
    resnet_ctx_backward / resnet_ctx_wgrad read.  st: flows/ctx_train_pack.structure; context (B, C) float32 with unit inner stride
    is passed with its row stride (0 for context.expand(B, C))."""
    L.require_device(x, context, blob, table, dtype=torch.float32)
    if x.dtype != torch.float32 or context.dtype != torch.float32:
        raise NotImplementedError("resnet_ctx_forward_train: float32 only")
    B = x.shape[0]
    if x.dim() != 2 or x.shape[1] != st["nI"] or context.dim() != 2 or tuple(context.shape) != (B, st["C"]):
        raise ValueError("resnet_ctx_forward_train: x (%d, %d) and context (%d, %d) expected, got %s %s"
                         % (B, st["nI"], B, st["C"], tuple(x.shape), tuple(context.shape)))
    context, ldc = _context_rows(context)
    x = x.contiguous()
    out = torch.empty(B, st["O"], dtype=x.dtype, device=x.device)
    n = L.size("nf_resnet_ctx_save_floats", B, st["nI"], st["C"], st["H"], st["NB"])
    save = torch.empty(max(n, 1), dtype=x.dtype, device=x.device)
    L.call("nf_resnet_ctx_forward_train", ptr(x), st["nI"], ptr_any(context), ldc, ptr(out), ptr(save), ptr(blob), ptr(table), B,
           st["nI"], st["C"], st["H"], st["O"], st["NB"], L.stream())
    return out, save


def resnet_ctx_backward(g_out, save, blob, table, st):
    """Input-gradient chain of the gated ResidualNet (nf_resnet_ctx_backward): (g_x (B, nI), g_context (B, C), G) -- G holds every
    layer's output gradient for resnet_ctx_wgrad."""
    L.require_device(g_out, save, blob, table, dtype=torch.float32)
    B = g_out.shape[0]
    g_out = g_out.contiguous()
    n = L.size("nf_resnet_ctx_grad_floats", B, st["H"], st["NB"])
    G = torch.empty(max(n, 1), dtype=g_out.dtype, device=g_out.device)
    gx = torch.empty(B, st["nI"], dtype=g_out.dtype, device=g_out.device)
    gc = torch.empty(B, st["C"], dtype=g_out.dtype, device=g_out.device)
    L.call("nf_resnet_ctx_backward", ptr(g_out), ptr(save), ptr(G), ptr(gx), ptr(gc), ptr(blob), ptr(table), B, st["nI"], st["C"],
           st["H"], st["O"], st["NB"], L.stream())
    return gx, gc, G


def resnet_ctx_wgrad(g_out, save, G, table, jobs, st):
    """Every weight / bias gradient of the gated ResidualNet (nf_resnet_ctx_wgrad: one launch over 64 x 64 tiles and row chunks + a
    fixed-order reduction): the flat buffer in the parameter order of flows/ctx_train_pack.params_of."""
    L.require_device(g_out, save, G, table, jobs, dtype=torch.float32)
    B = g_out.shape[0]
    g_out = g_out.contiguous()
    if B == 0:                  # (nothing to reduce: the kernels launch nothing, the gradients are zero)
        return torch.zeros(st["nflat"], dtype=g_out.dtype, device=g_out.device)
    njobs = int(jobs.shape[0])
    n = L.size("nf_resnet_ctx_scratch_floats", B, njobs)
    part = torch.empty(max(n, 1), dtype=g_out.dtype, device=g_out.device)
    grads = torch.empty(st["nflat"], dtype=g_out.dtype, device=g_out.device)
    L.call("nf_resnet_ctx_wgrad", ptr(g_out), ptr(save), ptr(G), ptr(grads), ptr(part), ptr(jobs), njobs, ptr(table), B, st["H"],
           st["NB"], L.stream())
    return grads


def made_forward_affine(x, blob, table, hidden_padded, logdet=None, acc=None):
    """MaskedAffineAutoregressive.forward (autoregressive.py:24-27, :101-110 over nets/made.py:296-304) as one launch
    (nf_made_forward_affine); blob / table from flows/made_pack.pack_made_forward."""
    L.require_device(x, blob, table, dtype=torch.float32)
    if x.dtype != torch.float32:
        raise NotImplementedError("made_forward_affine: float32 only")
    B, D = x.shape
    x = _a16(x.contiguous(), D % 4 == 0)
    y = torch.empty_like(x)
    logdet, acc = _ld_buffer(logdet, acc, B, x)
    L.call("nf_made_forward_affine", ptr(x), ptr(y), ptr(logdet), ptr(blob), ptr(table), B, D, hidden_padded, acc, L.stream())
    return y, logdet


def affine_wide(z, blob, table, hidden_padded, direction, logdet=None, acc=None):
    """A MaskedAffineFlow(MLP, MLP) / AffineCouplingBlock(MLP) beyond the chain kernel's shapes (coupling.py:117-171, :209-229,
    :232-267 over nets/mlp.py:5-58) as one launch (nf_affine_wide); blob / table from flows/affine_wide_pack.pack."""
    L.require_device(z, blob, table, logdet, dtype=torch.float32)
    if z.dtype != torch.float32:
        raise NotImplementedError("affine_wide: float32 only")
    B, D = z.shape
    z = _a16(z.contiguous(), D % 4 == 0)
    y = torch.empty_like(z)
    logdet, acc = _ld_buffer(logdet, acc, B, z)
    L.call("nf_affine_wide", ptr(z), ptr(y), ptr(logdet), ptr(blob), ptr(table), B, D, hidden_padded, direction, acc, L.stream())
    return y, logdet


def affine_wide_apply(z, P, modes, smap, nets, direction):
    """The coupling map of a wide RealNVP layer on the raw conditioner output P (B, >= 2 D: 2 f / 2 f + 1 = feature f's scale / shift
    parameter; coupling.py:209-229, :117-171) -- nf_affine_wide_apply: (y (B, D), log-det (B)), written.  modes: the int32 words of
    flows/affine_wide_pack.mode_words; smap: _lib.SCALE code or 4 (masked); nets: bit 0 = s, bit 1 = t."""
    L.require_device(z, P, modes, dtype=torch.float32)
    B, D = z.shape
    if P.dim() != 2 or P.shape[0] < B or P.shape[1] < 2 * D or modes.dtype != torch.int32 or modes.numel() < (D + 15) // 16:
        raise ValueError("affine_wide_apply: P is (>= B, >= 2 D), modes one int32 word per 16 features")
    z = _a16(z.contiguous(), D % 4 == 0)
    P = P.contiguous()
    y = torch.empty_like(z)
    ld = torch.empty(B, dtype=z.dtype, device=z.device)
    L.call("nf_affine_wide_apply", ptr(z), ptr(P), ptr(modes), ptr(y), ptr(ld), B, D, P.shape[1], smap, nets, direction, L.stream())
    return y, ld


def affine_wide_apply_bwd(z, P, gy, gld, modes, smap, nets, direction, rows_padded, ld_out):
    """The backward of affine_wide_apply (nf_affine_wide_apply_bwd): (gz (B, D) through the element-wise map only, gP (rows_padded,
    ld_out): the conditioner output's gradient in the padded shape made_backward / made_wgrad take as g_params, zeros in the padding).
    gy / gld may be None (zeros; no tensor is built)."""
    L.require_device(z, P, gy, gld, modes, dtype=torch.float32)
    B, D = z.shape
    if P.dim() != 2 or P.shape[0] < B or P.shape[1] < 2 * D or modes.dtype != torch.int32 or modes.numel() < (D + 15) // 16:
        raise ValueError("affine_wide_apply_bwd: P is (>= B, >= 2 D), modes one int32 word per 16 features")
    L.check_count("affine_wide_apply_bwd", "gy", gy, B * D, "B D")
    L.check_count("affine_wide_apply_bwd", "gld", gld, B, "B")
    z = _a16(z.contiguous(), D % 4 == 0)
    P = P.contiguous()
    gy = None if gy is None else _a16(gy.contiguous(), D % 4 == 0)
    gld = None if gld is None else gld.contiguous()
    gz = torch.empty_like(z)
    gP = torch.empty(rows_padded, ld_out, dtype=z.dtype, device=z.device)
    L.call("nf_affine_wide_apply_bwd", ptr(z), ptr(P), ptr(gy), ptr(gld), ptr(modes), ptr(gz), ptr(gP), B, rows_padded, D, P.shape[1],
           ld_out, smap, nets, direction, L.stream())
    return gz, gP


def made_forward_spline(x, blob, table, hidden_padded, tail_bound, min_bin_width=1e-3, min_bin_height=1e-3, min_derivative=1e-3,
                        logdet=None, acc=None):
    """neural_spline/autoregressive.py:94-134 density direction (MADE + 8-bin spline with linear tails) as one launch
    (nf_made_forward_spline); blob / table from flows/made_pack.pack_made_forward(made, 23, spline=True)."""
    L.require_device(x, blob, table, dtype=torch.float32)
    if x.dtype != torch.float32:
        raise NotImplementedError("made_forward_spline: float32 only")
    B, D = x.shape
    x = _a16(x.contiguous(), D % 4 == 0)
    y = torch.empty_like(x)
    logdet, acc = _ld_buffer(logdet, acc, B, x)
    L.call("nf_made_forward_spline", ptr(x), ptr(y), ptr(logdet), ptr(blob), ptr(table), B, D, hidden_padded, acc,
           float(tail_bound), min_bin_width, min_bin_height, min_derivative, L.stream())
    return y, logdet


def made_forward_spline_ft(x, blob, table, ftable, hidden_padded, K, tails, min_bin_width=1e-3, min_bin_height=1e-3,
                           min_derivative=1e-3, logdet=None, acc=None):
    """made_forward_spline with a per-feature table (nf_made_forward_spline_ft): the density direction of the layers arnsf_inverse_ft
    samples -- permuted masks, per-feature tails ("feature") and bounds, the periodic preprocessing of circular coordinates
    (neural_spline/autoregressive.py:44-55, :94-134; utils/splines.py:48-66; utils/nn.py:64-129); blob / table / ftable from
    flows/made_pack.pack_made_forward_ft."""
    L.require_device(x, blob, table, ftable, dtype=torch.float32)
    if x.dtype != torch.float32:
        raise NotImplementedError("made_forward_spline_ft: float32 only")
    B, D = x.shape
    if ftable.dtype != torch.float32 or tuple(ftable.shape) != (8, D):
        raise ValueError("made_forward_spline_ft: ftable is the (8, D) float32 table of flows/maf_pack.py")
    x = x.contiguous()
    y = torch.empty_like(x)
    logdet, acc = _ld_buffer(logdet, acc, B, x)
    L.call("nf_made_forward_spline_ft", ptr(x), ptr(y), ptr(logdet), ptr(blob), ptr(table), ptr(ftable), B, D, hidden_padded, K,
           3 if tails == "feature" else L.TAILS[tails], min_bin_width, min_bin_height, min_derivative, acc, L.stream())
    return y, logdet


def made_forward(x, blob, table, hidden_padded, mult):
    """MADE.forward (nets/made.py:296-304) as one launch (nf_made_forward): (B, mult D) parameters."""
    L.require_device(x, blob, table, dtype=torch.float32)
    if x.dtype != torch.float32:
        raise NotImplementedError("made_forward: float32 only")
    B, D = x.shape
    x = _a16(x.contiguous(), D % 4 == 0)
    params = torch.empty(B, mult * D, dtype=x.dtype, device=x.device)
    L.call("nf_made_forward", ptr(x), ptr(params), ptr(blob), ptr(table), B, D, hidden_padded, mult, L.stream())
    return params


_ZERO1 = {}


def pack_gather(params, src):
    """The packed weight streams from the current parameters (nf_pack_gather): flat = [0, params flattened ...], out = flat[src]."""
    L.require_device(src, *params, dtype=torch.float32)
    zero = _ZERO1.get(src.device)
    if zero is None:
        zero = _ZERO1[src.device] = torch.zeros(1, dtype=torch.float32, device=src.device)
    out = torch.empty(src.numel(), dtype=torch.float32, device=src.device)
    if len(params) <= 16 and all(p.dtype == torch.float32 and p.is_contiguous() for p in params):
        # round 6: straight from the parameter tensors (no torch.cat per module and step)
        pp = _ptr_array(params)
        nn_ = (C.c_int64 * len(params))(*[p.numel() for p in params])
        L.call("nf_pack_gather_multi", pp, nn_, len(params), ptr(src), ptr(out), src.numel(), L.stream())
        return out
    flat = torch.cat([zero] + [p.detach().reshape(-1) for p in params])
    L.call("nf_pack_gather", ptr(flat), ptr(src), ptr(out), src.numel(), L.stream())
    return out


def pack_gather_batch(param_lists, src):
    """nf_pack_gather_batch: [flat_m[src]] for modules m of ONE structure (param_lists[m] = its <= 8 contiguous float32 parameter
    tensors, the same shapes for every module) -- one launch per 32 modules."""
    L.require_device(src, *[p for pl in param_lists for p in pl], dtype=torch.float32)
    n_mod, n_par = len(param_lists), len(param_lists[0])
    if n_par > 8 or any(len(pl) != n_par for pl in param_lists):
        raise NotImplementedError("pack_gather_batch: <= 8 parameters per module, the same number for all")
    shapes = [tuple(p.shape) for p in param_lists[0]]
    for pl in param_lists:
        if [tuple(p.shape) for p in pl] != shapes or any(p.dtype != torch.float32 or not p.is_contiguous() for p in pl):
            raise NotImplementedError("pack_gather_batch: contiguous float32 parameters of one structure")
    out = torch.empty(n_mod, src.numel(), dtype=torch.float32, device=src.device)
    outs = list(out.unbind(0))
    pp = _ptr_array([p for pl in param_lists for p in pl])
    nn_ = (C.c_int64 * n_par)(*[p.numel() for p in param_lists[0]])
    L.call("nf_pack_gather_batch", pp, nn_, n_par, ptr(src), _ptr_array(outs), src.numel(), n_mod, L.stream())
    return outs


def made_forward_train(x, blob, table, hidden_padded, out_features, num_blocks, rows=None, features=None):
    """MADE.forward / ResidualNet.forward under autograd (nf_made_forward_train): (params (B, out_features), save (2 NB + 1, Bp, Hp)
    pre-activations, bits (Bp / 64, 2 NB, 2, 512) ReLU signs), Bp = B rounded up to 64 -- the operands of made_backward / made_wgrad.
    out_features = mult D for a MADE (the table's hdr[12])."""
    L.require_device(x, blob, table, dtype=torch.float32)
    if x.dtype != torch.float32:
        raise NotImplementedError("made_forward_train: float32 only")
    B, D = x.shape
    if rows is not None:           # x is a padded buffer (rows >= B, row stride in the table's hdr[14]): the conv path
        B, D = rows, features
    x = _a16(x.contiguous(), D % 4 == 0)
    Bp = (B + 63) // 64 * 64
    params = torch.empty(B, out_features, dtype=x.dtype, device=x.device)
    save = torch.empty(2 * num_blocks + 1, Bp, hidden_padded, dtype=x.dtype, device=x.device)
    bits = torch.empty(max(Bp // 64, 1), 2 * num_blocks, 2, 512, dtype=torch.int32, device=x.device)
    L.call("nf_made_forward_train", ptr(x), ptr(params), ptr(save), ptr(bits), ptr(blob), ptr(table), B, D, hidden_padded,
           max(1, out_features // D), L.stream())
    return params, save, bits


def made_forward_train_ft(x, blob, table, hidden_padded, out_features, num_blocks):
    """made_forward_train for the degree-order packs of flows/made_pack.made_train_structure_ft (nf_made_forward_train_ft: the tile is
    gathered through the feature table behind `table` and fed with the periodic features whose live parameters end `blob`): (params
    (B, out_features) in position order, save, bits, x_pad (Bp, 128): the fed inputs as made_wgrad takes them, x_pos (B, D): the raw
    inputs in position order).  64-row tiles: its chain is made_backward(..., tile64=True)."""
    L.require_device(x, blob, table, dtype=torch.float32)
    if x.dtype != torch.float32:
        raise NotImplementedError("made_forward_train_ft: float32 only")
    B, D = x.shape
    x = x.contiguous()
    Bp = (B + 63) // 64 * 64
    params = torch.empty(B, out_features, dtype=x.dtype, device=x.device)
    save = torch.empty(2 * num_blocks + 1, Bp, hidden_padded, dtype=x.dtype, device=x.device)
    bits = torch.empty(max(Bp // 64, 1), 2 * num_blocks, 2, 512, dtype=torch.int32, device=x.device)
    x_pad = torch.empty(Bp, 128, dtype=x.dtype, device=x.device)
    x_pos = torch.empty(B, D, dtype=x.dtype, device=x.device)
    L.call("nf_made_forward_train_ft", ptr(x), ptr(params), ptr(save), ptr(bits), ptr(x_pad), ptr(x_pos), ptr(blob), ptr(table), B, D,
           hidden_padded, max(1, out_features // D), L.stream())
    return params, save, bits, x_pad, x_pos


def made_feed_ft_bwd(g_pre, g_xpos, x, ttable, feed, n_circ, has_bias):
    """The backward of made_forward_train_ft's gather + periodic feed (nf_made_feed_ft_bwd): (g_x (B, D) in column order =
    g_pre d + g_xpos scattered through the table, g_weights (n_circ, 2), g_bias (n_circ) or None); g_xpos may be None.  Deterministic:
    per-workgroup partials, fixed-order reduction."""
    L.require_device(g_pre, g_xpos, x, ttable, feed, dtype=torch.float32)
    B, D = x.shape
    g_pre = g_pre.contiguous()
    g_xpos = None if g_xpos is None else g_xpos.contiguous()
    g_x = torch.empty(B, D, dtype=x.dtype, device=x.device)
    g_w = torch.zeros(n_circ, 2, dtype=x.dtype, device=x.device) if n_circ else None
    g_b = torch.zeros(n_circ, dtype=x.dtype, device=x.device) if (n_circ and has_bias) else None
    part = torch.empty(512 * 3 * n_circ, dtype=x.dtype, device=x.device) if n_circ else None
    L.call("nf_made_feed_ft_bwd", ptr(g_pre), ptr(g_xpos), ptr(x), ptr(ttable), ptr(feed), ptr(g_x), ptr(g_w), ptr(g_b), ptr(part),
           B, D, n_circ, L.stream())
    return g_x, g_w, g_b


def made_backward(g_params, bits, blob, table, D, hidden_padded, num_blocks, rows=None, out_features=None, ld_out=None, want_G=True,
                  tile64=False):
    """The input-gradient chain of MADE (nf_made_backward): g_x (B, D) and every layer's output gradient G (2 NB + 1, Bp, Hp).
    rows / out_features / ld_out: g_params is a padded buffer (row strides in the table's hdr[14], hdr[15]) and so is the returned
    g_x (rows, ld_out): the conv path.  tile64: nf_made_backward_t64 (the chain of made_forward_train_ft, which has no 128-row tile)."""
    L.require_device(g_params, bits, blob, table, dtype=torch.float32)
    B = g_params.shape[0] if rows is None else rows
    md = g_params.shape[1] if out_features is None else out_features
    g_params = _a16(g_params.contiguous())
    Bp = (B + 63) // 64 * 64
    gx = torch.empty(B, D if ld_out is None else ld_out, dtype=g_params.dtype, device=g_params.device)
    G = torch.empty(2 * num_blocks + 1, Bp, hidden_padded, dtype=g_params.dtype, device=g_params.device) if want_G else None
    L.call("nf_made_backward_t64" if tile64 else "nf_made_backward", ptr(g_params), ptr(bits), ptr(gx), ptr(G), ptr(blob), ptr(table),
           B, D, hidden_padded, max(1, md // D), L.stream())
    return gx, G


def _pad_rows_cols(t, rows, cols):
    if t.shape[0] == rows and t.shape[1] == cols:
        return _a16(t.contiguous())
    return torch.nn.functional.pad(t, (0, cols - t.shape[1], 0, rows - t.shape[0])).contiguous()


def _made_wgrad_operands(g_params, x, Bp, Mp, Dx, nflat, B, ntiles):
    """(g_params padded to (Bp, Mp), x padded to (Bp, Dx), the zeroed flat gradient, the partial-sum scratch) of nf_made_wgrad[_pos]."""
    grads = torch.zeros(nflat, dtype=torch.float32, device=x.device)
    part = torch.empty(max(L.size("nf_made_wgrad_scratch_floats", B, ntiles), 1), dtype=torch.float32, device=x.device)
    return _pad_rows_cols(g_params, Bp, Mp), _pad_rows_cols(x, Bp, Dx), grads, part


def made_wgrad(g_params, x, G, save, wtable, stable, mask, ntiles, nflat, Mp, Dx, rows=None):
    """Every weight / bias gradient of the MADE (nf_made_wgrad): the flat vector in flows/made_pack.pack_made_backward's layout,
    masked entries zero."""
    L.require_device(g_params, x, G, save, wtable, stable, mask, dtype=torch.float32)
    B = g_params.shape[0] if rows is None else rows          # (rows: the operands are already padded buffers)
    Bp = G.shape[1]
    gp_pad, x_pad, grads, part = _made_wgrad_operands(g_params, x, Bp, Mp, Dx, nflat, B, ntiles)
    L.call("nf_made_wgrad", ptr(gp_pad), ptr(x_pad), ptr(_a16(G)), ptr(_a16(save)), ptr(grads), ptr(mask), ptr(part), ptr(wtable),
           ptr(stable), ntiles, B, L.stream())
    return grads


def made_wgrad_pos(g_params, x, gscratch, fscratch, wtable, stable, mask, ntiles, nflat, Mp, Dx, num_layers, positions):
    """nf_made_wgrad_pos (round 6): nf_made_wgrad with the hidden operands read from the one-pass kernels' scratches in place --
    gscratch from maf_solve_t(return_scratch=True), fscratch from maf_inverse_bits(return_scratch=True); tables from
    flows/maf_pack.position_wgrad_tables; mask / nflat / Mp / Dx of the MADE's ordinary backward pack (same flat layout).  The batch must
    be a multiple of 64 rows."""
    L.require_device(g_params, x, gscratch, fscratch, wtable, stable, mask, dtype=torch.float32)
    B = g_params.shape[0]
    if B % 64:
        raise NotImplementedError("made_wgrad_pos: a multiple of 64 rows")
    gp_pad, x_pad, grads, part = _made_wgrad_operands(g_params, x, B, Mp, Dx, nflat, B, ntiles)
    L.call("nf_made_wgrad_pos", ptr(gp_pad), ptr(x_pad), ptr(_a16(gscratch)), ptr(_a16(fscratch)), ptr(grads), ptr(mask), ptr(part),
           ptr(wtable), ptr(stable), ntiles, B, num_layers, positions, L.stream())
    return grads


def _host_table(table_host):
    """The host copy of a format-1 table as the contiguous int32 array the *_tri entry points read (keep it alive through the call)."""
    import numpy as np
    return np.ascontiguousarray(table_host, dtype=np.int32)


def maf_inverse(z, blob, table, hidden_padded, logdet=None, acc=None, num_blocks=2, table_host=None):
    """autoregressive.py:29-38 + :114-128 in one pass; blob/table from flows/maf_pack.pack_made.  config.maf_halves (default):
    nf_maf_inverse_h (32 samples per wave, 1..3 residual blocks); otherwise round 2's nf_maf_inverse (two blocks only).
    `table_host`: the host (numpy int32) copy of a FORMAT-1 table (pack_made(tri=True)) -> nf_maf_inverse_h_tri; a format-1 pack
    must come with it (the format-0 entry points cannot read its regular tiles)."""
    L.require_device(z, blob, table, dtype=torch.float32)
    if z.dtype != torch.float32:
        raise NotImplementedError("maf_inverse: float32 only")
    from . import config
    B, D = z.shape
    z = z.contiguous()
    y = torch.empty_like(z)
    logdet, acc = _ld_buffer(logdet, acc, B, z)
    if table_host is not None:
        th = _host_table(table_host)
        if int(th[7]) != 1:
            raise ValueError("maf_inverse: table_host is given for format-1 packs only")
        scratch = _scratch("nf_maf_inverse_h_scratch_floats", z.device, B, D, hidden_padded, num_blocks)
        L.call("nf_maf_inverse_h_tri", ptr(z), ptr(y), ptr(logdet), ptr(blob), ptr(table), th.ctypes.data, ptr(scratch), B, D,
               hidden_padded, num_blocks, acc, L.stream())
        return y, logdet
    if config.maf_halves or num_blocks != 2:
        scratch = _scratch("nf_maf_inverse_h_scratch_floats", z.device, B, D, hidden_padded, num_blocks)
        L.call("nf_maf_inverse_h", ptr(z), ptr(y), ptr(logdet), ptr(blob), ptr(table), ptr(scratch), B, D, hidden_padded,
               num_blocks, acc, L.stream())
        return y, logdet
    scratch = _scratch("nf_maf_inverse_scratch_floats", z.device, B, D, hidden_padded)
    L.call("nf_maf_inverse", ptr(z), ptr(y), ptr(logdet), ptr(blob), ptr(table), ptr(scratch), B, D, hidden_padded, acc,
           L.stream())
    return y, logdet


def maf_inverse_bits(z, blob, table, hidden_padded, num_blocks, tiles, table_host=None, return_scratch=False, want_params=False):
    """nf_maf_inverse_h_bits / nf_maf_inverse_h_tri_bits (table_host = the host copy of a format-1 table): the one-pass inverse that also
    leaves the pass's ReLU masks (uint32 words per 32-row wave, tile and lane, in the pack's positions) for maf_solve_t on a
    transposed pack of the same format.  Returns (y, logdet, bits [, scratch]); want_params (round 6, nf_maf_inverse_h_train): MADE's
    output at the solution, (B, 2 D), is appended."""
    L.require_device(z, blob, table, dtype=torch.float32)
    if z.dtype != torch.float32:
        raise NotImplementedError("maf_inverse_bits: float32 only")
    B, D = z.shape
    z = z.contiguous()
    y = torch.empty_like(z)
    logdet = torch.empty(B, dtype=z.dtype, device=z.device)
    scratch = _scratch("nf_maf_inverse_h_scratch_floats", z.device, B, D, hidden_padded, num_blocks)
    bits = torch.empty(max((B + 31) // 32 * tiles * 64 * num_blocks, 1), dtype=torch.int32, device=z.device)
    if want_params:
        prm = torch.empty(B, 2 * D, dtype=torch.float32, device=z.device)
        th = None if table_host is None else _host_table(table_host)
        L.call("nf_maf_inverse_h_train", ptr(z), ptr(y), ptr(logdet), ptr(blob), ptr(table),
               None if th is None else th.ctypes.data, ptr(scratch), ptr(bits), ptr(prm), B, D, hidden_padded, num_blocks,
               L.LD_WRITE, L.stream())
        return (y, logdet, bits, scratch, prm) if return_scratch else (y, logdet, bits, prm)
    if table_host is not None:
        th = _host_table(table_host)
        L.call("nf_maf_inverse_h_tri_bits", ptr(z), ptr(y), ptr(logdet), ptr(blob), ptr(table), th.ctypes.data, ptr(scratch),
               ptr(bits), B, D, hidden_padded, num_blocks, L.LD_WRITE, L.stream())
        return (y, logdet, bits, scratch) if return_scratch else (y, logdet, bits)
    L.call("nf_maf_inverse_h_bits", ptr(z), ptr(y), ptr(logdet), ptr(blob), ptr(table), ptr(scratch), ptr(bits), B, D,
           hidden_padded, num_blocks, L.LD_WRITE, L.stream())
    return (y, logdet, bits, scratch) if return_scratch else (y, logdet, bits)


def maf_solve_t(x, params, gx, gld, bits, blob, table, hidden_padded, num_blocks, return_scratch=False, table_host=None):
    """nf_maf_solve_t: v with  v s + J^T g_p(v, g_ld) = g_x  in one pass (the implicit backward of the MAF inverse);
    blob / table from flows/maf_pack.pack_made_transposed.  return_scratch: (v, scratch) -- the activation scratch for
    maf_scratch_rows."""
    L.require_device(x, params, gx, gld, bits, blob, table, dtype=torch.float32)
    if x.dtype != torch.float32:
        raise NotImplementedError("maf_solve_t: float32 only")
    B, D = x.shape
    x, params, gx = x.contiguous(), params.contiguous(), gx.contiguous()
    v = torch.empty_like(x)
    scratch = _scratch("nf_maf_solve_t_scratch_floats", x.device, B, D, hidden_padded, num_blocks)
    from . import config
    if table_host is not None and config.maf_solve_fast:      # round 6: the regular-8 tiles on the statically unrolled sequential part
        th = _host_table(table_host)
        L.call("nf_maf_solve_t_tri", ptr(x), ptr(params), ptr(gx), _cptr(gld), ptr(bits), ptr(v), ptr(blob), ptr(table),
               th.ctypes.data, ptr(scratch), B, D, hidden_padded, num_blocks, L.stream())
        return (v, scratch) if return_scratch else v
    L.call("nf_maf_solve_t", ptr(x), ptr(params), ptr(gx), _cptr(gld), ptr(bits), ptr(v), ptr(blob), ptr(table), ptr(scratch), B,
           D, hidden_padded, num_blocks, L.stream())
    return (v, scratch) if return_scratch else v


def maf_scratch_rows(scratch, pos_of_col, B, num_blocks, hidden_padded, sign=1.0, reverse_layers=False):
    """nf_maf_scratch_rows: the one-pass kernels' activation scratch as (2 num_blocks + 1, Bp, len(pos_of_col)) row-major tensors."""
    L.require_device(scratch, pos_of_col, dtype=torch.float32)
    ldo = pos_of_col.numel()
    Bp = (B + 63) // 64 * 64
    out = torch.empty(2 * num_blocks + 1, Bp, ldo, dtype=torch.float32, device=scratch.device)
    L.call("nf_maf_scratch_rows", ptr(scratch), ptr(pos_of_col), ptr(out), B, num_blocks, hidden_padded, ldo, sign,
           int(reverse_layers), L.stream())
    return out


def maf_scratch_layer(scratch, pos_of_col, B, num_blocks, hidden_padded, layer):
    """nf_maf_scratch_layer: ONE layer of a one-pass kernel's activation scratch as a (Bp, len(pos_of_col)) row-major tensor."""
    L.require_device(scratch, pos_of_col, dtype=torch.float32)
    ldo = pos_of_col.numel()
    Bp = (B + 63) // 64 * 64
    out = torch.empty(Bp, ldo, dtype=torch.float32, device=scratch.device)
    L.call("nf_maf_scratch_layer", ptr(scratch), ptr(pos_of_col), ptr(out), B, num_blocks, hidden_padded, ldo, layer, L.stream())
    return out


def arnsf_inverse(z, blob, table, hidden_padded, K, tails, tail_bound, min_bin_width=1e-3, min_bin_height=1e-3,
                  min_derivative=1e-3, logdet=None, acc=None):
    """neural_spline/autoregressive.py:94-134 inverse over affine/autoregressive.py:29-38 in one pass
    (nf_arnsf_inverse); blob/table from flows/maf_pack.pack_made(made, mult, rows=True)."""
    L.require_device(z, blob, table, dtype=torch.float32)
    if z.dtype != torch.float32:
        raise NotImplementedError("arnsf_inverse: float32 only")
    B, D = z.shape
    z = z.contiguous()
    y = torch.empty_like(z)
    logdet, acc = _ld_buffer(logdet, acc, B, z)
    scratch = _scratch("nf_maf_inverse_scratch_floats", z.device, B, D, hidden_padded)
    L.call("nf_arnsf_inverse", ptr(z), ptr(y), ptr(logdet), ptr(blob), ptr(table), ptr(scratch), B, D, hidden_padded, K,
           L.TAILS[tails], tail_bound, min_bin_width, min_bin_height, min_derivative, acc, L.stream())
    return y, logdet


def arnsf_inverse_ft(z, blob, table, ftable, hidden_padded, K, tails, min_bin_width=1e-3, min_bin_height=1e-3, min_derivative=1e-3,
                     logdet=None, acc=None):
    """arnsf_inverse with a per-feature table (nf_arnsf_inverse_ft): permuted masks, per-feature tails ("feature") and bounds and the
    periodic preprocessing of circular coordinates (neural_spline/autoregressive.py:44-55, :94-134; utils/splines.py:48-66;
    utils/nn.py:64-129); blob/table/ftable from flows/maf_pack.pack_made(made, mult, rows=True, features=(tails, tail_bound))."""
    L.require_device(z, blob, table, ftable, dtype=torch.float32)
    if z.dtype != torch.float32:
        raise NotImplementedError("arnsf_inverse_ft: float32 only")
    B, D = z.shape
    if ftable.dtype != torch.float32 or tuple(ftable.shape) != (8, D):
        raise ValueError("arnsf_inverse_ft: ftable is the (8, D) float32 table of flows/maf_pack.py")
    z = z.contiguous()
    y = torch.empty_like(z)
    logdet, acc = _ld_buffer(logdet, acc, B, z)
    scratch = _scratch("nf_maf_inverse_scratch_floats", z.device, B, D, hidden_padded)
    L.call("nf_arnsf_inverse_ft", ptr(z), ptr(y), ptr(logdet), ptr(blob), ptr(table), ptr(ftable), ptr(scratch), B, D, hidden_padded,
           K, 3 if tails == "feature" else L.TAILS[tails], min_bin_width, min_bin_height, min_derivative, acc, L.stream())
    return y, logdet


GLOW_CONV_WIDE, GLOW_CONV_SMALL, GLOW_CONV_TINY = 0, 1, 2


def glow_convnet_layout(B, H, W):
    """Which nf_glow_convnet kernel takes (B, *, H, W) inputs: GLOW_CONV_WIDE, _SMALL, _TINY or None."""
    code = L.query("nf_glow_convnet_layout", B, H, W)
    return code if code >= 0 else None


def glow_convnet_pack(w1, b1, w2, b2, w3, b3, layout=GLOW_CONV_WIDE):
    """Packed weights of a GlowBlock conditioner for glow_convnet (nf_glow_convnet_pack); None for unsupported shapes."""
    L.require_device(w1, b1, w2, b2, w3, b3, dtype=torch.float32)
    Cin, Cout, hidden = w1.shape[1], w3.shape[0], w1.shape[0]
    size = L.query("nf_glow_convnet_pack_size", Cin, Cout, hidden)
    if size <= 0 or (layout == GLOW_CONV_SMALL and Cout > 48):
        return None
    blob = torch.empty(size // 4, dtype=torch.float32, device=w1.device)
    L.call("nf_glow_convnet_pack", ptr(blob), ptr(w1.contiguous()), ptr(b1.contiguous()), ptr(w2.contiguous()),
           ptr(b2.contiguous()), ptr(w3.contiguous()), ptr(b3.contiguous()), Cin, Cout, hidden, layout, L.stream())
    return blob


def glow_convnet(x, blob, Cout, slope, layout=GLOW_CONV_WIDE, hidden=256):
    """cnn.py:5-63 for the GlowBlock network in one launch (nf_glow_convnet).  x: (B, Cin, H, W), possibly a channel
    slice of a contiguous NCHW tensor (planes contiguous, arbitrary image stride); blob packed for the same layout."""
    L.require_device(x, blob, dtype=torch.float32)
    B, Cin, H, W = x.shape
    if x.dtype != torch.float32 or x.stride(3) != 1 or x.stride(2) != W or x.stride(1) != H * W:
        raise NotImplementedError("glow_convnet: float32 with contiguous (H, W) planes")
    out = torch.empty(B, Cout, H, W, dtype=x.dtype, device=x.device)
    L.call("nf_glow_convnet", ptr_any(x), x.stride(0) if B > 1 else Cin * H * W, ptr(out), ptr(blob), B, Cin, H, W, Cout, hidden,
           slope, layout, L.stream())
    return out


def glow_block_table(entries, device):
    """DEVICE pointer table of nf_glow_level: `entries` = [(blob, mix_w, mix_b, mix_logdet), ...] in processing order (all
    float32, contiguous, on `device`).  Returns (int64 tensor of 4 n pointers, the entries -- keep both alive while a launch
    or a recorded graph may use the table)."""
    ptrs = []
    for blob, w, b_, l in entries:
        L.require_device(blob, w, b_, l)
        for t in (blob, w, b_, l):
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError("glow_block_table: float32 contiguous tensors")
            ptrs.append(t.data_ptr())
    return torch.tensor(ptrs, dtype=torch.int64).to(device), entries


def glow_level(in0, in1, in_squeezed, C, H, W, table, nblocks, layout, slope, scale_map, direction, cout0=None,
               out_squeezed=False, logdet=None, acc=None, hidden=256):
    """`nblocks` GlowBlocks of one shape in ONE persistent launch (nf_glow_level) with the level's glue folded in.
    Input: in_squeezed -> in0 is (B, C/4, 2H, 2W) read through Squeeze.inverse; else channels of in0 (B, cin0, H, W) then
    in1 (B, C - cin0, H, W) (in1 None: in0 has all C channels).  Output: out_squeezed -> (B, C/4, 2H, 2W) through
    Squeeze.forward; cout0 < C -> two tensors split after cout0 channels; else one (B, C, H, W) tensor.
    Returns (out0, out1 or None, logdet)."""
    L.require_device(in0, in1, table, dtype=torch.float32)
    if in0.dtype != torch.float32 or (in1 is not None and in1.dtype != torch.float32):
        raise NotImplementedError("glow_level: float32 only")
    in0 = in0.contiguous()
    in1 = None if in1 is None else in1.contiguous()
    B = in0.shape[0]
    cin0 = C if in_squeezed else in0.shape[1]
    if in_squeezed:
        assert tuple(in0.shape[1:]) == (C // 4, 2 * H, 2 * W), (in0.shape, C, H, W)
    else:
        assert tuple(in0.shape[2:]) == (H, W) and (cin0 == C or (in1 is not None and in1.shape[1] == C - cin0))
    if cout0 is None or out_squeezed:
        cout0 = C
    if out_squeezed:
        out0, out1 = torch.empty(B, C // 4, 2 * H, 2 * W, dtype=in0.dtype, device=in0.device), None
    else:
        out0 = torch.empty(B, cout0, H, W, dtype=in0.dtype, device=in0.device)
        out1 = torch.empty(B, C - cout0, H, W, dtype=in0.dtype, device=in0.device) if cout0 < C else None
    logdet, acc = _ld_buffer(logdet, acc, B, in0)
    L.call("nf_glow_level", ptr(in0), ptr(in1), cin0, 1 if in_squeezed else 0, ptr(out0), ptr(out1), cout0,
           1 if out_squeezed else 0, ptr(logdet), ptr(table), nblocks, B, C, H, W, hidden, slope, L.SCALE[scale_map], direction,
           acc, layout, L.stream())
    return out0, out1, logdet


def glow_block(z, blob, layout, mix_w, mix_b, mix_logdet, slope, scale_map, direction, logdet=None, acc=None, hidden=256,
               table=None):
    """GlowBlock.forward (direction 0) / .inverse (1) in one launch (nf_glow_level with one block): channel-split affine
    coupling with the packed conditioner `blob`, and [Invertible1x1Conv, ActNorm] as the per-pixel affine map (mix_w,
    mix_b) with log|det| per pixel mix_logdet (0-dim device tensor).  `table`: a cached glow_block_table of the block."""
    if table is None:
        table = glow_block_table([(blob, mix_w.contiguous(), mix_b.contiguous(), mix_logdet.to(z.dtype).contiguous())],
                                 z.device)[0]
    B, C, H, W = z.shape
    y, _, logdet = glow_level(z, None, False, C, H, W, table, 1, layout, slope, scale_map, direction, logdet=logdet, acc=acc,
                              hidden=hidden)
    return y, logdet


def logit(z, alpha, direction, logdet=None, acc=None):
    """transforms.py:8-47.  direction 0 = Logit.forward (sigmoid side), 1 = Logit.inverse (logit side)."""
    L.require_device(z)
    z = z.contiguous()
    B = z.shape[0]
    inner = z[0].numel() if B else int(math.prod(z.shape[1:]))
    y = torch.empty_like(z)
    logdet, acc = _ld_buffer(logdet, acc, B, z)
    L.call("nf_logit", ptr(z), ptr(y), ptr(logdet), B, inner, alpha, direction, acc, L.dtype_code(z), L.stream())
    return y, logdet


def diag_gaussian_log_prob_rows(z, loc_rows, log_scale_rows, row_idx=None, ls_shift=0.0, out=None, acc=None):
    """distributions/base.py:326-345: one (loc, log_scale) row per sample, picked by `row_idx` (class labels) or row b."""
    L.require_device(z, loc_rows, log_scale_rows, row_idx, out)
    B = z.shape[0]
    z = z.contiguous()
    d = z[0].numel() if B else int(math.prod(z.shape[1:]))
    if not L.rows_ok(loc_rows.numel(), log_scale_rows.numel(), d, B, row_idx is not None):
        raise ValueError("diag_gaussian_log_prob_rows: loc rows (%d elements) and log_scale rows (%d) must be equally many rows of d = %d "
                         "elements (z %s)%s" % (loc_rows.numel(), log_scale_rows.numel(), d, tuple(z.shape),
                                                "" if row_idx is not None else ", one row per sample"))
    L.check_count("diag_gaussian_log_prob_rows", "row_idx", row_idx, B, "B")
    L.check_count("diag_gaussian_log_prob_rows", "out", out, B, "B")
    loc_rows = loc_rows.contiguous().view(-1, d)
    log_scale_rows = log_scale_rows.contiguous().view(-1, d)
    out, acc = _ld_buffer(out, acc, B, z)
    if B == 0:          # (an empty batch of blended rows has no row at all, which the entry point refuses: nothing to compute)
        return out
    if row_idx is not None:
        row_idx = row_idx.to(torch.long).contiguous()
    L.call("nf_diag_gaussian_log_prob_rows", ptr(z), ptr(loc_rows), ptr(log_scale_rows), ptr(row_idx), loc_rows.shape[0],
           ls_shift, ptr(out), B, d, acc, L.dtype_code(z), L.stream())
    return out


def linear_wgrad(dy, x, want_bias=True, relu_x=False, skip_every=0):
    """dW = dy^T x (x -> relu(x) with relu_x), db = dy.sum(0) for a Linear layer (nf_linear_wgrad[_act|_skip], split-K fp32
    MFMA, deterministic reduction).  skip_every > 1: every skip_every-th column of dy is padding and has no output row."""
    L.require_device(dy, x, dtype=torch.float32)
    if dy.dtype != torch.float32 or x.dtype != torch.float32:
        raise NotImplementedError("linear_wgrad: float32 only")
    dy, x = dy.contiguous(), x.contiguous()
    B, M = dy.shape
    N = x.shape[1]
    dy, x = _a16(dy, N % 4 == 0), _a16(x, N % 4 == 0)          # (N % 4 != 0: the element-wise kernel)
    Mo = M - M // skip_every if skip_every else M
    dW = torch.empty(Mo, N, dtype=torch.float32, device=dy.device)
    db = torch.empty(Mo, dtype=torch.float32, device=dy.device) if want_bias else None
    scratch = _scratch("nf_linear_wgrad_scratch_floats", dy.device, B, M, N)
    L.call("nf_linear_wgrad_skip", ptr(dy), ptr(x), ptr(dW), ptr(db), ptr(scratch), B, M, N, 0, int(relu_x), int(skip_every),
           L.stream())
    return dW, db


def linear_wgrad_pair(dy0, x0, dy1, x1, relu_x=False):
    """(dW0, db0, dW1, db1) of two same-shape Linear layers in one partial launch + one reduction (nf_linear_wgrad_pair)."""
    L.require_device(dy0, x0, dy1, x1, dtype=torch.float32)
    dy0, x0, dy1, x1 = (_a16(t.contiguous()) for t in (dy0, x0, dy1, x1))
    if dy0.shape != dy1.shape or x0.shape != x1.shape or any(t.dtype != torch.float32 for t in (dy0, x0, dy1, x1)):
        raise ValueError("linear_wgrad_pair: two float32 problems of the same shape")
    B, M = dy0.shape
    N = x0.shape[1]
    out = torch.empty(2, M * N + M, dtype=torch.float32, device=dy0.device)     # dW | db per problem
    n = L.query("nf_linear_wgrad_scratch_floats", B, M, N)
    scratch = torch.empty(max(2 * n, 1), dtype=torch.float32, device=dy0.device)
    w0, b0, w1, b1 = out[0, :M * N], out[0, M * N:], out[1, :M * N], out[1, M * N:]
    L.call("nf_linear_wgrad_pair", ptr(dy0), ptr(x0), ptr(w0), ptr(b0), ptr(dy1), ptr(x1), ptr(w1), ptr(b1), ptr(scratch), B, M,
           N, 0, int(relu_x), L.stream())
    return w0.view(M, N), b0, w1.view(M, N), b1


def mfma_clock_mhz(device, iters=20000):
    """Shader clock (MHz) under fp32-MFMA load (nf_mfma_clock_probe): what the matrix pipe runs at while a kernel keeps it busy."""
    out = torch.zeros(2, dtype=torch.int64, device=device)
    sink = torch.zeros(1, dtype=torch.float32, device=device)
    L.call("nf_mfma_clock_probe", ptr(out), ptr(sink), iters, L.stream())
    c, w = out.tolist()
    return 100.0 * c / max(w, 1)


def lu_fwd(x, UpT, LT, bias=None, ld_const=None, ld_sign=1.0, logdet=None, acc=None):
    """(u, y, logdet): u = U x[perm], y = L u + bias per row with the constant log-det, D = 64, LDS-DMA tiles (nf_lu_fwd); the
    arguments of rows_matvec2 with the TRANSPOSED factor images (UpT, LT of lu_factors)."""
    L.require_device(x, UpT, LT, bias, ld_const, logdet, dtype=torch.float32)
    x = _a16(x.contiguous())
    B, D = x.shape
    u, y = torch.empty_like(x), torch.empty_like(x)
    logdet, acc = _ld_buffer(logdet, acc, B, x, want=ld_const is not None)
    L.call("nf_lu_fwd", ptr(x), ptr(UpT.contiguous()), ptr(LT.contiguous()), ptr(bias), ptr(u), ptr(y),
           ptr(logdet if ld_const is not None else None), ptr(ld_const), ld_sign, acc, B, D, L.stream())
    return u, y, logdet


def lu_bwd(gy, u, x, Lm, Up, db_out=None):
    """(gx, dL, db, dUp) of LULinearPermute's batch side in the density direction, D = 64, one pass over the rows (nf_lu_bwd);
    db_out: where the bias gradient (D floats) is written instead of a new tensor."""
    L.require_device(gy, u, x, Lm, Up, dtype=torch.float32)
    gy, u, x, Lm, Up = _a16(gy.contiguous()), _a16(u.contiguous()), _a16(x.contiguous()), Lm.contiguous(), Up.contiguous()
    B, D = gy.shape
    n = L.query("nf_lu_bwd_scratch_floats", B)
    if n <= 0 or D != 64 or gy.dtype != torch.float32:
        raise NotImplementedError("lu_bwd: float32, D = 64, batch a multiple of 64")
    scratch = torch.empty(n, dtype=torch.float32, device=gy.device)
    out = torch.empty(2 * D * D + D, dtype=torch.float32, device=gy.device)
    dL, dUp, db = out[:D * D], out[D * D:2 * D * D], out[2 * D * D:]
    if db_out is not None:
        if db_out.numel() != D or db_out.dtype != torch.float32 or not db_out.is_contiguous() or db_out.device != gy.device:
            raise ValueError("lu_bwd: db_out = a contiguous float32 (D) tensor on the inputs' device")
        db = db_out
    gx = torch.empty_like(gy)
    L.call("nf_lu_bwd", ptr(gy), ptr(u), ptr(x), ptr(Lm), ptr(Up), ptr(gx), ptr(dL), ptr(db), ptr(dUp), ptr(scratch), B, D,
           L.stream())
    return gx, dL.view(D, D), db, dUp.view(D, D)


def resblock_bwd(gh, t, h_in, w1, w2, x=None, wfull=None, gx=None, col_map=None, n_cols=0):
    """Backward of one residual block (hidden 128) in one pass over the rows (nf_resblock_bwd): returns
    (gh_in, dW1, db1, dW2, db2); with x / wfull / gx also the initial Linear layer behind the block:
    gx += gh_in @ wfull.t() in place (wfull (64, 128): the layer's weight transposed on full rows), and
    (None, dW1, db1, dW2, db2, dW0 (128, 64), db0) is returned; col_map (64 int32, -1 = drop):
    dW0 is compacted to the (128, n_cols) columns it names."""
    L.require_device(gh, t, h_in, w1, w2, x, wfull, gx, col_map, dtype=torch.float32)
    gh, t, h_in, w1, w2 = _a16(gh.contiguous()), _a16(t.contiguous()), _a16(h_in.contiguous()), w1.contiguous(), w2.contiguous()
    if any(v.dtype != torch.float32 for v in (gh, t, h_in, w1, w2)):
        raise ValueError("resblock_bwd: float32 only")
    B, H = gh.shape
    init = x is not None
    n = L.query("nf_resblock_bwd_scratch_floats", B, int(init))
    if n <= 0 or H != 128:
        raise NotImplementedError("resblock_bwd: hidden 128, batch a multiple of 64")
    scratch = torch.empty(n, dtype=torch.float32, device=gh.device)
    out = torch.empty(2, H * H + H, dtype=torch.float32, device=gh.device)      # (dW2 | db2), (dW1 | db1)
    w2g, b2g, w1g, b1g = out[0, :H * H], out[0, H * H:], out[1, :H * H], out[1, H * H:]
    if init:
        if not (x.is_contiguous() and gx.is_contiguous() and wfull.is_contiguous()) or x.shape[1] != 64 or \
                tuple(wfull.shape) != (64, 128):
            raise ValueError("resblock_bwd: contiguous x / gx (B, 64) and wfull (64, 128)")
        if gx.data_ptr() % 16:          # (updated in place: a copy would not reach the caller)
            raise ValueError("resblock_bwd: gx must be 16-byte aligned")
        x, wfull = _a16(x), _a16(wfull)
        nc = int(n_cols) if col_map is not None else 64
        out0 = torch.empty(H * nc + H, dtype=torch.float32, device=gh.device)
        gh_in, w0g, b0g = None, out0[:H * nc], out0[H * nc:]
    else:
        gh_in, w0g, b0g = torch.empty_like(gh), None, None
    L.call("nf_resblock_bwd", ptr(gh), ptr(t), ptr(h_in), ptr(w1), ptr(w2), ptr(gh_in), ptr(w1g), ptr(b1g), ptr(w2g), ptr(b2g),
           ptr(x), ptr(wfull), ptr(gx), ptr(w0g), ptr(b0g), ptr(col_map), int(n_cols), ptr(scratch), B, H, 64, L.stream())
    if init:
        return None, w1g.view(H, H), b1g, w2g.view(H, H), b2g, w0g.view(H, nc), b0g
    return gh_in, w1g.view(H, H), b1g, w2g.view(H, H), b2g


def bias_leaky_relu_(y, bias, negative_slope):
    """In place y = leaky_relu(y + bias[c]) on a contiguous NCHW tensor (nf_bias_leaky_relu)."""
    L.require_device(y, bias)
    if not y.is_contiguous():
        raise ValueError("bias_leaky_relu_: contiguous NCHW tensor required")
    B, Cc = y.shape[0], y.shape[1]
    HW = int(math.prod(y.shape[2:]))
    L.call("nf_bias_leaky_relu", ptr(y), ptr(bias.contiguous()), B, Cc, HW, negative_slope, L.dtype_code(y), L.stream())
    return y


def realnvp_chain(z, blob, d, hmax, direction, logdet=None, acc=None):
    """A stack of MaskedAffineFlow(MLP s, MLP t) / ActNorm / AffineCouplingBlock(MLP) + Permute layers in one launch (nf_realnvp_chain)."""
    L.require_device(z, blob, dtype=torch.float32)
    if z.dtype != torch.float32:
        raise NotImplementedError("realnvp_chain: float32 only")
    z = z.contiguous()
    B = z.shape[0]
    y = torch.empty_like(z)
    logdet, acc = _ld_buffer(logdet, acc, B, z)
    L.call("nf_realnvp_chain", ptr(z), ptr(y), ptr(logdet), ptr(blob), B, d, hmax, direction, acc, L.stream())
    return y, logdet


def realnvp_rows(hmax, act):
    """Rows per workgroup of the RealNVP training kernels for this LDS footprint (nf_realnvp_train_rows); 0 = does not fit."""
    rows = L.query("nf_realnvp_train_rows", int(hmax), int(act))
    if rows == L.ENOTSUP:
        return 0
    if rows < 0:
        L.check(rows, "nf_realnvp_train_rows")
    return rows


def realnvp_chain_train_fwd(z, blob, nrec, d, hmax, act, direction):
    """nf_realnvp_chain_train_fwd: (y, per-row log-det, save (nrec, B, d) = every executed record's input)."""
    L.require_device(z, blob, dtype=torch.float32)
    if z.dtype != torch.float32 or not z.is_contiguous():
        raise NotImplementedError("realnvp_chain_train_fwd: contiguous float32 only")
    B = z.shape[0]
    y = torch.empty_like(z)
    logdet = torch.empty(B, dtype=z.dtype, device=z.device)
    save = torch.empty(nrec, B, d, dtype=z.dtype, device=z.device)
    L.call("nf_realnvp_chain_train_fwd", ptr(z), ptr(y), ptr(logdet), ptr(save), ptr(blob), B, d, hmax, act, direction, L.stream())
    return y, logdet, save


def realnvp_chain_bwd(save, gy, gld, blob, d, hmax, act, direction, wmask, want_gz):
    """nf_realnvp_chain_bwd: (gz or None, the parameter gradients in the blob's layout or None when wmask == 0)."""
    L.require_device(save, gy, gld, blob, dtype=torch.float32)
    B, nblob = save.shape[1], blob.numel()
    gz = torch.empty(B, d, dtype=save.dtype, device=save.device) if want_gz else None
    slabs = grads = None
    if wmask:
        slabs = torch.empty(L.size("nf_realnvp_train_scratch_floats", B, hmax, act, nblob), dtype=save.dtype, device=save.device)
        grads = torch.empty(nblob, dtype=save.dtype, device=save.device)
    L.call("nf_realnvp_chain_bwd", ptr(save), _cptr(gy), _cptr(gld), ptr(gz), ptr(blob), ptr(slabs), ptr(grads), B, d, hmax, act,
           nblob, direction, wmask, L.stream())
    return gz, grads


def rank1_rows(d):
    """Rows per workgroup of the rank-1 chain kernels (nf_rank1_rows): 256 for d <= 16, 16 up to d = 128; 0 = d is not taken."""
    rows = L.query("nf_rank1_rows", int(d))
    if rows == L.ENOTSUP:
        return 0
    if rows < 0:
        L.check(rows, "nf_rank1_rows")
    return rows


def _rank1_shape(entry, z, P, kinds, direction):
    """(B, d, K) of a rank-1 chain call after its operand checks: z (B, d) contiguous, P (K, 2 d + 4) (flows/rank1_pack.py), `kinds`
    = the record kinds, known on the host; in direction 1 every record must be leaky Planar (kind 1): ValueError before any launch."""
    if z.dim() != 2 or P.dim() != 2 or not z.is_contiguous() or not P.is_contiguous():
        raise ValueError("%s: z (B, d) and P (K, 2 d + 4) must be contiguous matrices" % entry)
    B, d = z.shape
    K = P.shape[0]
    L.check_count(entry, "P", P, K * (2 * d + 4), "K (2 d + 4)")
    if len(kinds) != K or any(k not in (0, 1, 2) for k in kinds):
        raise ValueError("%s: %d record kinds %r for K = %d records" % (entry, len(kinds), tuple(kinds), K))
    if direction not in (0, 1):
        raise ValueError("%s: direction must be 0 or 1" % entry)
    if direction == 1 and any(k != 1 for k in kinds):
        raise ValueError("%s: direction 1 takes leaky Planar records (kind 1) only, got kinds %r" % (entry, tuple(kinds)))
    return B, d, K


def rank1_chain(z, P, kinds, direction, logdet=None, acc=None):
    """A run of Planar / Radial layers in one launch (nf_rank1_chain): (y, logdet); logdet combined by `acc` when given."""
    L.require_device(z, P, logdet, dtype=torch.float32)
    B, d, K = _rank1_shape("rank1_chain", z, P, kinds, direction)
    y = torch.empty_like(z)
    logdet, acc = _ld_buffer(logdet, acc, B, z)
    L.check_count("rank1_chain", "logdet", logdet, B, "B")
    L.call("nf_rank1_chain", ptr(z), ptr(y), ptr(logdet), ptr(P), B, d, K, direction, acc, L.stream())
    return y, logdet


def rank1_chain_train_fwd(z, P, kinds, direction):
    """nf_rank1_chain_train_fwd: (y, per-row log-det, save (K, B) = every executed record's lin / r)."""
    L.require_device(z, P, dtype=torch.float32)
    B, d, K = _rank1_shape("rank1_chain_train_fwd", z, P, kinds, direction)
    y = torch.empty_like(z)
    logdet = torch.empty(B, dtype=z.dtype, device=z.device)
    save = torch.empty(K, B, dtype=z.dtype, device=z.device)
    L.call("nf_rank1_chain_train_fwd", ptr(z), ptr(y), ptr(logdet), ptr(save), ptr(P), B, d, K, direction, L.stream())
    return y, logdet, save


def rank1_chain_bwd(y, save, gy, gld, P, kinds, direction, need_gP, want_gz):
    """nf_rank1_chain_bwd: (gz or None, gP (K, 2 d + 4) or None when not need_gP).  gy / gld may be None (zeros)."""
    L.require_device(y, save, gy, gld, P, dtype=torch.float32)
    B, d, K = _rank1_shape("rank1_chain_bwd", y, P, kinds, direction)
    L.check_count("rank1_chain_bwd", "save", save, K * B, "K B")
    L.check_count("rank1_chain_bwd", "gy", gy, B * d, "B d")
    L.check_count("rank1_chain_bwd", "gld", gld, B, "B")
    gz = torch.empty_like(y) if want_gz else None
    slabs = gP = None
    if need_gP:
        slabs = torch.empty(L.size("nf_rank1_train_scratch_floats", B, d, K), dtype=y.dtype, device=y.device)
        gP = torch.empty_like(P)
    L.call("nf_rank1_chain_bwd", ptr(y), ptr(save.contiguous()), _cptr(gy), _cptr(gld), ptr(gz), ptr(P), ptr(slabs), ptr(gP), B, d, K,
           direction, 1 if need_gP else 0, L.stream())
    return gz, gP


def density2d_grid(B):
    """Workgroups (of 256 rows) of an nf_density2d launch on B rows; rows beyond grid x 256 are reached by its grid-stride loop."""
    return L.query("nf_density2d_grid", int(B))


def density2d(z, kind, n, rec, dscale=None, want_grad=False):
    """nf_density2d: (lp (B), d lp / d z (B, 2) or None) of a closed-form 2-D density on z (B, 2) in one launch.  kind / n / rec: the
    table of include/nf_mi355x.h (rec: up to 8 Python floats); dscale: CircularGaussianMixture's `scale` buffer (device)."""
    L.require_device(z, dscale, dtype=torch.float32)
    if z.dim() != 2 or z.shape[1] != 2 or not z.is_contiguous():
        raise ValueError("density2d: z must be a contiguous (B, 2) matrix, got %s" % (tuple(z.shape),))
    L.check_count("density2d", "dscale", dscale, 1, "one float")
    B = z.shape[0]
    lp = torch.empty(B, dtype=z.dtype, device=z.device)
    gz = torch.empty_like(z) if want_grad else None
    rec_host = (C.c_float * len(rec))(*rec)
    L.call("nf_density2d", ptr(z), ptr(lp), ptr(gz), int(kind), int(n), rec_host, len(rec), ptr(dscale), B, L.stream())
    return lp, gz


def gmm_rows(d):
    """Rows per workgroup of the mixture kernels (nf_gmm_rows): 256 for d <= 16, 16 up to d = 128; 0 = d is not taken."""
    rows = L.query("nf_gmm_rows", int(d))
    if rows == L.ENOTSUP:
        return 0
    if rows < 0:
        L.check(rows, "nf_gmm_rows")
    return rows


def _gmm_shape(entry, z, R, M):
    """(B, d) of a mixture call after its operand checks: z (B, d) contiguous, R a contiguous vector of 2 M d + M floats."""
    if z.dim() != 2 or R.dim() != 1 or not z.is_contiguous() or not R.is_contiguous():
        raise ValueError("%s: z (B, d) and R (2 M d + M) must be contiguous" % entry)
    B, d = z.shape
    L.check_count(entry, "R", R, 2 * M * d + M, "2 M d + M")
    return B, d


def gmm_log_prob(z, R, M, out=None, acc=None):
    """nf_gmm_log_prob: log-density (B) of the diagonal mixture with record R; combined into `out` by `acc` when given."""
    L.require_device(z, R, out, dtype=torch.float32)
    B, d = _gmm_shape("gmm_log_prob", z, R, M)
    out, acc = _ld_buffer(out, acc, B, z)
    L.check_count("gmm_log_prob", "out", out, B, "B")
    L.call("nf_gmm_log_prob", ptr(z), ptr(R), ptr(out), B, M, d, acc, L.stream())
    return out


def gmm_log_prob_bwd(z, R, M, lp, g, want_gz, want):
    """nf_gmm_log_prob_bwd: (gz or None, gR (2 M d + M) or None when want == 0).  want: bit 0 loc, 1 log_scale, 2 logw."""
    L.require_device(z, R, lp, g, dtype=torch.float32)
    B, d = _gmm_shape("gmm_log_prob_bwd", z, R, M)
    L.check_count("gmm_log_prob_bwd", "lp", lp, B, "B")
    L.check_count("gmm_log_prob_bwd", "g", g, B, "B")
    gz = torch.empty_like(z) if want_gz else None
    slabs = gR = None
    if want:
        slabs = torch.empty(L.size("nf_gmm_scratch_floats", B, M, d), dtype=z.dtype, device=z.device)
        gR = torch.empty_like(R)
    L.call("nf_gmm_log_prob_bwd", ptr(z), ptr(R), ptr(lp.contiguous()), ptr(g.contiguous()), ptr(gz), ptr(slabs), ptr(gR), B, M, d,
           int(want), L.stream())
    return gz, gR


def hmc2d_grid(B):
    """Workgroups (of 256 rows) of an nf_hmc2d launch on B rows; rows beyond grid x 256 are reached by its grid-stride loop."""
    return L.query("nf_hmc2d_grid", int(B))


def mh2d_grid(B):
    """Workgroups (of 256 rows) of an nf_mh2d launch on B rows."""
    return L.query("nf_mh2d_grid", int(B))


def hmc2d_bwd_grid(B):
    """Workgroups (of 256 rows) of an nf_hmc2d_bwd launch on B rows."""
    return L.query("nf_hmc2d_bwd_grid", int(B))


def _h2_target(entry, terms):
    """The host tables and device pointers of a launch's target from stochastic_route.target_terms' list: (tkind, trec, aux tensors)."""
    if not 1 <= len(terms) <= 2:
        raise ValueError("%s: a target has one or two terms, got %d" % (entry, len(terms)))
    tkind, trec, aux = [], [], []
    for w, kind, n, rec, a0, a1 in terms:
        if len(rec) > 8:
            raise ValueError("%s: a record holds at most 8 floats" % entry)
        tkind += [int(kind), int(n)]
        trec += [float(w)] + [float(x) for x in rec] + [0.0] * (8 - len(rec))
        L.check_count(entry, "a0", a0, 1 if kind == 6 else 2, "kind 6: scale; kind 7: loc")
        L.check_count(entry, "a1", a1, 2, "kind 7: log_scale")
        aux += [a0, a1]
    aux += [None] * (4 - len(aux))
    return (C.c_int * len(tkind))(*tkind), (C.c_float * len(trec))(*trec), aux


def _h2_rows(entry, z, **rows):
    if z.dim() != 2 or z.shape[1] != 2 or not z.is_contiguous():
        raise ValueError("%s: z must be a contiguous (B, 2) matrix, got %s" % (entry, tuple(z.shape)))
    for name, (t, n) in rows.items():
        L.check_count(entry, name, t, n, "per row of z %s" % (tuple(z.shape),))
        if t is not None and not t.is_contiguous():
            raise ValueError("%s: %s must be contiguous" % (entry, name))
    return z.shape[0]


def hmc2d(z, eps, u, log_step_size, log_mass, terms, steps, max_abs_grad=0.0, want_side=False):
    """nf_hmc2d: one HamiltonianMonteCarlo transition on z (B, 2) in one launch for given noise eps (B, 2) and uniforms u (B):
    (z_out, log_det, accept (B floats), side (B, 8) or None).  terms: stochastic_route.target_terms; log_step_size / log_mass: two
    floats each in device memory; max_abs_grad 0 = no clipping.  side (training): the tangents of z_new to log_step_size and
    log_mass, and grad log p at z and at z_out."""
    tkind, trec, aux = _h2_target("hmc2d", terms)
    L.require_device(z, eps, u, log_step_size, log_mass, *aux, dtype=torch.float32)
    B = _h2_rows("hmc2d", z, eps=(eps, 2 * z.shape[0]), u=(u, z.shape[0]), log_step_size=(log_step_size, 2), log_mass=(log_mass, 2))
    z_out = torch.empty_like(z)
    log_det = torch.empty(B, dtype=z.dtype, device=z.device)
    accept = torch.empty(B, dtype=z.dtype, device=z.device)
    side = torch.empty((B, 8), dtype=z.dtype, device=z.device) if want_side else None
    L.call("nf_hmc2d", ptr(z), ptr(eps), ptr(u), ptr(log_step_size), ptr(log_mass), tkind, trec, _cptr(aux[0]), _cptr(aux[1]),
           _cptr(aux[2]), _cptr(aux[3]), len(terms), int(steps), float(max_abs_grad), ptr(z_out), ptr(log_det), ptr(accept), ptr(side), B,
           L.stream())
    return z_out, log_det, accept, side


def hmc2d_bwd(gz_out, gld, accept, side, want_gz, want):
    """nf_hmc2d_bwd: (gz (B, 2) or None, gpar (4) = [g log_step_size | g log_mass] or None when want == 0).  gz_out / gld: the
    cotangents, either may be None; want: bit 0 log_step_size, bit 1 log_mass.  want == 0: no slab work, one launch."""
    L.require_device(gz_out, gld, accept, side, dtype=torch.float32)
    B = accept.numel()
    L.check_count("hmc2d_bwd", "side", side, 8 * B, "8 B")
    L.check_count("hmc2d_bwd", "gz_out", gz_out, 2 * B, "2 B")
    L.check_count("hmc2d_bwd", "gld", gld, B, "B")
    gz = torch.empty((B, 2), dtype=side.dtype, device=side.device) if want_gz else None
    slabs = gpar = None
    if want:
        slabs = torch.empty(L.size("nf_hmc2d_bwd_scratch_floats", B), dtype=side.dtype, device=side.device)
        gpar = torch.zeros(4, dtype=side.dtype, device=side.device) if B == 0 else torch.empty(4, dtype=side.dtype, device=side.device)
    L.call("nf_hmc2d_bwd", _cptr(gz_out), _cptr(gld), ptr(accept), ptr(side), ptr(gz), ptr(slabs), ptr(gpar), int(want), B, L.stream())
    return gz, gpar


def mh2d(z, eps, u, scale, terms, steps, want_side=False):
    """nf_mh2d: `steps` random-walk Metropolis-Hastings steps on z (B, 2) in one launch for given noise eps (steps, B, 2) and
    uniforms u (steps, B); scale: the proposal's buffer (one or two floats, device).  (z_out, log_det, gside (B, 4) or None):
    gside = grad log p at z | at z_out."""
    tkind, trec, aux = _h2_target("mh2d", terms)
    L.require_device(z, eps, u, scale, *aux, dtype=torch.float32)
    steps = int(steps)
    B = _h2_rows("mh2d", z, eps=(eps, steps * 2 * z.shape[0]), u=(u, steps * z.shape[0]))
    if scale.numel() not in (1, 2) or not scale.is_contiguous():
        raise ValueError("mh2d: scale holds one or two contiguous floats, got shape %s" % (tuple(scale.shape),))
    z_out = torch.empty_like(z)
    log_det = torch.empty(B, dtype=z.dtype, device=z.device)
    gside = torch.empty((B, 4), dtype=z.dtype, device=z.device) if want_side else None
    L.call("nf_mh2d", ptr(z), ptr(eps), ptr(u), ptr(scale), scale.numel(), tkind, trec, _cptr(aux[0]), _cptr(aux[1]), _cptr(aux[2]),
           _cptr(aux[3]), len(terms), steps, ptr(z_out), ptr(log_det), ptr(gside), B, L.stream())
    return z_out, log_det, gside


def lipmlp_width(hmax):
    """The padded hidden width of the residual-flow kernels for a widest hidden layer `hmax` (nf_lipmlp_width): 32, 64 or 128; 0 =
    not taken."""
    hp = L.query("nf_lipmlp_width", int(hmax))
    if hp == L.ENOTSUP:
        return 0
    if hp < 0:
        L.check(hp, "nf_lipmlp_width")
    return hp


def _lipmlp_rows(entry, blob, K, nres, hp, *rows):
    """B of a residual-flow call after its operand checks: every row operand a contiguous (B, 2) matrix of one shape, blob a
    contiguous vector of nf_lipmlp_blob_floats(K, nres, hp) floats (flows/lipmlp_pack.py)."""
    z = rows[0]
    if any(t.dim() != 2 or t.shape[1] != 2 or t.shape != z.shape or not t.is_contiguous() for t in rows):
        raise ValueError("%s: the row operands must be contiguous (B, 2) matrices of one shape" % entry)
    if blob.dim() != 1 or not blob.is_contiguous():
        raise ValueError("%s: blob must be a contiguous vector" % entry)
    L.check_count(entry, "blob", blob, L.size("nf_lipmlp_blob_floats", int(K), int(nres), int(hp)), "K 16 + nres (2 hp^2 + 7 hp + 4)")
    return z.shape[0]


def lipmlp_chain(z, blob, K, nres, hp, logdet=None, acc=None):
    """A run of [Residual | ActNorm | AffineConstFlow] layers in the Residuals' density direction as one launch (nf_lipmlp_chain):
    (y, logdet); logdet combined by `acc` when given."""
    L.require_device(z, blob, logdet, dtype=torch.float32)
    B = _lipmlp_rows("lipmlp_chain", blob, K, nres, hp, z)
    y = torch.empty_like(z)
    logdet, acc = _ld_buffer(logdet, acc, B, z)
    L.check_count("lipmlp_chain", "logdet", logdet, B, "B")
    L.call("nf_lipmlp_chain", ptr(z), ptr(y), ptr(logdet), ptr(blob), blob.numel(), B, int(hp), int(K), int(nres), acc, L.stream())
    return y, logdet


def lipmlp_apply(x, y, blob, hp, mode, count=None, atol=1e-5, rtol=1e-5):
    """One LipschitzMLP g in one launch (nf_lipmlp_apply).  mode 0: x + g(x).  mode 1: the fixed-point step y - g(x); `count` (one
    int32 on the device, zeroed by the caller) receives the number of elements whose squared step is not below atol + |y| rtol."""
    L.require_device(x, y, blob, count, dtype=torch.float32)
    if mode not in (0, 1):
        raise ValueError("lipmlp_apply: mode must be 0 or 1")
    B = _lipmlp_rows("lipmlp_apply", blob, 1, 1, hp, *((x,) if mode == 0 else (x, y)))
    if mode == 1 and (count is None or count.dtype != torch.int32 or count.numel() != 1):
        raise ValueError("lipmlp_apply: mode 1 needs `count`, one int32 on the device")
    out = torch.empty_like(x)
    L.call("nf_lipmlp_apply", ptr(x), ptr(y if mode == 1 else None), ptr(out), ptr(count if mode == 1 else None), ptr(blob),
           blob.numel(), B, int(hp), mode, float(atol), float(rtol), L.stream())
    return out


def lipmlp_train_rows(hp):
    """Rows per workgroup of the residual-flow BACKWARD kernel (nf_lipmlp_train_rows): 2048 / hp."""
    rows = L.query("nf_lipmlp_train_rows", int(hp))
    if rows < 0:
        L.check(rows, "nf_lipmlp_train_rows")
    return rows


LIPMLP_TRAIN_MAX_TERMS = 32     # series terms of one nf_lipmlp_train_fwd call (they travel in the launch arguments)


def lipmlp_train_fwd(x, blob, hp, kind, coef=(), vareps=None):
    """nf_lipmlp_train_fwd on ONE Residual record: (y (B, 2), ld (B), jhat (B, 4) = d ld / d J).  kind: 0 brute force, 1 Hutchinson,
    2 Neumann, 3 exact trace; coef: Python floats, coef[k - 1] = the weight of series term k (kinds 1 - 3, at most 32); vareps (B, 2):
    the probe vectors of kinds 1 and 2."""
    L.require_device(x, blob, vareps, dtype=torch.float32)
    if kind not in (0, 1, 2, 3):
        raise ValueError("lipmlp_train_fwd: kind must be 0 .. 3")
    if kind in (1, 2) and vareps is None:
        raise ValueError("lipmlp_train_fwd: kinds 1 and 2 need vareps (B, 2)")
    B = _lipmlp_rows("lipmlp_train_fwd", blob, 1, 1, hp, *((x,) if vareps is None else (x, vareps)))
    y = torch.empty_like(x)
    ld = torch.empty(B, dtype=x.dtype, device=x.device)
    jhat = torch.empty(B, 4, dtype=x.dtype, device=x.device)
    coef = [float(c) for c in coef] if kind else []
    coef_host = (C.c_float * max(len(coef), 1))(*coef)
    L.call("nf_lipmlp_train_fwd", ptr(x), ptr(vareps), ptr(y), ptr(ld), ptr(jhat), ptr(blob), blob.numel(), B, int(hp), int(kind),
           len(coef), coef_host, L.stream())
    return y, ld, jhat


def lipmlp_train_bwd(x, gy, jhat, w, blob, hp, want_gblob, want_gx=True):
    """nf_lipmlp_train_bwd: (gx (B, 2) or None, gblob or None when not want_gblob -- then no slab is allocated and no reduction is
    launched).  gy (B, 2) / w (B): the cotangents of y and of ld, of any strides (a non-contiguous one is copied); None = zeros."""
    L.require_device(x, gy, jhat, w, blob, dtype=torch.float32)
    B = _lipmlp_rows("lipmlp_train_bwd", blob, 1, 1, hp, x)
    if gy is not None and gy.shape != x.shape:      # (autograd hands over expanded / strided cotangents: _cptr copies those)
        raise ValueError("lipmlp_train_bwd: gy has shape %s, x %s" % (tuple(gy.shape), tuple(x.shape)))
    L.check_count("lipmlp_train_bwd", "jhat", jhat, 4 * B, "4 B")
    L.check_count("lipmlp_train_bwd", "w", w, B, "B")
    gx = torch.empty_like(x) if want_gx else None
    slabs = gblob = None
    if want_gblob and B:
        slabs = torch.empty(L.size("nf_lipmlp_train_scratch_floats", B, int(hp)), dtype=x.dtype, device=x.device)
        gblob = torch.empty_like(blob)
    elif want_gblob:
        gblob = torch.zeros_like(blob)
    # contiguous copies of strided cotangents stay referenced until the launch is enqueued: a copy dropped inside the argument list
    # hands its block back to the allocator, and the next copy in the same list can land on it
    gy, jhat, w = (None if t is None else t.contiguous() for t in (gy, jhat, w))
    L.call("nf_lipmlp_train_bwd", ptr(x), ptr(gy), ptr(jhat), ptr(w), ptr(gx), ptr(blob), ptr(slabs), ptr(gblob), blob.numel(), B,
           int(hp), 1 if slabs is not None else 0, L.stream())
    return gx, gblob


LIPMLP_ND_MAX_RES = 8           # Residual records of one nf_lipmlp_nd_chain call
LIPMLP_ND_MAX_TERMS = 48        # series terms per record (they travel in the launch arguments)


def lipmlp_nd_rows(hp, d):
    """Rows per workgroup of the d-dimensional residual-flow kernels (nf_lipmlp_nd_rows)."""
    rows = L.query("nf_lipmlp_nd_rows", int(hp), int(d))
    if rows < 0:
        L.check(rows, "nf_lipmlp_nd_rows")
    return rows


def _lipmlp_nd_rows(entry, blob, K, nres, hp, *rows):
    """(B, d) of a d-dimensional residual-flow call after its operand checks: every row operand a contiguous (B, d) matrix of one
    shape, blob a contiguous vector of nf_lipmlp_nd_blob_floats(K, nres, hp, d) floats (flows/lipmlp_nd_pack.py)."""
    z = rows[0]
    if any(t.dim() != 2 or t.shape != z.shape or not t.is_contiguous() for t in rows):
        raise ValueError("%s: the row operands must be contiguous (B, d) matrices of one shape" % entry)
    if blob.dim() != 1 or not blob.is_contiguous():
        raise ValueError("%s: blob must be a contiguous vector" % entry)
    L.check_count(entry, "blob", blob, L.size("nf_lipmlp_nd_blob_floats", int(K), int(nres), int(hp), int(z.shape[1])),
                  "K (16 + 2 dp) + nres (2 hp^2 + 2 dp hp + 3 hp + dp)")
    return z.shape


def lipmlp_nd_chain(z, vareps, blob, K, nres, hp, terms, coefs, logdet=None, acc=None):
    """A run of [Residual | ActNorm | AffineConstFlow] layers on (B, d) rows, 3 <= d <= 64, in the Residuals' density direction as
    one launch (nf_lipmlp_nd_chain): (y, logdet); logdet combined by `acc` when given.  vareps (nres, B, d): the probe vectors;
    terms: nres term counts (1 .. 48); coefs: per Residual record the Python floats coef(1) .. coef(terms)."""
    L.require_device(z, vareps, blob, logdet, dtype=torch.float32)
    B, d = _lipmlp_nd_rows("lipmlp_nd_chain", blob, K, nres, hp, z)
    if vareps.shape != (nres, B, d) or not vareps.is_contiguous():
        raise ValueError("lipmlp_nd_chain: vareps must be a contiguous (nres, B, d) tensor, got %s" % (tuple(vareps.shape),))
    terms = [int(t) for t in terms]
    if len(terms) != nres or len(coefs) != nres or any(len(c) != t for c, t in zip(coefs, terms)):
        raise ValueError("lipmlp_nd_chain: one term count and one list of that many coefficients per Residual record")
    y = torch.empty_like(z)
    logdet, acc = _ld_buffer(logdet, acc, B, z)
    L.check_count("lipmlp_nd_chain", "logdet", logdet, B, "B")
    nterms_host = (C.c_int * max(nres, 1))(*terms)
    coef_host = (C.c_float * (max(nres, 1) * LIPMLP_ND_MAX_TERMS))()
    for r, c in enumerate(coefs):
        for k, v in enumerate(c[:LIPMLP_ND_MAX_TERMS]):
            coef_host[r * LIPMLP_ND_MAX_TERMS + k] = float(v)
    L.call("nf_lipmlp_nd_chain", ptr(z), ptr(vareps), ptr(y), ptr(logdet), ptr(blob), blob.numel(), B, d, int(hp), int(K), int(nres),
           nterms_host, coef_host, acc, L.stream())
    return y, logdet


def lipmlp_nd_apply(x, y, blob, hp, mode, count=None, atol=1e-5, rtol=1e-5):
    """One LipschitzMLP g on (B, d) rows in one launch (nf_lipmlp_nd_apply).  mode 0: x + g(x).  mode 1: the fixed-point step
    y - g(x); `count` (one int32 on the device, zeroed by the caller) receives the number of elements whose squared step is not below
    atol + |y| rtol."""
    L.require_device(x, y, blob, count, dtype=torch.float32)
    if mode not in (0, 1):
        raise ValueError("lipmlp_nd_apply: mode must be 0 or 1")
    B, d = _lipmlp_nd_rows("lipmlp_nd_apply", blob, 1, 1, hp, *((x,) if mode == 0 else (x, y)))
    if mode == 1 and (count is None or count.dtype != torch.int32 or count.numel() != 1):
        raise ValueError("lipmlp_nd_apply: mode 1 needs `count`, one int32 on the device")
    out = torch.empty_like(x)
    L.call("nf_lipmlp_nd_apply", ptr(x), ptr(y if mode == 1 else None), ptr(out), ptr(count if mode == 1 else None), ptr(blob),
           blob.numel(), B, d, int(hp), mode, float(atol), float(rtol), L.stream())
    return out
