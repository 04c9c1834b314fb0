"""Shared by the host and GPU tests of the wide RealNVP coupling layers' training route (autograd.AffineWideFn): a numpy restatement
of the two element-wise kernels of csrc/affine_wide_train.hip, a plain-torch restatement of the two layer types (the formulas of
affine/coupling.py:209-229 and :117-171 over the layer's own conditioner modules; runs on the CPU in any dtype), the fixtures' loader
and the gradient entries the reference's autograd leaves exactly 0."""
import numpy as np
import torch

import affine_wide_cases as cases
from conftest import golden_state, load_golden


def load_layer(nfa, name):
    """(layer with the fixture's weights, the inference fixture, the training fixture) of case `name`."""
    g = load_golden("affine_wide_" + name)
    layer = cases.build(nfa, name)
    layer.load_state_dict({k: torch.from_numpy(v) for k, v in golden_state(g).items()})
    return layer, g, load_golden("grad_affine_wide_" + name)


def torch_layer(layer, z, direction):
    """(y, ld) of the layer in plain torch ops on its own conditioner modules."""
    from normflows_amd.autograd import _coupling_formula
    from normflows_amd.flows import realnvp_pack
    if hasattr(layer, "b"):
        b = layer.b.to(z.dtype)
        zm = b * z
        sc = layer.s(zm) if layer.s is not None else torch.zeros_like(z)
        sh = layer.t(zm) if layer.t is not None else torch.zeros_like(z)
        if direction == 0:
            return zm + (1 - b) * (z * torch.exp(sc) + sh), torch.sum((1 - b) * sc, dim=1)
        return zm + (1 - b) * (z - sh) * torch.exp(-sc), -torch.sum((1 - b) * sc, dim=1)
    d = z.shape[1]
    c1, flip = realnvp_pack.block_split(layer, d)
    c = layer.flows[1]
    z1 = z[:, d - c1:] if flip else z[:, :c1]
    return _coupling_formula(z, c.param_map(z1), c1, flip, c._smap(), direction)


def _sig(x):
    return 1.0 / (1.0 + np.exp(-x))


def apply_np(z, P, modes, smap, nets, direction):
    """nf_affine_wide_apply: (y, ld) from z (B, d), P (B, >= 2 d), the d mode codes."""
    d = z.shape[1]
    sc, sh = P[:, 0:2 * d:2], P[:, 1:2 * d:2]
    tr = modes != 0
    if smap == 4:
        b = (modes == 0).astype(z.dtype)
        sc = sc if nets & 1 else np.zeros_like(z)
        sh = sh if nets & 2 else np.zeros_like(z)
        ld = ((1 - b) * sc).sum(1)
        y = b * z + (1 - b) * (z * np.exp(sc) + sh) if direction == 0 else b * z + (1 - b) * (z - sh) * np.exp(-sc)
        return y, ld if direction == 0 else -ld
    if smap == 3:
        t, ldt = (z + sh if direction == 0 else z - sh), np.zeros_like(z)
    elif smap == 0:
        t, ldt = (z * np.exp(sc) + sh if direction == 0 else (z - sh) * np.exp(-sc)), sc
    else:
        sg = _sig(sc + 2.0)
        if smap == 1:
            t, ldt = (z / sg + sh if direction == 0 else (z - sh) * sg), -np.log(sg)
        else:
            t, ldt = (z * sg + sh if direction == 0 else (z - sh) / sg), np.log(sg)
    ld = np.where(tr, ldt, 0.0).sum(1)
    return np.where(tr, t, z), ld if direction == 0 else -ld


def apply_bwd_np(z, P, gy, gld, modes, smap, nets, direction):
    """nf_affine_wide_apply_bwd: (gz through the element-wise map, gP (B, 2 d))."""
    B, d = z.shape
    sc, sh = P[:, 0:2 * d:2], P[:, 1:2 * d:2]
    gl = gld[:, None]
    tr = modes != 0
    gsc, gsh = np.zeros_like(z), np.zeros_like(z)
    if smap == 4:
        b = (modes == 0).astype(z.dtype)
        nb = 1 - b
        sc = sc if nets & 1 else np.zeros_like(z)
        sh = sh if nets & 2 else np.zeros_like(z)
        e = np.exp(sc if direction == 0 else -sc)
        gz = gy * (b + nb * e)
        if direction == 0:
            gsc, gsh = nb * (gy * z * e + gl), nb * gy
        else:
            gsc, gsh = -nb * (gy * (z - sh) * e + gl), -nb * gy * e
        gsc = gsc if nets & 1 else np.zeros_like(z)
        gsh = gsh if nets & 2 else np.zeros_like(z)
    else:
        if smap == 3:
            gv, gsh = gy, (gy if direction == 0 else -gy)
        elif smap == 0:
            e = np.exp(sc if direction == 0 else -sc)
            gv = gy * e
            if direction == 0:
                gsh, gsc = gy, gy * z * e + gl
            else:
                gsh, gsc = -gy * e, -(gy * (z - sh) * e + gl)
        else:
            sg = _sig(sc + 2.0)
            om = 1 - sg
            mult = (smap == 2) == (direction == 0)
            v = z if direction == 0 else z - sh
            if mult:
                gv, gsc = gy * sg, gy * v * sg * om + gl * om
            else:
                gv, gsc = gy / sg, -(gy * v * om / sg + gl * om)
            gsh = gy if direction == 0 else -gv
        gz = np.where(tr, gv, gy)
        gsc, gsh = np.where(tr, gsc, 0.0), np.where(tr, gsh, 0.0)
    gP = np.zeros((B, 2 * d), dtype=z.dtype)
    gP[:, 0::2], gP[:, 1::2] = gsc, gsh
    return gz, gP


def exact_zero_entries(layer, name):
    """[(parameter name, boolean array over its shape)] of the gradient entries the reference's autograd leaves exactly 0: a masked
    flow's first-layer weight columns f with b_f = 0 (both nets: the reference feeds b * z) and its final-layer rows and biases of
    features with b_f = 1 (multiplied by 1 - b).  A block has none."""
    c = cases.CASES[name]
    if c["kind"] != "masked":
        return []
    b = cases.mask(c)
    out = []
    params = dict(layer.named_parameters())
    for net in ("s", "t"):
        if c[net] is None:
            continue
        lin_ids = sorted({int(k.split(".")[2]) for k in params if k.startswith(net + ".net.")})
        first, last = "%s.net.%d" % (net, lin_ids[0]), "%s.net.%d" % (net, lin_ids[-1])
        m = np.zeros(tuple(params[first + ".weight"].shape), dtype=bool)
        m[:, b == 0.0] = True
        out.append((first + ".weight", m))
        m = np.zeros(tuple(params[last + ".weight"].shape), dtype=bool)
        m[b == 1.0, :] = True
        out.append((last + ".weight", m))
        out.append((last + ".bias", b == 1.0))
    return out


def param_order(nfa, layer, d):
    """Parameter names in the order of AffineWideFn's params (affine_wide_pack.linears: weight, bias per Linear)."""
    from normflows_amd.flows import affine_wide_pack as awp
    st = awp.structure(layer, d)
    names = {id(p): k for k, p in layer.named_parameters()}
    return [names[id(t)] for l in awp.linears(st) for t in (l.weight, l.bias)]
