"""The coupling block record of the RealNVP chain kernels restated in plain torch (any device, any dtype; float64 on the CPU pins the
fixtures): Split -> AffineCoupling -> Merge for the channel / channel_inv modes (coupling.py:117-171, :232-267, reshape.py:30-34,
59-64; the checkerboard modes on 2-D rows as well: they stay outside the record) with a nets.MLP param_map; every other flow of
a stack goes through realnvp_train_emulator.chain (MaskedAffineFlow, ActNorm / AffineConstFlow, Permute).  Reads the tensors of the given flow modules and runs no method of theirs, so autograd differentiates
exactly what is written here."""
import torch

import realnvp_train_emulator as base


def block(f, x, inverse):
    """(y, per-row log-det) of one AffineCouplingBlock `f` (its three sub-flows in f.flows) on (B, d) rows."""
    d = x.shape[1]
    coupling = f.flows[1]
    mode = f.flows[0].mode
    if "checkerboard" in mode:                  # (reshape.py:35-46 on 2-D rows: the odd columns are one set, the even ones the other)
        i1 = torch.arange(1 if mode == "checkerboard" else 0, d, 2)
    else:                                       # chunk(2, dim=1): the first chunk has ceil(d/2) columns
        n_first = (d + 1) // 2
        i1 = torch.arange(0, n_first) if mode == "channel" else torch.arange(n_first, d)
    i2 = torch.tensor([i for i in range(d) if i not in set(i1.tolist())])
    i1, i2 = i1.to(x.device), i2.to(x.device)
    z1, z2 = x[:, i1], x[:, i2]
    param = base.mlp(coupling.param_map, z1)
    if coupling.scale:
        shift, s = param[:, 0::2], param[:, 1::2]
        if coupling.scale_map == "exp":
            y2, ld = ((z2 - shift) * torch.exp(-s), -s.sum(1)) if inverse else (z2 * torch.exp(s) + shift, s.sum(1))
        else:
            sg = torch.sigmoid(s + 2)
            if coupling.scale_map == "sigmoid":
                y2, ld = ((z2 - shift) * sg, torch.log(sg).sum(1)) if inverse else (z2 / sg + shift, -torch.log(sg).sum(1))
            else:
                assert coupling.scale_map == "sigmoid_inv"
                y2, ld = ((z2 - shift) / sg, -torch.log(sg).sum(1)) if inverse else (z2 * sg + shift, torch.log(sg).sum(1))
    else:
        y2, ld = (z2 - param if inverse else z2 + param), torch.zeros(x.shape[0], dtype=x.dtype, device=x.device)
    inv = torch.empty(d, dtype=torch.long, device=x.device)
    inv[torch.cat([i1, i2])] = torch.arange(d, device=x.device)
    return torch.cat([z1, y2], 1)[:, inv], ld       # the merge puts the halves back where they came from


def chain(flows, x, inverse):
    """(y, per-row log-det) of `flows` applied in order (inverse: in reverse order with the inverse formulas)."""
    ld = torch.zeros(x.shape[0], dtype=x.dtype, device=x.device)
    for f in (reversed(list(flows)) if inverse else flows):
        x, l = block(f, x, inverse) if hasattr(f, "split_mode") else base.chain([f], x, inverse)
        ld = ld + l
    return x, ld


def blob_chain(blob, x, inverse):
    """(y, per-row log-det) of the run that the chain blob `blob` (core._pack_realnvp / realnvp_pack's gather) describes, reading
    the blob the way csrc/realnvp_chain.hip does: header, record offsets, then per record its kind, header and MLPs.  The
    MaskedAffineFlow record's non-finite -> NaN rule is left out (the fixtures hold finite values)."""
    b = blob.double().tolist()
    nrec, d = int(b[0]), int(b[1])
    x = x.double()
    ld = torch.zeros(x.shape[0], dtype=torch.float64)

    def net(o, inp):
        nlin, slope = int(b[o]), b[o + 1]
        sizes = [int(v) for v in b[o + 2:o + 3 + nlin]]
        o += 3 + nlin
        for k in range(nlin):
            w = torch.tensor(b[o:o + sizes[k + 1] * sizes[k]], dtype=torch.float64).view(sizes[k + 1], sizes[k])
            o += w.numel()
            inp = inp @ w.t() + torch.tensor(b[o:o + sizes[k + 1]], dtype=torch.float64)
            o += sizes[k + 1]
            if k < nlin - 1:
                inp = torch.where(inp > 0, inp, inp * slope)
        return inp, o

    sign = -1.0 if inverse else 1.0
    for q in (range(nrec - 1, -1, -1) if inverse else range(nrec)):
        o = int(b[4 + q])
        kind = int(b[o])
        if kind == 1:
            s, t = (torch.tensor(b[o + 4 + k * d:o + 4 + (k + 1) * d], dtype=torch.float64) for k in (0, 1))
            x = (x - t) * torch.exp(-s) if inverse else x * torch.exp(s) + t
            ld = ld + sign * s.sum()
        elif kind == 2:
            m = torch.tensor(b[o + 4:o + 4 + d], dtype=torch.float64)
            zm, p = m * x, o + 4 + d
            s = t = torch.zeros_like(x)
            if b[o + 1]:
                s, p = net(p, zm)
            if b[o + 2]:
                t, p = net(p, zm)
            x = zm + (1 - m) * ((x - t) * torch.exp(-s) if inverse else x * torch.exp(s) + t)
            ld = ld + sign * ((1 - m) * s).sum(1)
        else:
            assert kind == 3
            c1, code = int(b[o + 1]), int(b[o + 2])
            c2, flip, smap = d - c1, code & 1, code >> 1
            pf, pi = ([int(v) for v in b[o + 4 + k * d:o + 4 + (k + 1) * d]] for k in (0, 1))
            if inverse and b[o + 3]:
                x = x[:, pi]
            o1, o2 = (c2, 0) if flip else (0, c1)
            z2 = x[:, o2:o2 + c2]
            par, _ = net(o + 4 + 2 * d, x[:, o1:o1 + c1])
            sh, sc = (par, None) if smap == 3 else (par[:, 0::2], par[:, 1::2])
            if smap == 3:
                y2 = z2 - sh if inverse else z2 + sh
            elif smap == 0:
                y2 = (z2 - sh) * torch.exp(-sc) if inverse else z2 * torch.exp(sc) + sh
                ld = ld + sign * sc.sum(1)
            else:
                sg = torch.sigmoid(sc + 2)
                mult = (smap == 2) == (not inverse)
                y2 = ((z2 - sh) * sg if mult else (z2 - sh) / sg) if inverse else ((z2 * sg if mult else z2 / sg) + sh)
                ld = ld + (1.0 if mult else -1.0) * torch.log(sg).sum(1)
            x = x.clone()
            x[:, o2:o2 + c2] = y2
            if not inverse and b[o + 3]:
                x = x[:, pf]
    return x, ld


def grads(flows, x, cz, cl, inverse):
    """(z, ld, gx, {id(parameter): gradient}) of loss = sum(z * cz) + sum(ld * cl)."""
    params = [p for f in flows for p in f.parameters()]
    xx = x.detach().clone().requires_grad_(True)
    z, ld = chain(flows, xx, inverse)
    got = torch.autograd.grad((z * cz).sum() + (ld * cl).sum(), [xx] + params, allow_unused=True)
    return z.detach(), ld.detach(), got[0], {id(p): (torch.zeros_like(p) if g is None else g) for p, g in zip(params, got[1:])}
