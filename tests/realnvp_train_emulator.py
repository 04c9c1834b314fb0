"""The formulas of a RealNVP-style stack restated in plain torch (any device, any dtype; float64 on the CPU pins the fixtures):
MaskedAffineFlow (coupling.py:209-229), AffineConstFlow / ActNorm once initialised (coupling.py:38-54), Permute (mixing.py:9-54), nets.MLP (mlp.py:5-58:
Linear + LeakyReLU).  Reads the tensors of the given flow modules and runs no method of theirs, so autograd differentiates
exactly what is written here."""
import torch


def mlp(net, x):
    lin = [m for m in net.net if isinstance(m, torch.nn.Linear)]
    slopes = [m.negative_slope for m in net.net if isinstance(m, torch.nn.LeakyReLU)]
    for k, l in enumerate(lin):
        x = x @ l.weight.t() + l.bias
        if k < len(lin) - 1:
            x = torch.where(x > 0, x, x * slopes[k])
    return x


def chain(flows, x, inverse):
    """(y, per-row log-det) of `flows` applied in order (inverse: in reverse order with the inverse formulas)."""
    ld = torch.zeros(x.shape[0], dtype=x.dtype, device=x.device)
    nan = torch.tensor(float("nan"), dtype=x.dtype, device=x.device)
    for f in (reversed(list(flows)) if inverse else flows):
        if hasattr(f, "b"):
            zm = f.b * x
            s = mlp(f.s, zm) if isinstance(f.s, torch.nn.Module) else torch.zeros_like(x)
            t = mlp(f.t, zm) if isinstance(f.t, torch.nn.Module) else torch.zeros_like(x)
            s, t = torch.where(torch.isfinite(s), s, nan), torch.where(torch.isfinite(t), t, nan)
            if inverse:
                x = zm + (1 - f.b) * (x - t) * torch.exp(-s)
                ld = ld - ((1 - f.b) * s).sum(1)
            else:
                x = zm + (1 - f.b) * (x * torch.exp(s) + t)
                ld = ld + ((1 - f.b) * s).sum(1)
        elif hasattr(f, "mode"):            # Permute (mixing.py:9-54): data movement, log-det 0
            if f.mode == "shuffle":
                x = x[:, f.inv_perm if inverse else f.perm]
            else:
                cut = (x.shape[1] + 1) // 2 if inverse else x.shape[1] // 2
                x = torch.cat([x[:, cut:], x[:, :cut]], dim=1)
        else:
            if inverse:
                x = (x - f.t) * torch.exp(-f.s)
                ld = ld - f.s.sum()
            else:
                x = x * torch.exp(f.s) + f.t
                ld = ld + f.s.sum()
    return x, ld


def grads(flows, x, cz, cl, inverse):
    """(z, ld, gx, {id(parameter): gradient}) of loss = sum(z * cz) + sum(ld * cl)."""
    params = [p for f in flows for p in f.parameters()]
    xx = x.detach().clone().requires_grad_(True)
    z, ld = chain(flows, xx, inverse)
    got = torch.autograd.grad((z * cz).sum() + (ld * cl).sum(), [xx] + params, allow_unused=True)
    return z.detach(), ld.detach(), got[0], {id(p): (torch.zeros_like(p) if g is None else g) for p, g in zip(params, got[1:])}
