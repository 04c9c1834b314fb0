"""A torch emulator of the arithmetic of csrc/lipmlp_train.hip on the CPU, in the blob's own dtype (float32 like the kernels, or
float64 to check the formulas themselves): the forward-mode tangent streams, the per-row closed-form estimators with their
cotangent Jhat = d ld / d J, and the hand-written backward through the value stream and the two tangent streams.  No autograd
inside: what it returns is what the kernels are specified to return (include/nf_mi355x.h), summed over rows in one piece instead of
tile by tile.

    fwd(x, blob, hp, kind, coef, vareps)        -> y, ld, jhat        (ops.lipmlp_train_fwd)
    bwd(x, gy, jhat, w, blob, hp, want_gblob)   -> gx, gblob          (ops.lipmlp_train_bwd)
    patched(monkeypatch)                        ops' two entry points replaced by these (and counted)"""
import torch

HDR = 16


def _views(blob, hp):
    """(nmid, c (4), [(W (in, out), b)] hidden-to-hidden included, W_last (2, hp), b_last) of one Residual record."""
    hdr, blk = blob[:HDR], blob[HDR:]
    nmid = int(hdr[1])
    layers = [(blk[:2 * hp].view(2, hp), blk[2 * hp:3 * hp])]
    for m in range(nmid):
        o = 3 * hp + m * (hp * hp + hp)
        layers.append((blk[o:o + hp * hp].view(hp, hp), blk[o + hp * hp:o + hp * hp + hp]))
    o = 3 * hp + 2 * (hp * hp + hp)
    return nmid, hdr[2:6], layers, blk[o:o + 2 * hp].view(2, hp), blk[o + 2 * hp:o + 2 * hp + 2]


def _swish(p, c):
    """f, f', q (f'' = c q, df'/dc = p q) and df/dc of f(p) = p sigmoid(c p) / 1.1."""
    s = torch.sigmoid(c * p)
    ss = s * (1 - s)
    return p * s / 1.1, (s + c * p * ss) / 1.1, ss * (2 + c * p * (1 - 2 * s)) / 1.1, p * p * ss / 1.1


def _streams(x, blob, hp):
    """The pre-activations [(p_l, tau_l^0, tau_l^1)] of layer 0 .. nmid + 1 (layer 0: x and the unit vectors), then g and J."""
    nmid, c, layers, Wl, bl = _views(blob, hp)
    B = x.shape[0]
    eye = torch.eye(2, dtype=x.dtype).expand(B, 2, 2)
    pre = [(x, eye[:, :, 0], eye[:, :, 1])]
    for l, (W, b) in enumerate(layers):
        p, t0, t1 = pre[-1]
        f, df, _, _ = _swish(p, c[l])
        pre.append((f @ W + b, (df * t0) @ W, (df * t1) @ W))
    p, t0, t1 = pre[-1]
    f, df, _, _ = _swish(p, c[nmid + 1])
    g = f @ Wl.t() + bl
    J = torch.stack([(df * t0) @ Wl.t(), (df * t1) @ Wl.t()], 2)        # J[b, i, j] = d g_i / d x_j
    return pre, g, J


def estimate(kind, coef, J, v):
    """(ld (B), Jhat (B, 2, 2)) of include/nf_mi355x.h's table, by the kernel's recurrences."""
    B = J.shape[0]
    eye = torch.eye(2, dtype=J.dtype).expand(B, 2, 2)
    if kind == 0:
        A = eye + J
        return torch.log(torch.abs(torch.linalg.det(A))), torch.linalg.inv(A).transpose(1, 2)
    ld, Jh = torch.zeros(B, dtype=J.dtype), torch.zeros(B, 2, 2, dtype=J.dtype)
    Jt = J.transpose(1, 2)
    if kind == 1:
        L, G = v, v.unsqueeze(2) * v.unsqueeze(1)
        for k in range(1, len(coef) + 1):
            L = torch.bmm(L.unsqueeze(1), J).squeeze(1)
            a = (-1) ** (k + 1) * coef[k - 1] / k
            ld = ld + a * (L * v).sum(1)
            Jh = Jh + a * G
            G = torch.bmm(G, Jt) + L.unsqueeze(2) * v.unsqueeze(1)
    elif kind == 2:
        L = n = v
        for k in range(1, len(coef) + 1):
            L = torch.bmm(L.unsqueeze(1), J).squeeze(1)
            n = n + (-1) ** k * coef[k - 1] * L
        ld = (n * torch.bmm(J, v.unsqueeze(2)).squeeze(2)).sum(1)
        Jh = n.unsqueeze(2) * v.unsqueeze(1)
    else:
        P = eye
        for k in range(1, len(coef) + 1):
            a = (-1) ** (k + 1) * coef[k - 1] / k
            Jh = Jh + a * k * P.transpose(1, 2)
            P = torch.bmm(P, J)
            ld = ld + a * (P[:, 0, 0] + P[:, 1, 1])
    return ld, Jh


def fwd(x, blob, hp, kind, coef=(), vareps=None):
    _, g, J = _streams(x, blob, hp)
    ld, Jh = estimate(kind, [float(c) for c in coef], J, vareps)
    return x + g, ld, Jh.reshape(-1, 4)


def bwd(x, gy, jhat, w, blob, hp, want_gblob, want_gx=True):
    nmid, c, layers, Wl, bl = _views(blob, hp)
    pre, _, _ = _streams(x, blob, hp)
    B = x.shape[0]
    gy = torch.zeros_like(x) if gy is None else gy
    w = torch.zeros(B, dtype=x.dtype) if w is None else w
    Jh = jhat.view(B, 2, 2) * w.view(B, 1, 1)
    ph, th = gy, [Jh[:, :, 0], Jh[:, :, 1]]                 # cotangents of p_{L+1} = g and of tau_{L+1}^j = J[:, j]
    gblob = torch.zeros_like(blob)
    ghdr, gblk = gblob[:HDR], gblob[HDR:]
    o_last = 3 * hp + 2 * (hp * hp + hp)
    mats = layers + [(Wl.t(), bl)]                          # every linear layer as (in, out)
    for l in range(nmid + 1, -1, -1):
        W, _ = mats[l]
        p, t0, t1 = pre[l]
        f, df, q, dc = _swish(p, c[l])
        gW = f.t() @ ph + (df * t0).t() @ th[0] + (df * t1).t() @ th[1]         # (in, out)
        gb = ph.sum(0)
        if l == nmid + 1:
            gblk[o_last:o_last + 2 * hp] = gW.t().reshape(-1)
            gblk[o_last + 2 * hp:o_last + 2 * hp + 2] = gb
        elif l == 0:
            gblk[:2 * hp], gblk[2 * hp:3 * hp] = gW.reshape(-1), gb
        else:
            o = 3 * hp + (l - 1) * (hp * hp + hp)
            gblk[o:o + hp * hp], gblk[o + hp * hp:o + hp * hp + hp] = gW.reshape(-1), gb
        ah, al0, al1 = ph @ W.t(), th[0] @ W.t(), th[1] @ W.t()
        ta = t0 * al0 + t1 * al1
        ghdr[2 + l] = (dc * ah + p * q * ta).sum()
        ph, th = df * ah + c[l] * q * ta, [df * al0, df * al1]
    return (gy + ph if want_gx else None), (gblob if want_gblob else None)


def patched(monkeypatch):
    """Replace ops.lipmlp_train_fwd / _bwd by the emulator; returns the call counts {"fwd": n, "bwd": n, "want": [..]}."""
    from normflows_amd import ops
    calls = {"fwd": 0, "bwd": 0, "want": []}

    def f(x, blob, hp, kind, coef=(), vareps=None):
        calls["fwd"] += 1
        return fwd(x, blob, hp, kind, coef, vareps)

    def b(x, gy, jhat, w, blob, hp, want_gblob, want_gx=True):
        calls["bwd"] += 1
        calls["want"].append(bool(want_gblob))
        return bwd(x, gy, jhat, w, blob, hp, want_gblob, want_gx)

    monkeypatch.setattr(ops, "lipmlp_train_fwd", f)
    monkeypatch.setattr(ops, "lipmlp_train_bwd", b)
    return calls
