"""float32 NumPy emulation of the residual-flow kernels' arithmetic (csrc/lipmlp.hip) on the packed blob of flows/lipmlp_pack.py: the
same header and block layout, the same forward-mode tangent recurrences, every intermediate rounded to float32 (the order of the
sums inside a product is NumPy's, not the kernel's).  What it checks on the CPU: the blob's layout and padding, the Swish derivative,
the tangent streams, the determinant and its sign conventions, the affine records and the fixed-point step with its count."""
import numpy as np

HDR = 16
f32 = np.float32


def rstride(hp):
    return 2 * hp * hp + 7 * hp + 4


def swish(p, c):
    s = (f32(1) / (f32(1) + np.exp(-c * p, dtype=f32))).astype(f32)
    h = (p * s / f32(1.1)).astype(f32)
    dh = ((s + c * p * s * (f32(1) - s)) / f32(1.1)).astype(f32)
    return h, dh


def net(hdr, W, x, hp, tangents=True):
    """(g (B, 2), J (B, 2, 2) with J[b, j, i] = dg_j / dx_i or None) of one record's network on x (B, 2)."""
    nmid = int(hdr[1])
    a, da = swish(x, f32(hdr[2]))
    W0, b0 = W[:2 * hp].reshape(2, hp), W[2 * hp:3 * hp]
    pre = (a @ W0 + b0).astype(f32)
    h, dh = swish(pre, f32(hdr[3]))
    t = [(W0[i][None, :] * da[:, i:i + 1] * dh).astype(f32) for i in range(2)] if tangents else []
    for m in range(nmid):
        o = 3 * hp + m * (hp * hp + hp)
        Wm, bm = W[o:o + hp * hp].reshape(hp, hp), W[o + hp * hp:o + hp * hp + hp]
        pre = (h @ Wm + bm).astype(f32)
        h, dh = swish(pre, f32(hdr[4 + m]))
        t = [((ti @ Wm).astype(f32) * dh).astype(f32) for ti in t]
    o = 3 * hp + 2 * (hp * hp + hp)
    Wl, bl = W[o:o + 2 * hp].reshape(2, hp), W[o + 2 * hp:o + 2 * hp + 2]
    g = (h @ Wl.T + bl).astype(f32)
    if not tangents:
        return g, None
    J = np.stack([(ti @ Wl.T).astype(f32) for ti in t], axis=2)
    return g, J


def chain(blob, K, hp, x):
    """(y, [log-det of every record], their sum) of nf_lipmlp_chain."""
    blob = np.asarray(blob, f32)
    x = np.asarray(x, f32).copy()
    lds = []
    for q in range(K):
        hdr = blob[q * HDR:(q + 1) * HDR]
        kind = int(hdr[0])
        if kind == 0:
            off = K * HDR + int(hdr[11]) * rstride(hp)
            g, J = net(hdr, blob[off:off + rstride(hp)], x, hp)
            x = (x + g).astype(f32)
            det = ((J[:, 0, 0] + f32(1)) * (J[:, 1, 1] + f32(1)) - J[:, 0, 1] * J[:, 1, 0]).astype(f32)
            lds.append(np.log(np.abs(det)).astype(f32))
        else:
            e, t = hdr[6:8], hdr[8:10]
            x = ((x * e + t) if kind == 1 else ((x - t) * e)).astype(f32)
            lds.append(np.full(x.shape[0], hdr[10], f32))
    total = np.zeros(x.shape[0], f32)
    for l in lds:
        total = (total + l).astype(f32)
    return x, lds, total


def fixed_point(blob, hp, y, atol=1e-5, rtol=1e-5, cap=1000):
    """(x, further steps) of the sampling route's loop over nf_lipmlp_apply mode 1 on a K = 1 blob."""
    blob = np.asarray(blob, f32)
    y = np.asarray(y, f32)
    hdr, W = blob[:HDR], blob[HDR:]

    def step(x):
        out = (y - net(hdr, W, x, hp, tangents=False)[0]).astype(f32)
        d = (out - x).astype(f32)
        return out, int(np.sum(~(d * d / (f32(atol) + np.abs(y) * f32(rtol)) < 1)))

    x, bad = step(y)
    i = 0
    while bad:
        x, bad = step(x)
        i += 1
        if i > cap:
            break
    return x, i
