"""A float32 NumPy restatement of the d-dimensional residual-flow kernels' arithmetic (csrc/lipmlp_nd.hip) on the packed blob
(flows/lipmlp_nd_pack.py): from blob, noise and coefficients alone it gives what nf_lipmlp_nd_chain / nf_lipmlp_nd_apply compute.  It
reads the blob by the layout table of include/nf_mi355x.h -- headers, affine slots, weight blocks, zero padding to hp and dp -- and
the coefficient convention a_k = (-1)^(k+1) coef(k) / k, so a packer or a table that drifts from the kernels' shows up on a machine
without a GPU.  The products are NumPy's: the summation order inside a product differs from the kernels' FMA chains."""
import numpy as np

HDR = 16
F = np.float32


def dpad(d):
    return (d + 3) // 4 * 4


def rstride(hp, d):
    return 2 * hp * hp + 2 * dpad(d) * hp + 3 * hp + dpad(d)


def blob_floats(K, nres, hp, d):
    return K * HDR + K * 2 * dpad(d) + nres * rstride(hp, d)


def swish(p, c):
    """(f(p), f'(p)) of f(p) = p sigmoid(c p) / 1.1, as lm_swish writes them."""
    s = F(1) / (F(1) + np.exp(-c * p, dtype=F))
    return (p * s / F(1.1)).astype(F), ((s + c * p * s * (F(1) - s)) / F(1.1)).astype(F)


def block(blob, K, ri, hp, d):
    dp = dpad(d)
    w = blob[K * HDR + K * 2 * dp + ri * rstride(hp, d):][:rstride(hp, d)]
    o = 0
    out = {}
    for name, n, shape in (("W0", dp * hp, (dp, hp)), ("b0", hp, (hp,)), ("W1", hp * hp, (hp, hp)), ("b1", hp, (hp,)),
                           ("W2", hp * hp, (hp, hp)), ("b2", hp, (hp,)), ("Wl", hp * dp, (hp, dp)), ("bl", dp, (dp,))):
        out[name] = w[o:o + n].reshape(shape)
        o += n
    assert o == rstride(hp, d)
    return out


def value(hdr, blk, x):
    """(g(x) (B, dp), [f'(x), f'(p_1), ...]) of one network on padded rows x (B, dp)."""
    nmid = min(max(int(hdr[1]), 0), 2)
    a, d0 = swish(x, F(hdr[2]))
    derivs = [d0]
    h, dh = swish(a @ blk["W0"] + blk["b0"], F(hdr[3]))
    derivs.append(dh)
    for m in range(nmid):
        h, dh = swish(h @ blk["W%d" % (1 + m)] + blk["b%d" % (1 + m)], F(hdr[4 + m]))
        derivs.append(dh)
    return (h @ blk["Wl"] + blk["bl"]).astype(F), derivs


def tangent(hdr, blk, derivs, w):
    """J w through the same weights: t = w o f'(x); t <- (t W) o f'(p) per hidden layer; the last product has no Swish behind it."""
    nmid = min(max(int(hdr[1]), 0), 2)
    t = ((w * derivs[0]) @ blk["W0"]) * derivs[1]
    for m in range(nmid):
        t = (t @ blk["W%d" % (1 + m)]) * derivs[2 + m]
    return (t @ blk["Wl"]).astype(F)


def chain(blob, K, nres, hp, d, x, vareps, terms, coefs):
    """(y (B, d), [log-det of every record in execution order, (B)]) of nf_lipmlp_nd_chain."""
    blob = np.asarray(blob, dtype=F)
    assert blob.size == blob_floats(K, nres, hp, d), (blob.size, blob_floats(K, nres, hp, d))
    dp = dpad(d)
    B = x.shape[0]
    xs = np.zeros((B, dp), dtype=F)
    xs[:, :d] = x
    lds = []
    for q in range(K):
        hdr = blob[q * HDR:(q + 1) * HDR]
        kind = int(hdr[0])
        if kind == 0:
            ri = min(max(int(hdr[11]), 0), nres - 1)
            blk = block(blob, K, ri, hp, d)
            v = np.zeros((B, dp), dtype=F)
            v[:, :d] = vareps[ri]
            g, derivs = value(hdr, blk, xs)
            xs = xs + g
            w, ld, sgn = v, np.zeros(B, dtype=F), F(1)
            for k in range(1, int(terms[ri]) + 1):
                w = tangent(hdr, blk, derivs, w)
                ld = (ld + sgn * F(coefs[ri][k - 1]) / F(k) * (v * w).sum(1, dtype=F)).astype(F)
                sgn = -sgn
            lds.append(ld)
        else:
            e = blob[K * HDR + q * 2 * dp:][:dp]
            t = blob[K * HDR + q * 2 * dp + dp:][:dp]
            xs = (xs * e + t if kind == 1 else (xs - t) * e).astype(F)
            lds.append(np.full(B, hdr[10], dtype=F))
    assert not xs[:, d:].any(), "a padded column left zero"
    return xs[:, :d], lds


def apply(blob, hp, d, x, y=None, atol=1e-5, rtol=1e-5):
    """nf_lipmlp_nd_apply: mode 0 (y None): x + g(x); mode 1: (y - g(x), the number of elements that have not converged)."""
    blob = np.asarray(blob, dtype=F)
    dp = dpad(d)
    xs = np.zeros((x.shape[0], dp), dtype=F)
    xs[:, :d] = x
    g = value(blob[:HDR], block(blob, 1, 0, hp, d), xs)[0][:, :d]
    if y is None:
        return x + g
    out = (y - g).astype(F)
    return out, int((~((out - x) ** 2 / (F(atol) + np.abs(y) * F(rtol)) < 1)).sum())


def sample(blob, hp, d, y):
    """(x, further steps) of the fixed-point iteration x <- y - g(x) from x = y under the reference's stop rule."""
    x, bad = apply(blob, hp, d, y, y)
    i = 0
    while bad and i <= 1000:
        x, bad = apply(blob, hp, d, x, y)
        i += 1
    return x, i
