"""NumPy float64 restatement of the formulas of csrc/density2d.hip and csrc/gmm.hip: the same records, the same analytic gradients
with the same conventions at the kinks (abs: derivative 0 at 0; the 2-norm and the 4-norm: derivative 0 at the origin), the same
streaming log-sum-exp, the same four sums of the mixture's backward.  tests/test_host_targets.py checks it against the float64 legs
of the reference's fixtures: that pins the mathematics the kernels implement without a GPU."""
import numpy as np

TWO_MODES, SINUSOIDAL, SIN_GAP, SIN_SPLIT, SMILEY, RINGS, CIRC_GMM = range(7)


def _sign(x):
    return (x > 0).astype(np.float64) - (x < 0).astype(np.float64)


def _ring(z0, z1, loc, inv_den):
    n = np.sqrt(z0 * z0 + z1 * z1)
    u = (n - loc) * inv_den
    with np.errstate(divide="ignore", invalid="ignore"):
        gn = np.where(n > 0, -u * inv_den / n, 0.0)
    return -0.5 * u * u, gn * z0, gn * z1


def _two_bumps(a, eps, inv_s, c):
    v = (a - eps) * inv_s
    e = np.exp(-c * (a * eps))
    sg = e / (1 + e)
    return -0.5 * v * v + np.log(1 + e), -v * inv_s - sg * c * eps, v * inv_s - sg * c * a


def _envelope(z0, z1, k4):
    a, b = z0 * z0, z1 * z1
    return -0.5 * (a * a + b * b) * k4, -2 * a * z0 * k4, -2 * b * z1 * k4


def _stream_lse(ts, ds):
    """Streaming log-sum-exp over modes: ts / ds = per-mode (B) values and tuples of (B) derivatives.  Returns (lse, sums of the
    softmax-weighted derivatives)."""
    mx, S, T = ts[0].copy(), np.ones_like(ts[0]), [d.copy() for d in ds[0]]
    for t, d in zip(ts[1:], ds[1:]):
        up = t > mx
        with np.errstate(over="ignore"):       # (the branch np.where does not take)
            f = np.where(up, np.exp(mx - t), 1.0)
            e = np.where(up, 1.0, np.exp(t - mx))
        S = S * f + e
        T = [Tk * f + e * dk for Tk, dk in zip(T, d)]
        mx = np.where(up, t, mx)
    return mx + np.log(S), [Tk / S for Tk in T]


def density2d(z, kind, n, rec, scale=None):
    """(lp (B), d lp / d z (B, 2)) as the kernel computes them, in float64.  rec: the record of dist_route.record."""
    z = np.asarray(z, dtype=np.float64)
    z0, z1 = z[:, 0], z[:, 1]
    p = list(rec) + [0.0] * 8
    if kind == TWO_MODES:
        v, g0, g1 = _ring(z0, z1, p[0], p[1])
        b, da, _ = _two_bumps(np.abs(z0), p[2], p[3], p[4])
        v, g0 = v + b, g0 + da * _sign(z0)
    elif kind == SMILEY:
        v, g0, g1 = _ring(z0, z1, p[0], p[1])
        y = z1 + p[2]
        u = (np.abs(y) - p[3]) * p[1]
        v, g1 = v - 0.5 * u * u, g1 - u * p[1] * _sign(y)
    elif kind in (SINUSOIDAL, SIN_GAP, SIN_SPLIT):
        v, g0, g1 = _envelope(z0, z1, p[2])
        sn, dw1 = np.sin(p[0] * z0), p[0] * np.cos(p[0] * z0)
        if kind == SINUSOIDAL:
            u = (z1 - sn) * p[1]
            v, g1, g0 = v - 0.5 * u * u, g1 - u * p[1], g0 + u * p[1] * dw1
        else:
            t = (z0 - p[5]) / p[6]
            if kind == SIN_GAP:
                h = p[4] * np.exp(-0.5 * t * t) * 0.5
                dh = -h * t / p[6]
            else:
                sg = 1 / (1 + np.exp(-t))
                h = p[4] * sg * 0.5
                dh = h * (1 - sg) / p[6]
            y = z1 - sn + h
            b, da, deps = _two_bumps(np.abs(y), np.abs(h), p[1], p[3])
            dy = da * _sign(y)
            v, g1, g0 = v + b, g1 + dy, g0 + dy * (dh - dw1) + deps * _sign(h) * dh
    elif kind == RINGS:
        nrm = np.sqrt(z0 * z0 + z1 * z1)
        us = [nrm - p[0] * (i + 1) for i in range(n)]
        v, (T0,) = _stream_lse([-(u * u) * p[1] for u in us], [(-2 * u * p[1],) for u in us])
        with np.errstate(divide="ignore", invalid="ignore"):
            gn = np.where(nrm > 0, T0 / nrm, 0.0)
        g0, g1 = gn * z0, gn * z1
    elif kind == CIRC_GMM:
        s = float(scale)
        inv2s2 = 1 / (2 * s * s)
        cx = [2 * np.sin(p[0] * i) for i in range(n)]
        cy = [2 * np.cos(p[0] * i) for i in range(n)]
        v, (g0, g1) = _stream_lse([-((z0 - a) ** 2 + (z1 - b) ** 2) * inv2s2 for a, b in zip(cx, cy)],
                                  [(-2 * (z0 - a) * inv2s2, -2 * (z1 - b) * inv2s2) for a, b in zip(cx, cy)])
        v = v - np.log(p[1] * s * s * n)
    else:
        raise ValueError(kind)
    return v, np.stack([g0, g1], 1)


def gmm_record(loc, log_scale, weight_scores):
    """R = [loc | log_scale | log_softmax(weight_scores)] from the (1, M, d), (1, M, d), (1, M) parameters."""
    ws = np.asarray(weight_scores, dtype=np.float64).reshape(-1)
    logw = ws - ws.max() - np.log(np.exp(ws - ws.max()).sum())
    return np.concatenate([np.asarray(loc, np.float64).reshape(-1), np.asarray(log_scale, np.float64).reshape(-1), logw])


def _gmm_terms(z, R, M):
    d = z.shape[1]
    loc, ls, logw = R[:M * d].reshape(M, d), R[M * d:2 * M * d].reshape(M, d), R[2 * M * d:]
    inv = np.exp(-ls)
    u = (z[:, None, :] - loc[None]) * inv[None]                    # eps (B, M, d)
    t = (logw - 0.5 * d * np.log(2 * np.pi) - ls.sum(1))[None] - 0.5 * (u * u).sum(2)
    return u, inv, t


def gmm_log_prob(z, R, M):
    z = np.asarray(z, dtype=np.float64)
    _, _, t = _gmm_terms(z, R, M)
    lp, _ = _stream_lse([t[:, m] for m in range(M)], [()] * M)
    return lp


def gmm_log_prob_bwd(z, R, M, lp, g):
    """(gz (B, d), gR (2 M d + M)): the responsibilities recomputed from the saved lp, then the kernel's four sums."""
    z = np.asarray(z, dtype=np.float64)
    u, inv, t = _gmm_terms(z, R, M)
    w = g[:, None] * np.exp(t - lp[:, None])                       # g_b r_bm
    gl = w[:, :, None] * u * inv[None]                             # w (z - loc) e^{-2 ls}
    gz = -gl.sum(1)
    gloc = gl.sum(0)
    gls = (w[:, :, None] * (u * u - 1)).sum(0)
    return gz, np.concatenate([gloc.reshape(-1), gls.reshape(-1), w.sum(0)])


def gmm_leaf_grads(gR, weight_scores, M, d):
    """The record's gradient carried to the leaves: loc and log_scale as they are, weight_scores through log_softmax's backward."""
    ws = np.asarray(weight_scores, dtype=np.float64).reshape(-1)
    sm = np.exp(ws - ws.max())
    sm /= sm.sum()
    glw = gR[2 * M * d:]
    return gR[:M * d].reshape(1, M, d), gR[M * d:2 * M * d].reshape(1, M, d), (glw - sm * glw.sum()).reshape(1, M)
