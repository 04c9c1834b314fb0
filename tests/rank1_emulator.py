"""NumPy emulator of the rank-1 chain kernels' arithmetic (csrc/rank1_chain.hip) on the records P (K, 2 d + 4) of
flows/rank1_pack.py, in float32: forward and inverse with the saved scalars, and the backward that starts from the OUTPUT and
rebuilds every record's input from its output and the saved scalar.  Pins the formulas and the reconstruction without a GPU."""
import numpy as np

F = np.float32


def _act(kind, lin, slope):
    """h, h', h'', hg of a Planar record: tanh with sech^2 = 4 e^2 / (1 + e^2)^2, e = exp(-|lin|); leaky with the (x < 0) rule.
    hg = the derivative on the path of z' (LeakyReLU's own backward: x > 0 ? 1 : slope): differs from h' at lin == 0 only."""
    if kind == 0:
        e = np.exp(-np.abs(lin), dtype=F)
        e2 = e * e
        q = F(1) + e2
        h = np.tanh(lin, dtype=F)
        hp = F(4) * e2 / (q * q)
        return h, hp, F(-2) * h * hp, hp
    neg = lin < 0
    return (np.where(neg, slope * lin, lin).astype(F), np.where(neg, slope, F(1)).astype(F), np.zeros_like(lin),
            np.where(lin > 0, F(1), slope).astype(F))


def _record(P, d, ri):
    rec = P[ri]
    return int(rec[0]), rec[1], rec[2], rec[3], rec[4:4 + d], rec[4 + d:4 + 2 * d]


def forward(P, x, direction=0):
    """(y, ld, save (K, B)) of x (B, d) through the records, direction 0 forward / 1 inverse (records reversed, leaky only)."""
    P, v = np.asarray(P, F), np.array(x, F)
    K, (B, d) = P.shape[0], v.shape
    ld, save = np.zeros(B, F), np.zeros((K, B), F)
    with np.errstate(all="ignore"):
        for q in range(K):
            kind, s0, s1, s2, A, Bv = _record(P, d, q if direction == 0 else K - 1 - q)
            if kind == 2:
                dz = v - A
                r = np.sqrt((dz * dz).sum(1, dtype=F))
                c = s0 + r
                h, h_ = s1 / c, -s1 * r / (c * c)
                v = v + h[:, None] * dz
                ld = ld + s2 * np.log(F(1) + h) + np.log(F(1) + h + h_)
                save[q] = r
            else:
                lin = (v * A).sum(1, dtype=F) + s0
                save[q] = lin
                if direction == 0:
                    h, hp, _, _ = _act(kind, lin, s2)
                    v = v + h[:, None] * Bv
                    ld = ld + np.log(np.abs(F(1) + s1 * hp))
                else:
                    assert kind == 1, "only leaky Planar records have an inverse"
                    a_ = np.where(lin < 0, s2, F(1)).astype(F)
                    inner = a_ * s1
                    v = v - (a_ * lin / (F(1) + inner))[:, None] * Bv
                    ld = ld - np.log(np.abs(F(1) + inner))
    return v.astype(F), ld.astype(F), save


def backward(P, y, save, gy, gld, direction=0):
    """(gz, gP) from the output y, the saved scalars and the cotangents: the kernels' walk."""
    P, v, g, gl = np.asarray(P, F), np.array(y, F), np.array(gy, F), np.asarray(gld, F)
    K, (B, d) = P.shape[0], v.shape
    gP = np.zeros_like(P)
    with np.errstate(all="ignore"):
        for q in range(K - 1, -1, -1):
            ri = q if direction == 0 else K - 1 - q
            kind, s0, s1, s2, A, Bv = _record(P, d, ri)
            s = save[q]
            if kind == 2:
                c = s0 + s
                h = s1 / c
                dz = (v - A) / (F(1) + h)[:, None]
                v = A + dz
                c2 = c * c
                h_ = -s1 * s / c2
                D2 = F(1) + h + h_
                gh = (g * dz).sum(1, dtype=F) + gl * (s2 / (F(1) + h) + F(1) / D2)
                gh_ = gl / D2
                dh, t3 = -s1 / c2, F(2) * s1 * s / (c2 * c)
                g_r = gh * dh + gh_ * (dh + t3)
                gP[ri, 1] = (gh * dh + gh_ * t3).sum(dtype=F)
                gP[ri, 2] = (gh / c - gh_ * s / c2).sum(dtype=F)
                gdz = g * h[:, None] + np.where(s > 0, g_r / np.where(s > 0, s, F(1)), F(0))[:, None] * dz
                g = g + gdz
                gP[ri, 4:4 + d] = -gdz.sum(0, dtype=F)
            else:
                ug = (g * Bv).sum(1, dtype=F)
                if direction == 0:
                    h, hp, hpp, hg = _act(kind, s, s2)
                    D = F(1) + s1 * hp
                    g_lin = ug * hg + gl * s1 * hpp / D
                    gs1 = gl * hp / D
                    zc = h
                else:
                    a_ = np.where(s < 0, s2, F(1)).astype(F)
                    den = F(1) / (F(1) + a_ * s1)
                    zc = -(a_ * s * den)
                    g_lin = -ug * a_ * den
                    gs1 = ug * a_ * a_ * s * den * den - gl * a_ * den
                v = v - zc[:, None] * Bv
                gP[ri, 1], gP[ri, 2] = g_lin.sum(dtype=F), gs1.sum(dtype=F)
                gP[ri, 4 + d:4 + 2 * d] = (g * zc[:, None]).sum(0, dtype=F)
                gP[ri, 4:4 + d] = (g_lin[:, None] * v).sum(0, dtype=F)
                g = g + g_lin[:, None] * A
    return g.astype(F), gP
