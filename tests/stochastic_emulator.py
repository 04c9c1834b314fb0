"""NumPy float64 restatement of the arithmetic of csrc/hmc2d.hip: the target of a launch as one or two weighted terms (the seven
kinds of target_emulator.density2d, or kind 7: a 2-D diagonal Gaussian), the HMC transition with the clipped force, the Metropolis
test on `u < prob`, the tangents of z_new to log_step_size and log_mass (the force is a constant: running scalars per dimension),
the backward with its parameter sums, and the random-walk Metropolis-Hastings steps.  tests/test_host_stochastic.py checks it
against the float64 legs of the reference's fixtures: that pins the mathematics the kernels implement without a GPU."""
import numpy as np

import target_emulator as te

GAUSS = 7


def target(terms, z):
    """(lp (B), d lp / d z (B, 2)) of terms = [(weight, kind, n, record, a0, a1)]: a0 = scale for kind 6; a0, a1 = loc, log_scale
    (two floats each) for kind 7."""
    z = np.asarray(z, dtype=np.float64)
    lp, g = np.zeros(len(z)), np.zeros((len(z), 2))
    for w, kind, n, rec, a0, a1 in terms:
        if kind == GAUSS:
            loc, ls = np.asarray(a0, np.float64).reshape(2), np.asarray(a1, np.float64).reshape(2)
            inv = np.exp(-ls)
            u = (z - loc) * inv
            v, gv = -np.log(2 * np.pi) - ls.sum() - 0.5 * (u * u).sum(1), -u * inv
        else:
            v, gv = te.density2d(z, kind, n, rec, None if a0 is None else float(np.asarray(a0).reshape(-1)[0]))
        lp, g = lp + w * v, g + w * gv
    return lp, g


def _clip(g, c):
    return np.clip(g, -c, c) if c else g


def hmc2d(terms, z, eps, u, lss, lm, steps, clip=0.0):
    """One transition: dict with z_out, log_det, accept, log_ratio (log of the acceptance probability) and the sidecar's
    tan_lss, tan_lm (B, 2) = d z_new / d log_step_size, d z_new / d log_mass, g_in, g_out = grad log p at z and at z_out; lp_in,
    lp_new, kin_in, kin_new: the four terms of the log-ratio."""
    z, eps, u = (np.asarray(a, dtype=np.float64) for a in (z, eps, u))
    lss, lm = np.asarray(lss, np.float64).reshape(2), np.asarray(lm, np.float64).reshape(2)
    s, em = np.exp(lss), np.exp(lm)
    p = eps * np.exp(0.5 * lm)
    lp0, g_in = target(terms, z)
    zn, pn, lpn, gn = z.copy(), p.copy(), lp0, g_in
    zs, zm, ps, pm = np.zeros_like(z), np.zeros_like(z), np.zeros_like(z), 0.5 * p
    for _ in range(steps):
        gc = _clip(gn, clip)
        ph = pn + (s / 2) * gc
        ps = ps + (s / 2) * gc
        zn = zn + s * (ph / em)
        zs = zs + s * (ph / em) + s * (ps / em)
        zm = zm + s * (pm / em - ph / em)
        lpn, gn = target(terms, zn)
        gc = _clip(gn, clip)
        pn = ph + (s / 2) * gc
        ps = ps + (s / 2) * gc
    lr = lpn - lp0 - 0.5 * (pn * pn / em).sum(1) + 0.5 * (p * p / em).sum(1)
    with np.errstate(over="ignore", divide="ignore"):
        acc = u < np.exp(lr)
    a2 = acc[:, None]
    return {"z_out": np.where(a2, zn, z), "log_det": np.where(acc, lp0 - lpn, 0.0), "accept": acc, "log_ratio": lr, "tan_lss": zs,
            "tan_lm": zm, "g_in": g_in, "g_out": np.where(a2, gn, g_in), "lp_in": lp0, "lp_new": lpn, "kin_in": 0.5 * (p * p / em).sum(1),
            "kin_new": 0.5 * (pn * pn / em).sum(1)}


def hmc2d_bwd(fwd, gz_out, gld):
    """(gz (B, 2), g log_step_size (2), g log_mass (2)) from hmc2d's dict and the cotangents (None = zero)."""
    B = len(fwd["accept"])
    gz_out = np.zeros((B, 2)) if gz_out is None else np.asarray(gz_out, np.float64)
    gld = np.zeros(B) if gld is None else np.asarray(gld, np.float64)
    gz = gz_out + gld[:, None] * (fwd["g_in"] - fwd["g_out"])
    v = fwd["accept"][:, None] * (gz_out - gld[:, None] * fwd["g_out"])
    return gz, (v * fwd["tan_lss"]).sum(0), (v * fwd["tan_lm"]).sum(0)


def mh2d(terms, z, eps, u, scale, steps):
    """`steps` random-walk steps: dict with z_out, log_det, accept (steps, B), log_ratio (steps, B), g_in, g_out, and lp_cur,
    lp_prop (steps, B): the two log-densities of each step's ratio."""
    z, eps, u = (np.asarray(a, dtype=np.float64) for a in (z, eps, u))
    sc = np.asarray(scale, np.float64).reshape(-1)
    sc = np.array([sc[0], sc[-1]])
    lp, g = target(terms, z)
    g_in, ld = g, np.zeros(len(z))
    accs, lrs, lps, lqs = [], [], [], []
    for i in range(steps):
        q = eps[i] * sc + z
        lq, h = target(terms, q)
        lr = lq - lp
        lps.append(lp), lqs.append(lq)
        with np.errstate(over="ignore", divide="ignore"):
            acc = u[i] <= np.minimum(np.exp(lr), 1.0)
        acc &= ~np.isnan(lr)
        z = np.where(acc[:, None], q, z)
        ld = np.where(acc, ld + (lp - lq), ld)
        lp, g = np.where(acc, lq, lp), np.where(acc[:, None], h, g)
        accs.append(acc), lrs.append(lr)
    return {"z_out": z, "log_det": ld, "accept": np.array(accs).reshape(steps, len(z)), "log_ratio": np.array(lrs).reshape(steps, len(z)),
            "g_in": g_in, "g_out": g, "lp_cur": np.array(lps).reshape(steps, len(z)), "lp_prop": np.array(lqs).reshape(steps, len(z))}


def mh2d_bwd(fwd, gz_out, gld):
    gz = np.zeros_like(fwd["g_in"]) if gz_out is None else np.asarray(gz_out, np.float64)
    return gz if gld is None else gz + np.asarray(gld, np.float64)[:, None] * (fwd["g_in"] - fwd["g_out"])
