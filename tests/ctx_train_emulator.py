"""numpy walk of csrc/resnet_ctx_train.hip over the padded blob, table and weight-gradient jobs of flows/ctx_train_pack.py: the
training forward, the input-gradient backward and the tiled weight gradients, in float64, reading every matrix at the offsets the
kernels read (tests/test_host_ctx_train.py checks it against autograd through the float64 ResidualNet)."""
import numpy as np

from normflows_amd.flows.ctx_train_pack import JOB, RT_B0, RT_BF, RT_BLK, RT_W0, RT_W0T, RT_WCT, RT_WF, RT_WFT


def _m(blob, off, rows, cols):
    return blob[off:off + rows * cols].reshape(rows, cols)


def emulate(blob, table, jobs, x, c, g_out):
    """(out, g_x, g_c, flat weight / bias gradients) of the gated net for x (B, nI), c (B, C) and the output gradient g_out (B, O)."""
    nI, C, PI, Kin, H, Hp, NB, O, Op = [int(v) for v in table[:9]]
    PC = Kin - PI
    B = x.shape[0]
    Bp = (B + 63) // 64 * 64
    xin = np.zeros((Bp, Kin))
    xin[:B, :nI] = x
    xin[:B, PI:PI + C] = c
    relu = lambda v: np.maximum(v, 0.0)
    sig = lambda v: 1.0 / (1.0 + np.exp(-v))
    save = [xin @ _m(blob, table[RT_W0], Hp, Kin).T + blob[table[RT_B0]:table[RT_B0] + Hp]]
    h = save[0]
    for b in range(NB):
        bt = table[RT_BLK + 8 * b:RT_BLK + 8 * b + 8]
        t = relu(h) @ _m(blob, bt[0], Hp, Hp).T + blob[bt[1]:bt[1] + Hp]
        u = relu(t) @ _m(blob, bt[2], Hp, Hp).T + blob[bt[3]:bt[3] + Hp]
        sa = sig(xin[:, PI:] @ _m(blob, bt[4], Hp, PC).T + blob[bt[5]:bt[5] + Hp])
        h = h + u * sa
        save += [t, u, sa, h]
    out = (h @ _m(blob, table[RT_WF], Op, Hp).T + blob[table[RT_BF]:table[RT_BF] + Op])[:B, :O]

    gout = np.zeros((Bp, Op))
    gout[:B, :O] = g_out
    g = gout @ _m(blob, table[RT_WFT], Hp, Op).T
    G = [None] * (3 * NB + 1)
    gin = np.zeros((Bp, Kin))
    for b in reversed(range(NB)):
        bt = table[RT_BLK + 8 * b:RT_BLK + 8 * b + 8]
        t, u, sa = save[1 + 4 * b], save[2 + 4 * b], save[3 + 4 * b]
        ga = g * u * sa * (1.0 - sa)
        gu = g * sa
        gt = (gu @ _m(blob, bt[6], Hp, Hp).T) * (t > 0)
        gin[:, PI:] += ga @ _m(blob, table[RT_WCT + b], PC, Hp).T
        g = g + (gt @ _m(blob, bt[7], Hp, Hp).T) * (save[4 * b] > 0)
        G[1 + 3 * b], G[2 + 3 * b], G[3 + 3 * b] = gt, gu, ga
    G[0] = g
    gin += g @ _m(blob, table[RT_W0T], Kin, Hp).T

    nflat = int(max(j[9] + j[1] * j[10] for j in jobs))
    nflat = max(nflat, int(max(j[11] + j[1] for j in jobs)))
    flat = np.full(nflat, np.nan)
    for j in np.asarray(jobs).reshape(-1, JOB):
        gsel, N, asel, akoff, KP, rl, K1, P1, K2, wout, ldW, bout, n0, k0 = [int(v) for v in j[:14]]
        Gm = gout[:B] if gsel < 0 else G[gsel][:B]
        A = (xin if asel < 0 else save[asel])[:B, akoff:]
        if rl:
            A = relu(A)
        for nl in range(64):
            n = n0 + nl
            if n >= N:
                continue
            for kl in range(64):
                p = k0 + kl
                col = -1 if p >= KP else (p if p < K1 else -1) if p < P1 else (K1 + p - P1 if p - P1 < K2 else -1)
                if col >= 0:
                    flat[wout + n * ldW + col] = Gm[:, n] @ A[:, p]
            if bout >= 0 and k0 == 0:
                flat[bout + n] = Gm[:, n].sum()
    return out, gin[:B, :nI], gin[:B, PI:PI + C], flat
