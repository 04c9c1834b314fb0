"""numpy walk-through of the per-feature variant of the incremental AR-NSF inverse exactly as csrc/maf_inverse.hip performs it
(maf_inverse_kernel<true, true>, nf_arnsf_inverse_ft), driven by the blob / table / ftable of
flows/maf_pack.pack_made(made, mult, rows=True, features=(tails, tail_bound)).  Test infrastructure: validates the packing and the
schedule on CPU."""
import numpy as np

from maf_emulator import ENT, HDR, MAX_STEPS, TILE, _from_a_operand

FT_COL, FT_TAILS, FT_BOUND, FT_SCALE, FT_WSIN, FT_WCOS, FT_BIAS, FT_PERIODIC = range(8)


def feed(ftable, f, x):
    """What the conditioner reads of the finished feature f (ft_feed): the periodic features of a circular coordinate, else x."""
    if int(ftable[FT_PERIODIC].view(np.int32)[f]) == 0:
        return x
    a = np.float64(ftable[FT_SCALE, f]) * x
    return np.float64(ftable[FT_WSIN, f]) * np.sin(a) + np.float64(ftable[FT_WCOS, f]) * np.cos(a) + np.float64(ftable[FT_BIAS, f])


def emulate_inverse_ft(blob, table, ftable, z, element):
    """`element(f, params (B, mult), z_f (B,)) -> (x_f, logabsdet_f)`: the inverse spline of the schedule's feature f (the caller reads
    its tails type and bound from ftable[FT_TAILS, f] / ftable[FT_BOUND, f] as the kernel does).  Returns (x, logdet) with x in
    COLUMN order."""
    blob = blob.astype(np.float64)
    z = np.asarray(z, dtype=np.float64)
    B = z.shape[0]
    D, Dp, H, Hp, T, mult = [int(v) for v in table[:6]]
    assert ftable.shape == (8, D) and ftable.dtype == np.float32
    col = ftable[FT_COL].view(np.int32)
    y = np.zeros((B, D))
    X = np.zeros((B, Dp))                      # the feature scratch: conditioner inputs in degree order
    S = np.zeros((5, B, Hp))
    x0, ld = element(0, np.broadcast_to(blob[:mult], (B, mult)), z[:, col[0]])
    ld = np.array(ld, dtype=np.float64)
    y[:, col[0]] = x0
    X[:, 0] = feed(ftable, 0, x0)
    for t in range(T):
        e = HDR + ENT * t
        dlo, ns, K0, off = [int(v) for v in table[e:e + 4]]
        masks = table[e + 4:e + 4 + MAX_STEPS].view(np.uint32)
        Kh = TILE * t

        def a_block(K):
            nonlocal off
            a = _from_a_operand(blob[off:off + K * TILE], K) if K else np.zeros((TILE, 0))
            off += K * TILE
            return a
        A0 = a_block(K0)
        Ah = [a_block(Kh) for _ in range(4)]
        AF = [a_block(Kh) for _ in range(ns)]
        bias = blob[off:off + 5 * TILE].reshape(5, TILE); off += 5 * TILE
        W0d = blob[off:off + TILE * MAX_STEPS].reshape(TILE, MAX_STEPS); off += TILE * MAX_STEPS
        Wd = blob[off:off + 4 * TILE * TILE].reshape(4, TILE, TILE); off += 4 * TILE * TILE
        biasF = blob[off:off + ns * TILE].reshape(ns, TILE); off += ns * TILE
        WFd = blob[off:off + ns * mult * TILE].reshape(ns, mult, TILE); off += ns * mult * TILE
        pre = np.zeros((5, B, TILE))
        pre[0] = X[:, :K0] @ A0.T + bias[0]
        for l in range(1, 5):
            pre[l] = S[l - 1][:, :Kh] @ Ah[l - 1].T + bias[l]
        xg = np.zeros((B, MAX_STEPS + 1))
        xg[:, 0] = X[:, dlo - 1]                # the carry: the previous tile's last feed
        for s in range(ns):
            f = dlo + s
            units = [u for u in range(TILE) if (int(masks[s]) >> u) & 1]
            for u in units:
                h = pre[0][:, u] + xg[:, :MAX_STEPS] @ W0d[u]
                pre[2][:, u] += h
                pre[0][:, u] = np.maximum(h, 0)
            for u in units:
                pre[1][:, u] = np.maximum(pre[1][:, u] + pre[0] @ Wd[0][u], 0)
            for u in units:
                h1 = pre[2][:, u] + pre[1] @ Wd[1][u]
                pre[4][:, u] += h1
                pre[2][:, u] = np.maximum(h1, 0)
            for u in units:
                pre[3][:, u] = np.maximum(pre[3][:, u] + pre[2] @ Wd[2][u], 0)
            for u in units:
                pre[4][:, u] = pre[4][:, u] + pre[3] @ Wd[3][u]
            prm = (S[4][:, :Kh] @ AF[s].T + biasF[s])[:, :mult] + pre[4] @ WFd[s].T
            xn, d = element(f, prm, z[:, col[f]])
            ld = ld + d
            y[:, col[f]] = xn
            g = feed(ftable, f, xn)
            X[:, f] = g
            xg[:, s + 1] = g
        for l in range(5):
            S[l][:, TILE * t:TILE * (t + 1)] = pre[l]
    return y, ld
