"""numpy float32 walk-through of nf_affine_wide exactly as csrc/affine_wide.hip (made_fwd_body.hpp, EPI 4) performs it, driven by the
packed blob / table of flows/affine_wide_pack.py: every wave walks its own stream (bias group, then the A fragments of the item) in
the kernel's item order with the table's k-group counts; the x tile holds 0 for the zero-fed features; the ReLU keeps NaN; final
rows 2 f / 2 f + 1 are feature f's scale / shift parameter; the element-wise map follows the feature table's modes and hdr[24]; the
log-det is summed in the kernel's order (per lane-half over its 8 features of a row-block, the two halves, then the row-blocks 0..7).
Test infrastructure: validates the packing on the CPU against the reference's stored outputs."""
import numpy as np

from made_fwd_emulator import HDR, KG, RING, ROWS, _bias_from_group, _rows_from_stream

MASKED, EXP, SIGMOID, SIGMOID_INV, NONE = 4, 0, 1, 2, 3
F = np.float32


def modes_of(table):
    D, Dp, nitems = int(table[0]), int(table[1]), int(table[10])
    words = table[HDR + 8 * nitems * 2:HDR + 8 * nitems * 2 + Dp // 16].view(np.uint32)
    assert table.size == HDR + 8 * nitems * 2 + Dp // 16
    m = ((words[:, None] >> (2 * np.arange(16, dtype=np.uint32))[None, :]) & 3).reshape(-1).astype(np.int64)
    assert (m[D:] == 0).all()
    return m[:D]


def items_of(table):
    nitems = int(table[10])
    return table[HDR:HDR + 8 * nitems * 2].reshape(8, nitems, 2)


def _relu(v):
    return np.where(v < 0, F(0), v)          # (NaN stays NaN: torch's LeakyReLU(0))


def conditioner(blob, table, z):
    """(B, NFB * 32) final-layer outputs in float32, the streams walked as the kernel walks them."""
    D, Dp, H, Hp, NSB, NB, mult, NFB, nrounds, total, nitems = [int(v) for v in table[:11]]
    assert blob.dtype == np.float32 and blob.size == total and int(table[13]) == 1 and NB == 1 and nrounds == 1 and NFB <= 8
    assert nitems == 2 * 3 + 2 and Hp == 256 * NSB and Dp % 32 == 0
    tab = items_of(table)
    assert (tab[:, 4:6, 1] == -1).all() and (tab[:, 4:6, 0] == 0).all()          # no second linear of a block
    modes = modes_of(table)
    z = np.asarray(z, dtype=F)
    B = z.shape[0]
    xin = np.zeros((B, Dp), dtype=F)
    xin[:, :D] = np.where(modes[None, :] == 2, F(0), z)
    pos = [int(table[16 + w]) for w in range(8)]
    start = list(pos)

    def item(w, i, act):
        nkg, rb = int(tab[w, i, 0]), int(tab[w, i, 1])
        if rb < 0:
            assert nkg == 0
            return rb, None
        acc = np.tile(_bias_from_group(blob[pos[w]:pos[w] + 4 * 256]), (B, 1)).astype(F)
        pos[w] += 4 * 256
        if nkg:
            assert nkg % 4 == 0 and KG * nkg <= act.shape[1]
            W = _rows_from_stream(blob[pos[w]:pos[w] + 256 * nkg], nkg)
            with np.errstate(invalid="ignore", over="ignore"):
                acc = acc + (act[:, :KG * nkg] @ W.T).astype(F)
            pos[w] += 256 * nkg
        return rb, acc

    def hidden_layer(l, act):
        # 512 slots: wave w owns row-blocks {w, 15 - w} for both sample blocks; 256 slots: row-block w for sample block 0 and 7 - w for
        # sample block 1 (wave 7 - w holds the other halves: the same weights once more)
        out = np.zeros((2, B, Hp), dtype=F)
        owned = set()
        for w in range(8):
            for s in range(2):
                rb, acc = item(w, 2 * l + s, act)
                assert rb == (w if s == 0 else Hp // ROWS - 1 - w)       # (the kernel takes the row-block from w, not from the table)
                for sb in ((0, 1) if NSB == 2 else (s,)):
                    assert (sb, rb) not in owned                          # one owner per row-block and sample block
                    owned.add((sb, rb))
                    out[sb][:, rb * ROWS:(rb + 1) * ROWS] = acc
        assert len(owned) == 2 * (Hp // ROWS) and np.array_equal(out[0], out[1], equal_nan=True)
        return out[0]

    h = _relu(hidden_layer(0, xin))
    h = _relu(hidden_layer(1, h))
    out = np.zeros((2, B, 8 * ROWS), dtype=F)                # final row-block w for sample block 0, 7 - w for sample block 1
    owned = set()
    for w in range(8):
        for s in range(2):
            rb, acc = item(w, 6 + s, h)
            want = w if s == 0 else 7 - w
            assert rb == (want if want < NFB else -1)
            if rb >= 0:
                assert (s, rb) not in owned
                owned.add((s, rb))
                out[s][:, rb * ROWS:(rb + 1) * ROWS] = acc
    assert owned == {(s, rb) for s in range(2) for rb in range(NFB)} and np.array_equal(out[0], out[1], equal_nan=True)
    out = out[0]
    for w in range(8):                                       # the wrap-around copy behind every stream
        n = pos[w] - start[w]
        assert n > 0 and np.array_equal(blob[pos[w]:pos[w] + RING * 256], np.resize(blob[start[w]:pos[w]], RING * 256)), w
        assert pos[w] + RING * 256 == (int(table[16 + w + 1]) if w < 7 else total)
    return out


def emulate(blob, table, z, direction):
    """(y, log-det) of nf_affine_wide with acc = write."""
    D = int(table[0])
    smap = int(table[24])
    modes = modes_of(table)
    z = np.asarray(z, dtype=F)
    B = z.shape[0]
    out = conditioner(blob, table, z)
    y = z.copy()
    term = np.zeros((B, 16 * 8), dtype=F)                    # per feature: what it adds to the log-det
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for f in range(D):
            mode = int(modes[f])
            if mode == 0 and smap != MASKED:
                continue
            sc, sh, v = out[:, 2 * f].copy(), out[:, 2 * f + 1].copy(), z[:, f]
            if smap == MASKED:
                bi = F(1) if mode == 0 else F(0)
                if not int(table[25]) & 1:
                    sc[:] = 0
                if not int(table[25]) & 2:
                    sh[:] = 0
                sc[~np.isfinite(sc)] = np.nan
                sh[~np.isfinite(sh)] = np.nan
                zm = bi * v
                if direction == 0:
                    y[:, f] = zm + (F(1) - bi) * (v * np.exp(sc) + sh)
                else:
                    y[:, f] = zm + (F(1) - bi) * (v - sh) * np.exp(-sc)
                term[:, f] = (F(1) - bi) * sc
            elif smap == NONE:
                y[:, f] = v + sh if direction == 0 else v - sh
            elif smap == EXP:
                y[:, f] = v * np.exp(sc) + sh if direction == 0 else (v - sh) * np.exp(-sc)
                term[:, f] = sc
            else:
                sg = F(1) / (F(1) + np.exp(-(sc + F(2))))
                lg = np.log(sg)
                if smap == SIGMOID:
                    y[:, f] = v / sg + sh if direction == 0 else (v - sh) * sg
                    term[:, f] = -lg
                else:
                    y[:, f] = v * sg + sh if direction == 0 else (v - sh) / sg
                    term[:, f] = lg
        ld = np.zeros(B, dtype=F)
        for fb in range(8):                                  # lane-half hh owns features 16 fb + 4 q + 2 hh + e, in the order q, e
            half = []
            for hh in range(2):
                a = np.zeros(B, dtype=F)
                for q in range(4):
                    for e in range(2):
                        f = 16 * fb + 4 * q + 2 * hh + e
                        if f < D and (modes[f] != 0 or smap == MASKED):
                            a = a + term[:, f]
                half.append(a)
            part = half[0] + half[1]
            ld = ld + (part if direction == 0 else -part)
    assert y.dtype == F and ld.dtype == F
    return y, ld
