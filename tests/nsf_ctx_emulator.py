"""numpy walk-through of the CONDITIONAL NSF coupling layer's conditioner exactly as csrc/nsf_ctx.hip walks the packed streams of
flows/nsf_ctx_pack.py: the x tile with the context at positions [Dp, Dp + PC), the initial layer as an identity item + a context item,
per residual block the W1 items, then per hidden item the GLU gate item (over the context positions) and the W2 item, h += u sigmoid(g);
the final layer in groups as tests/nsf_wide_emulator.py.  Test infrastructure: pins the packing on CPU against the dense ResidualNet."""
import numpy as np

from nsf_wide_emulator import _bias, _rows

HDR, ROWS, KG, RING = 32, 32, 8, 8


def emulate_conditioner_ctx(blob, table, x, context):
    """(B, nT, 3 K) parameter lists as the kernel's lanes hold them (widths / heights still carry log2(e) / sqrt(hidden)), from full
    rows x (B, D) and the context (B, C)."""
    blob = blob.astype(np.float64)
    D, Dp, H, Hp, NB, nI, nT, par_i, par_t, G, nfi, total, nhi, has_lu, TR, PI = [int(v) for v in table[:16]]
    K, C, PC = int(table[24]), int(table[25]), int(table[26])
    assert has_lu == 0 and Hp in (128, 256) and TR == (128 if Hp == 128 else 64) and nhi == 1
    assert PC == (C + 31) // 32 * 32 and Dp + PC <= 128 and PI % 32 == 0 and (Dp - PI) % 32 == 0
    MP = 3 * K
    FPL = 48 // MP
    FPG = 2 * FPL
    assert G == (nT + FPG - 1) // FPG
    nh = (2 + 3 * NB) * nhi
    nitems = nh + nfi
    tab = table[HDR:HDR + 8 * nitems * 3].reshape(8, nitems, 3)
    x = np.asarray(x, dtype=np.float64)
    context = np.asarray(context, dtype=np.float64)
    B = x.shape[0]
    assert context.shape == (B, C)
    tile = np.zeros((B, 128))                                 # positions: identity | transform | context | (unused)
    tile[:, :nI] = x[:, par_i::2]
    tile[:, PI:PI + nT] = x[:, par_t::2]
    tile[:, Dp:Dp + C] = context
    xin, xctx = tile[:, :Dp], tile[:, Dp:Dp + PC]
    pos = [int(table[16 + w]) for w in range(8)]
    start = list(pos)
    idx = [0] * 8

    def layer(act, want_kg):
        """The next hidden item of every wave over `act`: (B, Hp) output."""
        out = np.full((B, Hp), np.nan)
        for w in range(8):
            nkg, rb, sb0 = [int(v) for v in tab[w, idx[w]]]
            idx[w] += 1
            assert KG * nkg == want_kg and KG * nkg <= act.shape[1] and rb == w % (Hp // ROWS)
            assert not act[:, KG * nkg:].any()                 # what the k-loop skips is padding: exact zeros
            acc = np.tile(_bias(blob[pos[w]:pos[w] + 1024]), (B, 1))
            pos[w] += 1024
            acc = acc + act[:, :KG * nkg] @ _rows(blob[pos[w]:pos[w] + 256 * nkg], nkg).T
            pos[w] += 256 * nkg
            prev = out[:, rb * ROWS:(rb + 1) * ROWS]
            assert np.isnan(prev).all() or np.array_equal(prev, acc)
            out[:, rb * ROWS:(rb + 1) * ROWS] = acc
        assert not np.isnan(out).any()
        return out

    Kh = (H + 31) // 32 * 32
    h = layer(xin[:, :PI], PI)
    h = h + layer(xctx, PC)                                   # the context item: zero bias, added to the accumulators
    for b in range(NB):
        t = layer(np.maximum(h, 0.0), Kh)
        gate = 1.0 / (1.0 + np.exp(-layer(xctx, PC)))
        u = layer(np.maximum(t, 0.0), Kh)
        h = h + u * gate
    assert idx == [nh] * 8
    prm = np.zeros((B, FPG * G, MP))
    seen = set()
    for w in range(8):
        for j in range(nfi):
            nkg, g, sb0 = [int(v) for v in tab[w, nh + j]]
            if g < 0:
                continue
            assert (g, sb0) not in seen and sb0 in range(0, TR // 32, 2)
            seen.add((g, sb0))
            acc = np.zeros((3, B, ROWS))
            for r3 in range(3):
                acc[r3] = np.tile(_bias(blob[pos[w]:pos[w] + 1024]), (B, 1))
                pos[w] += 1024
            frag = blob[pos[w]:pos[w] + 3 * 256 * nkg].reshape(nkg, 3, 256)
            pos[w] += 3 * 256 * nkg
            assert KG * nkg == Kh and not h[:, KG * nkg:].any()
            for r3 in range(3):
                acc[r3] += h[:, :KG * nkg] @ _rows(np.ascontiguousarray(frag[:, r3]).reshape(-1), nkg).T
            for r3 in range(3):
                for rho in range(ROWS):
                    q, hh, i = rho >> 3, (rho >> 2) & 1, rho & 3
                    v = 16 * r3 + 4 * q + i
                    prm[:, FPG * g + FPL * hh + v // MP, v % MP] = acc[r3][:, rho]
    assert seen == {(g, sb0) for g in range(G) for sb0 in range(0, TR // 32, 2)}
    for w in range(8):
        assert np.array_equal(blob[pos[w]:pos[w] + RING * 256], np.resize(blob[start[w]:pos[w]], RING * 256)), w
        assert pos[w] + RING * 256 == (int(table[16 + w + 1]) if w < 7 else total) and pos[w] > start[w]
    return prm[:, :nT]
