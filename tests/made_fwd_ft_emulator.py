"""numpy walk-through of the per-feature density kernel exactly as csrc/made_fwd_ft.hip performs it (made_fwd_ft_kernel,
nf_made_forward_spline_ft), driven by the blob / table / ftable of flows/made_pack.pack_made_forward_ft: the degree-order gather of
the tile, the periodic feed, every wave's stream of items with their masked k-group ranges, the final layer's one item per feature
with its slot layout, the scatter back to columns.  Test infrastructure: validates the packing and the schedule on CPU."""
import numpy as np

from arnsf_ft_emulator import FT_COL, feed

HDR, ROWS, KG, TR, NW = 32, 32, 8, 64, 8
SLOT_H, SLOT_D = 11, 21


def _bias(flat):
    """[4 q][2 hh][32 m][4] -> b[8 q + 4 hh + i] (every lane m of a half holds the same four)."""
    g = flat.reshape(4, 2, ROWS, 4)
    assert (g == g[:, :, :1]).all()
    return g[:, :, 0, :].reshape(ROWS)


def _a(flat, nkg):
    """[nkg][2 hh][32 m][4] -> W[m][8 kg + 4 hh + i]."""
    return flat.reshape(nkg, 2, ROWS, 4).transpose(2, 0, 1, 3).reshape(ROWS, KG * nkg)


def read_streams(blob, table):
    """Per wave the items in consumption order: [(nkg, id, bias (32,), W (32, 8 nkg))]; the stream ends with a copy of its first 8
    entries (the ring wraps into the next tile)."""
    nitems = int(table[10])
    out = []
    for w in range(NW):
        off = start = int(table[16 + w])
        items = []
        for i in range(nitems):
            nkg, ident = (int(v) for v in table[HDR + 2 * (w * nitems + i):HDR + 2 * (w * nitems + i) + 2])
            if ident < 0:
                assert nkg == 0
                items.append(None)
                continue
            assert nkg % 4 == 0
            b = _bias(blob[off:off + 4 * 256]); off += 4 * 256
            W = _a(blob[off:off + nkg * 256], nkg); off += nkg * 256
            items.append((nkg, ident, b, W))
        end = int(table[16 + w + 1]) if w + 1 < NW else int(table[9])
        assert end - off == 8 * 256 and np.array_equal(blob[off:end], np.resize(blob[start:off], 8 * 256))
        out.append(items)
    return out


def emulate_forward_ft(blob, table, ftable, x, element):
    """`element(f, slots (rows, 32), x_f (rows,)) -> (y_f, logabsdet_f)`: the density-direction spline of the schedule's feature f on
    its 32-slot parameter list (widths 0.., heights 11.., derivative logit j in slot 21 + j; the caller reads type and bound from
    ftable as the kernel does).  Returns (y, logdet), y in COLUMN order."""
    blob = blob.astype(np.float64)
    x = np.asarray(x, dtype=np.float64)
    B = x.shape[0]
    D, Dp, H, Hp, NSB, NB, mult = (int(v) for v in table[:7])
    nfi = int(table[8])
    assert ftable.shape == (8, D) and ftable.dtype == np.float32 and int(table[11]) == 2
    col = ftable[FT_COL].view(np.int32)
    assert sorted(col.tolist()) == list(range(D))
    streams = read_streams(blob, table)
    HRB = 8 * NSB
    nh = 2 * (1 + 2 * NB)
    assert int(table[10]) == nh + nfi
    y = np.zeros((B, D))
    ld = np.zeros(B)
    for row0 in range(0, B, TR):
        nrows = min(TR, B - row0)
        raw = np.zeros((TR, Dp))
        fed = np.zeros((TR, Dp))
        for f in range(D):
            raw[:nrows, f] = x[row0:row0 + nrows, col[f]]
            fed[:, f] = feed(ftable, f, raw[:, f])

        def layer(l, inp, add=None):
            """Hidden layer l over every wave's two items; NSB = 1: item s covers sample block s only."""
            out = np.zeros((TR, Hp)) if add is None else add.copy()
            done = np.zeros((TR, HRB), dtype=int)
            for w in range(NW):
                for s in range(2):
                    nkg, rb, b, W = streams[w][2 * l + s]
                    assert rb == (w, HRB - 1 - w)[s]
                    rows = slice(0, TR) if NSB == 2 else slice(32 * s, 32 * s + 32)
                    out[rows, 32 * rb:32 * rb + 32] += inp[rows, :KG * nkg] @ W.T + b
                    done[rows, rb] += 1
            assert (done == 1).all()
            return out
        h = layer(0, fed)
        for b in range(NB):
            t = layer(1 + 2 * b, np.maximum(h, 0))
            h = layer(2 + 2 * b, np.maximum(t, 0), add=h)
        seen = np.zeros(D, dtype=int)
        yt = raw.copy()
        for w in range(NW):
            for j in range(nfi):
                it = streams[w][nh + j]
                if it is None:
                    continue
                nkg, f, b, W = it
                slots = h[:, :KG * nkg] @ W.T + b
                yf, lad = element(f, slots, raw[:, f])
                yt[:, f] = yf
                ld[row0:row0 + nrows] += np.asarray(lad)[:nrows]
                seen[f] += 1
        assert (seen == 1).all()
        for f in range(D):
            y[row0:row0 + nrows, col[f]] = yt[:nrows, f]
    return y, ld


def two_tile_ring_walk(blob, table):
    """Two tiles of a persistent workgroup of made_fwd_ft_kernel over every wave's stream (made_fwd_emulator.RingWalk = mlp_tile.hpp's
    MfRing on entry indices): 2 (1 + 2 NB) hidden items, then nfi final items [nkg, feature], all through mf_item -- four bias entries +
    nkg A entries each; `if (f < 0) continue;` consumes nothing.  At the start of the second tile the ring must hold stream entries
    0..7 (it is not reloaded) and no request may have left the wave's stream.  Returns the number of 4-entry groups each wave consumes
    per tile."""
    from made_fwd_emulator import two_tile_ring_walk as walk
    assert int(table[11]) == 2
    return walk(blob, table)
