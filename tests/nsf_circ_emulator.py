"""numpy float64 walk-through of the circular NSF coupling layer exactly as csrc/nsf_circ.hip runs it from the blob / table / ftable of
flows/nsf_circ_pack.py: the x tile in position order, the conditioner's input fed through the per-feature table (ft_feed: the periodic
features of a circular identity coordinate), nsf_wide's streams for the network (tests/nsf_wide_emulator.py walks them), the lane's 3 K
slots per transform feature (K widths | K heights | derivatives 1 .. K - 1 | derivative 0) through the spline with type and bound of the
feature's position, the batch-shared spline on the identity half before (sampling) or after (density) the conditioner, and 0 / log-det 0
outside an interval in both halves.  Test infrastructure: pins packing, table and order on CPU against the reference's outputs."""
import numpy as np

from arnsf_ft_emulator import FT_BOUND, FT_COL, FT_TAILS, feed
from nsf_wide_emulator import emulate_conditioner

LOG2E = 1.4426950408889634


def _spline(oracle, K, kind, bound, w, h, d_full, x, inverse):
    """One feature's spline under list tails (utils/splines.py:48-57): d_full (B, K + 1) logits with the edges overwritten by type --
    the oracle's linear tails take logits 1 .. K - 1, its circular tails 0 .. K - 1 --, and 0 / 0 outside the interval (:31-32)."""
    d = d_full[:, 1:K] if kind == 1 else d_full[:, :K]
    y, lad = oracle.rqs_spline(np.ascontiguousarray(x), np.ascontiguousarray(w), np.ascontiguousarray(h), np.ascontiguousarray(d),
                               inverse=inverse, tails="linear" if kind == 1 else "circular", tail_bound=float(bound))
    out = ~((x >= -bound) & (x <= bound))
    return np.where(out, 0.0, y), np.where(out, 0.0, lad)


def emulate_layer(oracle, blob, table, ftable, uncond, x, direction, min_derivative=1e-3):
    """(y (B, D), logdet (B), conditioner parameter lists (B, nT, 3 K) as the lanes hold them) of rows x (B, D) in `direction` (0 density,
    1 sampling).  uncond = (widths (nI, K), heights (nI, K), derivatives (nI, K + 1)) of the batch-shared spline, float64."""
    D, Dp, H, Hp, NB, nI, nT, par_i, par_t, G, nfi, total, nhi, has_lu, TR, PI = [int(v) for v in table[:16]]
    K = int(table[24])
    assert has_lu == 0 and int(table[25]) == 1 and Hp in (128, 256) and ftable.shape == (8, Dp) and ftable.dtype == np.float32
    codes, bound = ftable[FT_TAILS].view(np.int32), ftable[FT_BOUND].astype(np.float64)
    col = ftable[FT_COL].view(np.int32)
    assert np.array_equal(col[:nI], np.arange(par_i, D, 2)) and np.array_equal(col[PI:PI + nT], np.arange(par_t, D, 2))
    assert (col[nI:PI] == -1).all() and (col[PI + nT:] == -1).all() and not ftable[1:, nI:PI].any() and not ftable[1:, PI + nT:].any()
    assert not ftable[3:, PI:].any()                                 # the preprocessing only touches identity features
    x = np.asarray(x, dtype=np.float64)
    B = x.shape[0]
    tile = np.zeros((B, Dp))
    tile[:, :nI] = x[:, par_i::2]
    tile[:, PI:PI + nT] = x[:, par_t::2]
    ld = np.zeros(B)
    uw, uh, ud = uncond

    def identity(inverse):
        nonlocal ld
        for i in range(nI):
            y, lad = _spline(oracle, K, int(codes[i]), bound[i], np.tile(uw[i], (B, 1)), np.tile(uh[i], (B, 1)), np.tile(ud[i], (B, 1)),
                             tile[:, i], inverse)
            tile[:, i] = y
            ld += lad

    if direction == 1:
        identity(True)
    fed = np.zeros((B, D))                                           # the fed identity positions, handed on as columns of a row
    for i in range(nI):
        fed[:, par_i + 2 * i] = feed(ftable, i, tile[:, i])
    prm, _ = emulate_conditioner(blob, table, fed, 0)               # (contracts over the identity positions only)
    for j in range(nT):
        p = prm[:, j]
        d_full = np.concatenate([p[:, 3 * K - 1:], p[:, 2 * K:3 * K - 1], np.zeros((B, 1))], 1)   # slot 3K - 1 = derivative 0; K unused
        sc = LOG2E                                                    # widths / heights carry log2(e) / sqrt(hidden): exp2 = softmax
        y, lad = _spline(oracle, K, int(codes[PI + j]), bound[PI + j], p[:, :K] / sc, p[:, K:2 * K] / sc, d_full, tile[:, PI + j],
                         direction == 1)
        tile[:, PI + j] = y
        ld += lad
    if direction == 0:
        identity(False)
    out = np.zeros((B, D))
    out[:, par_i::2] = tile[:, :nI]
    out[:, par_t::2] = tile[:, PI:PI + nT]
    return out, ld, prm


def two_tile_ring_walk(blob, table):
    """Two tiles of a persistent workgroup of nsf_circ_kernel over every wave's stream (made_fwd_emulator.RingWalk = mlp_tile.hpp's
    MfRing on entry indices): (1 + 2 NB) nhi hidden items through mf_item, nfi final items [nkg, group, sample block] through
    mf_final_item with its compile-time ring phases; an entry with group < 0 is skipped and consumes nothing.  At the start of the
    second tile the ring must hold stream entries 0..7 and no request may have left the wave's stream.  Returns the number of 4-entry
    groups each wave consumes per tile."""
    from made_fwd_emulator import RingWalk
    HDR = 32
    NB, nfi, total, nhi, has_lu = int(table[4]), int(table[10]), int(table[11]), int(table[12]), int(table[13])
    assert has_lu == 0 and total == blob.size
    nh = (1 + 2 * NB) * nhi
    tab = table[HDR:HDR + 8 * (nh + nfi) * 3].reshape(8, nh + nfi, 3)
    out = []
    for w in range(8):
        ring = RingWalk(blob, int(table[16 + w]), int(table[16 + w + 1]) if w < 7 else total)
        per_tile = []
        for tile in range(2):
            for i in range(nh + nfi):
                nkg, ident = int(tab[w, i, 0]), int(tab[w, i, 1])
                if i < nh:
                    assert ident >= 0
                    ring.item(nkg)
                elif ident >= 0:
                    ring.final_item(nkg)
                else:
                    assert nkg == 0
            per_tile.append(ring.next_tile())
        assert per_tile[0] == per_tile[1] and per_tile[0] % 4 == 0 and ring.last < len(ring.e)
        out.append(per_tile[0] // 4)
    return out
