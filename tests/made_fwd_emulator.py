"""numpy walk-through of the one-launch MADE forward exactly as csrc/made_fwd.hip performs it, driven by the packed blob / table
of flows/made_pack.py: every wave walks its own stream (bias group, then the A fragments of the item) in the kernel's item order.
Test infrastructure: validates the packing (slot order, per-wave streams, prefix k-group counts, biases, the wrap-around copy) on
CPU against the dense masked MADE."""
import numpy as np

HDR, ROWS, KG, RING = 32, 32, 8, 8


def _rows_from_stream(a, nkg):
    return a.reshape(nkg, 2, ROWS, 4).transpose(2, 0, 1, 3).reshape(ROWS, KG * nkg)


def _bias_from_group(g):
    g = g.reshape(4, 2, ROWS, 4)
    assert np.array_equal(g, np.broadcast_to(g[:, :, :1, :], g.shape))      # the same for every lane of a half
    return g[:, :, 0, :].reshape(32)                                          # index 8 q + 4 hh + i


def emulate_forward(blob, table, x):
    """MADE output (B, mult D) in the reference's row order, float64 arithmetic on the packed float32 weights."""
    blob = blob.astype(np.float64)
    D, Dp, H, Hp, NSB, NB, mult, NFB, nrounds, total, nitems = [int(v) for v in table[:11]]
    assert blob.size == total and nitems == 2 * (1 + 2 * NB) + 2 * nrounds and Hp == 256 * NSB and Dp % 32 == 0
    tab = table[HDR:HDR + 8 * nitems * 2].reshape(8, nitems, 2)
    x = np.asarray(x, dtype=np.float64)
    B = x.shape[0]
    xin = np.zeros((B, Dp))
    xin[:, :D] = x
    pos = [int(table[16 + w]) for w in range(8)]
    start = list(pos)

    def item(w, i, act):
        nkg, rb = int(tab[w, i, 0]), int(tab[w, i, 1])
        if rb < 0:
            return rb, None
        acc = np.tile(_bias_from_group(blob[pos[w]:pos[w] + 4 * 256]), (B, 1))
        pos[w] += 4 * 256
        if nkg:
            assert nkg % 4 == 0 and KG * nkg <= act.shape[1]
            W = _rows_from_stream(blob[pos[w]:pos[w] + 256 * nkg], nkg)
            acc = acc + act[:, :KG * nkg] @ W.T
            pos[w] += 256 * nkg
        return rb, acc

    def hidden_layer(l, act):
        out = np.full((B, Hp), np.nan)
        for w in range(8):
            for s in range(2):
                rb, acc = item(w, 2 * l + s, act)
                out[:, rb * ROWS:(rb + 1) * ROWS] = acc
        assert not np.isnan(out).any()                       # every row-block has exactly one owner
        return out

    h = hidden_layer(0, xin)                                 # initial layer: raw h0
    plain = bool(table[13])
    for b in range(NB):                                      # nets/made.py:196-214
        t = hidden_layer(1 + 2 * b, np.maximum(h, 0.0))
        if plain:                                            # x -> W0 -> relu -> W1 -> relu -> Wf: the final layer sees relu(t)
            assert NB == 1 and (tab[:, 4:6, 1] == -1).all()
            h = np.maximum(t, 0.0)
            break
        h = h + hidden_layer(2 + 2 * b, np.maximum(t, 0.0))
    out = np.full((B, NFB * ROWS), np.nan)
    for r in range(nrounds):                                 # the final layer sees the raw block output (:303-304)
        for w in range(8):
            for s in range(2):
                rb, acc = item(w, 2 * (1 + 2 * NB) + 2 * r + s, h)
                if rb >= 0:
                    out[:, rb * ROWS:(rb + 1) * ROWS] = acc
    assert not np.isnan(out).any()
    for w in range(8):                                       # the wrap-around copy behind every stream
        n = pos[w] - start[w]
        assert np.array_equal(blob[pos[w]:pos[w] + RING * 256], np.resize(blob[start[w]:pos[w]], RING * 256)), w
        assert pos[w] + RING * 256 == (int(table[16 + w + 1]) if w < 7 else total) and n > 0
    return out[:, :(int(table[12]) if table[12] else mult * D)]


def work_per_wave(table):
    """MFMAs per wave and 64-row tile (a k-group of a row-block = 4 MFMAs per 32-sample block)."""
    NSB, NB, nitems = int(table[4]), int(table[5]), int(table[10])
    tab = table[HDR:HDR + 8 * nitems * 2].reshape(8, nitems, 2)
    nh = 2 * (1 + 2 * NB)                                   # hidden items: NSB sample blocks each; final items: one
    return 4 * (NSB * tab[:, :nh, 0].sum(axis=1) + tab[:, nh:, 0].sum(axis=1))


def work_fraction(table):
    """MFMAs the schedule executes / the dense count (padded sizes)."""
    D, Dp, H, Hp, NSB, NB, mult, NFB, nrounds, total, nitems = [int(v) for v in table[:11]]
    dense = (Hp // ROWS) * (Dp // KG) + 2 * NB * (Hp // ROWS) * (Hp // KG) + NFB * (Hp // KG)
    return int(work_per_wave(table).sum()) / (8 * dense)


def emulate_forward_spline(blob, table, x):
    """The spline variant (flows/made_pack.py spline=True): (B, D, 24) parameter lists as the kernel's lanes hold them (widths /
    heights carry log2(e)), float64 arithmetic on the packed float32 weights."""
    blob = blob.astype(np.float64)
    D, Dp, H, Hp, NSB, NB, mult, G, nfi, total, nitems, spl = [int(v) for v in table[:12]]
    assert spl == 1 and mult == 23 and blob.size == total and nitems == 2 * (1 + 2 * NB) + nfi
    tab = table[HDR:HDR + 8 * nitems * 2].reshape(8, nitems, 2)
    x = np.asarray(x, dtype=np.float64)
    B = x.shape[0]
    xin = np.zeros((B, Dp))
    xin[:, :D] = x
    pos = [int(table[16 + w]) for w in range(8)]
    start = list(pos)

    def hidden_layer(l, act):
        out = np.full((B, Hp), np.nan)
        for w in range(8):
            for s in range(2):
                nkg, rb = int(tab[w, 2 * l + s, 0]), int(tab[w, 2 * l + s, 1])
                acc = np.tile(_bias_from_group(blob[pos[w]:pos[w] + 1024]), (B, 1))
                pos[w] += 1024
                if nkg:
                    acc = acc + act[:, :KG * nkg] @ _rows_from_stream(blob[pos[w]:pos[w] + 256 * nkg], nkg).T
                    pos[w] += 256 * nkg
                out[:, rb * ROWS:(rb + 1) * ROWS] = acc
        assert not np.isnan(out).any()
        return out

    h = hidden_layer(0, xin)
    for b in range(NB):
        t = hidden_layer(1 + 2 * b, np.maximum(h, 0.0))
        h = h + hidden_layer(2 + 2 * b, np.maximum(t, 0.0))
    prm = np.full((B, 4 * G, 24), np.nan)
    nh = 2 * (1 + 2 * NB)
    seen = set()
    for w in range(8):
        for j in range(nfi):
            nkg, g = int(tab[w, nh + j, 0]), int(tab[w, nh + j, 1])
            if g < 0:
                continue
            assert g not in seen and nkg % 4 == 0
            seen.add(g)
            acc = np.zeros((3, B, ROWS))
            for r3 in range(3):
                acc[r3] = np.tile(_bias_from_group(blob[pos[w]:pos[w] + 1024]), (B, 1))
                pos[w] += 1024
            if nkg:
                frag = blob[pos[w]:pos[w] + 3 * 256 * nkg].reshape(nkg, 3, 256)
                pos[w] += 3 * 256 * nkg
                for r3 in range(3):
                    acc[r3] += h[:, :KG * nkg] @ _rows_from_stream(np.ascontiguousarray(frag[:, r3]).reshape(-1), nkg).T
            for r3 in range(3):
                for rho in range(ROWS):
                    q, hh, i = rho >> 3, (rho >> 2) & 1, rho & 3
                    v = 16 * r3 + 4 * q + i
                    prm[:, 4 * g + 2 * hh + v // 24, v % 24] = acc[r3][:, rho]
    assert seen == set(range(G))
    for w in range(8):
        assert np.array_equal(blob[pos[w]:pos[w] + RING * 256], np.resize(blob[start[w]:pos[w]], RING * 256)), w
        assert pos[w] + RING * 256 == (int(table[16 + w + 1]) if w < 7 else total)
    return prm[:, :D]


# ---- the register weight ring over two tiles of one persistent workgroup (csrc/mlp_tile.hpp MfRing) ---------------------------------
class RingWalk:
    """One wave's MfRing on stream-entry INDICES (an entry = 256 floats: one 16-byte load per lane), exactly as mlp_tile.hpp moves it:
    mf_ring_start requests entries 0..7 once; every consumed entry is re-requested 8 entries ahead of the item's own position
    (`ap + e + 8`); items with an even number of 4-entry groups swap the ring halves; the tile loop only resets `ap` -- nothing is
    reloaded between tiles.  Every value the kernel multiplies with is checked to BE the stream entry the schedule means (by index, or --
    behind the wrap -- by content), and no request may leave the wave's stream."""

    def __init__(self, blob, start, end):
        assert (end - start) % 256 == 0 and 0 <= start < end <= blob.size
        self.e = blob[start:end].reshape(-1, 256)
        self.a = list(range(8))                              # mf_ring_start
        assert len(self.e) >= 8
        self.ap, self.last, self.consumed = 0, 7, 0

    def _take(self, idx, e):                                 # mf_take / the bias and A reads of mf_item, mf_group
        held, want = self.a[idx], self.ap + e
        assert held == want or np.array_equal(self.e[held], self.e[want]), (
            "ring register %d holds stream entry %d where the item reads entry %d" % (idx, held, want))
        nxt = self.ap + e + 8
        assert nxt < len(self.e), "request of entry %d behind the wave's stream of %d entries" % (nxt, len(self.e))
        self.a[idx] = nxt
        self.last = max(self.last, nxt)
        self.consumed += 1

    def _swap(self):
        self.a = self.a[4:] + self.a[:4]

    def item(self, nkg):                                     # mf_item: 4 bias entries + nkg A entries
        assert nkg % 4 == 0
        for q in range(4):
            self._take(q, q)
        kg = 0
        while kg + 8 <= nkg:
            for j in range(4):
                self._take(4 + j, 4 + kg + j)
            for j in range(4):
                self._take(j, 8 + kg + j)
            kg += 8
        if kg < nkg:
            for j in range(4):
                self._take(4 + j, 4 + kg + j)
        else:
            self._swap()
        self.ap += 4 + nkg

    def final_item(self, nkg):                               # mf_final_item: 12 bias entries + 3 nkg A entries, compile-time phases
        assert nkg % 4 == 0
        for e in range(12):
            self._take(e & 7, e)
        kg = 0
        while kg + 8 <= nkg:
            for k in range(8):
                for r3 in range(3):
                    self._take((4 + 3 * k + r3) & 7, 12 + 3 * kg + 3 * k + r3)
            kg += 8
        if kg < nkg:
            for k in range(4):
                for r3 in range(3):
                    self._take((4 + 3 * k + r3) & 7, 12 + 3 * kg + 3 * k + r3)
        else:
            self._swap()
        self.ap += 12 + 3 * nkg

    def next_tile(self):                                     # `ring.ap = stream + lane * 4` at the top of the persistent loop
        """The ring must hold stream entries 0..7 (the packer's wrap copy behind the stream); returns the entries one tile consumed."""
        n = self.ap
        assert self.a == list(range(n, n + 8)), ("ring phase at the end of a tile", self.a, n)
        for j in range(8):
            assert np.array_equal(self.e[self.a[j]], self.e[j]), "ring register %d does not hold stream entry %d at the start of the next tile" % (j, j)
        assert len(self.e) == n + 8, "the stream is %d entries, a tile consumes %d (+ 8 of the wrap)" % (len(self.e), n)
        self.ap = 0
        return n


def two_tile_ring_walk(blob, table, entry=2):
    """Two tiles of a persistent workgroup of made_fwd_kernel / made_fwd_ft_kernel / made_fwd_train*_kernel over every wave's stream:
    hidden items through mf_item, the final items through mf_item (`entry` = 2: [nkg, rb | feature]; nf_made_forward, _ft, _train) or
    mf_final_item (spline groups, hdr[11] = 1); entries with a negative id are skipped and consume nothing.  Returns the number of
    4-entry groups each wave consumes per tile."""
    NB, nitems = int(table[5]), int(table[10])
    groups_final = int(table[11]) == 1
    nh = 2 * (1 + 2 * NB)
    tab = table[HDR:HDR + 8 * nitems * entry].reshape(8, nitems, entry)
    total = int(table[9])                                    # (a training pack's periodic feed follows the streams)
    assert total <= blob.size
    out = []
    for w in range(8):
        ring = RingWalk(blob, int(table[16 + w]), int(table[16 + w + 1]) if w < 7 else total)
        per_tile = []
        for tile in range(2):
            for i in range(nitems):
                nkg, ident = int(tab[w, i, 0]), int(tab[w, i, 1])
                if ident < 0:
                    assert nkg == 0
                    continue
                if i >= nh and groups_final:
                    ring.final_item(nkg)
                else:
                    ring.item(nkg)
            per_tile.append(ring.next_tile())
        assert per_tile[0] == per_tile[1] and per_tile[0] % 4 == 0 and ring.last < len(ring.e)
        out.append(per_tile[0] // 4)
    return out


def two_tile_ring_walk_backward(blob, table):
    """two_tile_ring_walk for made_bwd_kernel (flows/made_pack._pack_backward_from: entries [nkg, rb, kg0, -]): the 2 NC chunk items of
    Wf^T and the 4 NB block items always run; only a round of the last product W0^T skips (rb < 0) and consumes nothing."""
    NB, NC, nitems, total = int(table[5]), int(table[7]), int(table[10]), int(table[9])
    tab = table[HDR:HDR + 8 * nitems * 4].reshape(8, nitems, 4)
    nh = 2 * NC + 4 * NB
    assert total <= blob.size and nitems == nh + max(int(table[8]), 1)
    out = []
    for w in range(8):
        ring = RingWalk(blob, int(table[16 + w]), int(table[16 + w + 1]) if w < 7 else total)
        per_tile = []
        for tile in range(2):
            for i in range(nitems):
                nkg, rb = int(tab[w, i, 0]), int(tab[w, i, 1])
                if rb < 0:                                   # (also the plain-MLP mode's absent second linear)
                    assert nkg == 0 and (i >= nh or int(table[13]))
                    continue
                ring.item(nkg)
            per_tile.append(ring.next_tile())
        assert per_tile[0] == per_tile[1] and per_tile[0] % 4 == 0 and ring.last < len(ring.e)
        out.append(per_tile[0] // 4)
    return out
