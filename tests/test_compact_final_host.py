"""CPU-side tests of the COMPACT final section of the 8-bin fused blob (csrc/fused_common.hpp compact_row): the layout the
inference kernels stream is a bijection with the promised order, and a spline evaluated from its 21 rows per feature (logit 0 of
both softmaxes == 0) is the spline of the 23 original rows."""
import os

import numpy as np
import pytest

K, M, H = 8, 23, 128
NROWBLOCKS, DIFF = 21, 1 << 16


@pytest.fixture(scope="module")
def nfa():
    import __graft_entry__
    import normflows_amd
    if not os.path.exists(normflows_amd.native_library_path()):
        __graft_entry__.build()
    return normflows_amd


def _lane_half_slots(lib, hh):
    """The 336 entries of lane-half hh's list: C register reg of row-block rb is MFMA row 8 (reg / 4) + 4 hh + reg % 4."""
    return [lib.nf_rqs_fused_compact_row(K, rb, 8 * (reg >> 2) + 4 * hh + (reg & 3)) for rb in range(NROWBLOCKS) for reg in range(16)]


def test_compact_final_layout_is_a_bijection(nfa):
    lib = nfa._lib.lib()
    assert lib.nf_rqs_fused_compact_row(4, 0, 0) == -95 and lib.nf_rqs_fused_compact_row(16, 0, 0) == -95    # 8 bins only
    assert lib.nf_rqs_fused_compact_row(8, 21, 0) == -22 and lib.nf_rqs_fused_compact_row(8, 0, 32) == -22
    assert lib.nf_rqs_fused_compact_row(8, -1, 0) == -22
    every = [lib.nf_rqs_fused_compact_row(K, rb, rho) for rb in range(NROWBLOCKS) for rho in range(32)]
    assert all(e >= 0 for e in every) and len(set(every)) == 21 * 32          # 21 x 32 MFMA rows, no padding, nothing twice
    want = {(tf * M + p) | (DIFF if p < 2 * K else 0) for tf in range(32) for p in range(M) if p not in (0, K)}
    assert set(every) == want                                                 # 32 features x 21 compact rows
    seen = []
    for hh in range(2):
        slots = _lane_half_slots(lib, hh)
        assert len(slots) == 336
        for i in range(16):                                                   # 16 whole features, 21 values each, in order
            rows = slots[21 * i:21 * i + 21]
            tf = (rows[0] & (DIFF - 1)) // M
            assert rows == [(tf * M + 1 + c) | DIFF for c in range(7)] + [(tf * M + K + 1 + c) | DIFF for c in range(7)] + \
                [tf * M + 2 * K + c for c in range(7)]
            assert (tf % 8) // 4 == hh
            # pair j = i // 2 is group j of the 24-stage order: same two features, same order
            g = i // 2
            legacy = [lib.nf_rqs_fused_final_row(K, g, rb, 8 * (reg >> 2) + 4 * hh + (reg & 3)) for rb in range(3) for reg in range(16)]
            assert legacy[24 * (i % 2)] == tf * M
            seen.append(tf)
    assert sorted(seen) == list(range(32))
    # pair j's 42 values are complete after ceil(42 (j + 1) / 16) row-blocks
    assert [-(-42 * (j + 1) // 16) for j in range(8)] == [3, 6, 8, 11, 14, 16, 19, 21]


def test_pack_size_grows_by_the_compact_section(nfa):
    lib = nfa._lib.lib()
    for nblk in (0, 1, 2, 3, 7, 16):
        small = 128 + 256 * nblk + 768 + 864 + 128
        padded = -(-(small + 672) // 1024) * 1024
        assert nfa._lib.query("nf_rqs_fused_pack_size", 32, 32, 128, nblk, 8) == 4 * (64 + padded + (1 + 8 * nblk + 24 + 2 + 21) * 4096)
    small = 128 + 512 + 768 + 864 + 128
    assert small + 672 == 3072                      # two blocks: the compact biases fill exactly what was padding
    for Kb in (4, 16):                              # other bin counts: no compact section
        small = 128 + 512 + 96 * Kb + 32 * 3 * (Kb + 1) + 128
        assert nfa._lib.query("nf_rqs_fused_pack_size", 32, 32, 128, 2, Kb) == 4 * (64 + -(-small // 1024) * 1024 + (1 + 16 + 3 * Kb + 2) * 4096)


# ---- float64 emulation: the spline of the 23 rows == the spline of the 21 compact rows with logit 0 = 0 --------------------------
TB, MINW, MINH, MIND = 3.0, 1e-3, 1e-3, 1e-3


def _knots(e):
    """e: (..., 8) un-normalised softmax terms -> (..., 9) knots on [-TB, TB]."""
    w = MINW + (1 - MINW * K) * e / e.sum(-1, keepdims=True)
    c = np.concatenate([np.zeros(e.shape[:-1] + (1,)), np.cumsum(w, -1)], -1)
    c = 2 * TB * c - TB
    c[..., 0], c[..., -1] = -TB, TB
    return c


def _spline(x, ew, eh, dlog, inverse):
    """Rational-quadratic spline with linear tails (utils/splines.py:16-219) from un-normalised softmax TERMS (n, 8) and the 7 inner
    derivative logits (n, 7); returns (y, logabsdet)."""
    cw, ch = _knots(ew), _knots(eh)
    const = np.log(np.exp(1 - MIND) - 1)
    dl = np.concatenate([np.full((len(x), 1), const), dlog, np.full((len(x), 1), const)], -1)
    d = MIND + np.logaddexp(0.0, dl)
    inside = (x >= -TB) & (x <= TB)
    xs = np.where(inside, x, 0.0)
    srch = ch if inverse else cw
    b = np.clip((xs[:, None] >= srch[:, 1:-1]).sum(-1), 0, K - 1)
    take = lambda a, i: np.take_along_axis(a, i[:, None], -1)[:, 0]   # noqa: E731
    w0, wb = take(cw, b), take(cw, b + 1) - take(cw, b)
    h0, hb = take(ch, b), take(ch, b + 1) - take(ch, b)
    d0, d1 = take(d, b), take(d, b + 1)
    delta = hb / wb
    if not inverse:
        th = (xs - w0) / wb
        t1 = th * (1 - th)
        den = delta + (d0 + d1 - 2 * delta) * t1
        y = h0 + hb * (delta * th * th + d0 * t1) / den
    else:
        dy = xs - h0
        s = d0 + d1 - 2 * delta
        a = dy * s + hb * (delta - d0)
        bb = hb * d0 - dy * s
        c = -delta * dy
        th = 2 * c / (-bb - np.sqrt(bb * bb - 4 * a * c))
        y = th * wb + w0
        den = delta + s * th * (1 - th)
    lad = np.log(delta * delta * (d1 * th * th + 2 * delta * th * (1 - th) + d0 * (1 - th) ** 2)) - 2 * np.log(den)
    if inverse:
        lad = -lad
    return np.where(inside, y, x), np.where(inside, lad, 0.0)


@pytest.mark.parametrize("inverse", [False, True])
def test_compact_rows_give_the_spline_of_the_original_rows(nfa, inverse):
    lib = nfa._lib.lib()
    rng = np.random.default_rng(11 + inverse)
    n = 64
    W = rng.normal(size=(32 * M, H)) * 0.3
    b = rng.normal(size=32 * M)
    # features whose logit 0 sits 60 nats above (tf 3: widths, tf 9: heights) and below (tf 5, tf 12) the others
    sq = np.sqrt(H)
    b[3 * M + 0] += 60 * sq
    b[9 * M + K] += 60 * sq
    b[5 * M + 0] -= 60 * sq
    b[12 * M + K] -= 60 * sq
    h = np.maximum(rng.normal(size=(n, H)), 0.0) * 0.5
    x = rng.uniform(-3.6, 3.6, size=(n, 32))
    x[0, :4] = [-3.0, 3.0, 0.0, 3.0000001]
    # the 23 original rows: softmax of raw / sqrt(hidden) (nsf/coupling.py:334-339)
    raw = h @ W.T + b                                    # (n, 736)
    raw = raw.reshape(n, 32, M)
    uw, uh = raw[..., :K] / sq, raw[..., K:2 * K] / sq
    ew = np.exp(uw - uw.max(-1, keepdims=True))
    eh = np.exp(uh - uh.max(-1, keepdims=True))
    # the compact section as the packer lays it out: differences, then log2(e) / sqrt(hidden) on widths / heights
    wh_scale = np.log2(np.e) / sq
    comp = np.zeros((n, 2, 336))
    for hh in range(2):
        for v, cr in enumerate(_lane_half_slots(lib, hh)):
            row = cr & (DIFF - 1)
            if cr & DIFF:
                row0 = row - row % M + (0 if row % M < K else K)
                comp[:, hh, v] = (h @ (W[row] - W[row0]) + (b[row] - b[row0])) * wh_scale
            else:
                comp[:, hh, v] = h @ W[row] + b[row]
    worst_y = worst_l = 0.0
    for hh in range(2):
        for i in range(16):                              # the lane-half's i-th feature: pair i // 2, element i % 2
            g = i // 2
            tf = 8 * (g // 2) + 4 * hh + 2 * (g % 2) + i % 2
            v = comp[:, hh, 21 * i:21 * i + 21]
            lw = np.concatenate([np.zeros((n, 1)), v[:, :7]], -1)        # logit 0 == 0
            lh = np.concatenate([np.zeros((n, 1)), v[:, 7:14]], -1)
            cw = np.exp2(lw - lw.max(-1, keepdims=True))
            ch = np.exp2(lh - lh.max(-1, keepdims=True))
            y1, l1 = _spline(x[:, tf], cw, ch, v[:, 14:], inverse)
            y0, l0 = _spline(x[:, tf], ew[:, tf], eh[:, tf], raw[:, tf, 2 * K:], inverse)
            assert np.isfinite(y1).all() and np.isfinite(l1).all()
            worst_y = max(worst_y, float(np.abs(y1 - y0).max()))
            worst_l = max(worst_l, float(np.abs(l1 - l0).max()))
    assert worst_y <= 1e-12 and worst_l <= 1e-12, (worst_y, worst_l)
