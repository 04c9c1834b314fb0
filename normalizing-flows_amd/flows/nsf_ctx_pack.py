"""Host-side packing for the CONDITIONAL NSF coupling layer in one launch (nf_nsf_wide_ctx, csrc/nsf_ctx.hip):
CoupledRationalQuadraticSpline(..., num_context_channels=C) (wrapper.py:20-35) whose ResidualNet reads a context
(nets/resnet.py:37-50, 92-104): the initial layer on cat(identity features, context), and per residual block a GLU gate
temps = t2 * sigmoid(context_layer(context)).

Geometry as flows/nsf_wide_pack.py (read its docstring first: row-blocks, k-groups, bias groups, A fragments, final-layer groups, the
per-wave streams with the wrapped copy of their first 8 entries), with these differences:
  * the x tile holds the context at positions [Dp, Dp + PC): PC = C rounded up to 32, the padding positions zero; Dp + PC <= 128;
  * the initial layer is TWO items per hidden item: the identity columns W0[:, :nI] over positions [0, PI) with the bias b0, then
    the context columns W0[:, nI:] over the PC context positions with a zero bias group (the kernel adds it to the accumulator);
  * a residual block is NHI W1 items (over the hidden width rounded up to 32, as in nsf_wide), then per hidden item its GATE item
    (context_layer: bias bc, A = Wc over the PC context positions) followed by its W2 item;
  * hidden widths up to 256 (Hp 128 | 256: one hidden item per wave; Hp 512 is not built, nsf_ctx.hip), no fused LU.

int32 table : hdr[32] = nsf_wide_pack's [D, Dp, H, Hp, NB, nI, nT, par_i, par_t, G, nfi, total floats, nhi, 0, TR, PI], hdr[16 + w] =
              offset (floats) of wave w's stream, hdr[24] = bins, hdr[25] = C, hdr[26] = PC; then per wave: nhi identity entries |
              nhi context entries | per block (nhi W1 entries, then per hidden item a gate entry and a W2 entry) | nfi final entries;
              hidden entry = [nkg, rb, sb0], final entry = [nkg, g, sb0] (g = -1: none).
"""
import numpy as np
import torch
from torch import nn

from .made_pack import ROWS, KG, RING, a_stream, bias_group
from .nsf_wide_pack import HDR, SUPPORTED_BINS, bins_geometry, final_row, geometry, hidden_item

MAX_HIDDEN = 256        # Hp 512 spills registers with the gate next to the block's accumulators (csrc/nsf_ctx.hip)


def padded_context(C):
    return (C + 31) // 32 * 32


def x_positions(D):
    """Dp: identity and transform features, each count rounded up to 32 (the same for either mask parity)."""
    return (D // 2 + 31) // 32 * 32 + ((D + 1) // 2 + 31) // 32 * 32


def supported(prqct):
    """True when the layer has the structure nf_nsf_wide_ctx implements (the caller keeps the layer-wise path otherwise)."""
    from .. import nets
    net = prqct.transform_net
    if not isinstance(net, nets.ResidualNet) or net.context_features is None or net.preprocessing is not None:
        return False
    if net.use_batch_norm or (net.dropout_probability != 0.0 and net.training):
        return False
    if not all(isinstance(b.activation, nn.ReLU) or b.activation is torch.nn.functional.relu for b in net.blocks):
        return False
    if prqct.tails != "linear" or getattr(prqct, "_per_feature", False) or prqct.unconditional_transform is None:
        return False
    K = prqct.num_bins
    if K not in SUPPORTED_BINS or prqct.min_bin_width * K > 1.0 or prqct.min_bin_height * K > 1.0:
        return False
    D, C = prqct.features, int(net.context_features)
    if not (2 <= D <= 128 and C >= 1 and 1 <= net.hidden_features <= MAX_HIDDEN and 1 <= len(net.blocks) <= 7):
        return False
    if x_positions(D) + padded_context(C) > 128:
        return False
    if net.initial_layer.weight.dtype != torch.float32:
        return False
    ii, ti = prqct.identity_features.cpu(), prqct.transform_features.cpu()
    alt0 = torch.equal(ii, torch.arange(0, D, 2)) and torch.equal(ti, torch.arange(1, D, 2))
    alt1 = torch.equal(ii, torch.arange(1, D, 2)) and torch.equal(ti, torch.arange(0, D, 2))
    return alt0 or alt1


def pack_nsf_ctx(prqct):
    """(blob float32 ndarray, table int32 ndarray) or None (outside the kernel's structure).  One pack serves both directions."""
    if not supported(prqct):
        return None
    net = prqct.transform_net
    D, H, NB, C = prqct.features, net.hidden_features, len(net.blocks), int(net.context_features)
    ident = prqct.identity_features.cpu().numpy()
    trans = prqct.transform_features.cpu().numpy()
    nI, nT = len(ident), len(trans)
    par_i, par_t = int(ident[0]), int(trans[0])
    Hp = 128 if H <= 128 else 256
    PI, PT, PC = (nI + 31) // 32 * 32, (nT + 31) // 32 * 32, padded_context(C)
    Dp = PI + PT
    assert Dp == x_positions(D) and Dp + PC <= 128
    nhi, NS, TR = geometry(Hp)
    K = prqct.num_bins
    M_, MP_, FPL, FPG, nfi_max = bins_geometry(K)
    G = (nT + FPG - 1) // FPG
    nsp = TR // 64
    nfi = (G * nsp + 7) // 8
    if nfi > nfi_max:
        return None
    f32 = lambda t: t.detach().cpu().numpy().astype(np.float32)

    w0 = f32(net.initial_layer.weight)                       # (H, nI + C): cat(identity features, context)
    if w0.shape[1] != nI + C:
        return None
    W0i = np.zeros((Hp, PI), dtype=np.float32)
    W0i[:H, :nI] = w0[:, :nI]
    W0c = np.zeros((Hp, PC), dtype=np.float32)
    W0c[:H, :C] = w0[:, nI:]
    b0 = np.zeros(Hp, dtype=np.float32)
    b0[:H] = f32(net.initial_layer.bias)
    zero = np.zeros(Hp, dtype=np.float32)
    Kh = (H + 31) // 32 * 32

    def hidden(lin, cols, ncols):
        W = np.zeros((Hp, cols), dtype=np.float32)
        W[:H, :ncols] = f32(lin.weight)
        b = np.zeros(Hp, dtype=np.float32)
        b[:H] = f32(lin.bias)
        return W, b

    # the stream's layers in consumption order, per hidden item of a wave (nsf_ctx.hip): [(W, b), ...] groups of "all items" or "per item"
    head = [(W0i, b0), (W0c, zero)]
    blocks = []
    for blk in net.blocks:
        l1, l2 = blk.linear_layers
        blocks.append((hidden(l1, Kh, H), hidden(blk.context_layer, PC, C), hidden(l2, Kh, H)))

    wf, bf = f32(net.final_layer.weight), f32(net.final_layer.bias)
    if wf.shape[0] != M_ * nT:
        return None
    wh_scale = np.float32(1.4426950408889634 / np.sqrt(float(H)))          # log2(e) / sqrt(hidden): rqs_regs takes exp2
    WF = np.zeros((G, 3, ROWS, Kh), dtype=np.float32)
    BF = np.zeros((G, 3, ROWS), dtype=np.float32)
    for g in range(G):
        for r3 in range(3):
            for rho in range(ROWS):
                row = final_row(g, r3, rho, nT, K)
                if row >= 0:
                    sc = wh_scale if (row % M_) < 2 * K else np.float32(1.0)
                    WF[g, r3, rho, :H] = wf[row] * sc
                    BF[g, r3, rho] = bf[row] * sc

    nh = (2 + 3 * NB) * nhi
    nitems = nh + nfi
    hdr = np.zeros(HDR, dtype=np.int32)
    tab = np.zeros((8, nitems, 3), dtype=np.int32)
    chunks, off = [], 0
    for w in range(8):
        hdr[16 + w] = off
        stream, idx = [], 0

        def item(Wl, bl, i):
            nonlocal idx
            rb, sb0 = hidden_item(Hp, w, i)
            tab[w, idx] = (Wl.shape[1] // KG, rb, sb0)
            idx += 1
            stream.append(bias_group(bl[rb * ROWS:(rb + 1) * ROWS]))
            stream.append(a_stream(Wl[rb * ROWS:(rb + 1) * ROWS]))

        for Wl, bl in head:
            for i in range(nhi):
                item(Wl, bl, i)
        for (l1, gate, l2) in blocks:
            for i in range(nhi):
                item(*l1, i)
            for i in range(nhi):
                item(*gate, i)
                item(*l2, i)
        assert idx == nh
        for j in range(nfi):
            g, sp = divmod(w + 8 * j, nsp)
            if g >= G:
                tab[w, nh + j] = (0, -1, 0)
                continue
            nkg = Kh // KG
            tab[w, nh + j] = (nkg, g, 2 * sp)
            for r3 in range(3):
                stream.append(bias_group(BF[g, r3]))
            frag = np.stack([a_stream(WF[g, r3]).reshape(nkg, 256) for r3 in range(3)], axis=1)   # [nkg][3][256]
            stream.append(frag.reshape(-1))
        stream = np.concatenate(stream)
        stream = np.concatenate([stream, np.resize(stream, RING * 256)])
        chunks.append(stream)
        off += stream.size
    hdr[:16] = [D, Dp, H, Hp, NB, nI, nT, par_i, par_t, G, nfi, off, nhi, 0, TR, PI]
    hdr[24], hdr[25], hdr[26] = K, C, PC
    blob = np.concatenate(chunks).astype(np.float32)
    assert blob.size == off and off < 2 ** 31
    return blob, np.concatenate([hdr, tab.reshape(-1)]).astype(np.int32)
