"""Host-side packing for the CONDITIONAL NSF coupling layer in one launch (nf_nsf_wide_ctx, csrc/nsf_ctx.hip):
CoupledRationalQuadraticSpline(..., num_context_channels=C) (wrapper.py:20-35) whose ResidualNet reads a context
(nets/resnet.py:37-50, 92-104): the initial layer on cat(identity features, context), and per residual block a GLU gate
temps = t2 * sigmoid(context_layer(context)).

Geometry as flows/nsf_wide_pack.py (read its docstring first: row-blocks, k-groups, bias groups, A fragments, final-layer groups, the
per-wave streams with the wrapped copy of their first 8 entries; its layer_conditions, final_groups and write_streams do the work here),
with these differences:
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

from .nsf_wide_pack import final_groups, geometry, hidden_item, layer_conditions, padded_linear, positions, write_streams

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
    D, C = prqct.features, int(net.context_features)
    if not (2 <= D <= 128 and C >= 1 and 1 <= net.hidden_features <= MAX_HIDDEN and 1 <= len(net.blocks) <= 7):
        return False
    if x_positions(D) + padded_context(C) > 128:
        return False
    return layer_conditions(prqct) is not None


def pack_nsf_ctx(prqct):
    """(blob float32 ndarray, table int32 ndarray) or None (outside the kernel's structure).  One pack serves both directions."""
    if not supported(prqct):
        return None
    net = prqct.transform_net
    D, H, NB, C, K = prqct.features, net.hidden_features, len(net.blocks), int(net.context_features), prqct.num_bins
    nI, nT, par_i, par_t, PI, Dp, _ = positions(prqct)
    Hp = 128 if H <= 128 else 256
    PC = padded_context(C)
    assert Dp == x_positions(D) and Dp + PC <= 128
    nhi, NS, TR = geometry(Hp)
    finals = final_groups(net.final_layer, nT, K, H, TR)
    w0 = net.initial_layer.weight.detach().cpu().numpy().astype(np.float32)      # (H, nI + C): cat(identity features, context)
    if finals is None or w0.shape[1] != nI + C:
        return None
    Kh = (H + 31) // 32 * 32
    # the initial layer as two items: the identity columns with the bias, the context columns with a zero bias group (the kernel adds)
    W0c = np.zeros((Hp, PC), dtype=np.float32)
    W0c[:H, :C] = w0[:, nI:]
    head = [padded_linear(net.initial_layer, Hp, PI, w0[:, :nI]), (W0c, np.zeros(Hp, dtype=np.float32))]
    blocks = [(padded_linear(blk.linear_layers[0], Hp, Kh), padded_linear(blk.context_layer, Hp, PC),
               padded_linear(blk.linear_layers[1], Hp, Kh)) for blk in net.blocks]

    def items(w):    # the wave's hidden items in consumption order (nsf_ctx.hip): per block the W1 items, then per hidden item gate and W2
        at = lambda i: hidden_item(Hp, w, i)
        out = [l + at(i) for l in head for i in range(nhi)]
        for l1, gate, l2 in blocks:
            out += [l1 + at(i) for i in range(nhi)]
            out += [l + at(i) for i in range(nhi) for l in (gate, l2)]
        return out

    hdr = [D, Dp, H, Hp, NB, nI, nT, par_i, par_t, 0, 0, 0, nhi, 0, TR, PI]
    return write_streams(hdr, {24: K, 25: C, 26: PC}, items, finals)
