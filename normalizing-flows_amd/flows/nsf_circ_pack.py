"""Host-side packing for the CIRCULAR NSF coupling layer in one launch (nf_nsf_wide_ft, csrc/nsf_circ.hip):
CircularCoupledRationalQuadraticSpline (wrapper.py:88-185): tails given per feature as a list of "linear" / "circular"
(utils/splines.py:48-57), a scalar or per-feature tail bound, and a PeriodicFeaturesElementwise preprocessing (utils/nn.py:64-129) in
front of the ResidualNet for the circular identity coordinates.

Geometry as flows/nsf_wide_pack.py (read its docstring first; its positions, padded_linear, final_groups and write_streams do the work
here): blob and table are nsf_wide_pack's for a layer without LU, with one difference.  The final Linear has 3 K + 1 rows per transform
feature; the last derivative row is always overwritten (by the constant for a linear feature, by derivative 0 for a circular one) and is
not packed.  A lane's 3 K slots per feature are K widths | K heights | derivatives 1 .. K - 1 | derivative 0 -- the linear-tails layout
with derivative 0 in the slot that layout pads (nsf_wide_pack.final_row, list_tails) -- so the kernel runs the register spline of
nsf_wide with the end derivative chosen per feature: the constant (linear) or the slot (circular).

What differs per feature travels in `ftable`, float32 [8][Dp]: the rows of flows/maf_pack.py's per-feature table (column, tails code,
bound, scale, w_sin, w_cos, bias, periodic flag; maf_pack.feature_rows / table_from_rows) with one column per POSITION of the sorted x
tile: identity features at [0, nI), transform features at [PI, PI + nT), column -1 and zeros at the padding positions.  The preprocessing
only touches identity features, so the periodic rows are zero at transform positions.  table[25] = 1 marks the list-tails layout.
"""
import numpy as np
import torch

from .maf_pack import feature_rows, table_from_rows
from .nsf_wide_pack import final_groups, geometry, hidden_item, layer_conditions, padded_linear, positions, write_streams

MAX_HIDDEN = 256        # Hp 512 is not built (csrc/nsf_circ.hip)


def _rows(prqct):
    """(identity rows, transform rows) of maf_pack.feature_rows for a layer with the structure nf_nsf_wide_ft implements, or None:
    nsf_wide_pack's conditions with list tails, a plain-ReLU ResidualNet within the built shapes, and tails, bounds and a
    preprocessing of both halves that the per-feature table can express."""
    from .. import nets
    net, u = prqct.transform_net, prqct.unconditional_transform
    if not (isinstance(net, nets.ResidualNet) and net.is_plain_relu(preprocessing=True)):
        return None
    if not (2 <= prqct.features <= 128 and 1 <= net.hidden_features <= MAX_HIDDEN and 1 <= len(net.blocks) <= 7):
        return None
    if layer_conditions(prqct, list_tails=True) is None or not isinstance(u.tails, (list, tuple)):
        return None
    pre = net.preprocessing
    if pre is not None and not (isinstance(pre, nets.PeriodicFeaturesElementwise) and isinstance(pre.activation, torch.nn.Identity)):
        return None
    ri = feature_rows(len(prqct.identity_features), u.tails, u.tail_bound, pre)
    rt = feature_rows(len(prqct.transform_features), prqct.tails, prqct.tail_bound, None)
    return None if ri is None or rt is None else (ri, rt)


def supported(prqct):
    """True when the layer has the structure nf_nsf_wide_ft implements (the caller keeps the layer-wise path otherwise)."""
    return _rows(prqct) is not None


def pack_nsf_circ(prqct):
    """(blob float32, table int32, ftable float32 (8, Dp)) or None (outside the kernel's structure).  One pack serves both directions."""
    rows = _rows(prqct)
    if rows is None:
        return None
    ri, rt = rows
    net = prqct.transform_net
    D, H, NB, K = prqct.features, net.hidden_features, len(net.blocks), prqct.num_bins
    nI, nT, par_i, par_t, PI, Dp, _ = positions(prqct)
    Hp = 128 if H <= 128 else 256
    nhi, NS, TR = geometry(Hp)
    finals = final_groups(net.final_layer, nT, K, H, TR, list_tails=True)
    if finals is None or net.initial_layer.weight.shape[1] != nI:
        return None
    Kh = (H + 31) // 32 * 32
    layers = [padded_linear(net.initial_layer, Hp, PI)] + [padded_linear(lin, Hp, Kh) for blk in net.blocks for lin in blk.linear_layers]

    def hidden(w):
        return [(Wl, bl) + hidden_item(Hp, w, i) for Wl, bl in layers for i in range(nhi)]

    head = [D, Dp, H, Hp, NB, nI, nT, par_i, par_t, 0, 0, 0, nhi, 0, TR, PI]
    blob, table = write_streams(head, {24: K, 25: 1}, hidden, finals)
    ftable = np.zeros((8, Dp), dtype=np.float32)
    col_i = -np.ones(PI, dtype=np.int64)
    col_i[:nI] = np.arange(nI)
    col_t = -np.ones(Dp - PI, dtype=np.int64)
    col_t[:nT] = np.arange(nT)
    ftable[:, :PI] = table_from_rows(col_i, *ri)
    ftable[:, PI:] = table_from_rows(col_t, *rt)
    # row 0: the column of the ROW a position holds (the kernel's own position arithmetic; kept for the table's one convention)
    icol = ftable.view(np.int32)[0]
    icol[:nI] = prqct.identity_features.cpu().numpy()
    icol[PI:PI + nT] = prqct.transform_features.cpu().numpy()
    return blob, table, ftable
