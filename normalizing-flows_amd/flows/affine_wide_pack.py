"""Host-side packing for the one-launch wide RealNVP coupling layer (nf_affine_wide, csrc/affine_wide.hip).

A MaskedAffineFlow(b, t = MLP, s = MLP) (normflows/flows/affine/coupling.py:174-229) or an AffineCouplingBlock(MLP) with a channel /
channel_inv split (:99-171, :232-267) whose conditioners are nets.MLP([in, H1, H2, out]) with LeakyReLU(0.0) (nets/mlp.py:5-58) runs
on the MADE tile engine's plain-MLP mode (flows/made_pack._mlp_layers / _pack_forward_from, csrc/made_fwd_body.hpp EPI 4).  This
module only rearranges weights.  ONE formulation serves both layer types:

  * x tile = the whole z row; the initial layer contracts over the columns the conditioner sees.  MaskedAffineFlow: column f of
    both nets' first weight times b_f (the reference feeds b * z); AffineCouplingBlock: the param_map's first weight on the z1
    columns (realnvp_pack.block_split), zero elsewhere.
  * hidden slots = [s-net units | t-net units], each net zero-padded to its wider hidden layer, the t units on a 32-slot boundary;
    the hidden-to-hidden weight is block-diagonal.  With the engine's prefix skipping (a row-block's stream stops at the last
    k-group its mask reaches) the s row-blocks stop at the s columns and the t row-blocks run over all of them: two nets of equal
    width H cost 3 H^2 of MFMA work for 2 H^2 useful (derived from the geometry, not measured).  A block's single MLP has no such
    overhead.
  * final layer: row 2 f = feature f's scale parameter (s-net row f | param[:, 1::2]), row 2 f + 1 = its shift parameter (t-net row f
    | param[:, 0::2]; the only non-zero row with scale=False).  Rows of a missing net and of a block's identity features are zero; a
    MaskedAffineFlow keeps the rows of its identity features (the reference multiplies them by 1 - b = 0, which lets a non-finite
    s_f / t_f through as NaN: the epilogue evaluates that expression).
  * behind the items the table carries one word per 16 features, 2 bits each: 0 = identity, 1 = transformed (MaskedAffineFlow, b_f =
    0), 2 = transformed and fed to the conditioner as 0 (a block's z2 columns, which its param_map never sees); hdr[24] = the scale
    map (_lib.SCALE; MASKED = the masked flow's exp with its non-finite -> NaN rule), hdr[25] = which nets a masked flow has (bit 0:
    s, bit 1: t; a missing net's parameter is the constant 0), hdr[13] = 1 (plain MLP).

Non-finite values.  An inf / NaN in z, and a non-finite s / t / param_map output, land where the layer-wise route puts them.  One
difference remains: the zero blocks of the stacked weights are multiplied like any other, so a non-finite HIDDEN activation of one
net (finite inputs and weights do not produce one) reaches the other net's outputs as NaN (0 * inf), where the layer-wise route
keeps that other net finite.  Under autograd (train_structure, autograd.AffineWideFn; config.affine_wide_train) there is a second one
for a block: the MADE training forward has no zero-fed tile, so the z2 columns meet the ZERO WEIGHTS of the initial layer, and a
non-finite z2 entry turns the whole row into NaN (0 * inf) where the layer-wise route keeps it finite.  Finite inputs are unaffected.
"""
import numpy as np
import torch

from . import made_pack

MAX_D = 128
MAX_SLOTS = 512
CHAIN_D, CHAIN_WIDTH = 16, 64       # what the chain kernels take (core._realnvp_record_ok, core._block_net)
MASKED = 4                          # hdr[24] of a MaskedAffineFlow
IDENTITY, TRANSFORM, TRANSFORM_ZERO_FED = 0, 1, 2


def _net(net, who, n_in, n_out):
    """The three Linears of a conditioner the kernel takes, or the reason (str) it does not."""
    from .. import core
    pm = core._plain_mlp(net)
    if pm is None:
        return "%s is not a plain nets.MLP (Linear + LeakyReLU only: no output_fn, no dropout)" % who
    lin, slope = pm
    if len(lin) != 3:
        return "%s has %d hidden layers, the kernel takes two" % (who, len(lin) - 1)
    if slope != 0.0:
        return "%s has LeakyReLU slope %g, the kernel takes 0" % (who, slope)
    if any(l.bias is None for l in lin):
        return "%s has a Linear without bias" % who
    if any(p.dtype != torch.float32 for l in lin for p in (l.weight, l.bias)):
        return "%s holds %s weights, the kernel takes float32" % (who, lin[0].weight.dtype)
    if lin[0].in_features != n_in or lin[2].out_features != n_out:
        return "%s maps %d -> %d features, the layer needs %d -> %d" % (who, lin[0].in_features, lin[2].out_features, n_in, n_out)
    return lin


def structure(flow, d):
    """What can be decided from attributes alone (no device read; done on every call): a dict with `kind` ("masked" | "block"), the
    nets' Linears and the sizes, or the reason (str) the layer is declined."""
    from . import realnvp_pack
    from .affine import AffineCoupling, AffineCouplingBlock, MaskedAffineFlow
    if not 2 <= d <= MAX_D:
        return "d = %d, the kernel takes 2 <= d <= %d" % (d, MAX_D)
    if isinstance(flow, MaskedAffineFlow):
        if flow.b.numel() != d:
            return "the mask has %d entries for d = %d" % (flow.b.numel(), d)
        if flow.b.dtype != torch.float32:
            return "the mask is %s, the kernel takes float32" % flow.b.dtype
        if flow.s is None and flow.t is None:
            return "neither s nor t: nothing to fuse"
        nets = []
        for who, net in (("s", flow.s), ("t", flow.t)):
            lin = None if net is None else _net(net, who, d, d)
            if isinstance(lin, str):
                return lin
            nets.append(lin)
        st = dict(kind="masked", s=nets[0], t=nets[1], smap=MASKED)
    elif isinstance(flow, AffineCouplingBlock):
        if flow.split_mode not in ("channel", "channel_inv"):
            return "split mode %s: only channel / channel_inv are one kernel" % flow.split_mode
        if len(flow.flows) != 3 or not isinstance(flow.flows[1], AffineCoupling):
            return "not the Split / AffineCoupling / Merge triple"
        from .._lib import SCALE
        c1, flip = realnvp_pack.block_split(flow, d)
        c = flow.flows[1]
        lin = _net(c.param_map, "param_map", c1, (d - c1) * (2 if c.scale else 1))
        if isinstance(lin, str):
            return lin
        st = dict(kind="block", net=lin, c1=c1, flip=flip, smap=SCALE[c._smap()])
    else:
        return "%s is neither a MaskedAffineFlow nor an AffineCouplingBlock" % type(flow).__name__
    lins = [l for k in ("s", "t", "net") if st.get(k) is not None for l in st[k]]
    if d <= CHAIN_D and all(l.out_features <= CHAIN_WIDTH for l in lins):
        return "d <= %d and every width <= %d: the chain kernels' shape" % (CHAIN_D, CHAIN_WIDTH)
    # slots: [s | t] (a block: its one net), each net padded to its wider hidden layer, the second on a 32-slot boundary
    offs, total = [], 0
    for k in ("s", "t", "net"):
        if st.get(k) is not None:
            total = (total + 31) // 32 * 32
            offs.append((k, total))
            total += max(st[k][0].out_features, st[k][1].out_features)
    if total > MAX_SLOTS:
        return "%d hidden slots, the kernel holds %d" % (total, MAX_SLOTS)
    st.update(d=d, offs=dict(offs), slots=total, Hp=256 if total <= 256 else 512)
    return st


def supported(flow, d, z=None):
    """None when nf_affine_wide takes the layer on (B, d) inputs (and the input `z`, when one is given), else the reason (str) it is
    declined.  Reads the mask's values (a device read): the route caches the answer with the pack."""
    if z is not None:
        if z.dim() != 2 or z.shape[1] != d:
            return "input of shape %s: the kernel takes (B, %d)" % (tuple(z.shape), d)
        if z.dtype != torch.float32:
            return "%s input, the kernel takes float32" % z.dtype
        if not z.is_cuda:
            return "input on %s: the kernel runs on the GPU" % z.device
    st = structure(flow, d)
    if isinstance(st, str):
        return st
    return _mask_reason(flow, st)


def _mask_reason(flow, st):
    if st["kind"] == "masked":
        b = flow.b.detach().reshape(-1).cpu().numpy()
        if not np.all((b == 0.0) | (b == 1.0)):
            return "the mask is not binary"
    return None


def _w(t):
    return t.detach().cpu().numpy().astype(np.float32)


def slot_layers(flow, d, wb=None):
    """The layer as the slot-layer dict made_pack._pack_forward_from takes (as made_pack._mlp_layers builds for one MLP), with
    `modes` (d codes) and `smap`; a str = the reason it is declined.  wb: {id(Linear): (weight, bias)} arrays to rearrange instead of
    the parameters (tests: where every weight lands)."""
    st = structure(flow, d)
    if isinstance(st, str):
        return st
    why = _mask_reason(flow, st)
    if why is not None:
        return why
    Hp, Dp = st["Hp"], (d + 31) // 32 * 32
    NFB = (2 * d + made_pack.ROWS - 1) // made_pack.ROWS
    W = [np.zeros(s, dtype=np.float32) for s in ((Hp, Dp), (Hp, Hp), (NFB * made_pack.ROWS, Hp))]
    M = [np.zeros(w.shape, dtype=bool) for w in W]
    Bv = [np.zeros(w.shape[0], dtype=np.float32) for w in W]
    get = (lambda l: (_w(l.weight), _w(l.bias))) if wb is None else (lambda l: tuple(np.asarray(a, dtype=np.float32) for a in wb[id(l)]))
    if st["kind"] == "masked":
        b = flow.b.detach().reshape(-1).cpu().numpy().astype(np.float32)
        modes = np.where(b == 1.0, IDENTITY, TRANSFORM)
        in_cols, in_scale = np.nonzero(b == 1.0)[0], b          # column f times b_f: b * z folded into the pack
        # (net, its final rows: feature f -> row 2 f (s) | 2 f + 1 (t), from the net's own row f).  EVERY feature's rows, the identity
        # features' too: the reference multiplies by 1 - b instead of selecting, so a non-finite s_f / t_f at an identity feature
        # turns y_f and the log-det into NaN (0 * NaN) -- the epilogue evaluates the same expression (affine.hip)
        every = np.arange(d)
        jobs = [(k, st[k], 2 * every + (0 if k == "s" else 1), every) for k in ("s", "t") if st[k] is not None]
    else:
        c1, flip = st["c1"], st["flip"]
        c2 = d - c1
        z1 = np.arange(c1) + (c2 if flip else 0)
        z2 = np.arange(c2) + (0 if flip else c1)
        modes = np.full(d, IDENTITY)
        modes[z2] = TRANSFORM_ZERO_FED
        in_cols, in_scale = z1, None
        scale = st["smap"] != 3
        # param[:, 0::2] = shift -> row 2 f + 1, param[:, 1::2] = scale -> row 2 f (coupling.py:131-132); scale=False: shift only
        rows = np.concatenate([2 * z2 + 1, 2 * z2]) if scale else 2 * z2 + 1
        src = np.concatenate([2 * np.arange(c2), 2 * np.arange(c2) + 1]) if scale else np.arange(c2)
        jobs = [("net", st["net"], rows, src)]
    for k, lin, out_rows, src_rows in jobs:
        o = st["offs"][k]
        (w0, b0), (w1, b1), (w2, b2) = (get(l) for l in lin)
        h1, h2 = w0.shape[0], w1.shape[0]
        if st["kind"] == "masked":
            W[0][o:o + h1, in_cols] = w0[:, in_cols] * in_scale[in_cols]
            M[0][o:o + h1, :d] = True          # (the zero columns are contracted too: b * z of a non-finite z is NaN in the reference)
        else:
            W[0][o:o + h1, in_cols] = w0
            M[0][o:o + h1, in_cols] = True
        Bv[0][o:o + h1] = b0
        W[1][o:o + h2, o:o + h1] = w1
        M[1][o:o + h2, o:o + h1] = True
        Bv[1][o:o + h2] = b1
        W[2][out_rows, o:o + h2] = w2[src_rows]
        M[2][out_rows, o:o + h2] = True
        Bv[2][out_rows] = b2[src_rows]
    layers = [(W[0], M[0], Bv[0]), (W[1], M[1], Bv[1]), None, (W[2], M[2], Bv[2])]
    return dict(D=d, H=st["slots"], NB=1, Hp=Hp, NSB=Hp // 256, Dp=Dp, NFB=NFB, MD=2 * d, mult=2, order=np.arange(st["slots"]),
                slot_of=np.arange(st["slots"]), layers=layers, plain=True, modes=modes.astype(np.int64), smap=int(st["smap"]),
                offs=st["offs"])


# ---- under autograd: the MADE training kernels in plain-MLP mode around nf_affine_wide_apply / _bwd (autograd.AffineWideFn) ------------
def linears(st):
    """The Linears of structure()'s dict in parameter order: s's three, then t's (a block: the param_map's)."""
    return [l for k in ("s", "t", "net") if st.get(k) is not None for l in st[k]]


def _train_key(flow, st):
    import hashlib
    shapes = tuple(tuple(l.weight.shape) for l in linears(st))
    if st["kind"] == "masked":
        b = flow.b.detach().reshape(-1).cpu().numpy().astype(np.float32)
        return ("affine_wide", "masked", st["d"], shapes, st["s"] is not None, st["t"] is not None, hashlib.sha1(b.tobytes()).hexdigest())
    return ("affine_wide", "block", st["d"], shapes, st["c1"], bool(st["flip"]), int(st["smap"]))


def _train_masks(sl, kind):
    """The weight problems' masks over the STACKED parameter layout ((slots, d), (slots, slots), (2 d, slots)): where nf_made_wgrad
    writes.  Everything else stays the exact 0 the reference's autograd gives: the zero blocks of the stacked weights, and for a masked
    flow the first-layer columns f with b_f = 0 (the reference feeds b * z) and the final rows of features with b_f = 1 (multiplied by
    1 - b).  A block's param_map has no columns for z2 and no rows for z1 to begin with."""
    H, d = sl["H"], sl["D"]
    (_, M0, _), (_, M1, _), _, (_, Mf, _) = sl["layers"]
    m0, m1, mf = M0[:H, :d].copy(), M1[:H, :H].copy(), Mf[:2 * d, :H].copy()
    if kind == "masked":
        ident = sl["modes"] == IDENTITY
        m0[:, ~ident] = False
        mf[np.repeat(ident, 2), :] = False
    return [m0, m1, mf]


def _carve_recipes(st, sl):
    """Per parameter (weight, bias of every Linear in linears() order) where its gradient sits in the stacked flat result: (problem,
    "w" | "b", row slice, column slice, swap) -- views of the stacked problems; swap: a block's final rows come in (scale, shift) pairs
    and leave as the param_map's (shift, scale) rows."""
    d, out = st["d"], []
    for k in ("s", "t", "net"):
        if st.get(k) is None:
            continue
        o = st["offs"][k]
        l0, l1, _ = st[k]
        h1, h2 = l0.out_features, l1.out_features
        if st["kind"] == "masked":
            cols, rows, swap = slice(0, d), slice(0 if k == "s" else 1, 2 * d, 2), False
        else:
            c1, c2 = st["c1"], d - st["c1"]
            z1_0, z2_0 = (c2 if st["flip"] else 0), (0 if st["flip"] else c1)
            cols = slice(z1_0, z1_0 + c1)
            scale = st["smap"] != 3
            rows, swap = (slice(2 * z2_0, 2 * z2_0 + 2 * c2), True) if scale else (slice(2 * z2_0 + 1, 2 * z2_0 + 2 * c2, 2), False)
        out += [(0, "w", slice(o, o + h1), cols, False), (0, "b", slice(o, o + h1), None, False),
                (1, "w", slice(o, o + h2), slice(o, o + h1), False), (1, "b", slice(o, o + h2), None, False),
                (2, "w", rows, slice(o, o + h2), swap), (2, "b", rows, None, swap)]
    return out


def train_structure(flow, d):
    """The value-independent part of the layer's training packs (made_pack.train_structure over slot_layers with values and with the
    positions of made_pack.index_arrays), shared between layers of one structure (made_pack._shared), or the reason (str) the layer
    is declined -- exactly structure() + the binary-mask check, the layers nf_affine_wide takes.  The dict of
    made_pack.train_structure (the forward / backward streams are gathered from the live parameters in every forward: flat = [0, the
    weight and bias of every Linear in linears() order]) with
      bwd["table"][14] = bwd["Mp"]   g_params arrives in the padded shape nf_affine_wide_apply_bwd writes (no pad copy)
      modes, smap, nets              the operands of nf_affine_wide_apply / _bwd
      carve                          _carve_recipes: every parameter's gradient as a view of nf_made_wgrad's stacked flat result.

    Non-finite values under autograd.  As at inference, with one more difference for a block: its z2 columns meet ZERO WEIGHTS here
    instead of a zeroed tile, so a non-finite z2 entry turns the whole row into NaN (0 * inf) where the layer-wise route keeps it
    finite.  Finite inputs are unaffected."""
    st = structure(flow, d)
    if isinstance(st, str):
        return st

    def build():
        sl_v = slot_layers(flow, d)
        if isinstance(sl_v, str):
            return sl_v
        lins = linears(st)
        idx = made_pack.index_arrays([tuple(l.weight.shape) for l in lins])
        sl_i = slot_layers(flow, d, wb={id(l): wb for l, wb in zip(lins, idx)})
        sl_v["masks"] = sl_i["masks"] = _train_masks(sl_v, st["kind"])
        ts = made_pack.train_structure(sl_v, sl_i)
        ts["bwd"]["table"][14] = ts["bwd"]["Mp"]
        ts.update(modes=mode_words(sl_v["modes"], sl_v["Dp"]), smap=int(sl_v["smap"]), d=d,
                  nets=(1 if "s" in sl_v["offs"] else 0) | (2 if "t" in sl_v["offs"] else 0), carve=_carve_recipes(st, sl_v))
        return ts
    return made_pack._shared(_train_key(flow, st), build)


def carve(flat, offsets, recipes):
    """Every parameter's gradient in its own shape out of nf_made_wgrad's flat result (torch or numpy)."""
    out = []
    for prob, what, rows, cols, swap in recipes:
        woff, shape, boff, n = offsets[prob]
        g = flat[woff:woff + shape[0] * shape[1]].reshape(shape)[rows, cols] if what == "w" else flat[boff:boff + n][rows]
        if swap:          # (scale, shift) pairs -> the param_map's (shift, scale) rows: the one copy of this carve
            g = g.reshape((g.shape[0] // 2, 2) + tuple(g.shape[1:]))
            g = (g.flip(1) if hasattr(g, "flip") else g[:, ::-1]).reshape((-1,) + tuple(g.shape[2:]))
        out.append(g)
    return out


def mode_words(modes, Dp):
    """One int32 per 16 features, 2 bits each (feature 16 k + j at bits 2 j)."""
    m = np.zeros(Dp, dtype=np.int64)
    m[:len(modes)] = modes
    return (m.reshape(-1, 16) << (2 * np.arange(16))).sum(axis=1).astype(np.uint32).view(np.int32)


def pack(flow, d, wb=None):
    """(blob float32, table int32) of nf_affine_wide in the engine's forward format, or None when the layer is declined
    (`supported` says why)."""
    sl = slot_layers(flow, d, wb)
    if isinstance(sl, str):
        return None
    blob, table = made_pack._pack_forward_from(sl)
    table[24] = sl["smap"]
    table[25] = (1 if "s" in sl["offs"] else 0) | (2 if "t" in sl["offs"] else 0)      # a masked flow's nets: a missing one is the constant 0
    return blob, np.concatenate([table, mode_words(sl["modes"], sl["Dp"])]).astype(np.int32)
