"""The weight blob of the RealNVP training kernels (csrc/realnvp_train.hip) as a device gather from the live parameters.

The blob has the layout of core._pack_realnvp (the inference kernel's host-packed blob, csrc/realnvp_chain.hip):
    [nrec, d, hmax, 0, off_0 .. off_{nrec-1}, records]
    record ActNorm / AffineConst : [1, 0, 0, 0, s[d], t[d]]
    record MaskedAffine          : [2, has_s, has_t, 0, b[d], mlp_s?, mlp_t?]
    record CouplingBlock         : [3, c1, flip + 2 scale_map, has_perm, pf[d], pi[d], mlp]     (csrc/realnvp_block.hpp)
    mlp                          : [nlin, slope, n_0 .. n_nlin, then per linear: W (n_{k+1} x n_k row-major), bias (n_{k+1})]
Under autograd the parameters change every step, so the value-independent part is built once per run structure (`structure`):
`static` = the blob with zeros in place of every tensor value, `src` = for every blob position its position in
    flat = [0, static ..., tensor_0 ..., tensor_1 ..., ...]
and every forward gathers blob = flat[src] on the device (ops.pack_gather) from `tensors(run)` as they are in that call -- the
masks `b` included.  `slices[k]` = (offset, shape) of tensor k inside the blob: the gradient blob of nf_realnvp_chain_bwd has the
same layout, so tensor k's gradient is that slice of it.

A coupling block record is ONE AffineCouplingBlock whose param_map is a plain MLP together with the Permute that stands directly
behind it in `run` (`records`): two flows, one record -- the 64 layers of 32 x [block, Permute] are 32 records.  Its header and the
permutation's index maps are value-independent structure (`static`, `signature`): the maps come from Permute._index_maps, a host
copy cached on the buffers' versions, so no forward reads the device for them.
"""
import math

import torch

MAX_RECORDS = 32        # one bit pair per record in nf_realnvp_chain_bwd's 64-bit gradient mask


def _nets(f):
    from ..core import _plain_mlp
    from .affine import AffineCouplingBlock
    if isinstance(f, AffineCouplingBlock):
        return [(_plain_mlp(f.flows[1].param_map), 0)]
    return [(_plain_mlp(net), side) for net, side in ((f.s, 0), (f.t, 1)) if net is not None]


def records(run):
    """[(flow, Permute or None)] of the flows `run` (forward order), one entry per record: a Permute belongs to the record of the
    AffineCouplingBlock directly in front of it (core._run_chain_impl lets no other Permute into a run)."""
    from .affine import AffineCouplingBlock
    from .mixing import Permute
    out = []
    for f in run:
        if isinstance(f, Permute):
            assert out and isinstance(out[-1][0], AffineCouplingBlock) and out[-1][1] is None, "a Permute joins a run behind a block only"
            out[-1] = (out[-1][0], f)
        else:
            out.append((f, None))
    return out


def block_split(f, d):
    """(c1, flip) of an AffineCouplingBlock on (B, d) inputs: AffineCouplingBlock._fused's convention (reshape.py:30-34)."""
    return ((d + 1) // 2, 0) if f.split_mode == "channel" else (d // 2, 1)


def block_header(f, perm, d):
    """The value-independent floats of a coupling block record: [3, c1, flip + 2 scale_map, has_perm, pf[d], pi[d]]."""
    from .._lib import SCALE
    c1, flip = block_split(f, d)
    pf, pi = perm._index_maps() if perm is not None else (tuple(range(d)),) * 2
    assert len(pf) == len(pi) == d
    return [3.0, float(c1), float(flip + 2 * SCALE[f.flows[1]._smap()]), float(perm is not None)] + [float(v) for v in pf + pi]


def tensors(run):
    """The live tensors of the flows `run` (forward order) in blob order, each with (record, side): side 0 = the s-net (ActNorm: s;
    coupling block: its MLP), 1 = the t-net (t), None = the mask buffer b (no gradient)."""
    from .affine import AffineCouplingBlock, MaskedAffineFlow
    out = []
    for r, (f, _) in enumerate(records(run)):
        if isinstance(f, (MaskedAffineFlow, AffineCouplingBlock)):
            if isinstance(f, MaskedAffineFlow):
                out.append((f.b, r, None))
            for (lin, _), side in _nets(f):
                for l in lin:
                    out += [(l.weight, r, side), (l.bias, r, side)]
        else:
            out += [(f.s, r, 0), (f.t, r, 1)]
    return out


def signature(run, d):
    """What `structure` depends on: record kinds, layer sizes, slopes and a coupling block's header with its Permute's index maps
    (their cached host copy) -- no parameter value."""
    from .affine import AffineCouplingBlock, MaskedAffineFlow
    sig = [d]
    for f, perm in records(run):
        nets = tuple((side, slope) + tuple(tuple(l.weight.shape) for l in lin) for (lin, slope), side in _nets(f)) \
            if isinstance(f, (MaskedAffineFlow, AffineCouplingBlock)) else ()
        if isinstance(f, MaskedAffineFlow):
            sig.append((2, f.s is not None, f.t is not None) + nets)
        elif isinstance(f, AffineCouplingBlock):
            sig.append(tuple(block_header(f, perm, d)) + nets)
        else:
            sig.append((1,))
    return tuple(sig)


def mlp_footprint(lin, d):
    """(widest layer, floats of one MLP's Linear inputs) of one MLP: what the kernels keep in LDS per lane."""
    sizes = [lin[0].in_features] + [l.out_features for l in lin]
    return max([d] + sizes), max(d, sum(sizes[:-1]))


def structure(run, d):
    """dict(static, src: CPU tensors; slices, sides, hmax, act, nblob, nrec) of the flows `run` (forward order) on (B, d) inputs."""
    from .affine import AffineCouplingBlock, MaskedAffineFlow
    recs, hmax, act = [], d, d          # a record = list of floats (constants) and ("t", numel) placeholders
    for f, perm in records(run):
        if isinstance(f, (MaskedAffineFlow, AffineCouplingBlock)):
            if isinstance(f, MaskedAffineFlow):
                r = [2.0, float(f.s is not None), float(f.t is not None), 0.0, ("t", d)]
            else:
                r = block_header(f, perm, d)
            for (lin, slope), _ in _nets(f):
                sizes = [lin[0].in_features] + [l.out_features for l in lin]
                h, a = mlp_footprint(lin, d)
                hmax, act = max(hmax, h), max(act, a)
                r += [float(len(lin)), float(slope)] + [float(v) for v in sizes]
                for l in lin:
                    r += [("t", l.weight.numel()), ("t", l.bias.numel())]
            recs.append(r)
        else:
            recs.append([1.0, 0.0, 0.0, 0.0, ("t", d), ("t", d)])
    sizes_ = [sum(it[1] if isinstance(it, tuple) else 1 for it in r) for r in recs]
    offs, o = [], 4 + len(recs)
    for n in sizes_:
        offs.append(float(o))
        o += n
    nblob = o
    static = [float(len(recs)), float(d), float(hmax), 0.0] + offs
    src = list(range(1, 1 + len(static)))
    offsets, tpos = [], 1 + nblob         # tpos: position in `flat` of the next tensor's first element
    for r in recs:
        for it in r:
            if isinstance(it, tuple):
                offsets.append(len(static))
                src += range(tpos, tpos + it[1])
                static += [0.0] * it[1]
                tpos += it[1]
            else:
                src.append(1 + len(static))
                static.append(it)
    tl = tensors(run)
    assert len(static) == nblob == len(src) and len(offsets) == len(tl) and tpos < 2 ** 31
    assert all(t.numel() == n for (t, _, _), n in zip(tl, [it[1] for r in recs for it in r if isinstance(it, tuple)]))
    return {"static": torch.tensor(static, dtype=torch.float32), "src": torch.tensor(src, dtype=torch.int32),
            "slices": [(off, tuple(t.shape)) for off, (t, _, _) in zip(offsets, tl)], "sides": [(r, s) for _, r, s in tl],
            "hmax": hmax, "act": act, "nblob": nblob, "nrec": len(recs), "d": d}


def to_device(st, device):
    """`st` with static / src on `device` (uploaded once per structure and device: core caches the result)."""
    out = dict(st)
    out["static"], out["src"] = st["static"].to(device), st["src"].to(device)
    return out


def gather_reference(st, tensor_list):
    """blob = flat[src] in torch, on whatever device the inputs live: what ops.pack_gather computes (CPU tests)."""
    flat = torch.cat([torch.zeros(1), st["static"].reshape(-1).cpu()] + [t.detach().reshape(-1).float().cpu() for t in tensor_list])
    return flat[st["src"].long().cpu()]


def grad_mask(st, needs):
    """nf_realnvp_chain_bwd's wmask from the per-tensor `needs` flags (bit 2 r + side)."""
    m = 0
    for (r, side), need in zip(st["sides"], needs):
        if need and side is not None:
            m |= 1 << (2 * r + side)
    return m - (1 << 64) if m >= 1 << 63 else m          # (the C side takes the 64 bits as an int64_t)


def carve(st, grads, k):
    """Tensor k's gradient: its slice of the reduced gradient blob, shaped like the tensor."""
    off, shape = st["slices"][k]
    return grads[off:off + math.prod(shape)].view(shape)
