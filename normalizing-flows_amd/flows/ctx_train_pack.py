"""Host-side structure for the GLU-gated ResidualNet conditioner under autograd (csrc/resnet_ctx_train.hip): a ResidualNet with
context_features (nets/resnet.py:7-104) whose training forward, input-gradient backward and weight gradients run as HIP kernels.

The kernels read padded row-major matrices from one blob of floats:
  forward   W0 [Hp][Kin] (the input positions [x | 0 | c | 0]: x at [0, nI), the context at [PI, PI + C), PI = nI rounded up to 32),
            b0 [Hp]; per block W1, W2 [Hp][Hp], b1, b2, Wc [Hp][PC] (PC = C rounded up to 32), bc; Wf [Op][Hp], bf [Op]
  backward  WfT [Hp][Op], W0T [Kin][Hp]; per block W2T, W1T [Hp][Hp], WcT [PC][Hp]
Hp and Op are the hidden and output widths rounded up to 32; every padding entry is zero.  The blob is value-dependent and is
gathered on the device in every call (ops.pack_gather: blob = [0, params flattened ...][src]); `src`, the int32 table of offsets
and the weight-gradient job list are value-independent and built once per module (nets.ResidualNet._ctx_train_pack).

Parameter order (also the order of ResNetCtxFn's parameter arguments and of the flat gradient buffer):
  W0, b0, per block (W1, b1, W2, b2, Wc, bc), Wf, bf.

Weight-gradient jobs (16 int32 each): one per 64 x 64 tile of a layer's (units, input positions):
  gsel (-1: g_out, else a slot of the backward's G buffer), N, asel (-1: the saved input tile, else a slot of the forward's save
  buffer), akoff, KP, relu, K1, P1, K2 (position p -> column: p < P1 ? p if p < K1 : K1 + p - P1 if p - P1 < K2), wout, ldW, bout,
  n0, k0, 0, 0.
"""
import numpy as np
import torch
from torch import nn
from torch.nn import functional as F

MAX_HIDDEN = 256        # two hidden unit blocks per wave; wider would spill (csrc/resnet_ctx_train.hip)
MAX_BLOCKS = 4
MAX_POSITIONS = 128     # round32(nI) + round32(C)
TABLE_LEN = 52
RT_W0, RT_B0, RT_WF, RT_BF, RT_WFT, RT_W0T, RT_BLK, RT_WCT = 10, 11, 12, 13, 14, 15, 16, 48
JOB = 16
# Batches above this take the eager conditioner.  At 65 536 rows the kernels lose to it at D 64 (0.74-0.97x); at 32 768 rows the
# result varied between two runs (D 64 / C 16 / hidden 128: 0.88x, then 1.20x); at 4 096 and 16 384 rows they win by 1.4-3.0x
# (profiles/context_train_bench.json).
MAX_ROWS = 16384


def r32(n):
    return (n + 31) // 32 * 32


def supported(net):
    """None when a ResidualNet with context_features has the structure the kernels implement, else the reason it does not."""
    from ..nets import ResidualNet
    if not isinstance(net, ResidualNet) or net.context_features is None:
        return "not a ResidualNet with context_features"
    if net.preprocessing is not None:
        return "preprocessing"
    if net.use_batch_norm:
        return "batch norm"
    if net.dropout_probability != 0.0 and net.training:
        return "dropout in train mode"
    if not all(isinstance(b.activation, nn.ReLU) or b.activation is F.relu for b in net.blocks):
        return "activation other than ReLU"
    nb = len(net.blocks)
    if nb < 1 or nb > MAX_BLOCKS:
        return "num_blocks %d outside 1..%d" % (nb, MAX_BLOCKS)
    H = net.hidden_features
    if H > MAX_HIDDEN:
        return "hidden %d > %d" % (H, MAX_HIDDEN)
    C = net.context_features
    nI = net.initial_layer.weight.shape[1] - C
    if nI < 1 or r32(nI) + r32(C) > MAX_POSITIONS:
        return "round32(nI) + round32(C) > %d" % MAX_POSITIONS
    if any(p.dtype != torch.float32 for p in net.parameters()):
        return "not float32"
    return None


def params_of(net):
    out = [net.initial_layer.weight, net.initial_layer.bias]
    for b in net.blocks:
        l1, l2 = b.linear_layers
        out += [l1.weight, l1.bias, l2.weight, l2.bias, b.context_layer.weight, b.context_layer.bias]
    return out + [net.final_layer.weight, net.final_layer.bias]


def structure(nI, C, H, O, NB):
    """dict(src int32 gather indices into [0, params flattened ...], table int32 [TABLE_LEN], jobs int32 [njobs, 16], offsets of
    every parameter in the flat gradient buffer, nflat, and the padded sizes)."""
    Hp, Op, PI, PC = r32(H), r32(O), r32(nI), r32(C)
    Kin = PI + PC
    shapes = [(H, nI + C), (H,)] + [(H, H), (H,), (H, H), (H,), (H, C), (H,)] * NB + [(O, H), (O,)]
    poff, o = [], 0                       # offsets of the parameters in the flat buffer (no leading zero)
    for s in shapes:
        poff.append(o)
        o += int(np.prod(s))
    nflat = o

    segs = []
    table = np.zeros(TABLE_LEN, np.int32)
    table[:9] = [nI, C, PI, Kin, H, Hp, NB, O, Op]
    total = [0]

    def seg(idx):
        off = total[0]
        segs.append(idx.reshape(-1).astype(np.int32))
        total[0] += idx.size
        return off

    def wmat(k, rows, cols, nrows, ncols, transpose=False, colmap=None):
        """[rows][cols] padded image of parameter k (a weight (nrows, ncols)); transpose: image[c][u] = W[u][c]; colmap: position ->
        column (-1 = zero)."""
        idx = np.zeros((rows, cols), np.int64)
        if transpose:
            for c in range(rows):
                cc = c if colmap is None else colmap[c]
                if cc < 0 or cc >= ncols:
                    continue
                idx[c, :nrows] = 1 + poff[k] + np.arange(nrows) * ncols + cc
        else:
            for u in range(nrows):
                if colmap is None:
                    idx[u, :ncols] = 1 + poff[k] + u * ncols + np.arange(ncols)
                else:
                    ok = colmap >= 0
                    idx[u, :cols][ok] = 1 + poff[k] + u * ncols + colmap[ok]
        return idx

    def bvec(k, rows, n):
        idx = np.zeros(rows, np.int64)
        idx[:n] = 1 + poff[k] + np.arange(n)
        return idx

    pos = np.full(Kin, -1, np.int64)
    pos[:nI] = np.arange(nI)
    pos[PI:PI + C] = nI + np.arange(C)
    table[RT_W0] = seg(wmat(0, Hp, Kin, H, nI + C, colmap=pos))
    table[RT_B0] = seg(bvec(1, Hp, H))
    for b in range(NB):
        k = 2 + 6 * b
        bt = RT_BLK + 8 * b
        table[bt + 0] = seg(wmat(k, Hp, Hp, H, H))
        table[bt + 1] = seg(bvec(k + 1, Hp, H))
        table[bt + 2] = seg(wmat(k + 2, Hp, Hp, H, H))
        table[bt + 3] = seg(bvec(k + 3, Hp, H))
        table[bt + 4] = seg(wmat(k + 4, Hp, PC, H, C))
        table[bt + 5] = seg(bvec(k + 5, Hp, H))
        table[bt + 6] = seg(wmat(k + 2, Hp, Hp, H, H, transpose=True))
        table[bt + 7] = seg(wmat(k, Hp, Hp, H, H, transpose=True))
        table[RT_WCT + b] = seg(wmat(k + 4, PC, Hp, H, C, transpose=True))
    kf = 2 + 6 * NB
    table[RT_WF] = seg(wmat(kf, Op, Hp, O, H))
    table[RT_BF] = seg(bvec(kf + 1, Op, O))
    table[RT_WFT] = seg(wmat(kf, Hp, Op, O, H, transpose=True))
    table[RT_W0T] = seg(wmat(0, Kin, Hp, H, nI + C, transpose=True, colmap=pos))
    src = np.concatenate(segs).astype(np.int32)

    jobs = []

    def layer(gsel, N, asel, akoff, KP, relu, K1, P1, K2, k, ldW):
        for n0 in range(0, N, 64):
            for k0 in range(0, KP, 64):
                jobs.append([gsel, N, asel, akoff, KP, relu, K1, P1, K2, poff[k], ldW, poff[k + 1], n0, k0, 0, 0])

    layer(0, H, -1, 0, Kin, 0, nI, PI, C, 0, nI + C)
    for b in range(NB):
        k = 2 + 6 * b
        layer(1 + 3 * b, H, 4 * b, 0, H, 1, H, H, 0, k, H)              # W1: g_t x relu(h_b)
        layer(2 + 3 * b, H, 1 + 4 * b, 0, H, 1, H, H, 0, k + 2, H)      # W2: g_u x relu(t_b)
        layer(3 + 3 * b, H, -1, PI, C, 0, C, C, 0, k + 4, C)            # Wc: g_a x c
    layer(-1, O, 4 * NB, 0, H, 0, H, H, 0, kf, H)                       # Wf: g_out x h_NB
    return dict(src=src, table=table, jobs=np.asarray(jobs, np.int32).reshape(-1, JOB), shapes=shapes, poff=poff, nflat=nflat,
                nI=nI, C=C, H=H, Hp=Hp, O=O, Op=Op, NB=NB, PI=PI, Kin=Kin)


def structure_for(net):
    C = net.context_features
    return structure(net.initial_layer.weight.shape[1] - C, C, net.hidden_features, net.final_layer.weight.shape[0],
                     len(net.blocks))


def gather_host(params, st):
    """The blob as the device gather builds it (ops.pack_gather), in numpy: for the CPU emulator."""
    flat = np.concatenate([np.zeros(1, np.float64)] + [np.asarray(p, np.float64).reshape(-1) for p in params])
    return flat[st["src"]]
