"""CPU tests of the conditional NSF coupling layer in one launch (csrc/nsf_ctx.hip, flows/nsf_ctx_pack.py, nf_nsf_wide_ctx): the
packed streams walked as the kernel walks them reproduce the float64 ResidualNet with context, the packer declines what the kernel does
not cover, the context-free pack is unchanged, the C ABI rejects bad arguments without a GPU, and no instantiation uses scratch."""
import copy
import ctypes
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT


@pytest.fixture(scope="module")
def nfa():
    import __graft_entry__
    import normflows_amd
    if not os.path.exists(normflows_amd.native_library_path()):
        __graft_entry__.build()
    return normflows_amd


def _layer(nfa, D, C, H, NB, K, rev=False, seed=0, **kw):
    torch.manual_seed(seed)
    layer = nfa.flows.CoupledRationalQuadraticSpline(D, NB, H, num_context_channels=C, num_bins=K, init_identity=False,
                                                     reverse_mask=rev, **kw)
    with torch.no_grad():
        for p in layer.parameters():
            p.add_(0.05 * torch.randn_like(p))
    return layer.eval()


# Hp 128 (128-row tiles) and Hp 256; K 4 / 8 / 16; odd D and C, C not a multiple of 4, PC 32 and 64, Dp 32 / 64 / 96, both parities
@pytest.mark.parametrize("D,C,H,NB,K,rev", [(6, 3, 40, 2, 8, False), (64, 16, 136, 1, 4, False), (17, 33, 200, 1, 16, True),
                                            (64, 16, 256, 2, 8, True), (16, 4, 128, 2, 8, False), (64, 64, 256, 2, 8, False),
                                            (65, 32, 128, 1, 4, True), (9, 7, 96, 3, 16, False), (5, 1, 33, 2, 4, True)])
def test_nsf_ctx_pack_matches_dense_conditioner(nfa, D, C, H, NB, K, rev):
    """flows/nsf_ctx_pack.py + the kernel's walk over the per-wave streams (tests/nsf_ctx_emulator.py) reproduce the reference-layout
    conditioner ResidualNet(identity features, context) (nets/resnet.py:37-50, 92-104: initial layer on cat(identity, context), the
    GLU gate per block) computed densely in float64.  One pack serves both directions: the conditioner sees the raw identity features
    in the density direction and their inverse-spline image in the sampling direction, the same network either way."""
    from normflows_amd.flows import nsf_ctx_pack
    from nsf_ctx_emulator import emulate_conditioner_ctx
    layer = _layer(nfa, D, C, H, NB, K, rev, seed=D + C + H)
    prqct = layer.prqct
    blob, table = nsf_ctx_pack.pack_nsf_ctx(prqct)
    assert table[0] == D and table[3] == (128 if H <= 128 else 256) and table[24] == K and table[25] == C
    assert table[26] == (C + 31) // 32 * 32 and blob.size % 256 == 0
    M_ = 3 * K - 1
    nT = len(prqct.transform_features)
    net64 = copy.deepcopy(prqct.transform_net).double()
    sc = 1.4426950408889634 / np.sqrt(float(H))
    g = torch.Generator().manual_seed(3)
    for rows in (torch.randn(7, D, generator=g), 4.0 * torch.randn(7, D, generator=g)):
        ctx = torch.randn(7, C, generator=g)
        with torch.no_grad():
            ref = net64(rows.double().index_select(1, prqct.identity_features), ctx.double()).numpy().reshape(7, nT, M_).copy()
        ref[:, :, :2 * K] *= sc
        got = emulate_conditioner_ctx(blob, table, rows.numpy(), ctx.numpy())
        assert np.max(np.abs(got[:, :, :M_] - ref)) < 1e-5 * max(1.0, np.abs(ref).max())     # (the scale is applied in float32)
        assert np.all(got[:, :, M_] == 0.0)


def test_nsf_ctx_pack_declines_unsupported(nfa):
    from torch import nn
    from normflows_amd.flows import nsf_ctx_pack
    pack = lambda layer: nsf_ctx_pack.pack_nsf_ctx(layer.prqct)
    assert pack(_layer(nfa, 8, 4, 64, 2, 8)) is not None
    assert pack(_layer(nfa, 8, 4, 64, 2, 8, activation=nn.Tanh)) is None                      # non-ReLU activation
    drop = _layer(nfa, 8, 4, 64, 2, 8, dropout_probability=0.1)
    assert pack(drop) is not None                                                              # eval: dropout is the identity
    assert pack(drop.train()) is None                                                          # dropout in training mode
    bn = _layer(nfa, 8, 4, 64, 2, 8)
    bn.prqct.transform_net.use_batch_norm = True
    assert pack(bn) is None                                                                    # batch norm
    pre = _layer(nfa, 8, 4, 64, 2, 8)
    pre.prqct.transform_net.preprocessing = nn.Identity()
    assert pack(pre) is None                                                                   # preprocessing
    circ = nfa.flows.CircularCoupledRationalQuadraticSpline(8, 2, 64, [1], num_context_channels=4, num_bins=8).eval()
    assert pack(circ) is None                                                                  # circular tails
    nou = _layer(nfa, 8, 4, 64, 2, 8)
    nou.prqct.unconditional_transform = None
    assert pack(nou) is None                                                                   # no unconditional transform
    odd = _layer(nfa, 8, 4, 64, 2, 8)
    odd.prqct.identity_features = torch.tensor([0, 1, 2, 3])
    odd.prqct.transform_features = torch.tensor([4, 5, 6, 7])
    assert pack(odd) is None                                                                   # a non-alternating mask
    assert pack(_layer(nfa, 65, 32, 64, 1, 8)) is not None                                     # Dp 96 + PC 32 = 128
    assert pack(_layer(nfa, 65, 33, 64, 1, 8)) is None                                         # Dp 96 + PC 64 > 128
    assert pack(_layer(nfa, 66, 1, 64, 1, 8)) is None                                          # Dp 128: no room for a context
    assert pack(_layer(nfa, 64, 65, 64, 1, 8)) is None                                         # Dp 64 + PC 96 > 128
    assert pack(_layer(nfa, 64, 64, 64, 1, 8)) is not None                                     # Dp 64 + PC 64 = 128
    assert pack(_layer(nfa, 8, 4, 300, 1, 8)) is None                                          # hidden > 256 (Hp 512 not built)
    assert pack(_layer(nfa, 8, 4, 64, 2, 10)) is None                                          # 10 bins
    plain = nfa.flows.CoupledRationalQuadraticSpline(8, 2, 64, num_bins=8)
    assert pack(plain) is None                                                                 # no context


def test_nsf_ctx_pack_boundary_widths(nfa):
    """The packer's Dp is the kernel's (C ABI) Dp for every D, either mask parity."""
    from normflows_amd.flows import nsf_ctx_pack
    for D in (2, 3, 63, 64, 65, 96, 97, 128):
        for rev in (False, True):
            prqct = _layer(nfa, D, 1, 32, 1, 8, rev).prqct
            ok = nsf_ctx_pack.x_positions(D) + 32 <= 128
            packed = nsf_ctx_pack.pack_nsf_ctx(prqct)
            assert (packed is not None) == ok, D
            if packed is not None:
                assert packed[1][1] == nsf_ctx_pack.x_positions(D)


def _by_value(n, i):
    return torch.sin(torch.arange(n, dtype=torch.float64) * 0.37 + i)


def _pack_digest(nfa, D, C, H, NB, K, rev, lu_direction=None):
    """sha256 of blob + table of the layer whose parameters (and LU matrix / bias, when asked for) are set by value."""
    from normflows_amd.flows import nsf_ctx_pack, nsf_wide_pack
    layer = nfa.flows.CoupledRationalQuadraticSpline(D, NB, H, num_context_channels=C, num_bins=K, init_identity=False,
                                                     reverse_mask=rev).eval()
    with torch.no_grad():
        for i, p in enumerate(layer.parameters()):
            p.copy_(_by_value(p.numel(), i).reshape(p.shape).float())
    if C is not None:
        blob, table = nsf_ctx_pack.pack_nsf_ctx(layer.prqct)
    elif lu_direction is None:
        blob, table = nsf_wide_pack.pack_nsf_wide(layer.prqct)
    else:
        lu = (_by_value(D * D, 0).reshape(D, D).numpy(), _by_value(D, 1).numpy())
        blob, table = nsf_wide_pack.pack_nsf_wide(layer.prqct, lu=lu, direction=lu_direction)
    assert not hasattr(layer.prqct, "_ctx_cache")
    return hashlib.sha256(blob.tobytes() + table.tobytes()).hexdigest()


def test_context_free_wide_pack_unchanged(nfa):
    """pack_nsf_wide's output for a context-free layer is byte-identical with the conditional pack present (digest of the pack of a
    layer with value-set parameters, recorded before nsf_ctx_pack.py existed); and every pack of PACK_DIGESTS -- plain, with the LU
    item in either position, conditional -- is byte-identical with what the two separate packers produced (recorded at commit
    767411e, the last one in which nsf_ctx_pack.py carried its own copy of the stream writer)."""
    digest = _pack_digest(nfa, 10, None, 160, 2, 8, False)
    assert digest == WIDE_PACK_DIGEST, digest
    for case, want in PACK_DIGESTS.items():
        got = _pack_digest(nfa, *case)
        assert got == want, (case, got)


WIDE_PACK_DIGEST = "d8e1479aec5bb4c9a7da9ea344b78ce190b222731460d5135e77721ce1ed4ceb"
# (D, C, hidden, blocks, bins, reverse_mask, LU direction): Hp 512, 4 and 16 bins, the LU item first / last, every conditional shape class
PACK_DIGESTS = {
    (128, None, 512, 2, 16, False, None): "853f8c4adabe3be6cc4b5fd8f101a41b3776147af1ef6e7739b8ed5a11b22735",
    (128, None, 512, 2, 16, False, 0): "2085ffd05b114256545b4da881bc634da2069339137eae6326c0f3f5bea37801",
    (128, None, 512, 2, 16, False, 1): "b492e69d62bed6c308ba2e3a5d392305839208769b2ef5626b940b3cf745cfe3",
    (7, None, 300, 2, 8, True, None): "9400f1cbb2811b5641680abf366507f51e10ee6efb728e9dd3ffa86e03f0267d",
    (7, None, 300, 2, 8, True, 0): "09be73ab68553d1bd65d4f8b822a8c4fb6d555fb0698cccb420acbab00393850",
    (7, None, 300, 2, 8, True, 1): "0d6fd4a98a28496ce2594dc1a15cb9fdb1eb86a904827d4698956cdc25f8cde1",
    (64, None, 256, 2, 4, False, None): "a68bd8bacdd6e120e7bc39898c6e12bc249ce1792e4cb183a12820d34b34a945",
    (6, 3, 40, 2, 8, False, None): "16b58683dac993cecaa9e7f3e3170b4b303fa5e4b822621557e5235d0238346d",
    (17, 33, 200, 1, 16, True, None): "1d786121a01c6eb4c37ab5b30b09bec2590532d0450a7fb7da7a8c549bc127f4",
    (64, 64, 256, 2, 8, False, None): "543d7cc6027f850e9766bba7d87a92d978c018eb79960d1f0347c2aa9d17a1f3",
    (65, 32, 128, 1, 4, True, None): "34c3ec37649460ac191a6100143f383e9f8390c7556ce4df23c03c2b19269d3c",
}


def test_nsf_wide_ctx_argument_validation_without_gpu(nfa):
    """nf_nsf_wide_ctx rejects bad arguments with the documented codes before any HIP call (this machine has no GPU)."""
    lib = nfa._lib.lib()
    i32, i64, f64, vp = ctypes.c_int, ctypes.c_int64, ctypes.c_double, ctypes.c_void_p
    nul, one = vp(0), vp(16)        # never dereferenced on the host

    def call(ptrs=one, B=5, ldc=4, D=8, C=4, Hp=256, K=8, direction=0, acc=0, mbw=1e-3):
        return lib.nf_nsf_wide_ctx(ptrs, ptrs, ptrs, ptrs, ptrs, ptrs, ptrs, i64(B), i64(ldc), i32(D), i32(C), i32(Hp), i32(K),
                                   i32(direction), i32(acc), f64(3.0), f64(mbw), f64(1e-3), f64(1e-3), nul)
    assert call(B=-1) == -22
    assert call(C=0) == -22
    assert call(ldc=-1) == -22
    assert call(direction=2) == -22
    assert call(acc=3) == -22
    assert call(D=1) == -22
    assert call(mbw=0.2) == -22                    # min_bin_width * K > 1
    assert call(Hp=512) == -95                     # not built (spills)
    assert call(Hp=192) == -95
    assert call(K=10) == -95
    assert call(D=65, C=33) == -95                 # Dp 96 + PC 64 > 128
    assert call(D=96, C=1) == -95                  # Dp 128 + PC 32
    assert call(D=64, C=65) == -95
    assert call(D=128, C=1) == -95
    assert call(ptrs=nul, B=0) == 0                # empty batch: OK without touching a pointer
    assert call(ptrs=nul) == -14
    assert call(ptrs=nul, D=64, C=64, Hp=128, K=16) == -14   # valid shape, NULL pointers
    assert call(ptrs=nul, ldc=0) == -14


def test_nsf_ctx_kernels_use_no_scratch(nfa):
    """Every instantiation of nsf_ctx_kernel (Hp 128 / 256 x both directions x 4 / 8 / 16 bins) is free of scratch memory."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    obj = os.path.join(ROOT, "normalizing-flows_amd", "lib", "obj", "nsf_ctx.o")
    seen = 0
    for name, d in kr.resources(obj).items():
        if "nsf_ctx_kernel" in name:
            seen += 1
            assert d["vgpr_spill_count"] == 0 and d["private_segment_fixed_size"] == 0, (name, d)
    assert seen == 12, seen


def test_ops_nsf_wide_ctx_needs_a_device(nfa):
    """No CPU path: ops.nsf_wide_ctx on host tensors raises before any launch."""
    x, c = torch.zeros(4, 8), torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match="MI355X"):
        nfa.ops.nsf_wide_ctx(x, c, torch.zeros(256), torch.zeros(64, dtype=torch.int32), torch.zeros(4, 27), 128, 0, 3.0)
