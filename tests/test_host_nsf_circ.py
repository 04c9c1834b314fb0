"""CPU tests of the circular NSF coupling layer in one launch (csrc/nsf_circ.hip, flows/nsf_circ_pack.py, nf_nsf_wide_ft) and of the
UniformGaussian base: the packed streams and the per-feature table walked as the kernel walks them (tests/nsf_circ_emulator.py)
against the reference's float64 outputs of seven layers in both directions, the packer's rejections, the unchanged AR packs after the
table helper moved, the C ABI's argument validation without a GPU, the base distribution against the reference, and the code
object's metadata."""
import ctypes
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

import circ_wide_cases as cw
from conftest import ROOT, assert_close, golden_state, load_golden


@pytest.fixture(scope="module")
def nfa():
    import __graft_entry__
    import normflows_amd
    if not os.path.exists(normflows_amd.native_library_path()):
        __graft_entry__.build()
    return normflows_amd


@pytest.mark.parametrize("name", sorted(cw.LAYERS))
def test_emulated_kernel_matches_reference_float64(nfa, oracle, name):
    """blob, table and ftable of the fixture layers (five at 8 bins; f and g at 4 and 16 bins, where a lane-half of the final layer
    holds four features / one feature instead of two) walked in the kernel's order, in float64.  The conditioner's parameter lists
    against the dense float64 network at 1e-5 of the largest value (test_host_context's bar: the log2(e) / sqrt(hidden) scale is
    applied in float32).  The layer's outputs / log-dets against the reference's float64 legs: the existing emulator tests' bar for this
    comparison is 1e-4 on the outputs and conftest.ld_tol on the log-det (test_host_arnsf_ft, there against a float32 leg).  Both sides
    are float64 here, over the same float32 weights; what separates them is one float32 rounding of each width / height row of the
    final layer (the folded scale: 6e-8 relative on a logit of at most ~10, so <= 1e-6 on a softmax weight and on an output of at
    most 3.5; the log-det sums up to 66 per-feature terms with that error each), so the bars asserted are 1e-6 on the outputs and 1e-5
    on the log-det in both directions -- inside the 1e-4 bars, and tight enough to notice a 1e-5 slip in the scale.  The four outside
    coordinates give exactly 0."""
    import copy
    from normflows_amd.flows import nsf_circ_pack
    from nsf_circ_emulator import emulate_layer
    layer, g = cw.layer(nfa, name), cw.golden(name)
    prqct = layer.prqct
    D, NB, H, ind_circ, tb, rev = cw.LAYERS[name]
    packed = nsf_circ_pack.pack_nsf_circ(prqct)
    assert packed is not None and nsf_circ_pack.supported(prqct)
    blob, table, ftable = packed
    assert table[0] == D and table[3] == (128 if H <= 128 else 256) and table[24] == cw.bins(name) and table[25] == 1
    u = prqct.unconditional_transform
    uncond = [t.detach().double().numpy() for t in (u.unnormalized_widths, u.unnormalized_heights, u.unnormalized_derivatives)]
    x = g["x"].astype(np.float64)
    K, nT = cw.bins(name), len(prqct.transform_features)
    net64 = copy.deepcopy(prqct.transform_net).double()
    for direction, zk, lk in ((0, "z_inv_f64", "ld_inv_f64"), (1, "z_fwd_f64", "ld_fwd_f64")):
        y, ld, prm = emulate_layer(oracle, blob, table, ftable, uncond, x, direction)
        ident = torch.from_numpy(y if direction == 1 else x).index_select(1, prqct.identity_features)
        with torch.no_grad():
            ref = net64(ident).numpy().reshape(-1, nT, 3 * K + 1).copy()
        ref[:, :, :2 * K] *= 1.4426950408889634 / np.sqrt(float(H))
        want = np.concatenate([ref[:, :, :2 * K], ref[:, :, 2 * K + 1:3 * K], ref[:, :, 2 * K:2 * K + 1]], 2)   # ..., d1 .. d(K-1), d0
        assert np.max(np.abs(prm - want)) < 1e-5 * max(1.0, np.abs(want).max())
        print("%s dir %d: emulator vs reference float64  y %.3e  ld %.3e" % (name, direction, np.abs(y - g[zk]).max(), np.abs(ld - g[lk]).max()))
        assert_close(y, g[zk], what="%s dir %d outputs" % (name, direction), rtol=1e-6, atol=1e-6)
        assert_close(ld, g[lk], what="%s dir %d log-det" % (name, direction), rtol=1e-5, atol=1e-5)
        for r, c in g["outside"]:
            assert y[r, c] == 0.0 and g[zk][r, c] == 0.0


def test_feature_table_in_position_order(nfa):
    """The table of layer (a): identity positions [0, 3), transform positions [32, 35), the rest padding; tails, bounds and the
    periodic rows of the identity half's circular coordinate."""
    from arnsf_ft_emulator import FT_BOUND, FT_COL, FT_PERIODIC, FT_SCALE, FT_TAILS
    from normflows_amd.flows import nsf_circ_pack
    _, table, ft = nsf_circ_pack.pack_nsf_circ(cw.layer(nfa, "a").prqct)
    assert ft.shape == (8, 64) and table[1] == 64 and table[15] == 32
    col = ft[FT_COL].view(np.int32)
    assert col[:3].tolist() == [0, 2, 4] and col[32:35].tolist() == [1, 3, 5] and (np.delete(col, [0, 1, 2, 32, 33, 34]) == -1).all()
    assert ft[FT_TAILS].view(np.int32)[[0, 1, 2, 32, 33, 34]].tolist() == [1, 1, 2, 2, 2, 1]
    assert np.array_equal(ft[FT_BOUND][[0, 1, 2, 32, 33, 34]], np.float32(cw.TB_A)[[0, 2, 4, 1, 3, 5]])
    assert ft[FT_PERIODIC].view(np.int32).nonzero()[0].tolist() == [2]
    # wrapper.py:104-107 indexes the tensor bound with the position among the identity features
    assert ft[FT_SCALE][2] == np.float32(np.pi) / np.float32(cw.TB_A[2])


def test_weight_ring_over_two_tiles_of_a_persistent_workgroup(nfa):
    """nsf_circ_kernel loads its register ring once per launch and only resets `ap` between tiles: every wave's stream of the seven
    fixture layers (Hp 128 on 128-row tiles and Hp 256 on 64-row tiles; 4, 8 and 16 bins: 8 / 4 / 2 transform features per final
    group) walked twice (tests/nsf_circ_emulator.two_tile_ring_walk: hidden items through mf_item, final groups through
    mf_final_item's compile-time ring phases, `g < 0` entries consume nothing).  Each multiplied value is the stream entry the schedule
    means, the ring holds entries 0..7 again at the start of the second tile, no request leaves the wave's stream; both parities of
    the number of 4-entry groups per wave occur, and a wrap copy of zeros is noticed."""
    from normflows_amd.flows import nsf_circ_pack
    from nsf_circ_emulator import two_tile_ring_walk
    parities = {}
    for name in sorted(cw.LAYERS):
        blob, table, _ = nsf_circ_pack.pack_nsf_circ(cw.layer(nfa, name).prqct)
        groups = two_tile_ring_walk(blob, table)
        assert len(groups) == 8 and min(groups) >= 1
        for g in groups:
            parities.setdefault(g % 2, name)
    print("4-entry groups per wave: odd in layer %s, even in layer %s" % (parities.get(1), parities.get(0)))
    assert set(parities) == {0, 1}, parities
    blob, table, _ = nsf_circ_pack.pack_nsf_circ(cw.layer(nfa, "c").prqct)
    blob = blob.copy()
    blob[int(table[17]) - 8 * 256:int(table[17])] = 0.0
    with pytest.raises(AssertionError):
        two_tile_ring_walk(blob, table)


def test_packer_rejections_keep_the_layerwise_path(nfa):
    """What nf_nsf_wide_ft does not cover is declined by the packer (None): the route then never enters the new branch.  That the five
    layers of circ_wide_cases.DECLINED still evaluate needs a device (the package has no CPU path):
    test_gpu_nsf_circ.test_declined_layers_keep_the_layerwise_path runs each of them."""
    from torch import nn
    from normflows_amd.flows import nsf_circ_pack
    mk = lambda **kw: nfa.flows.CircularCoupledRationalQuadraticSpline(8, 2, 32, [1, 4], **kw).eval()
    pack = lambda layer: nsf_circ_pack.pack_nsf_circ(layer.prqct)
    assert pack(mk()) is not None and nsf_circ_pack.supported(mk().prqct)
    for what in cw.DECLINED:
        layer = cw.declined_layer(nfa, what)
        assert pack(layer) is None and not nsf_circ_pack.supported(layer.prqct), what
    assert pack(mk(activation=nn.Tanh)) is None                                              # non-ReLU blocks
    assert pack(nfa.flows.CircularCoupledRationalQuadraticSpline(8, 2, 300, [1, 4]).eval()) is None    # hidden > 256 (Hp 512 not built)
    assert pack(nfa.flows.CoupledRationalQuadraticSpline(8, 2, 32)) is None                  # string tails: nf_nsf_wide's layer


def test_ar_packs_unchanged_by_table_helper(nfa):
    """flows/maf_pack.feature_table is now feature_rows + table_from_rows (shared with nsf_circ_pack): the per-feature AR packs are
    byte-identical to what the packer wrote before (tests/golden/arnsf_ft_pack_parent.npz: digests of blob / table / ftable and the
    ftable itself, recorded with the previous revision's packer)."""
    from normflows_amd.flows import maf_pack
    rec = load_golden("arnsf_ft_pack_parent")
    cases = cw.ar_pack_cases(nfa)
    assert len(cases) == 3
    for name, t in cases.items():
        packed = maf_pack.pack_made(t.autoregressive_net, mult=t._output_dim_multiplier(), rows=True, features=(t.tails, t.tail_bound))
        assert packed is not None, name
        assert packed[2].dtype == np.float32 and packed[2].tobytes() == rec[name + "__ftable"].tobytes(), name
        for part, a in zip(("blob", "table", "ftable"), packed):
            assert hashlib.sha256(a.tobytes()).digest() == rec["%s__%s_sha256" % (name, part)].tobytes(), (name, part)


def test_c_abi_argument_validation(nfa):
    """nf_nsf_wide_ft / nf_nsf_wide_tables_ft reject bad arguments with nf_nsf_wide_ctx's codes before any launch."""
    lib = nfa._lib.lib()
    i32, i64, f64, vp = ctypes.c_int, ctypes.c_int64, ctypes.c_double, ctypes.c_void_p
    null, one = vp(0), vp(16)

    def ft(K=8, hp=128, B=8, D=6, x=one, ftable=one, tabs=one, direction=0, acc=0, mbw=1e-3):
        return lib.nf_nsf_wide_ft(x, one, one, one, one, ftable, tabs, i64(B), i32(D), i32(hp), i32(K), i32(direction), i32(acc),
                                  f64(mbw), f64(1e-3), f64(1e-3), null)
    assert ft(x=null) == -14 and ft(ftable=null) == -14 and ft(tabs=null) == -14                     # -EFAULT
    assert ft(K=5) == -95 and ft(K=10) == -95 and ft(hp=512) == -95 and ft(hp=64) == -95            # -ENOTSUP
    assert ft(B=-1) == -22 and ft(D=1) == -22 and ft(D=129) == -22 and ft(direction=2) == -22 and ft(acc=2) == -22
    assert ft(mbw=0.2) == -22                                                                        # utils/splines.py:121-124
    assert ft(B=0) == 0 and ft(B=0, x=null) == 0
    tables = lambda K=8, nI=3, uw=one: lib.nf_nsf_wide_tables_ft(uw, one, one, one, one, one, i32(nI), i32(K), f64(1e-3), f64(1e-3),
                                                                  f64(1e-3), null)
    assert tables(K=5) == -95 and tables(nI=0) == -22 and tables(nI=65) == -22 and tables(uw=null) == -14
    declared = nfa._lib.exported_symbols_declared()
    assert "nf_nsf_wide_ft" in declared and "nf_nsf_wide_tables_ft" in declared


def test_uniform_gaussian_matches_reference(nfa):
    g = load_golden("uniform_gaussian")
    scale = torch.tensor(cw.MODEL_SCALE, dtype=torch.float32)
    q0 = nfa.distributions.UniformGaussian(6, [1, 3, 4], scale)
    assert q0 is not None and nfa.UniformGaussian is nfa.distributions.UniformGaussian
    ref = golden_state(g)
    sd = q0.state_dict()
    assert sorted(sd) == sorted(ref) == ["ind", "ind_", "inv_perm", "scale"]
    for k, v in ref.items():
        assert tuple(sd[k].shape) == v.shape and sd[k].numpy().dtype == v.dtype and np.array_equal(sd[k].numpy(), v), k
    lp = q0.log_prob(torch.from_numpy(g["z"])).numpy()
    assert lp.dtype == np.float32
    np.testing.assert_allclose(lp, g["log_prob"], rtol=1e-6, atol=0)
    torch.manual_seed(5)
    z = q0.sample(4096)
    half = scale[[1, 3, 4]] / 2
    assert z.shape == (4096, 6) and bool((z[:, [1, 3, 4]].abs() <= half).all()) and float(z[:, [1, 3, 4]].abs().max()) > 0.9 * float(half.min())
    assert bool((z[:, [0, 2, 5]].abs() > scale[[0, 2, 5]]).any())                             # the others are Gaussian, not clipped
    torch.manual_seed(6)
    z, lq = q0(50)
    assert torch.equal(lq, q0.log_prob(z))
    one = nfa.distributions.UniformGaussian(3, 1)                                             # an int index, default scale
    assert one.ind.tolist() == [1] and one.ind_.tolist() == [0, 2] and one.inv_perm.tolist() == [1, 0, 2] and one.scale.tolist() == [1.0] * 3


def test_model_assembles_and_keeps_reference_state_layout(nfa):
    """The circular example model is buildable from this package and takes the reference's state dict (strict)."""
    m, g = cw.model(nfa)
    assert sorted(m.state_dict()) == sorted(golden_state(g))


def test_new_kernels_use_no_scratch(nfa):
    """Every instantiation of nsf_circ_kernel (4 / 8 / 16 bins, both directions, Hp 128 and 256) is free of scratch memory, read from
    the code object's metadata as test_host.test_tile_engine_and_maf_kernels_use_no_scratch does."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    seen = 0
    for name, d in kr.resources(os.path.join(ROOT, "normalizing-flows_amd", "lib", "obj", "nsf_circ.o")).items():
        if "nsf_circ_kernel" in name:
            seen += 1
            assert d["vgpr_spill_count"] == 0 and d["private_segment_fixed_size"] == 0, (name, d)
    assert seen == 12
