"""CPU-side tests of the per-feature AR-NSF sampling path (nf_arnsf_inverse_ft): the packer's degree-order schedule and feature
table (flows/maf_pack.py) walked by tests/arnsf_ft_emulator.py against the D-pass fixed point in float64 and against the reference's
stored outputs, the unchanged pack of the structures the packer took before, its rejections, and the C ABI's argument validation."""
import copy
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import assert_close, golden_state, ld_tol, load_golden

@pytest.fixture(scope="module")
def nfa():
    import __graft_entry__
    import normflows_amd
    if not os.path.exists(normflows_amd.native_library_path()):
        __graft_entry__.build()
    return normflows_amd


def fixture_layer(nfa, dtype=torch.float32):
    g = load_golden("circ_ar_perm_tb")
    bound = torch.from_numpy(g["sd__mprqat__tail_bound"])
    layer = nfa.flows.CircularAutoregressiveRationalQuadraticSpline(7, 2, 24, ind_circ=[0, 2, 5], num_bins=6, tail_bound=bound,
                                                                    permute_mask=True, init_identity=False)
    layer.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in golden_state(g).items()}, strict=True)
    return layer.to(dtype), g


def perturbed(layer, sigma, seed):
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in layer.parameters():
            p.add_(sigma * torch.randn(p.shape, generator=gen, dtype=p.dtype))
    return layer


def input_degrees(t):
    mult = t._output_dim_multiplier()
    return t.autoregressive_net.final_layer.degrees.numpy()[::mult]


def spline_column(K, tails, bound, prm, zf):
    """The inverse spline of one feature from its `mult` conditioner outputs (oracle, the precision of its inputs).  List tails are
    utils/splines.py:48-57: K + 1 derivative logits with the edges overwritten per type, and 0 / log-det 0 outside the interval."""
    import nf_oracle
    prm, zf = np.ascontiguousarray(prm), np.ascontiguousarray(zf)
    w, h, d = prm[:, :K], prm[:, K:2 * K], prm[:, 2 * K:]
    if isinstance(tails, tuple):                 # ("list", type): the per-feature branch
        kind = tails[1]
        d = d[:, 1:K] if kind == "linear" else d[:, :K]
        y, lad = nf_oracle.rqs_spline(zf, w, h, np.ascontiguousarray(d), inverse=True, tails=kind, tail_bound=float(bound))
        out = np.abs(zf) > bound
        return np.where(out, 0.0, y), np.where(out, 0.0, lad)
    return nf_oracle.rqs_spline(zf, w, h, d, inverse=True, tails=tails, tail_bound=float(bound))


def d_pass(t, z):
    """neural_spline/autoregressive.py:94-134 over affine/autoregressive.py:29-38 on a float64 copy of the layer: D passes of MADE (its
    preprocessing included), feature by feature through the oracle spline in COLUMN order."""
    t = copy.deepcopy(t).double()
    D, K, mult = t.features, t.num_bins, t._output_dim_multiplier()
    listed = isinstance(t.tails, (list, tuple))
    tb = t.tail_bound.double().numpy() if torch.is_tensor(t.tail_bound) else np.full(D, float(t.tail_bound))
    tails = [("list", t.tails[c]) if listed else t.tails for c in range(D)]
    out = np.zeros_like(z)
    with torch.no_grad():
        for _ in range(D):
            prm = t.autoregressive_net(torch.from_numpy(out)).view(-1, D, mult).numpy()
            cols = [spline_column(K, tails[c], tb[c], prm[:, c], z[:, c]) for c in range(D)]
            out = np.stack([c[0] for c in cols], 1)
    return out, np.stack([c[1] for c in cols], 1).sum(1)


def emulate(nfa, t, z):
    """The packed schedule of the float32 parameters' float64 images walked as the kernel walks it: type and bound of every step from
    the feature table."""
    from arnsf_ft_emulator import FT_BOUND, FT_TAILS, emulate_inverse_ft
    from normflows_amd.flows import maf_pack
    K, mult = t.num_bins, t._output_dim_multiplier()
    packed = maf_pack.pack_made(t.autoregressive_net, mult=mult, rows=True, features=(t.tails, t.tail_bound))
    assert packed is not None
    blob, table, ftable = packed
    listed = isinstance(t.tails, (list, tuple))
    codes = ftable[FT_TAILS].view(np.int32)

    def element(f, prm, zf):
        kind = {0: None, 1: "linear", 2: "circular"}[int(codes[f])]
        return spline_column(K, ("list", kind) if listed else kind, np.float64(ftable[FT_BOUND, f]), prm, zf)
    return emulate_inverse_ft(blob, table, ftable, z, element), (blob, table, ftable)


def inputs_inside(t, rows, seed, outside=()):
    D = t.features
    tb = t.tail_bound.double().numpy() if torch.is_tensor(t.tail_bound) else np.full(D, float(t.tail_bound))
    z = (torch.rand(rows, D, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).numpy() * 2 - 1) * tb * 0.98
    for r, c, v in outside:
        z[r, c] = v
    return z


def test_fixture_layer_schedule_matches_d_pass_and_reference(nfa):
    """(a) the fixture layer: permuted mask, list tails, tensor bound, periodic preprocessing.  The emulated schedule is the D-pass
    fixed point in float64 (1e-9) and the reference's stored sampling output at the fixture bars."""
    layer, g = fixture_layer(nfa)
    t = layer.mprqat
    assert not np.array_equal(input_degrees(t), np.arange(1, 8))
    z = g["x"].astype(np.float64)
    (x, ld), (_, _, ftable) = emulate(nfa, t, z)
    ref_x, ref_ld = d_pass(t, z)
    np.testing.assert_allclose(x, ref_x, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(ld, ref_ld, rtol=1e-9, atol=1e-9)
    assert x[0, 1] == 0.0 and x[1, 3] == 0.0                        # linear features outside their interval
    assert_close(x, g["z_fwd"].astype(np.float64), what="x vs reference", rtol=1e-4, atol=1e-4)
    assert_close(ld, g["ld_fwd"].astype(np.float64), what="ld vs reference", **ld_tol(np.float32, root_finding=True))
    # the table is in degree order
    from arnsf_ft_emulator import FT_BOUND, FT_COL, FT_PERIODIC, FT_TAILS
    col = ftable[FT_COL].view(np.int32)
    assert np.array_equal(input_degrees(t)[col], np.arange(1, 8))
    assert np.array_equal(ftable[FT_PERIODIC].view(np.int32), np.isin(col, [0, 2, 5]).astype(np.int32))
    assert np.array_equal(ftable[FT_TAILS].view(np.int32), np.where(np.isin(col, [0, 2, 5]), 2, 1))
    assert np.array_equal(ftable[FT_BOUND], g["sd__mprqat__tail_bound"][col])


def wide_circular_layer(nfa, seed=5):
    """(b) D = 40, hidden = 96, K = 8 on a permuted mask: four tiles; circular columns = the degree-1 feature, the last feature of
    tile 0 and a mid-tile feature of tile 1, read from the tile plan through col[]; tensor bounds."""
    from normflows_amd.flows import maf_pack
    D, H, K = 40, 96, 8

    def build(ind_circ, bound):
        torch.manual_seed(seed)          # (the permutation is the constructor's first draw: the same for every ind_circ)
        return nfa.flows.CircularAutoregressiveRationalQuadraticSpline(D, 2, H, ind_circ=ind_circ, num_bins=K, tail_bound=bound,
                                                                       permute_mask=True, init_identity=False)
    probe = build([0], 3.0).mprqat
    deg = input_degrees(probe)
    col = np.argsort(deg, kind="stable")
    tiles = maf_pack.plan_tiles(D, probe.autoregressive_net.initial_layer.degrees.numpy())[1]
    assert len(tiles) == 4
    (dlo0, ns0, _), (dlo1, ns1, _) = tiles[0], tiles[1]
    steps = [0, dlo0 + ns0 - 1, dlo1 + ns1 // 2]                      # schedule positions (degree - 1)
    ind_circ = sorted(int(col[f]) for f in steps)
    bound = 1.5 + 2.0 * torch.rand(D, generator=torch.Generator().manual_seed(seed + 1))
    bound[ind_circ] = float(np.pi)
    layer = build(ind_circ, bound)
    assert np.array_equal(input_degrees(layer.mprqat), deg) and not np.array_equal(deg, np.arange(1, D + 1))
    return perturbed(layer, 0.1, seed + 2), ind_circ, steps


def test_wide_circular_schedule_matches_d_pass(nfa):
    layer, ind_circ, steps = wide_circular_layer(nfa)
    t = layer.mprqat
    lin = [c for c in range(t.features) if c not in ind_circ]
    z = inputs_inside(t, 6, 3, outside=[(0, lin[3], 50.0), (1, lin[17], -60.0)])
    (x, ld), (_, _, ftable) = emulate(nfa, t, z)
    from arnsf_ft_emulator import FT_PERIODIC
    assert np.nonzero(ftable[FT_PERIODIC].view(np.int32))[0].tolist() == steps
    ref_x, ref_ld = d_pass(t, z)
    np.testing.assert_allclose(x, ref_x, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(ld, ref_ld, rtol=1e-9, atol=1e-9)
    assert x[0, lin[3]] == 0.0 and x[1, lin[17]] == 0.0


def test_permuted_linear_tails_schedule_matches_d_pass(nfa):
    """(c) plain linear tails (3K - 1 outputs per feature, identity outside the interval) with permute_mask=True."""
    torch.manual_seed(8)
    layer = nfa.flows.AutoregressiveRationalQuadraticSpline(9, 2, 40, num_bins=4, tail_bound=2.5, permute_mask=True,
                                                            init_identity=False)
    t = perturbed(layer, 0.1, 9).mprqat
    assert not np.array_equal(input_degrees(t), np.arange(1, 10))
    z = inputs_inside(t, 8, 4, outside=[(0, 2, 7.0), (3, 8, -4.0)])
    (x, ld), (_, _, ftable) = emulate(nfa, t, z)
    from arnsf_ft_emulator import FT_PERIODIC
    assert not ftable[FT_PERIODIC].view(np.int32).any()
    ref_x, ref_ld = d_pass(t, z)
    np.testing.assert_allclose(x, ref_x, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(ld, ref_ld, rtol=1e-9, atol=1e-9)
    assert x[0, 2] == 7.0 and x[3, 8] == -4.0


def test_plain_rows_pack_is_unchanged(nfa, monkeypatch):
    """An unpermuted, preprocessing-free MADE: pack_made(..., rows=True) never enters the per-feature branch, and the per-feature
    variant of the same MADE carries the very same blob and table (identity column order) -- the rows layout did not move."""
    from normflows_amd import nets
    from normflows_amd.flows import maf_pack
    torch.manual_seed(3)
    made = nets.MADE(features=9, hidden_features=40, num_blocks=2, output_multiplier=11)
    with torch.no_grad():
        for p in made.parameters():
            p.add_(0.1 * torch.randn_like(p))
    blob_f, table_f, ftable = maf_pack.pack_made(made, mult=11, rows=True, features=("linear", 2.5))

    def entered(*a, **k):
        raise AssertionError("per-feature branch entered")
    monkeypatch.setattr(maf_pack, "feature_table", entered)
    blob, table = maf_pack.pack_made(made, mult=11, rows=True)
    assert blob.tobytes() == blob_f.tobytes() and table.tobytes() == table_f.tobytes()
    assert np.array_equal(ftable[0].view(np.int32), np.arange(9)) and not ftable[3:].any()
    # and the plain layout keeps refusing what only the per-feature variant takes
    torch.manual_seed(3)
    permuted = nets.MADE(features=9, hidden_features=40, num_blocks=2, output_multiplier=11, permute_mask=True)
    assert maf_pack.pack_made(permuted, mult=11, rows=True) is None
    periodic = nets.MADE(features=9, hidden_features=40, num_blocks=2, output_multiplier=11,
                         preprocessing=nets.PeriodicFeaturesElementwise(9, [1, 4], 1.0))
    assert maf_pack.pack_made(periodic, mult=11, rows=True) is None
    assert maf_pack.pack_made(permuted, mult=2, features=("linear", 2.5)) is None           # rows layout only


def test_per_feature_pack_rejections(nfa):
    from normflows_amd import nets
    from normflows_amd.flows import maf_pack
    # K = 11 with list tails: 3K + 1 = 34 rows per feature do not fit one 32-row block
    t = nfa.flows.CircularAutoregressiveRationalQuadraticSpline(5, 2, 12, ind_circ=[1], num_bins=11, tail_bound=2.0).mprqat
    assert maf_pack.pack_made(t.autoregressive_net, mult=34, rows=True, features=(t.tails, t.tail_bound)) is None
    t = nfa.flows.CircularAutoregressiveRationalQuadraticSpline(5, 2, 12, ind_circ=[1], num_bins=10, tail_bound=2.0).mprqat
    assert maf_pack.pack_made(t.autoregressive_net, mult=31, rows=True, features=(t.tails, t.tail_bound)) is not None
    # a preprocessing with a non-identity activation
    pre = nets.PeriodicFeaturesElementwise(5, [1], 1.0, activation=torch.nn.Tanh())
    made = nets.MADE(features=5, hidden_features=12, num_blocks=2, output_multiplier=13, preprocessing=pre)
    assert maf_pack.pack_made(made, mult=13, rows=True, features=(["linear", "circular"] + ["linear"] * 3, 2.0)) is None
    # any other preprocessing
    made = nets.MADE(features=5, hidden_features=12, num_blocks=2, output_multiplier=13, preprocessing=torch.nn.Tanh())
    assert maf_pack.pack_made(made, mult=13, rows=True, features=("linear", 2.0)) is None
    # a MADE with context
    made = nets.MADE(features=5, hidden_features=12, context_features=3, num_blocks=2, output_multiplier=13)
    assert maf_pack.pack_made(made, mult=13, rows=True, features=(None, 1.0)) is None
    # fewer hidden units than degrees
    made = nets.MADE(features=12, hidden_features=4, num_blocks=2, output_multiplier=13, permute_mask=True)
    assert maf_pack.pack_made(made, mult=13, rows=True, features=(None, 1.0)) is None


def test_c_abi_argument_validation(nfa):
    """nf_arnsf_inverse_ft rejects what nf_arnsf_inverse rejects, with the same codes, before any launch."""
    lib = nfa._lib.lib()
    i32, i64, f64, vp = ctypes.c_int, ctypes.c_int64, ctypes.c_double, ctypes.c_void_p
    null, one = vp(0), vp(16)

    def ft(K, tails, hp=512, B=8, blob=one, ftable=one, mbw=1e-3):
        return lib.nf_arnsf_inverse_ft(one, one, one, blob, one, ftable, one, i64(B), i32(64), i32(hp), i32(K), i32(tails),
                                       f64(mbw), f64(1e-3), f64(1e-3), i32(0), null)
    assert ft(11, 3) == -95 and ft(11, 0) == -95 and ft(11, 2) == -95 and ft(12, 1) == -95        # 3K+1 | 3K | 3K-1 > 32 rows
    assert ft(8, 4) == -22 and ft(8, -1) == -22 and ft(0, 3) == -22 and ft(8, 3, hp=500) == -22 and ft(8, 3, hp=0) == -22
    assert ft(8, 3, mbw=0.2) == -22                                                                 # utils/splines.py:121-124
    assert ft(8, 3, blob=null) == -14 and ft(8, 3, ftable=null) == -14
    assert ft(8, 3, B=0) == 0 and ft(10, 3, B=0) == 0 and ft(11, 1, B=0) == 0
    assert "nf_arnsf_inverse_ft" in nfa._lib.exported_symbols_declared()
