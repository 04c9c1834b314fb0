"""CPU-side tests of the per-feature AR-NSF density path (nf_made_forward_spline_ft, csrc/made_fwd_ft.hip): the packer's degree-order
streams, slot layout and feature table (flows/made_pack.pack_made_forward_ft) walked by tests/made_fwd_ft_emulator.py against the
reference's stored density direction, the packer's eligibility, the C ABI's argument validation and the code object's resources."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from conftest import assert_close, golden_state, ld_tol, load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def nfa():
    import __graft_entry__
    import normflows_amd
    if not os.path.exists(normflows_amd.native_library_path()):
        __graft_entry__.build()
    return normflows_amd


def circular_fixture(nfa):
    g = load_golden("circ_ar_perm_tb")
    layer = nfa.flows.CircularAutoregressiveRationalQuadraticSpline(7, 2, 24, ind_circ=[0, 2, 5], num_bins=6,
                                                                    tail_bound=torch.from_numpy(g["sd__mprqat__tail_bound"]),
                                                                    permute_mask=True, init_identity=False)
    layer.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in golden_state(g).items()}, strict=True)
    return layer, g


def linear_fixture(nfa):
    g = load_golden("ar_perm_lin")
    layer = nfa.flows.AutoregressiveRationalQuadraticSpline(6, 2, 20, num_bins=4, tail_bound=2.5, permute_mask=True, init_identity=False)
    layer.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in golden_state(g).items()}, strict=True)
    return layer, g


def pack(t):
    from normflows_amd.flows import made_pack
    return made_pack.pack_made_forward_ft(t.autoregressive_net, t._output_dim_multiplier(), t.num_bins, t.tails, t.tail_bound)


def emulate(t, x):
    """The packed schedule on the float64 images of the float32 parameters; every feature's spline through the oracle with the type
    and bound of the feature table, its parameters read from the kernel's slots."""
    import nf_oracle
    from arnsf_ft_emulator import FT_BOUND, FT_TAILS
    from made_fwd_ft_emulator import SLOT_D, SLOT_H, emulate_forward_ft
    packed = pack(t)
    assert packed is not None
    blob, table, ftable = packed
    K = t.num_bins
    listed = isinstance(t.tails, (list, tuple))
    codes = ftable[FT_TAILS].view(np.int32)

    def element(f, slots, xf):
        kind = {0: None, 1: "linear", 2: "circular"}[int(codes[f])]
        bound = float(ftable[FT_BOUND, f])
        w, h = np.ascontiguousarray(slots[:, :K]), np.ascontiguousarray(slots[:, SLOT_H:SLOT_H + K])
        lo, hi = {"linear": (1, K), "circular": (0, K), None: (0, K + 1)}[kind]
        d = np.ascontiguousarray(slots[:, SLOT_D + lo:SLOT_D + hi])
        yv, lad = nf_oracle.rqs_spline(np.ascontiguousarray(xf), w, h, d, inverse=False, tails=kind, tail_bound=bound)
        if listed:                               # utils/splines.py:48-57: the outside inputs are never copied
            out = ~((xf >= -bound) & (xf <= bound))
            yv, lad = np.where(out, 0.0, yv), np.where(out, 0.0, lad)
        return yv, lad
    return emulate_forward_ft(blob, table, ftable, x, element), packed


def test_symbol_is_declared_exported_and_validates_its_arguments(nfa):
    assert "nf_made_forward_spline_ft" in nfa._lib.exported_symbols_declared()
    lib = nfa._lib.lib()
    assert hasattr(lib, "nf_made_forward_spline_ft") and hasattr(nfa.ops, "made_forward_spline_ft")
    assert nfa.config.arnsf_density_ft is True
    i32, i64, f64, vp = ctypes.c_int, ctypes.c_int64, ctypes.c_double, ctypes.c_void_p
    null, one = vp(0), vp(16)

    def ft(K, tails, hp=512, B=8, D=64, blob=one, ftable=one, mbw=1e-3, acc=0):
        return lib.nf_made_forward_spline_ft(one, one, one, blob, one, ftable, i64(B), i32(D), i32(hp), i32(K), i32(tails),
                                             f64(mbw), f64(1e-3), f64(1e-3), i32(acc), null)
    assert ft(11, 3) == -95 and ft(11, 0) == -95 and ft(11, 2) == -95 and ft(12, 1) == -95          # 3K+1 | 3K | 3K-1 > 32 rows
    assert ft(8, 3, hp=128) == -95 and ft(8, 3, hp=500) == -95
    assert ft(8, 4) == -22 and ft(8, -1) == -22 and ft(0, 3) == -22 and ft(8, 3, D=129) == -22 and ft(8, 3, D=1) == -22
    assert ft(8, 3, mbw=0.2) == -22 and ft(8, 3, acc=7) == -22
    assert ft(8, 3, blob=null) == -14 and ft(8, 3, ftable=null) == -14
    assert ft(8, 3, B=0) == 0 and ft(10, 3, B=0) == 0 and ft(11, 1, B=0) == 0


def test_circular_fixture_schedule_reproduces_the_reference_density(nfa):
    """Permuted mask, list tails, tensor bound, periodic feed (K 6, mult 19).  The emulated schedule against the reference's float64
    leg (the same float32 parameters widened: only summation order differs) and against its float32 leg at the fixture bars of
    tests/test_host_arnsf_ft.py."""
    layer, g = circular_fixture(nfa)
    t = layer.mprqat
    (z, ld), (_, table, ftable) = emulate(t, g["x"].astype(np.float64))
    np.testing.assert_allclose(z, g["z_inv_f64"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(ld, g["ld_inv_f64"], rtol=1e-9, atol=1e-9)
    assert z[0, 1] == 0.0 and z[1, 3] == 0.0                          # linear features outside their interval
    assert_close(z, g["z_inv"].astype(np.float64), what="z vs reference", rtol=1e-4, atol=1e-4)
    assert_close(ld, g["ld_inv"].astype(np.float64), what="ld vs reference", **ld_tol(np.float32))
    from arnsf_ft_emulator import FT_COL, FT_PERIODIC
    col = ftable[FT_COL].view(np.int32)
    deg = t.autoregressive_net.final_layer.degrees.numpy()[::19]
    assert np.array_equal(deg[col], np.arange(1, 8)) and not np.array_equal(col, np.arange(7))
    assert np.array_equal(ftable[FT_PERIODIC].view(np.int32), np.isin(col, [0, 2, 5]).astype(np.int32))
    assert table[3] == 256 and table[8] == 1 and table[11] == 2


def test_permuted_linear_fixture_schedule_reproduces_the_reference_density(nfa):
    """AutoregressiveRationalQuadraticSpline(permute_mask=True), scalar linear tails (D 6, hidden 20, K 4: mult 11 = 3K - 1, logits
    1 .. K - 1 in slots 21 ..), two entries outside the bound: identity there."""
    layer, g = linear_fixture(nfa)
    t = layer.mprqat
    assert t._permuted()
    (z, ld), _ = emulate(t, g["x"].astype(np.float64))
    np.testing.assert_allclose(z, g["z_inv_f64"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(ld, g["ld_inv_f64"], rtol=1e-9, atol=1e-9)
    assert z[0, 2] == 7.0 and z[3, 5] == -4.0
    assert_close(z, g["z_inv"].astype(np.float64), what="z vs reference", rtol=1e-4, atol=1e-4)
    assert_close(ld, g["ld_inv"].astype(np.float64), what="ld vs reference", **ld_tol(np.float32))


def test_wide_schedule_masked_ranges_and_two_sample_block_items(nfa):
    """Hidden 300 (512 slots: items span both sample blocks), D 33 (two 32-feature pads), K 10 list tails (31 slots), 70 rows (two
    tiles, the second ragged) against the layer's own eager float64 evaluation."""
    import copy
    torch.manual_seed(3)
    layer = nfa.flows.CircularAutoregressiveRationalQuadraticSpline(33, 1, 300, ind_circ=[1, 8, 32], num_bins=10, tail_bound=3.0,
                                                                    permute_mask=True, init_identity=False)
    t = layer.mprqat
    x = ((torch.rand(70, 33, generator=torch.Generator().manual_seed(4), dtype=torch.float64) * 2 - 1) * 2.9)
    x[5, 4] = 40.0
    (z, ld), (_, table, _) = emulate(t, x.numpy())
    assert table[3] == 512 and table[4] == 2 and table[8] == 5
    nitems = int(table[10])
    nkg = table[32:].reshape(8, nitems, 2)[:, :, 0]
    assert nkg[:, 2:6].max() == 40 and nkg[:, 2:6].min() < 40          # 300 units = 38 k-groups, rounded to 4; masked prefixes
    import nf_oracle
    with torch.no_grad():                        # the MADE module (its preprocessing included) in float64, then the oracle per COLUMN
        prm = copy.deepcopy(t.autoregressive_net).double()(x).view(70, 33, 31).numpy()
    zr, ldr = np.zeros((70, 33)), np.zeros(70)
    for c in range(33):
        kind = t.tails[c]
        d = prm[:, c, 21:30] if kind == "linear" else prm[:, c, 20:30]
        yv, lad = nf_oracle.rqs_spline(np.ascontiguousarray(x.numpy()[:, c]), np.ascontiguousarray(prm[:, c, :10]),
                                       np.ascontiguousarray(prm[:, c, 10:20]), np.ascontiguousarray(d), inverse=False, tails=kind,
                                       tail_bound=3.0)
        out = np.abs(x.numpy()[:, c]) > 3.0
        zr[:, c] = np.where(out, 0.0, yv)
        ldr += np.where(out, 0.0, lad)
    # (the table holds the periodic scale pi / bound as float32, 6e-8 relative, the module as a double: every feature downstream of a
    # circular one moves by that much times O(1) weights -- 1e-6, where an index error would show at O(1))
    np.testing.assert_allclose(z, zr, rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(ld, ldr, rtol=1e-6, atol=1e-6)
    assert z[5, 4] == 0.0


def test_full_block_k11_scalar_linear_schedule(nfa):
    """K = 11 with scalar linear tails on a permuted mask: 3K - 1 = 32 rows fill the feature's block (heights in slots 11 .. 21,
    logits 1 .. 10 in slots 22 .. 31; logit 11 is an edge and has no slot), against the MADE module in float64 + the oracle."""
    import copy
    import nf_oracle
    torch.manual_seed(12)
    t = nfa.flows.AutoregressiveRationalQuadraticSpline(5, 2, 12, num_bins=11, tail_bound=2.5, permute_mask=True,
                                                        init_identity=False).mprqat
    assert t._output_dim_multiplier() == 32
    with torch.no_grad():
        for p in t.parameters():
            p.mul_(1.5)
    x = (torch.rand(9, 5, generator=torch.Generator().manual_seed(2), dtype=torch.float64) * 2 - 1) * 2.45
    x[2, 1] = 9.0
    (z, ld), _ = emulate(t, x.numpy())
    with torch.no_grad():
        prm = copy.deepcopy(t.autoregressive_net).double()(x).view(9, 5, 32).numpy()
    zr, ldr = np.zeros((9, 5)), np.zeros(9)
    for c in range(5):
        yv, lad = nf_oracle.rqs_spline(np.ascontiguousarray(x.numpy()[:, c]), np.ascontiguousarray(prm[:, c, :11]),
                                       np.ascontiguousarray(prm[:, c, 11:22]), np.ascontiguousarray(prm[:, c, 22:]), inverse=False,
                                       tails="linear", tail_bound=2.5)
        zr[:, c] = yv
        ldr += lad
    np.testing.assert_allclose(z, zr, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(ld, ldr, rtol=1e-9, atol=1e-9)
    assert z[2, 1] == 9.0


def _cpu_case(nfa, monkeypatch, case):
    """tests/test_gpu_made_fwd_ft.build_case with the layer left on the CPU."""
    import test_gpu_made_fwd_ft as gpu_cases
    monkeypatch.setattr(gpu_cases, "DEV", "cpu")
    return gpu_cases.build_case(nfa, case)


RING_CASES = ["d2_h4_k4", "d33_h24_k6", "d128_h300_k10", "all_circular", "none_circular", "scalar_linear_permuted",
              "scalar_linear_k11_permuted", "scalar_linear_tensor_bound", "scalar_circular_tensor_bound"]


def test_weight_ring_over_two_tiles_of_a_persistent_workgroup(nfa, monkeypatch):
    """The register ring is loaded once per launch and only `ap` is reset between tiles: walking every wave's stream of every GPU-test
    shape twice (tests/made_fwd_ft_emulator.two_tile_ring_walk: four bias entries + nkg A entries per item, `f < 0` entries consume
    nothing, every entry re-requested 8 ahead), each multiplied value is the stream entry the schedule means, the ring holds entries
    0..7 again at the start of the second tile and no request leaves the wave's stream.  Both parities of the number of 4-entry groups
    per wave occur (odd: the last item ends in ring half 0 without a swap; even: through the swap)."""
    from made_fwd_ft_emulator import two_tile_ring_walk
    parities = {}
    for case in RING_CASES:
        blob, table, _ = pack(_cpu_case(nfa, monkeypatch, case))
        groups = two_tile_ring_walk(blob, table)
        assert len(groups) == 8 and min(groups) >= 1
        for g in groups:
            parities.setdefault(g % 2, case)
    print("4-entry groups per wave: odd in %s, even in %s" % (parities.get(1), parities.get(0)))
    assert set(parities) == {0, 1}, parities


@pytest.mark.parametrize("what", ["zero_wrap", "short_item", "skipped_item_with_entries"])
def test_ring_walk_notices_a_stream_the_kernel_would_misread(nfa, monkeypatch, what):
    """The walk fails on a wrap copy of zeros, on an item whose A entries are fewer than its table entry says, and on a skipped entry
    (feature < 0) that still owns stream entries."""
    from made_fwd_ft_emulator import two_tile_ring_walk
    blob, table, _ = pack(_cpu_case(nfa, monkeypatch, "d33_h24_k6"))
    blob, table = blob.copy(), table.copy()
    nitems = int(table[10])
    if what == "zero_wrap":
        blob[int(table[17]) - 8 * 256:int(table[17])] = 0.0
    elif what == "short_item":
        table[32 + 2 * 2] += 4                                   # wave 0, third item: four k-groups more than its stream holds
    else:
        table[32 + 2 * (nitems - 1) + 1] = -1                    # wave 0's last feature item marked absent, its entries still there
        table[32 + 2 * (nitems - 1)] = 0
    with pytest.raises(AssertionError):
        two_tile_ring_walk(blob, table)


def test_packer_eligibility(nfa):
    from normflows_amd import nets
    from normflows_amd.flows import made_pack, maf_pack
    C = nfa.flows.CircularAutoregressiveRationalQuadraticSpline
    t = C(5, 2, 12, ind_circ=[1], num_bins=11, tail_bound=2.0).mprqat                 # mult 34 > 32
    assert pack(t) is None
    t = C(5, 2, 12, ind_circ=[1], num_bins=10, tail_bound=2.0).mprqat                 # mult 31
    assert pack(t) is not None
    # K = 11 with scalar linear tails: 32 rows fill the block (logits 1 .. 10 in slots 22 .. 31); K = 12: 35 rows
    t = nfa.flows.AutoregressiveRationalQuadraticSpline(5, 2, 12, num_bins=11, permute_mask=True).mprqat
    assert pack(t) is not None
    assert maf_pack.pack_made(t.autoregressive_net, mult=32, rows=True, features=(t.tails, t.tail_bound)) is not None
    t = nfa.flows.AutoregressiveRationalQuadraticSpline(5, 2, 12, num_bins=12, permute_mask=True).mprqat
    assert pack(t) is None
    tails = ["linear", "circular"] + ["linear"] * 3
    pre = nets.PeriodicFeaturesElementwise(5, [1], 1.0, activation=torch.nn.Tanh())
    made = nets.MADE(features=5, hidden_features=12, num_blocks=2, output_multiplier=13, preprocessing=pre)
    assert made_pack.pack_made_forward_ft(made, 13, 4, tails, 2.0) is None            # a non-Identity periodic activation
    made = nets.MADE(features=5, hidden_features=12, context_features=3, num_blocks=2, output_multiplier=13)
    assert made_pack.pack_made_forward_ft(made, 13, 4, None, 1.0) is None             # context
    made = nets.MADE(features=5, hidden_features=12, num_blocks=2, output_multiplier=13, use_batch_norm=True)
    assert made_pack.pack_made_forward_ft(made, 13, 4, None, 1.0) is None             # batch norm
    made = nets.MADE(features=5, hidden_features=12, num_blocks=2, output_multiplier=13, dropout_probability=0.1).train()
    assert made_pack.pack_made_forward_ft(made, 13, 4, None, 1.0) is None             # dropout in train mode
    made = nets.MADE(features=5, hidden_features=12, num_blocks=2, output_multiplier=13)
    assert made_pack.pack_made_forward_ft(made, 12, 4, None, 1.0) is None             # mult is not K's
    made = nets.MADE(features=129, hidden_features=140, num_blocks=2, output_multiplier=13)
    assert made_pack.pack_made_forward_ft(made, 13, 4, None, 1.0) is None             # D > 128
    # everything the sampling packer takes (tests/test_host_arnsf_ft.py, tests/test_gpu_arnsf_ft.py) is taken here
    torch.manual_seed(5)
    for t in (C(40, 2, 96, ind_circ=[0, 7, 21], num_bins=8, tail_bound=1.5 + torch.rand(40), permute_mask=True).mprqat,
              C(5, 2, 12, ind_circ=[0, 1, 2, 3, 4], num_bins=10, tail_bound=float(np.pi)).mprqat,
              C(3, 2, 2, ind_circ=[1], num_bins=1, tail_bound=2.0).mprqat,
              nfa.flows.AutoregressiveRationalQuadraticSpline(33, 2, 96, num_bins=8, tail_bound=2.5, permute_mask=True).mprqat,
              nfa.flows.AutoregressiveRationalQuadraticSpline(9, 2, 40, num_bins=4, tail_bound=2.5, permute_mask=True).mprqat):
        assert maf_pack.pack_made(t.autoregressive_net, mult=t._output_dim_multiplier(), rows=True,
                                  features=(t.tails, t.tail_bound)) is not None
        assert pack(t) is not None
    # and shapes the sampling schedule cannot plan: fewer hidden units than degrees
    t = C(8, 2, 4, ind_circ=[1, 3], num_bins=4, tail_bound=2.5).mprqat
    assert pack(t) is not None


def test_new_kernels_use_no_scratch(nfa):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    obj = os.path.join(ROOT, "normalizing-flows_amd", "lib", "obj", "made_fwd_ft.o")
    seen = 0
    for name, d in kr.resources(obj).items():
        if "made_fwd_ft_kernel" in name:
            seen += 1
            assert d["vgpr_spill_count"] == 0 and d["private_segment_fixed_size"] == 0, (name, d)
    assert seen == 2, seen
