"""GPU tests (-m gpu) of the SECOND tile of every persistent tile-engine kernel.

Every tile-engine launcher sets grid = min(tiles, nf_persistent_workgroups()) and the kernel walks `for (tile = blockIdx.x; tile <
ntiles; tile += gridDim.x)`: a workgroup starts a second tile only when the batch exceeds 256 x tile rows.  Only there does it matter
that the register weight ring (csrc/mlp_tile.hpp MfRing) is NOT reloaded between tiles -- `ring.ap` is reset and the eight entries in
flight must be the packer's wrap copy of stream entries 0..7, which they are only if the kernel consumed exactly what the packer wrote
--, that the LDS regions are reused behind the trailing barrier alone, and that the loop-invariant pins act on the loop's back edge.

Inventory, re-derived from the launchers and the suite (batches in rows; "before" = the largest batch a GPU test ran before this module):

| entry point (file)                                              | tile rows | first batch with a second tile | before | here   |
|-----------------------------------------------------------------|-----------|--------------------------------|--------|--------|
| nf_made_forward_spline_ft (made_fwd_ft.hip)                     | 64        | 16 385                         | 130    | 16 449 |
| nf_nsf_wide_ft (nsf_circ.hip)                                   | 128 (Hp 128) / 64 (Hp 256) | 32 769 / 16 385 | 130    | 32 897 / 16 449 |
| nf_made_forward_train_ft (made_fwd_train_ft.hip), 256 slots     | 64        | 16 385                         | 16 512 (two workgroups) | 49 280 |
| nf_made_forward_train_ft, 512 slots                             | 64        | 16 385                         | 130    | 16 449 |
| ResNetFtFn route (nf_made_forward_train_ft / nf_made_backward_t64 / nf_made_feed_ft_bwd / nf_made_wgrad on a dense pack) | 64 | 16 385 | 130 | 16 449 |
| nf_made_forward_spline (made_fwd.hip, linear-tails AR-NSF)      | 64        | 16 385                         | 300 (layers inside models: ~1 000) | 16 449 |
| nf_nsf_wide_k, 4 and 16 bins (nsf_wide.hip)                     | 64 / 128  | 16 385 / 32 769                | 1 030 (65 536: 8 bins only) | 16 449 |
| nf_made_forward_train / nf_made_backward / nf_made_wgrad, spline rows (mult 23) | 64 | 16 385             | 70 (65 536: mult 2 only) | 16 449 |
| the same kernels on 128-row tiles (mf_tr128)                    | 128       | 49 280 (smallest multiple of 128 with mf_tr128 true beyond 256 tiles: r128 = 2, r64 = 4, 15 * 2 < 8 * 4) | 32 768 (one round) | 49 280 |

Covered before and not repeated here: nf_nsf_wide_ctx (65 536 / 65 537), nf_resnet_ctx_* (65 537), nf_rqs_coupling_bwd_ft_wave's
multi-pass cases, the fused benchmark chain and the MAF inverse at 65 536; nf_arnsf_inverse[_ft] has no grid cap.

Batches: B = 256 TR + TR + 1 (16 449 on 64-row tiles, 32 897 on 128-row tiles): workgroup 0 walks two full tiles, workgroup 1 a full
tile and then a ragged one-row tile, every other workgroup one tile; both are odd, so the training kernels stay on 64-row tiles.
B = 49 280 for mf_tr128.  The cap comes from nf_persistent_workgroups(), the tile rows from the pack's header (wide engines) or
nf_made_tile_rows (MADE engines).

Every case asserts: the one-launch route ran (spies) and B > cap x TR; two calls give identical bits; rows [256 TR, B) equal, bit for
bit, fresh calls on those rows alone (where they sit in FIRST-iteration tiles at the same tile positions) and rows [0, TR) a fresh
call on x[:TR]; rows [0, TR) and [256 TR, B) against a float64 deep copy of the layer on the layer-wise path at the bars of the
engine's small-batch parity test; under autograd every parameter gradient against float64 autograd of the eager modules over the whole
batch, the reference's own error taken from the eager float32 route on the same rows.  Weights and inputs come from the sibling
modules' builders (inputs within 0.98 x bound, two far-outside entries on linear features in the last two tiles)."""
import copy

import numpy as np
import pytest
import torch

import circ_wide_cases as cw
from conftest import assert_close, ld_tol
from test_gpu_made_fwd_ft import bounds_of, build_case, inputs, ld_bar, scale_weights
from test_gpu_circ_coupled_train import full_bound
from test_gpu_views import same

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def nfa():
    import normflows_amd
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    assert normflows_amd.native_library_path().endswith("normalizing-flows_amd/lib/libnf_mi355x.so")
    normflows_amd._lib.lib()
    return normflows_amd


@pytest.fixture
def spy(nfa, monkeypatch):
    """spy(*names): wraps nfa.ops.<name>; returns {name: calls} with the last return value of each under ("out", name)."""
    def install(*names):
        calls = {k: 0 for k in names}

        def wrap(real, key):
            def f(*a, **k):
                calls[key] += 1
                calls["out", key] = real(*a, **k)
                return calls["out", key]
            return f
        for k in names:
            monkeypatch.setattr(nfa.ops, k, wrap(getattr(nfa.ops, k), k))
        return calls
    return install


def N(t):
    return t.detach().cpu().numpy()


def cap(nfa):
    return nfa._lib.query("nf_persistent_workgroups")


def made_rows(nfa, B, D, hp):
    return nfa._lib.query("nf_made_tile_rows", B, D, hp)


def second_tile_batch(nfa, TR):
    """The smallest batch at which the persistent loop can go wrong: two full tiles for workgroup 0, a full and a one-row tile for 1."""
    return cap(nfa) * TR + TR + 1


def windows(nfa, TR, B):
    """[0, TR) and [cap TR, B) in pieces of at most cap TR rows: each a batch whose tiles are all first-iteration tiles."""
    r0 = cap(nfa) * TR
    assert B > r0, (B, r0)
    return [(0, TR)] + [(s, min(s + r0, B)) for s in range(r0, B, r0)]


def reference_rows(nfa, TR, B):
    r0 = cap(nfa) * TR
    return torch.cat([torch.arange(0, TR), torch.arange(r0, min(B, r0 + TR + 1))]).to(DEV)


def uniform_inputs(bound, B, seed, outside=()):
    """Uniform within 0.98 x bound (D,); `outside` = two linear columns: 50 in the last row (the ragged tile), -60 in the row before."""
    x = (torch.rand(B, bound.numel(), generator=torch.Generator().manual_seed(seed)) * 2 - 1) * bound * 0.98
    if outside:
        x[B - 1, outside[0]], x[B - 2, outside[1]] = 50.0, -60.0
    return x.to(DEV)


class switched_off:
    """The route's config switches off for the float64 / eager float32 reference."""

    def __init__(self, nfa, *names):
        self.cfg, self.names = nfa.config, names

    def __enter__(self):
        for n in self.names:
            getattr(self.cfg, "set_" + n)(False)

    def __exit__(self, *exc):
        for n in self.names:
            getattr(self.cfg, "set_" + n)(True)
        return False


def check_inference(nfa, what, call, call64, x, TR, calls, op, ld_kw):
    """call(x) -> (y, ld) on the one-launch route, call64(x64) -> the float64 layer-wise reference."""
    B = x.shape[0]
    assert B == second_tile_batch(nfa, TR), (B, TR)
    with torch.no_grad():
        y, ld = call(x)
        assert calls[op] == 1, calls
        y2, ld2 = call(x)
        assert same(y, y2) and same(ld, ld2), what + ": two calls differ"
        for lo, hi in windows(nfa, TR, B):
            ys, ls = call(x[lo:hi].contiguous())
            assert same(y[lo:hi], ys) and same(ld[lo:hi], ls), "%s: rows [%d, %d) differ from a fresh call on them" % (what, lo, hi)
        n = calls[op]
        rows = reference_rows(nfa, TR, B)
        y64, ld64 = call64(x[rows].double())
        assert calls[op] == n and y64.dtype == torch.float64
    dy, dl = (y[rows].double() - y64).abs(), (ld[rows].double() - ld64).abs()
    print("%s: %d rows vs float64: max|dy| %.3e (first tile %.3e, second-iteration tiles %.3e)  max|dld| %.3e (%.3e, %.3e)" % (
        what, len(rows), float(dy.max()), float(dy[:TR].max()), float(dy[TR:].max()), float(dl.max()), float(dl[:TR].max()),
        float(dl[TR:].max())))
    assert_close(N(y[rows]), N(y64).astype(np.float32), what=what + " y vs float64", rtol=1e-4, atol=1e-4)
    assert_close(N(ld[rows]), N(ld64).astype(np.float32), what=what + " ld vs float64", **ld_kw)
    return y, ld


# ---- 1. nf_made_forward_spline_ft ---------------------------------------------------------------------------------------------------
def ft_linear_columns(t):
    """(first, last) linear column of the transform, () when it has fewer than two."""
    if isinstance(t.tails, list):
        lin = [c for c, kind in enumerate(t.tails) if kind == "linear"]
    else:
        lin = list(range(t.features)) if t.tails == "linear" else []
    return (lin[0], lin[-1]) if len(lin) >= 2 else ()


@pytest.mark.parametrize("case", ["d33_h24_k6", "d128_h300_k10", "scalar_linear_permuted"])
def test_made_forward_spline_ft_second_tile(nfa, spy, case):
    """256 slots with a tensor bound, 512 slots (items over both sample blocks, mult 31) and scalar linear tails on a permuted mask
    at 16 449 rows; float64: the layer's deep copy with config.arnsf_density_ft off; log-det bar ld_bar(D) of
    tests/test_gpu_made_fwd_ft.py."""
    t = build_case(nfa, case)
    pk = t._packed_fwd_ft(torch.device(DEV))
    TR = made_rows(nfa, 0, t.features, pk[3])
    x = uniform_inputs(bounds_of(t), second_tile_batch(nfa, TR), 7, ft_linear_columns(t))
    calls = spy("made_forward_spline_ft")
    t64 = copy.deepcopy(t).double()

    def call64(x64):
        with switched_off(nfa, "arnsf_density_ft"):
            return t64.forward(x64)
    y, _ = check_inference(nfa, case, t.forward, call64, x, TR, calls, "made_forward_spline_ft", ld_bar(t.features))
    out = ft_linear_columns(t)
    if out:                                      # list tails: 0 outside, scalar linear tails: the identity
        want = (0.0, 0.0) if isinstance(t.tails, list) else (50.0, -60.0)
        assert (float(y[-1, out[0]]), float(y[-2, out[1]])) == want


def test_a_wrap_copy_of_zeros_changes_exactly_the_second_iteration_rows(nfa, spy, monkeypatch):
    """Sensitivity: with the packer's wrap copy replaced by zeros of the same length (in bounds, finite, no kernel change) the ring holds
    zeros for stream entries 0..7 of every tile after a workgroup's first.  Rows below 256 TR keep their bits, every row from 256 TR on
    differs -- the one difference the small-batch tests of tests/test_gpu_made_fwd_ft.py cannot see."""
    from normflows_amd.flows import made_pack
    t_ok, t_bad = build_case(nfa, "d33_h24_k6"), build_case(nfa, "d33_h24_k6")      # (seeded by the case's name: the same weights)
    real = made_pack.pack_made_forward_ft

    def zero_wrap(*a, **k):
        packed = real(*a, **k)
        blob, table = packed[0].copy(), packed[1]
        ends = [int(table[16 + w]) for w in range(1, 8)] + [int(table[9])]
        for e in ends:
            blob[e - made_pack.RING * 256:e] = 0.0
        return (blob,) + tuple(packed[1:])
    TR = made_rows(nfa, 0, 33, 256)
    r0 = cap(nfa) * TR
    x = uniform_inputs(bounds_of(t_ok), second_tile_batch(nfa, TR), 7)
    calls = spy("made_forward_spline_ft")
    with torch.no_grad():
        y, ld = t_ok.forward(x)
        monkeypatch.setattr(made_pack, "pack_made_forward_ft", zero_wrap)
        ym, ldm = t_bad.forward(x)
    assert calls["made_forward_spline_ft"] == 2
    assert bool(torch.isfinite(ym).all()) and bool(torch.isfinite(ldm).all())
    assert torch.equal(y[:r0], ym[:r0]) and torch.equal(ld[:r0], ldm[:r0])
    assert bool((y[r0:] != ym[r0:]).any(1).all()) and bool((ld[r0:] != ldm[r0:]).all())


# ---- 2. nf_nsf_wide_ft ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a", "c", "f", "g"])
@pytest.mark.parametrize("direction", [0, 1])
def test_nsf_wide_ft_second_tile(nfa, spy, name, direction):
    """Layers a (Hp 128: 128-row tiles, 32 897 rows), c (Hp 256: 64-row tiles, 16 449 rows), f and g (4 and 16 bins: 8 / 2 transform
    features per final group) in both directions; float64: the layer's deep copy with config.nsf_circular off; log-det bar
    conftest.ld_tol, with the root-finding allowance in the sampling direction."""
    layer = cw.layer(nfa, name).to(DEV)
    p = layer.prqct
    D = cw.LAYERS[name][0]
    TR = int(p._circ_pack(torch.zeros(1, D, device=DEV), None)[1][14])
    assert TR == (128 if cw.LAYERS[name][2] <= 128 else 64)
    lin = [c for c in range(D) if c not in cw.LAYERS[name][3]]
    x = uniform_inputs(full_bound(layer, D), second_tile_batch(nfa, TR), 11, (lin[0], lin[-1]))
    calls = spy("nsf_wide_ft")
    l64 = copy.deepcopy(layer).double()

    def call64(x64):
        with switched_off(nfa, "nsf_circular"):
            return l64.forward(x64) if direction == 1 else l64.inverse(x64)
    call = layer.forward if direction == 1 else layer.inverse
    y, _ = check_inference(nfa, "%s dir %d" % (name, direction), call, call64, x, TR, calls, "nsf_wide_ft",
                           ld_tol(np.float32, root_finding=direction == 1))
    assert float(y[-1, lin[0]]) == 0.0 and float(y[-2, lin[-1]]) == 0.0


# ---- 3. nf_made_forward_spline -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,H", [(33, 96), (128, 512)])
def test_made_forward_spline_second_tile(nfa, spy, D, H):
    """The linear-tails AR-NSF density direction, 256 and 512 slots, weights as test_made_forward_spline_one_launch_vs_layerwise builds
    them; float64: the layer's deep copy with config.made_fused off; log-det bar ld_bar(D) (a sum of D terms)."""
    from test_gpu_parity import _perturb
    torch.manual_seed(D * 11 + H)
    layer = nfa.flows.AutoregressiveRationalQuadraticSpline(D, 2, H, num_bins=8, tail_bound=3, init_identity=False)
    _perturb(layer, 0.2 if D < 40 else 0.05, 9)
    layer = layer.to(DEV)
    t = layer.mprqat
    packed = t.autoregressive_net.packed_forward(DEV, spline=True)
    assert packed is not None
    TR = made_rows(nfa, 0, D, packed[2])
    x = uniform_inputs(torch.full((D,), 3.0), second_tile_batch(nfa, TR), D, (0, D - 1))
    calls = spy("made_forward_spline")
    l64 = copy.deepcopy(layer).double()

    def call64(x64):
        with switched_off(nfa, "made_fused"):
            return l64.inverse(x64)
    y, _ = check_inference(nfa, "d%d_h%d" % (D, H), layer.inverse, call64, x, TR, calls, "made_forward_spline", ld_bar(D))
    assert float(y[-1, 0]) == 50.0 and float(y[-2, D - 1]) == -60.0


# ---- 4. nf_nsf_wide_k ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [4, 16])
@pytest.mark.parametrize("direction", [0, 1])
def test_nsf_wide_k_second_tile(nfa, spy, K, direction):
    """D 64 / hidden 256 with 4 and 16 bins (8 / 2 transform features per final-layer group), weights as
    test_nsf_wide_one_launch_vs_layerwise_and_oracle builds them; float64: the layer's deep copy with config.nsf_wide off; log-det bar
    conftest.ld_tol, with the root-finding allowance in the sampling direction."""
    D, H = 64, 256
    torch.manual_seed(D * 7 + H)
    layer = nfa.flows.CoupledRationalQuadraticSpline(D, 2, H, num_bins=K, init_identity=False)
    with torch.no_grad():
        for p_ in layer.parameters():
            p_.add_(0.04 * torch.randn_like(p_))
        u = layer.prqct.unconditional_transform
        u.unnormalized_widths.normal_()
        u.unnormalized_heights.normal_()
        u.unnormalized_derivatives.normal_()
    layer = layer.to(DEV)
    wide = layer.prqct._wide_pack(torch.zeros(1, D, device=DEV), None)
    assert wide is not None
    TR = int(wide[1][14])
    x = uniform_inputs(torch.full((D,), 3.0), second_tile_batch(nfa, TR), 3, (0, D - 1))
    calls = spy("nsf_wide")
    l64 = copy.deepcopy(layer).double()

    def call64(x64):
        with switched_off(nfa, "nsf_wide"):
            return l64.forward(x64) if direction == 1 else l64.inverse(x64)
    call = layer.forward if direction == 1 else layer.inverse
    y, _ = check_inference(nfa, "K %d dir %d" % (K, direction), call, call64, x, TR, calls, "nsf_wide",
                           ld_tol(np.float32, root_finding=direction == 1))
    assert float(y[-1, 0]) == 50.0 and float(y[-2, D - 1]) == -60.0


# ---- 5 - 7. the training routes ------------------------------------------------------------------------------------------------------
def train_step(fn, params, x, cz, cl):
    """[z, ld, gx, every parameter gradient] of loss = sum(z cz) + sum(ld cl) through fn."""
    for p in params:
        p.grad = None
    xx = x.clone().requires_grad_(True)
    z, ld = fn(xx)
    ((z * cz).sum() + (ld * cl).sum()).backward()
    return [z.detach(), ld.detach(), xx.grad] + [torch.zeros_like(p) if p.grad is None else p.grad.clone() for p in params]


def check_training(nfa, what, module, fn_of, x, cz, cl, TR, calls, fwd_op, route, off, D, atomics=()):
    """fn_of(module) -> the differentiable call; route = {op: launches per step}; off = the switches of the eager route; fwd_op = the
    op whose first output holds the conditioner's parameter rows; atomics = parameters whose gradient the route sums with float32
    atomics by design (no run-to-run bit equality is promised for them)."""
    B = x.shape[0]
    assert B > cap(nfa) * TR
    names = ["gx"] + [k for k, _ in module.named_parameters()]
    params = list(module.parameters())
    fn = fn_of(module)
    got = train_step(fn, params, x, cz, cl)
    assert {k: calls[k] for k in route} == route, calls
    calls["first", fwd_op] = calls["out", fwd_op]          # (what the whole-batch forward returned: parameter rows, save, bits, ...)
    rows_all = calls["first", fwd_op][0]
    again = train_step(fn, params, x, cz, cl)
    for k, a, b in zip(["z", "ld"] + names, got, again):
        assert same(a, b) or any(k.startswith(p) for p in atomics), "%s: %s differs between two steps" % (what, k)
    for lo, hi in windows(nfa, TR, B):
        sub = train_step(fn, params, x[lo:hi].contiguous(), cz[lo:hi].contiguous(), cl[lo:hi].contiguous())
        for k, a, b in zip(("z", "ld", "gx"), got[:3], sub[:3]):
            assert same(a[lo:hi], b), "%s: %s rows [%d, %d) differ from a fresh step on them" % (what, k, lo, hi)
        assert same(rows_all[lo:hi], calls["out", fwd_op][0]), "%s: parameter rows [%d, %d)" % (what, lo, hi)
    n = {k: calls[k] for k in route}
    m64 = copy.deepcopy(module).double()
    with switched_off(nfa, *off):
        ref = train_step(fn_of(m64), list(m64.parameters()), x.double(), cz.double(), cl.double())
        own = train_step(fn, params, x, cz, cl)
    assert {k: calls[k] for k in route} == n, "the reference took the route under test"
    rows = reference_rows(nfa, TR, B)
    dz, dl = (got[0][rows].double() - ref[0][rows]).abs(), (got[1][rows].double() - ref[1][rows]).abs()
    print("%s: %d rows vs float64: max|dz| %.3e (second-iteration tiles %.3e) max|dld| %.3e (%.3e); eager float32: %.3e %.3e" % (
        what, len(rows), float(dz.max()), float(dz[TR:].max()), float(dl.max()), float(dl[TR:].max()),
        float((own[0][rows].double() - ref[0][rows]).abs().max()), float((own[1][rows].double() - ref[1][rows]).abs().max())))
    assert_close(N(got[0][rows]), N(ref[0][rows]).astype(np.float32), what=what + " z vs float64", rtol=1e-4, atol=1e-4)
    assert_close(N(got[1][rows]), N(ref[1][rows]).astype(np.float32), what=what + " ld vs float64", **ld_bar(D))

    def err(a, r):
        return float((a.double() - r).abs().max()) / max(1.0, float(r.abs().max()))
    e_got, e_own = [err(got[2][rows], ref[2][rows])], [err(own[2][rows], ref[2][rows])]
    for k, a, o, r in zip(names[1:], got[3:], own[3:], ref[3:]):
        if r.numel():
            e_got.append(err(a, r))
            e_own.append(err(o, r))
    worst = int(np.argmax(e_got))
    print("%s: gradients vs float64 autograd over %d rows: worst %.3e of scale (%s; eager float32 %.3e), q90 %.3e, eager float32 q90 %.3e"
          % (what, B, e_got[worst], names[worst], e_own[worst], np.quantile(e_got, 0.9), np.quantile(e_own, 0.9)))
    assert max(e_got) < 1e-3, (names[worst], e_got[worst])
    assert np.quantile(e_got, 0.9) <= 4 * max(np.quantile(e_own, 0.9), 1e-7), (np.quantile(e_got, 0.9), np.quantile(e_own, 0.9))
    return got


FT_ROUTE = {"made_forward_train_ft": 1, "made_feed_ft_bwd": 1, "made_backward": 1, "made_wgrad": 1}


def cotangents(B, D, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(B, D, generator=gen).to(DEV), torch.randn(B, generator=gen).to(DEV)


def test_made_ft_training_512_slots_second_tile(nfa, spy):
    """MadeFtFn, forward + backward of one layer: D 33 / hidden 300 (512 slots), circular + permuted, weights x 1.5 as
    tests/test_gpu_arnsf_train_ft.py's shapes, 16 449 rows.  Gradient bars of test_fixtures_vs_reference_autograd: 1e-3 of scale, q90
    within 4 x the eager float32 route's own error against float64 (floor 1e-7)."""
    torch.manual_seed(33300)
    t = nfa.flows.CircularAutoregressiveRationalQuadraticSpline(33, 2, 300, ind_circ=[0, 7, 32], num_bins=8, tail_bound=3.0,
                                                                permute_mask=True, init_identity=False).mprqat
    t = scale_weights(t).to(DEV)
    TR = made_rows(nfa, 0, 33, 512)
    B = second_tile_batch(nfa, TR)
    x = uniform_inputs(bounds_of(t), B, 9, (1, 31))
    cz, cl = cotangents(B, 33, 4)
    calls = spy(*FT_ROUTE)
    got = check_training(nfa, "MadeFtFn d33 h300", t, lambda m: m.forward, x, cz, cl, TR, calls, "made_forward_train_ft", FT_ROUTE,
                         ("arnsf_train_ft", "made_train"), 33)
    assert float(got[0][-1, 1]) == 0.0 and float(got[0][-2, 31]) == 0.0


def test_made_ft_training_at_the_tr128_batch(nfa, spy):
    """MadeFtFn on the D 24 / hidden 40 shape of test_batch_where_the_other_made_kernels_take_128_row_tiles at B = 49 280, where
    mf_tr128 is true for nf_made_forward_train with more than 256 tiles of 128 rows: this route still runs 64-row tiles (the ReLU-sign
    words of both sample blocks' registers stay in the low 16 bits: one sample block per item), 770 of them, four per workgroup."""
    torch.manual_seed(24)
    t = nfa.flows.CircularAutoregressiveRationalQuadraticSpline(24, 2, 40, ind_circ=[2, 9, 13, 23], num_bins=8, tail_bound=3.0,
                                                                permute_mask=True, init_identity=False).mprqat
    t = scale_weights(t).to(DEV)
    B = 49280
    assert made_rows(nfa, B, 24, 256) == 128 and made_rows(nfa, 0, 24, 256) == 64
    x = inputs(t, B, 9)
    cz, cl = cotangents(B, 24, 4)
    calls = spy(*FT_ROUTE)
    check_training(nfa, "MadeFtFn d24 h40", t, lambda m: m.forward, x, cz, cl, made_rows(nfa, 0, 24, 256), calls, "made_forward_train_ft", FT_ROUTE,
                   ("arnsf_train_ft", "made_train"), 24)
    bits = calls["first", "made_forward_train_ft"][2]
    assert int((bits >> 16).abs().max()) == 0            # (64-row tiles: NS = 1, bit 16 s + r with s = 0 only)


@pytest.mark.parametrize("d", ["inv", "fwd"])
def test_resnet_ft_training_second_tile(nfa, spy, d):
    """ResNetFtFn: CircularCoupledRationalQuadraticSpline(64, 2, 256, 8 bins) under autograd in both directions at 16 449 rows, the
    layer's own initialisation (init_identity = False); the eager route = config.nsf_circular_train off."""
    torch.manual_seed(64256)
    layer = nfa.flows.CircularCoupledRationalQuadraticSpline(64, 2, 256, ind_circ=list(range(0, 64, 3)), num_bins=8, tail_bound=3.0,
                                                             init_identity=False).to(DEV)
    TR = made_rows(nfa, 0, 32, 256)
    B = second_tile_batch(nfa, TR)
    x = uniform_inputs(full_bound(layer, 64), B, 7, (1, 62))
    cz, cl = cotangents(B, 64, 5)
    route = dict(FT_ROUTE, rqs_coupling_bwd_ft_wave=1)
    calls = spy(*route)
    got = check_training(nfa, "ResNetFtFn " + d, layer, lambda m: (m.inverse if d == "inv" else m.forward), x, cz, cl, TR, calls,
                         "made_forward_train_ft", route, ("nsf_circular_train",), 64,
                         atomics=("prqct.unconditional_transform.",))      # (ops.rqs_coupling_bwd_ft_wave: the batch-shared spline's)
    assert float(got[0][-1, 1]) == 0.0 and float(got[0][-2, 62]) == 0.0


MADE_ROUTE = {"made_forward_train": 1, "made_backward": 1, "made_wgrad": 1}


def arnsf_d32(nfa, sigma=0.05):
    """AutoregressiveRationalQuadraticSpline(32, 2, 64, 8 bins) built as test_autoregressive_layers_training_vs_reference_autograd
    builds the layer of tests/golden/grad_arnsf_d32_h64.npz, perturbed by `sigma` (test_gpu_parity._perturb's milder setting)."""
    torch.manual_seed(2032)
    layer = nfa.flows.AutoregressiveRationalQuadraticSpline(32, 2, 64, num_bins=8, tail_bound=3, init_identity=False)
    gen = torch.Generator().manual_seed(8)
    with torch.no_grad():
        for p in layer.parameters():
            p.add_(sigma * torch.randn(p.shape, generator=gen, dtype=p.dtype))
    return layer.to(DEV)


@pytest.mark.parametrize("B", [16449, 49280])
def test_made_training_spline_rows_second_tile(nfa, spy, B):
    """MadeFn with the linear-tails AR-NSF layer (D 32 / hidden 64 / K 8: 23 parameter rows per feature) in the density direction: at
    16 449 rows on 64-row tiles, at 49 280 rows on 128-row tiles (mf_tr128; the ReLU-sign words then carry the second sample block's
    registers in their high 16 bits), 385 of them.
    The weights are perturbed by 0.05, not by the 0.2 of the 70-row fixture: at 0.2 four or five rows in 16 449 sit in bins steep
    enough for |gx| ~ 1e4, they dominate every parameter gradient, and the EAGER float32 route is itself 1.1e-2 (16 449 rows) / 6.4e-2
    (49 280 rows) of scale from float64 autograd on them (the kernels 7.7e-2 / 2.8e-2, on the same first-round rows, none within 100
    ulps of a knot): no float32 route can hold the 1e-3 bar there.  At 0.05 the eager route is 2.3e-5 / 1.9e-5 of scale from float64,
    well inside a third of the bar, so a route that holds it is right and one that does not is wrong."""
    layer = arnsf_d32(nfa)
    TR = made_rows(nfa, B, 32, 256)
    assert TR == (128 if B == 49280 else 64) and (B == 49280 or B == second_tile_batch(nfa, TR))
    x = uniform_inputs(torch.full((32,), 3.0), B, 8, (0, 31))
    cz, cl = cotangents(B, 32, 6)
    calls = spy(*MADE_ROUTE)
    got = check_training(nfa, "MadeFn B %d" % B, layer, lambda m: m.inverse, x, cz, cl, TR, calls, "made_forward_train", MADE_ROUTE,
                         ("made_train",), 32)
    assert float(got[0][-1, 0]) == 50.0 and float(got[0][-2, 31]) == -60.0
    bits = calls["first", "made_forward_train"][2]       # (Bp / 64 tile slots; 128-row tiles fill the first half of them)
    high = int((bits[:B // TR] >> 16).abs().max())
    assert (high != 0) == (TR == 128)
