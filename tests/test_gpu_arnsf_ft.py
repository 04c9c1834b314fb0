"""GPU tests (-m gpu) of the one-launch sampling direction of the circular / mask-permuted autoregressive spline layers
(nf_arnsf_inverse_ft, csrc/maf_inverse.hip maf_inverse_kernel<true, true>): against the reference's stored outputs
(tests/golden/circ_ar_perm_tb.npz), against the project's own D-pass loop, on inputs outside the intervals, outside the kernel's
limits (the loop stays) and as the graph-free forward of the implicit differentiation."""
import numpy as np
import pytest
import torch

from conftest import assert_close, golden_state, ld_tol, load_golden

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
    """Counts the launches of the per-feature kernel and the runs of the D-pass loop."""
    from normflows_amd.flows.autoregressive import Autoregressive
    calls = {"ft": 0, "loop": 0}
    ft, loop = nfa.ops.arnsf_inverse_ft, Autoregressive._inverse_loop

    def ft_(*a, **k):
        calls["ft"] += 1
        return ft(*a, **k)

    def loop_(self, *a, **k):
        calls["loop"] += 1
        return loop(self, *a, **k)
    monkeypatch.setattr(nfa.ops, "arnsf_inverse_ft", ft_)
    monkeypatch.setattr(Autoregressive, "_inverse_loop", loop_)
    return calls


def N(t):
    return t.detach().cpu().numpy()


def scale_weights(layer, by=1.5):
    with torch.no_grad():
        for p in layer.parameters():
            p.mul_(by)
    return layer


def bounds_of(t):
    tb = t.tail_bound
    return tb.detach().cpu() if torch.is_tensor(tb) else torch.full((t.features,), float(tb))


def inputs(t, B, seed, outside_rows=0):
    """Rows inside 0.98 of every interval; the first `outside_rows` rows get one LINEAR feature far outside its interval."""
    tb = bounds_of(t)
    z = (torch.rand(B, t.features, generator=torch.Generator().manual_seed(seed)) * 2 - 1) * tb * 0.98
    listed = isinstance(t.tails, (list, tuple))
    lin = [c for c in range(t.features) if not listed or t.tails[c] == "linear"]
    inside = np.ones(B, dtype=bool)
    for r in range(min(outside_rows, B if lin else 0)):
        z[r, lin[(3 * r + 1) % len(lin)]] = (50.0, -60.0)[r & 1]
        inside[r] = False
    return z.to(DEV), inside


def test_fixture_layer_vs_reference(nfa, spy):
    """The reference's CircularAutoregressiveRationalQuadraticSpline with a permuted mask, a tensor tail bound and two linear inputs
    outside their interval: sampling (one launch of the per-feature kernel, never the D-pass loop) and density direction."""
    g = load_golden("circ_ar_perm_tb")
    layer = nfa.flows.CircularAutoregressiveRationalQuadraticSpline(7, 2, 24, ind_circ=[0, 2, 5], num_bins=6,
                                                                    tail_bound=torch.from_numpy(g["sd__mprqat__tail_bound"]),
                                                                    permute_mask=True, init_identity=False)
    layer.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in golden_state(g).items()}, strict=True)
    layer = layer.to(DEV)
    x = torch.from_numpy(g["x"]).to(DEV)
    with torch.no_grad():
        z, ld = layer.forward(x)
        assert spy == {"ft": 1, "loop": 0}
        print("sampling: max|dx| %.3e  max|dld| %.3e" % (np.abs(N(z) - g["z_fwd"]).max(), np.abs(N(ld) - g["ld_fwd"]).max()))
        assert N(z)[0, 1] == 0.0 and N(z)[1, 3] == 0.0
        assert_close(N(z), g["z_fwd"], what="z_fwd", rtol=1e-4, atol=1e-4)
        assert_close(N(ld), g["ld_fwd"], what="ld_fwd", **ld_tol(np.float32, root_finding=True))
        z, ld = layer.inverse(x)
        assert_close(N(z), g["z_inv"], what="z_inv", rtol=1e-4, atol=1e-4)
        assert_close(N(ld), g["ld_inv"], what="ld_inv", **ld_tol(np.float32))


def build_case(nfa, case):
    """(transform, the parameter whose update must reach the pack) of one of the one-pass-vs-loop cases."""
    if case == "wide_circular":          # D 40, H 96, K 8: four tiles; circular = degree 1, the end of tile 0, the middle of tile 1
        from normflows_amd.flows import maf_pack
        D, H, K = 40, 96, 8

        def build(ind_circ, bound):
            torch.manual_seed(5)         # (the permutation is the constructor's first draw: the same for every ind_circ)
            return nfa.flows.CircularAutoregressiveRationalQuadraticSpline(D, 2, H, ind_circ=ind_circ, num_bins=K, tail_bound=bound,
                                                                           permute_mask=True, init_identity=False)
        probe = build([0], 3.0).mprqat
        mult = probe._output_dim_multiplier()
        deg = probe.autoregressive_net.final_layer.degrees.numpy()[::mult]
        col = np.argsort(deg, kind="stable")
        tiles = maf_pack.plan_tiles(D, probe.autoregressive_net.initial_layer.degrees.numpy())[1]
        assert len(tiles) == 4 and not np.array_equal(deg, np.arange(1, D + 1))
        ind_circ = sorted(int(col[f]) for f in (0, tiles[0][0] + tiles[0][1] - 1, tiles[1][0] + tiles[1][1] // 2))
        bound = 1.5 + 2.0 * torch.rand(D, generator=torch.Generator().manual_seed(6))
        bound[ind_circ] = float(np.pi)
        t = build(ind_circ, bound).mprqat
    elif case == "all_circular_k10":     # R = 3K + 1 = 31 rows per feature
        torch.manual_seed(15)
        t = nfa.flows.CircularAutoregressiveRationalQuadraticSpline(5, 2, 12, ind_circ=[0, 1, 2, 3, 4], num_bins=10,
                                                                    tail_bound=float(np.pi), init_identity=False).mprqat
    elif case == "smallest":             # D 3, two hidden units, one bin, one row
        torch.manual_seed(4)
        t = nfa.flows.CircularAutoregressiveRationalQuadraticSpline(3, 2, 2, ind_circ=[1], num_bins=1, tail_bound=2.0,
                                                                    init_identity=False).mprqat
    else:                                # linear tails (3K - 1 rows per feature, identity outside) on a permuted mask
        torch.manual_seed(41)
        t = nfa.flows.AutoregressiveRationalQuadraticSpline(33, 2, 96, num_bins=8, tail_bound=2.5, permute_mask=True,
                                                            init_identity=False).mprqat
        assert t._permuted()
    t = scale_weights(t).to(DEV)
    pre = t.autoregressive_net.preprocessing
    return t, (pre.weights if hasattr(pre, "weights") else t.autoregressive_net.final_layer.bias)


@pytest.mark.parametrize("case,B", [("wide_circular", 130), ("all_circular_k10", 64), ("smallest", 1), ("permuted_linear", 65)])
def test_one_launch_matches_d_pass_loop(nfa, spy, case, B):
    """nf_arnsf_inverse_ft against the project's D-pass loop (bars of test_arnsf_incremental_inverse_matches_d_pass), the density
    direction as its inverse on the rows inside every interval, the accumulate protocol and the re-pack after a parameter update."""
    from normflows_amd.flows.autoregressive import Autoregressive
    t, updated = build_case(nfa, case)
    K = t.num_bins
    z, inside = inputs(t, B, 7, outside_rows=4 if B > 8 else 0)
    with torch.no_grad():
        x, ld = t.inverse(z)
        assert spy == {"ft": 1, "loop": 0}
        xr, ldr = Autoregressive.inverse(t, z)
        assert spy == {"ft": 1, "loop": 1}
        print("%s: max|dx| %.3e  max|dld| %.3e" % (case, float((x - xr).abs().max()), float((ld - ldr).abs().max())))
        assert_close(N(x), N(xr), what="x", rtol=1e-4, atol=2e-4)
        assert_close(N(ld), N(ldr), what="ld", rtol=1e-4, atol=1e-3)
        zb, ldb = t.forward(x)
        print("%s: round trip max|dz| %.3e  max|dld| %.3e" % (case, float((zb - z)[torch.from_numpy(inside)].abs().max()),
                                                              float((ldb + ld)[torch.from_numpy(inside)].abs().max())))
        assert_close(N(zb)[inside], N(z)[inside], what="roundtrip", rtol=1e-3, atol=1e-3)
        assert_close(N(ldb)[inside], -N(ld)[inside], what="roundtrip ld", rtol=1e-3, atol=1e-3)
        acc = torch.ones(B, device=DEV)
        pk = t._packed_ft(DEV)
        nfa.ops.arnsf_inverse_ft(z, pk[0], pk[1], pk[2], pk[3], K, "feature" if isinstance(t.tails, list) else t.tails,
                                 logdet=acc, acc=nfa.ops.L.LD_SUB)
        assert_close(N(acc), 1.0 - N(ld), what="acc", rtol=1e-5, atol=1e-5)
        updated.add_(0.1)
        x2, ld2 = t.inverse(z)
        x2r, ld2r = Autoregressive.inverse(t, z)
        assert_close(N(x2), N(x2r), what="x after update", rtol=1e-4, atol=2e-4)
        assert_close(N(ld2), N(ld2r), what="ld after update", rtol=1e-4, atol=1e-3)
        assert B == 1 or not np.allclose(N(x2), N(x))     # (a single row of the two-unit network may sit on dead ReLUs)


def test_inputs_outside_the_interval(nfa, spy):
    """A linear feature of a list-tails layer fed +-50: 0 in that column, nothing in the log-det, whatever the value; every later
    feature is conditioned on that 0 as in the loop."""
    from normflows_amd.flows.autoregressive import Autoregressive
    t, _ = build_case(nfa, "wide_circular")
    lin = [c for c in range(t.features) if t.tails[c] == "linear"]
    z, _ = inputs(t, 70, 11)
    za, zb = z.clone(), z.clone()
    cols = [lin[2], lin[9], lin[20]]
    for r, c in enumerate(cols):
        za[r, c], zb[r, c] = 50.0, -50.0
        za[64 + r, c], zb[64 + r, c] = -50.0, 77.0
    with torch.no_grad():
        xa, lda = t.inverse(za)
        xb, ldb = t.inverse(zb)
        xr, ldr = Autoregressive.inverse(t, za)
    assert spy == {"ft": 2, "loop": 1}
    for r, c in enumerate(cols):
        assert float(xa[r, c]) == 0.0 and float(xa[64 + r, c]) == 0.0
    assert torch.equal(xa, xb) and torch.equal(lda, ldb)
    assert_close(N(xa), N(xr), what="x", rtol=1e-4, atol=2e-4)
    assert_close(N(lda), N(ldr), what="ld", rtol=1e-4, atol=1e-3)


@pytest.mark.parametrize("D,H,K", [(5, 12, 11), (8, 4, 4)])
def test_outside_the_kernel_limits_the_loop_stays(nfa, spy, D, H, K):
    """3K + 1 > 32 rows per feature (K = 11 with list tails) and fewer hidden units than degrees: silently the D-pass loop."""
    from normflows_amd.flows.autoregressive import Autoregressive
    torch.manual_seed(D + K)
    t = scale_weights(nfa.flows.CircularAutoregressiveRationalQuadraticSpline(D, 2, H, ind_circ=[1, 3], num_bins=K, tail_bound=2.5,
                                                                              init_identity=False).mprqat).to(DEV)
    z, _ = inputs(t, 33, 3, outside_rows=2)
    with torch.no_grad():
        x, ld = t.inverse(z)
        assert spy == {"ft": 0, "loop": 1}
        xr, ldr = Autoregressive.inverse(t, z)
    assert_close(N(x), N(xr), what="x", rtol=1e-4, atol=2e-4)
    assert_close(N(ld), N(ldr), what="ld", rtol=1e-4, atol=1e-3)


def test_sampling_under_autograd_takes_the_one_launch_forward(nfa, spy, monkeypatch):
    """autograd.ArInverseImplicitFn on a circular layer (D 6, hidden 32): its graph-free forward is the per-feature kernel; the
    backward is unchanged, so the gradients equal those of the same function on the D-pass forward to 1e-5 of scale -- the kernel's
    x is as good a solution for the implicit differentiation as the loop's."""
    D, H, B = 6, 32, 200
    torch.manual_seed(6 * 7 + 32)
    layer = nfa.flows.CircularAutoregressiveRationalQuadraticSpline(D, 2, H, [1, 3],
                                                                    tail_bound=torch.tensor([5.0, 3.14159, 4.0, 3.14159, 5.0, 5.0]))
    gen = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for p in layer.parameters():
            p.add_(0.05 * torch.randn(p.shape, generator=gen))
    layer = layer.to(DEV)
    z0 = torch.randn(B, D, generator=torch.Generator().manual_seed(1)).clamp(-3.0, 3.0).to(DEV)
    cx, cl = torch.randn(B, D, device=DEV), torch.randn(B, device=DEV)
    res = []
    for routed in (True, False):
        if not routed:
            monkeypatch.setattr(type(layer.mprqat), "_packed_ft", lambda self, device: None)
        before = dict(spy)
        layer.zero_grad(set_to_none=True)
        with torch.enable_grad():
            z = z0.clone().requires_grad_(True)
            x, ld = layer.forward(z)
            ((x * cx).sum() + (ld * cl).sum()).backward()
        assert (spy["ft"] - before["ft"], spy["loop"] - before["loop"]) == ((1, 0) if routed else (0, 1))
        res.append([x.detach(), ld.detach(), z.grad] + [p.grad.clone() for p in layer.parameters()])
    for k, (a, b) in enumerate(zip(res[0], res[1])):
        err, scale = float((a - b).abs().max()), max(1.0, float(b.abs().max()))
        print("tensor %d: max|d| %.3e of scale %.3e" % (k, err, scale))
    for k, (a, b) in enumerate(zip(res[0], res[1])):
        if k >= 2:
            assert float((a - b).abs().max()) <= 1e-5 * max(1.0, float(b.abs().max())), k
