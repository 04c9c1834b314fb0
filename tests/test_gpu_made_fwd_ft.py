"""GPU tests (-m gpu) of the one-launch density direction of the circular / mask-permuted autoregressive spline layers
(nf_made_forward_spline_ft, csrc/made_fwd_ft.hip): against the reference's stored outputs (tests/golden/circ_ar_perm_tb.npz,
ar_perm_lin.npz), against the project's own layer-wise path (config.arnsf_density_ft = False) on the same weights at the shapes where
the kernel takes another path, on inputs outside the intervals, outside the kernel's limits (the old path stays), and for
determinism and stray writes."""
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
    """Counts the launches of the per-feature density kernel, the eager MADE passes and the element-wise spline launches."""
    calls = {"ft": 0, "made": 0, "rqs": 0}
    ft, made, rqs = nfa.ops.made_forward_spline_ft, nfa.nets.MADE.forward, nfa.ops.rqs_coupling

    def ft_(*a, **k):
        calls["ft"] += 1
        return ft(*a, **k)

    def made_(self, *a, **k):
        calls["made"] += 1
        return made(self, *a, **k)

    def rqs_(*a, **k):
        calls["rqs"] += 1
        return rqs(*a, **k)
    monkeypatch.setattr(nfa.ops, "made_forward_spline_ft", ft_)
    monkeypatch.setattr(nfa.nets.MADE, "forward", made_)
    monkeypatch.setattr(nfa.ops, "rqs_coupling", rqs_)
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
    return tb.detach().cpu().reshape(-1).expand(t.features) if torch.is_tensor(tb) else torch.full((t.features,), float(tb))


def inputs(t, B, seed):
    return ((torch.rand(B, t.features, generator=torch.Generator().manual_seed(seed)) * 2 - 1) * bounds_of(t) * 0.98).to(DEV)


def layerwise(nfa, t, x):
    nfa.config.set_arnsf_density_ft(False)
    try:
        with torch.no_grad():
            return t.forward(x)
    finally:
        nfa.config.set_arnsf_density_ft(True)


def ld_bar(D):
    """log-det against the layer-wise path: a sum of D terms, each a log of O(1) quantities computed from conditioner outputs that
    differ by float32 rounding between the two product orders (~1e-6 on the scaled weights) through hardware exp / log (<= 2 ulp):
    4e-6 per feature on top of the per-layer bar of conftest.ld_tol."""
    tol = ld_tol(np.float32)
    return dict(rtol=tol["rtol"], atol=max(tol["atol"], 4e-6 * D))


@pytest.mark.parametrize("name", ["circ_ar_perm_tb", "ar_perm_lin"])
def test_fixture_layers_vs_reference(nfa, spy, name):
    """Both fixture layers through layer.inverse(x): the new op exactly once, neither the eager MADE nor nf_rqs_coupling; outputs and
    log-dets at the fixture bars of tests/test_gpu_arnsf_ft.py, the float64 leg showing the reference's own float32 error."""
    g = load_golden(name)
    if name == "circ_ar_perm_tb":
        layer = nfa.flows.CircularAutoregressiveRationalQuadraticSpline(7, 2, 24, ind_circ=[0, 2, 5], num_bins=6,
                                                                        tail_bound=torch.from_numpy(g["sd__mprqat__tail_bound"]),
                                                                        permute_mask=True, init_identity=False)
    else:
        layer = nfa.flows.AutoregressiveRationalQuadraticSpline(6, 2, 20, num_bins=4, tail_bound=2.5, permute_mask=True,
                                                                init_identity=False)
    layer.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in golden_state(g).items()}, strict=True)
    layer = layer.to(DEV)
    x = torch.from_numpy(g["x"]).to(DEV)
    with torch.no_grad():
        z, ld = layer.inverse(x)
    assert spy == {"ft": 1, "made": 0, "rqs": 0}
    print("%s: max|dz| %.3e max|dld| %.3e; the reference's float32 vs float64: %.3e %.3e" % (
        name, np.abs(N(z) - g["z_inv"]).max(), np.abs(N(ld) - g["ld_inv"]).max(),
        np.abs(g["z_inv"] - g["z_inv_f64"]).max(), np.abs(g["ld_inv"] - g["ld_inv_f64"]).max()))
    assert_close(N(z), g["z_inv"], what="z_inv", rtol=1e-4, atol=1e-4)
    assert_close(N(ld), g["ld_inv"], what="ld_inv", **ld_tol(np.float32))
    assert_close(N(z), g["z_inv_f64"].astype(np.float32), what="z_inv f64", rtol=1e-4, atol=1e-4)
    assert_close(N(ld), g["ld_inv_f64"].astype(np.float32), what="ld_inv f64", **ld_tol(np.float32))
    if name == "circ_ar_perm_tb":
        assert N(z)[0, 1] == 0.0 and N(z)[1, 3] == 0.0
    else:
        assert N(z)[0, 2] == 7.0 and N(z)[3, 5] == -4.0


def build_case(nfa, case):
    C, A = nfa.flows.CircularAutoregressiveRationalQuadraticSpline, nfa.flows.AutoregressiveRationalQuadraticSpline
    M = nfa.flows.autoregressive.MaskedPiecewiseRationalQuadraticAutoregressive
    torch.manual_seed(sum(map(ord, case)))
    if case == "d2_h4_k4":                       # the smallest: D 2, four hidden units, mult 13
        t = C(2, 2, 4, ind_circ=[1], num_bins=4, tail_bound=2.0, init_identity=False).mprqat
    elif case == "d33_h24_k6":                   # D crosses the padding of 32, mult 19, a tensor bound, one residual block
        bound = 1.5 + 2.0 * torch.rand(33)
        bound[[0, 7, 32]] = float(np.pi)
        t = C(33, 1, 24, ind_circ=[0, 7, 32], num_bins=6, tail_bound=bound, init_identity=False).mprqat
    elif case == "d128_h300_k10":                # the largest: 512 slots (items over both sample blocks), mult 31
        t = C(128, 2, 300, ind_circ=list(range(0, 128, 5)), num_bins=10, tail_bound=3.0, init_identity=False).mprqat
    elif case == "all_circular":
        t = C(5, 2, 12, ind_circ=[0, 1, 2, 3, 4], num_bins=10, tail_bound=float(np.pi), init_identity=False).mprqat
    elif case == "none_circular":                # list tails, all linear, unpermuted: no periodic feed
        t = C(9, 2, 40, ind_circ=[], num_bins=4, tail_bound=2.5, permute_mask=False, init_identity=False).mprqat
    elif case == "scalar_linear_permuted":       # mult = 3K - 1 = 23, the identity outside
        t = A(33, 2, 96, num_bins=8, tail_bound=2.5, permute_mask=True, init_identity=False).mprqat
        assert t._permuted()
    elif case == "scalar_linear_k11_permuted":   # mult = 3K - 1 = 32: the block is full, logits 1 .. 10 in slots 22 .. 31
        t = A(7, 2, 24, num_bins=11, tail_bound=2.5, permute_mask=True, init_identity=False).mprqat
    elif case == "scalar_linear_tensor_bound":   # mult = 3K - 1 = 14, an unpermuted mask
        t = M(6, 16, num_bins=5, tails="linear", tail_bound=1.0 + torch.rand(6), init_identity=False)
    else:                                        # scalar circular tails (mult = 3K) with a tensor bound
        assert case == "scalar_circular_tensor_bound"
        t = M(6, 16, num_bins=5, tails="circular", tail_bound=1.0 + torch.rand(6), init_identity=False)
    return scale_weights(t).to(DEV)


CASES = [("d2_h4_k4", 1), ("d33_h24_k6", 65), ("d128_h300_k10", 130), ("all_circular", 65), ("none_circular", 130),
         ("scalar_linear_permuted", 65), ("scalar_linear_k11_permuted", 65), ("scalar_linear_tensor_bound", 130), ("scalar_circular_tensor_bound", 65)]


@pytest.mark.parametrize("case,B", CASES)
def test_one_launch_matches_the_layerwise_path(nfa, spy, case, B):
    """One launch against eager MaskedLinear modules + nf_rqs_coupling on the same scaled-up weights: one row, one tile plus a row,
    the persistent tile loop with a ragged tail; the accumulate protocol with both signs."""
    t = build_case(nfa, case)
    x = inputs(t, B, 7)
    if B > 8:                                    # entries outside the interval: 0 / 0 with list tails, the identity otherwise
        x[1, 0], x[B - 1, t.features - 1] = 50.0, -60.0
    with torch.no_grad():
        z, ld = t.forward(x)
    assert spy == {"ft": 1, "made": 0, "rqs": 0}
    zr, ldr = layerwise(nfa, t, x)
    assert spy["ft"] == 1 and spy["made"] >= 1 and spy["rqs"] >= 1
    print("%s: max|dz| %.3e  max|dld| %.3e" % (case, float((z - zr).abs().max()), float((ld - ldr).abs().max())))
    assert_close(N(z), N(zr), what="z", rtol=1e-4, atol=1e-4)
    assert_close(N(ld), N(ldr), what="ld", **ld_bar(t.features))
    pk = t._packed_fwd_ft(DEV)
    tails = "feature" if isinstance(t.tails, list) else t.tails
    for acc, sign in ((nfa.ops.L.LD_SUB, -1.0), (nfa.ops.L.LD_ADD, 1.0)):
        buf = torch.full((B,), 2.0, device=DEV)
        nfa.ops.made_forward_spline_ft(x, pk[0], pk[1], pk[2], pk[3], t.num_bins, tails, logdet=buf, acc=acc)
        assert_close(N(buf), 2.0 + sign * N(ld), what="acc %d" % acc, rtol=1e-6, atol=1e-5)


def test_outside_rows_and_circular_inputs_at_the_bound(nfa, spy):
    """Linear features of a list-tails layer far outside: exactly 0 there and nothing in the log-det, whatever the value; circular
    inputs AT the bound itself agree with the layer-wise path."""
    t = build_case(nfa, "d33_h24_k6")
    lin = [c for c in range(33) if t.tails[c] == "linear"]
    x = inputs(t, 70, 11)
    x[5, 0], x[66, 32] = float(t.tail_bound[0]), -float(t.tail_bound[32])
    xa, xb = x.clone(), x.clone()
    cols = [lin[2], lin[9], lin[20]]
    for r, c in enumerate(cols):
        xa[r, c], xb[r, c] = 50.0, -50.0
        xa[64 + r, c], xb[64 + r, c] = -50.0, 77.0
    with torch.no_grad():
        za, lda = t.forward(xa)
        zb, ldb = t.forward(xb)
    zr, ldr = layerwise(nfa, t, xa)
    for r, c in enumerate(cols):
        assert float(za[r, c]) == 0.0 and float(za[64 + r, c]) == 0.0
    # (the conditioner of the later features reads the INPUT, which differs: compare the outside entries and the rows' earlier part
    # through the layer-wise path instead of bit equality)
    assert_close(N(za), N(zr), what="z", rtol=1e-4, atol=1e-4)
    assert_close(N(lda), N(ldr), what="ld", **ld_bar(33))
    zr2, ldr2 = layerwise(nfa, t, xb)
    assert_close(N(zb), N(zr2), what="z b", rtol=1e-4, atol=1e-4)
    assert_close(N(ldb), N(ldr2), what="ld b", **ld_bar(33))


def test_outside_value_of_the_last_degree_cannot_matter(nfa, spy):
    """A row whose ONLY outside entry is the linear feature of the LAST degree: nothing downstream reads it, so whatever the value the
    output bits are the same, 0 in that column.  The circular columns are chosen after the permutation is known (the constructor's
    first draw: the same for every ind_circ), so the column of the last degree is always linear."""
    C = nfa.flows.CircularAutoregressiveRationalQuadraticSpline

    def build(ind_circ):
        torch.manual_seed(29)
        return C(9, 2, 20, ind_circ=ind_circ, num_bins=6, tail_bound=2.5, permute_mask=True, init_identity=False).mprqat
    col_last = int(np.argmax(build([0]).autoregressive_net.final_layer.degrees.numpy()[::19]))
    t = build([c for c in range(9) if c != col_last][:3])
    assert t.tails[col_last] == "linear" and t.tails.count("circular") == 3
    t = scale_weights(t).to(DEV)
    x = inputs(t, 70, 13)
    xc, xd = x.clone(), x.clone()
    xc[3, col_last], xd[3, col_last] = 50.0, -77.0
    xc[68, col_last], xd[68, col_last] = -50.0, 1e6
    with torch.no_grad():
        (zc, ldc), (zd, ldd) = t.forward(xc), t.forward(xd)
    assert spy["ft"] == 2 and spy["made"] == 0
    assert torch.equal(zc, zd) and torch.equal(ldc, ldd)
    assert float(zc[3, col_last]) == 0.0 and float(zc[68, col_last]) == 0.0


@pytest.mark.parametrize("case", ["k11_list", "context", "float64", "requires_grad"])
def test_outside_the_kernel_limits_the_old_path_stays(nfa, spy, case):
    C = nfa.flows.CircularAutoregressiveRationalQuadraticSpline
    torch.manual_seed(17)
    ctx = None
    if case == "k11_list":                       # 3K + 1 = 34 rows per feature
        t = C(5, 2, 12, ind_circ=[1, 3], num_bins=11, tail_bound=2.5, init_identity=False).mprqat
    elif case == "context":
        t = C(5, 2, 12, ind_circ=[1, 3], num_context_channels=3, num_bins=4, tail_bound=2.5, init_identity=False).mprqat
        ctx = torch.randn(33, 3, device=DEV)
    else:
        t = C(5, 2, 12, ind_circ=[1, 3], num_bins=4, tail_bound=2.5, init_identity=False).mprqat
    t = scale_weights(t).to(DEV)
    x = inputs(t, 33, 3)
    if case == "float64":
        t, x = t.double(), x.double()
    if case == "requires_grad":
        x.requires_grad_(True)
        z, ld = t.forward(x, ctx)
        (z.sum() + ld.sum()).backward()
        assert torch.isfinite(x.grad).all()
    else:
        with torch.no_grad():
            z, ld = t.forward(x, ctx)
    assert spy["ft"] == 0
    assert torch.isfinite(z).all() and torch.isfinite(ld).all()
    if case == "k11_list":                       # and stays right: the same layer in float64
        import copy
        with torch.no_grad():
            z64, ld64 = copy.deepcopy(t).double().forward(x.double())
        assert_close(N(z), N(z64).astype(np.float32), what="z", rtol=1e-4, atol=1e-4)
        assert_close(N(ld), N(ld64).astype(np.float32), what="ld", **ld_tol(np.float32))


def test_same_bits_twice_and_no_stray_writes(nfa):
    """The same input twice gives identical bits; canaries around y and logdet are intact after a B = 65 call."""
    t = build_case(nfa, "d33_h24_k6")
    B, D = 65, 33
    x = inputs(t, B, 5)
    with torch.no_grad():
        z1, l1 = t.forward(x)
        z2, l2 = t.forward(x)
    assert torch.equal(z1, z2) and torch.equal(l1, l2)
    pk = t._packed_fwd_ft(DEV)
    L, pad = nfa._lib, 256
    ybuf = torch.full((pad + B * D + pad,), 1234.5, device=DEV)
    lbuf = torch.full((pad + B + pad,), 1234.5, device=DEV)
    y, ld = ybuf[pad:pad + B * D], lbuf[pad:pad + B]
    L.call("nf_made_forward_spline_ft", L.ptr(x), L.ptr(y), L.ptr(ld), L.ptr(pk[0]), L.ptr(pk[1]), L.ptr(pk[2]), B, D, pk[3],
           t.num_bins, 3, t.min_bin_width, t.min_bin_height, t.min_derivative, L.LD_WRITE, L.stream())
    torch.cuda.synchronize()
    assert torch.equal(y.view(B, D), z1) and torch.equal(ld, l1)
    for buf, n in ((ybuf, B * D), (lbuf, B)):
        assert bool((buf[:pad] == 1234.5).all()) and bool((buf[pad + n:] == 1234.5).all())
