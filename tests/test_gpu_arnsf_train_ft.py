"""GPU tests (-m gpu) of the circular / mask-permuted autoregressive spline layers UNDER AUTOGRAD in the density direction on the MADE
training kernels (autograd.MadeFtFn: nf_made_forward_train_ft -> SplineFn, backward nf_made_backward -> nf_made_feed_ft_bwd ->
nf_made_wgrad on a degree-order pack): against the reference's autograd (tests/golden/grad_circ_ar_perm_*.npz,
grad_ar_perm_lin_d12_h24.npz), against the project's own eager path (config.arnsf_train_ft = False) on the same weights, at the batch
where the other MADE training kernels switch to 128-row tiles, for determinism and stray writes, with live parameters under an
optimizer, and outside the route (the eager path stays)."""
import copy

import numpy as np
import pytest
import torch

import ar_ft_train_cases as cases
from conftest import assert_close, golden_state, load_golden
from test_gpu_made_fwd_ft import build_case, inputs, ld_bar, scale_weights

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
OPS = ("made_forward_train_ft", "made_feed_ft_bwd", "made_backward", "made_wgrad")


@pytest.fixture(scope="module")
def nfa():
    import normflows_amd
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    assert normflows_amd.native_library_path().endswith("normalizing-flows_amd/lib/libnf_mi355x.so")
    normflows_amd._lib.lib()
    return normflows_amd


@pytest.fixture
def spy(nfa, monkeypatch):
    """Counts the launches of the four ops of the route and the eager MaskedLinear calls."""
    calls = {k: 0 for k in OPS + ("masked_linear",)}

    def wrap(real, key):
        def f(*a, **k):
            calls[key] += 1
            return real(*a, **k)
        return f
    for k in OPS:
        monkeypatch.setattr(nfa.ops, k, wrap(getattr(nfa.ops, k), k))
    monkeypatch.setattr(nfa.nets.MaskedLinear, "forward", wrap(nfa.nets.MaskedLinear.forward, "masked_linear"))
    return calls


def N(t):
    return t.detach().cpu().numpy()


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def step(t, x, cz, cl, which="both"):
    """[z, ld, gx, every parameter gradient] of loss = sum(z cz) + sum(ld cl) through t.forward (the density direction of the inner
    transform); which = "z" | "ld": one cotangent absent."""
    t.zero_grad(set_to_none=True)
    xx = x.clone().requires_grad_(True)
    z, ld = t.forward(xx)
    loss = (z * cz).sum() if which == "z" else ((ld * cl).sum() if which == "ld" else (z * cz).sum() + (ld * cl).sum())
    loss.backward()
    return [z.detach(), ld.detach(), xx.grad] + [p.grad.clone() for p in t.parameters()]


def eager(nfa, t, *a, **k):
    """The same step through eager MaskedLinear modules.  The route's switch alone does that for a permuted or periodic MADE; an
    unpermuted MADE with an Identity preprocessing (a tensor bound on scalar tails) would fall to autograd.MadeFn, the other
    hand-written route, so config.made_train goes off as well: the comparison is against torch's own linears in every case."""
    nfa.config.set_arnsf_train_ft(False)
    nfa.config.set_made_train(False)
    try:
        return step(t, *a, **k)
    finally:
        nfa.config.set_arnsf_train_ft(True)
        nfa.config.set_made_train(True)


def compare(t, got, ref, what=""):
    """The bars against the eager route: z 1e-4 / 1e-4, ld by ld_bar(D), every gradient 2e-4 of scale (the bar
    test_autoregressive_inverse_implicit_vs_d_pass_autograd uses for two float32 routes through one layer)."""
    assert_close(N(got[0]), N(ref[0]), what=what + " z", rtol=1e-4, atol=1e-4)
    assert_close(N(got[1]), N(ref[1]), what=what + " ld", **ld_bar(t.features))
    names = ["gx"] + [k for k, _ in t.named_parameters()]
    worst = 0.0
    for k, a, b in zip(names, got[2:], ref[2:]):
        assert a.shape == b.shape, (what, k)
        if b.numel() == 0:                          # (a periodic preprocessing without a circular column)
            continue
        e = float((a - b).abs().max()) / max(1.0, float(b.abs().max()))
        worst = max(worst, e)
        assert e <= 2e-4, (what, k, e)
    return worst


def masks_zero(t):
    for lin in t.autoregressive_net._linears():
        assert float((lin.weight.grad * (1 - lin.mask)).abs().max()) == 0.0


@pytest.mark.parametrize("name", cases.FIXTURES)
def test_fixtures_vs_reference_autograd(nfa, spy, name):
    """layer.inverse(x) + backward of the three fixtures: each of the four ops exactly once and no eager MaskedLinear; the bars of
    test_autoregressive_layers_training_vs_reference_autograd: outputs, gx and the strided gradient samples within 1e-3 of scale of
    the reference's float32 leg, sums within 1e-4 max(1, abs-sum), q90 of the errors against the float64 leg <= 4 x the reference's
    own (floor 1e-7), gradients exactly zero under every mask."""
    g = cases.load_case(name)
    layer = cases.make_layer(nfa, name, g).to(DEV)
    x = T(g["x"]).requires_grad_(True)
    z, ld = layer.inverse(x)
    ((z * T(g["cz"])).sum() + (ld * T(g["cl"])).sum()).backward()
    assert spy == {"made_forward_train_ft": 1, "made_feed_ft_bwd": 1, "made_backward": 1, "made_wgrad": 1, "masked_linear": 0}, spy
    stride = int(g["stride"])

    def err(a, ref):
        return np.abs(a.astype(np.float64) - ref) / max(1.0, float(np.abs(ref).max()))
    ours = {"z": N(z), "ld": N(ld), "gx": N(x.grad)}
    own, got = [], []
    for k, a in ours.items():
        print("%s %s: %.3e of scale vs the float32 leg" % (name, k, err(a, g[k + "_f32"]).max()))
        assert err(a, g[k + "_f32"]).max() < 1e-3, (k, err(a, g[k + "_f32"]).max())
        own.append(err(g[k + "_f32"], g[k + "_f64"]).max())
        got.append(err(a, g[k + "_f64"]).max())
    for k, p in layer.named_parameters():
        key = k.replace(".", "__")
        flat = N(p.grad).reshape(-1)
        ref32, ref64 = g["g_f32__" + key], g["g_f64__" + key]
        assert err(flat[::stride], ref32).max() < 1e-3, (k, err(flat[::stride], ref32).max())
        chk = g["chk_f64__" + key]
        assert abs(float(flat.astype(np.float64).sum()) - chk[0]) < 1e-4 * max(1.0, chk[1]), k
        own.append(err(ref32, ref64).max())
        got.append(err(flat[::stride], ref64).max())
    print("%s: q90 vs float64 %.3e, the reference's own %.3e" % (name, np.quantile(got, 0.9), np.quantile(own, 0.9)))
    assert np.quantile(got, 0.9) <= 4 * max(np.quantile(own, 0.9), 1e-7), (np.quantile(got, 0.9), np.quantile(own, 0.9))
    masks_zero(layer.mprqat)
    if name == "grad_ar_perm_lin_d12_h24":           # scalar linear tails: the identity beyond the bound
        out = np.abs(g["x"]) > 3.0
        assert out.any() and np.array_equal(N(z)[out], g["x"][out])


def periodic_bias_case(nfa):
    torch.manual_seed(41)
    t = nfa.flows.CircularAutoregressiveRationalQuadraticSpline(9, 2, 20, ind_circ=[1, 4, 7], num_bins=6, tail_bound=2.5,
                                                                init_identity=False).mprqat
    old = t.autoregressive_net.preprocessing
    pre = nfa.nets.PeriodicFeaturesElementwise(9, old.ind, old.scale, bias=True)
    with torch.no_grad():
        pre.weights.copy_(old.weights)
        pre.bias.copy_(torch.tensor([0.3, -0.2, 0.5]))
    t.autoregressive_net.preprocessing = pre
    return scale_weights(t).to(DEV)


CASES = [("d2_h4_k4", 1), ("d33_h24_k6", 65), ("d128_h300_k10", 130), ("all_circular", 65), ("none_circular", 130),
         ("scalar_linear_permuted", 65), ("scalar_linear_tensor_bound", 130), ("periodic_bias", 65)]


@pytest.mark.parametrize("case,B", CASES)
def test_new_route_matches_the_eager_route(nfa, spy, case, B):
    """The shapes of tests/test_gpu_made_fwd_ft.py (weights x 1.5) + a preprocessing with a non-zero bias: one row, one tile plus a
    row, ragged tails, 256 and 512 slots, with and without a permutation / periodic positions; entries far outside the interval; both
    cotangents and each one alone."""
    t = periodic_bias_case(nfa) if case == "periodic_bias" else build_case(nfa, case)
    D = t.features
    x = inputs(t, B, 7)
    listed = isinstance(t.tails, (list, tuple))
    if B > 8:
        x[1, 0], x[B - 1, D - 1] = 50.0, -60.0
    gen = torch.Generator().manual_seed(3)
    cz, cl = torch.randn(B, D, generator=gen).to(DEV), torch.randn(B, generator=gen).to(DEV)
    for which in ("both", "z", "ld"):
        for k in spy:
            spy[k] = 0
        got = step(t, x, cz, cl, which)
        assert spy == {"made_forward_train_ft": 1, "made_feed_ft_bwd": 1, "made_backward": 1, "made_wgrad": 1, "masked_linear": 0}, spy
        masks_zero(t)
        ref = eager(nfa, t, x, cz, cl, which)
        assert spy["made_forward_train_ft"] == 1 and spy["masked_linear"] >= 1
        worst = compare(t, got, ref, "%s %s" % (case, which))
        print("%s %s: max|dz| %.3e max|dld| %.3e worst gradient %.3e of scale" % (
            case, which, float((got[0] - ref[0]).abs().max()), float((got[1] - ref[1]).abs().max()), worst))
    if B > 8 and listed:                            # list tails: 0 beyond the interval (utils/splines.py:48-57), nothing in its own gradient path
        assert float(got[0][1, 0]) == 0.0 and float(got[0][B - 1, D - 1]) == 0.0
    if case == "periodic_bias":
        pre = t.autoregressive_net.preprocessing
        assert pre.bias.grad is not None and float(pre.bias.grad.abs().max()) > 0.0


def test_batch_where_the_other_made_kernels_take_128_row_tiles(nfa, spy):
    """D 24 / hidden 40 / K 8 / 4 circular / permuted at B = 16 512, the smallest batch at which mf_tr128 switches on for the MADE
    training kernels.  This route always runs 64-row tiles, forward and chain alike (the `bits` layout depends on the tile height), so
    outputs and gx are bit-identical whatever nf_config_made_tr128 says, and both settings meet the eager route's bars."""
    torch.manual_seed(24)
    t = nfa.flows.CircularAutoregressiveRationalQuadraticSpline(24, 2, 40, ind_circ=[2, 9, 13, 23], num_bins=8, tail_bound=3.0,
                                                                permute_mask=True, init_identity=False).mprqat
    t = scale_weights(t).to(DEV)
    B = 16512
    x = inputs(t, B, 9)
    gen = torch.Generator().manual_seed(4)
    cz, cl = torch.randn(B, 24, generator=gen).to(DEV), torch.randn(B, generator=gen).to(DEV)
    lib = nfa._lib.lib()
    prev = lib.nf_config_made_tr128(1)
    try:
        on = step(t, x, cz, cl)
        lib.nf_config_made_tr128(0)
        off = step(t, x, cz, cl)
    finally:
        lib.nf_config_made_tr128(prev)
    assert spy["made_forward_train_ft"] == 2 and spy["masked_linear"] == 0
    for a, b in zip(on[:3], off[:3]):
        assert torch.equal(a, b)
    ref = eager(nfa, t, x, cz, cl)
    compare(t, on, ref, "tr128 on")
    compare(t, off, ref, "tr128 off")


def test_same_bits_twice_and_no_stray_writes(nfa):
    """The same step twice gives bit-identical outputs and gradients; canaries around params, x_pos, the fed buffer, g_x and the
    periodic gradient vector are intact after B = 65 calls of the two new entry points."""
    t = build_case(nfa, "d33_h24_k6")
    B, D = 65, 33
    x = inputs(t, B, 5)
    gen = torch.Generator().manual_seed(6)
    cz, cl = torch.randn(B, D, generator=gen).to(DEV), torch.randn(B, generator=gen).to(DEV)
    a, b = step(t, x, cz, cl), step(t, x, cz, cl)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    fwd, bwd, ft, plist = t._train_packs_ft(torch.device(DEV))
    MD, NB, hp, Bp = bwd["MD"], bwd["NB"], fwd[2], 128
    want = nfa.ops.made_forward_train_ft(x, fwd[0], fwd[1], hp, MD, NB)
    L, pad, C = nfa._lib, 256, 1234.5

    def canary(n):
        buf = torch.full((pad + n + pad,), C, device=DEV)
        return buf, buf[pad:pad + n]
    pbuf, params = canary(B * MD)
    xbuf, x_pos = canary(B * D)
    fbuf, x_pad = canary(Bp * 128)
    save = torch.empty(2 * NB + 1, Bp, hp, device=DEV)
    bits = torch.empty(Bp // 64, 2 * NB, 2, 512, dtype=torch.int32, device=DEV)
    L.call("nf_made_forward_train_ft", L.ptr(x), L.ptr(params), L.ptr(save), L.ptr(bits), L.ptr(x_pad), L.ptr(x_pos), L.ptr(fwd[0]),
           L.ptr(fwd[1]), B, D, hp, MD // D, L.stream())
    torch.cuda.synchronize()
    assert torch.equal(params.view(B, MD), want[0]) and torch.equal(x_pos.view(B, D), want[4])
    assert torch.equal(x_pad.view(Bp, 128), want[3]) and torch.equal(save, want[1]) and torch.equal(bits, want[2])
    assert torch.equal(x_pos.view(B, D), x[:, ft["col"]])
    assert float(x_pad.view(Bp, 128)[B:].abs().max()) == 0.0 and float(x_pad.view(Bp, 128)[:, D:].abs().max()) == 0.0
    g_pre, g_xpos = torch.randn(B, D, device=DEV), torch.randn(B, D, device=DEV)
    n = ft["n_circ"]
    feed = fwd[0][ft["feed_off"]:]
    gx_w, gw_w, _ = nfa.ops.made_feed_ft_bwd(g_pre, g_xpos, x, ft["ttable"], feed, n, False)
    gbuf, g_x = canary(B * D)
    wbuf, g_w = canary(2 * n)
    part = torch.empty(512 * 3 * n, device=DEV)
    L.call("nf_made_feed_ft_bwd", L.ptr(g_pre), L.ptr(g_xpos), L.ptr(x), L.ptr(ft["ttable"]), L.ptr(feed), L.ptr(g_x), L.ptr(g_w),
           L.ptr(None), L.ptr(part), B, D, n, L.stream())
    torch.cuda.synchronize()
    assert torch.equal(g_x.view(B, D), gx_w) and torch.equal(g_w.view(n, 2), gw_w)
    for buf, m in ((pbuf, B * MD), (xbuf, B * D), (fbuf, Bp * 128), (gbuf, B * D), (wbuf, 2 * n)):
        assert bool((buf[:pad] == C).all()) and bool((buf[pad + m:] == C).all())


def test_live_parameters_under_fused_adam(nfa, spy):
    """Three fused-Adam steps on a circular layer, the periodic weights among the parameters: after each the new route's outputs and
    gradients still meet the bars against the eager route on the CURRENT weights -- no stale pack, no stale periodic weights."""
    t = build_case(nfa, "d33_h24_k6")
    B, D = 65, 33
    x = inputs(t, B, 8)
    gen = torch.Generator().manual_seed(2)
    cz, cl = torch.randn(B, D, generator=gen).to(DEV), torch.randn(B, generator=gen).to(DEV)
    pre = t.autoregressive_net.preprocessing
    assert any(p is pre.weights for p in t.parameters())
    opt = torch.optim.Adam(t.parameters(), lr=3e-3, fused=True)
    before = pre.weights.detach().clone()
    for it in range(3):
        got = step(t, x, cz, cl)
        opt.step()
        got = step(t, x, cz, cl)
        ref = eager(nfa, t, x, cz, cl)
        compare(t, got, ref, "after step %d" % it)
    assert spy["made_forward_train_ft"] == 6 and not torch.equal(before, pre.weights.detach())


def check_layer_grads(layer, g, rtol, atol):
    """tests/test_gpu_training.py's check against a layer_grads fixture (both directions)."""
    cz, cl = T(g["cz"]).to(next(layer.parameters()).dtype), T(g["cl"]).to(next(layer.parameters()).dtype)
    for name, fn in (("inv", layer.inverse), ("fwd", layer.forward)):
        x = T(g["x"]).to(cz.dtype).requires_grad_(True)
        layer.zero_grad()
        z, ld = fn(x)
        ((z * cz).sum() + (ld * cl).sum()).backward()
        assert_close(N(x.grad), g["gx_" + name], what="gx_" + name, rtol=rtol, atol=atol)
        for k, p_ in layer.named_parameters():
            ref = g["g_%s__%s" % (name, k.replace(".", "__"))]
            scale = max(1.0, float(np.abs(ref).max()))
            got = np.zeros_like(ref) if p_.grad is None else N(p_.grad)
            assert_close(got, ref, what="%s grad %s" % (name, k), rtol=rtol, atol=atol * scale)


@pytest.mark.parametrize("case", ["float64", "switch_off", "higher_order", "context"])
def test_outside_the_route_the_eager_path_stays(nfa, spy, case):
    """Float64, the switch off, config.higher_order_gradients() and a context each leave all four ops at zero; the first three still
    match the reference fixture grad_circ_autoregressive at its test's bars, and double backward works inside
    higher_order_gradients()."""
    C = nfa.flows.CircularAutoregressiveRationalQuadraticSpline
    if case == "context":
        torch.manual_seed(17)
        t = scale_weights(C(5, 2, 12, ind_circ=[1, 3], num_context_channels=3, num_bins=4, tail_bound=2.5, init_identity=False).mprqat)
        t = t.to(DEV)
        x = inputs(t, 33, 3).requires_grad_(True)
        z, ld = t.forward(x, torch.randn(33, 3, device=DEV))
        (z.sum() + ld.sum()).backward()
        assert torch.isfinite(x.grad).all() and all(spy[k] == 0 for k in OPS) and spy["masked_linear"] >= 1
        return
    g = load_golden("grad_circ_autoregressive")
    layer = C(5, 2, 12, ind_circ=[0, 3], num_bins=4, tail_bound=2.5, permute_mask=False, init_identity=False)
    layer.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in golden_state(g).items()}, strict=True)
    layer = layer.to(torch.float64 if case == "float64" else torch.float32).to(DEV)
    if case == "float64":
        check_layer_grads(layer, g, rtol=2e-3, atol=2e-4)
    elif case == "switch_off":
        nfa.config.set_arnsf_train_ft(False)
        try:
            check_layer_grads(layer, g, rtol=2e-3, atol=2e-4)
        finally:
            nfa.config.set_arnsf_train_ft(True)
    else:
        with nfa.config.higher_order_gradients():
            check_layer_grads(layer, g, rtol=2e-3, atol=2e-4)
            x = T(g["x"]).requires_grad_(True)
            z, ld = layer.inverse(x)
            (gx,) = torch.autograd.grad((z * T(g["cz"])).sum() + (ld * T(g["cl"])).sum(), x, create_graph=True)
            gx.pow(2).sum().backward()
            assert torch.isfinite(x.grad).all() and float(x.grad.abs().max()) > 0.0
    assert all(spy[k] == 0 for k in OPS), spy
    assert spy["masked_linear"] >= 1
    # and with everything on, the same fixture takes the new route
    for k in spy:
        spy[k] = 0
    if case == "switch_off":
        check_layer_grads(layer, g, rtol=2e-3, atol=2e-4)
        assert spy["made_forward_train_ft"] >= 1 and spy["made_feed_ft_bwd"] >= 1
