"""GPU tests (-m gpu) of the circular NSF coupling layer UNDER AUTOGRAD on HIP kernels: the conditioner on the MADE training kernels
through a dense, periodically fed pack (autograd.ResNetFtFn: nf_made_forward_train_ft, nf_made_backward, nf_made_feed_ft_bwd,
nf_made_wgrad) and the spline's backward on wave-private tiles (nf_rqs_coupling_bwd_ft_wave) -- against the reference's autograd
(tests/golden/grad_circ_cpl_*.npz), against the project's own eager route (config.nsf_circular_train = False) on the same weights, the
new kernel alone against nf_rqs_coupling_bwd_ft, with live parameters under an optimizer, and outside the route (the eager path stays)."""
import os
import sys

import numpy as np
import pytest
import torch

import circ_coupled_train_cases as cases
from conftest import assert_close
from test_gpu_made_fwd_ft import ld_bar

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MADE_OPS = ("made_forward_train_ft", "made_backward", "made_feed_ft_bwd", "made_wgrad")
WAVE = "rqs_coupling_bwd_ft_wave"
ROUTE = {k: 1 for k in MADE_OPS + (WAVE,)}


@pytest.fixture(scope="module")
def nfa():
    import normflows_amd
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    assert normflows_amd.native_library_path().endswith("normalizing-flows_amd/lib/libnf_mi355x.so")
    normflows_amd._lib.lib()
    return normflows_amd


@pytest.fixture
def spy(nfa, monkeypatch):
    """Counts the launches of the route's ops, of the spline backward's common entry (rqs_coupling_bwd: every spline backward passes
    it) and the eager Linear calls."""
    calls = {k: 0 for k in MADE_OPS + (WAVE, "rqs_coupling_bwd", "linear")}

    def wrap(real, key):
        def f(*a, **k):
            calls[key] += 1
            return real(*a, **k)
        return f
    for k in MADE_OPS + (WAVE, "rqs_coupling_bwd"):
        monkeypatch.setattr(nfa.ops, k, wrap(getattr(nfa.ops, k), k))
    monkeypatch.setattr(nfa.nets.Linear, "forward", wrap(nfa.nets.Linear.forward, "linear"))
    return calls


def route_counts(spy):
    return {k: spy[k] for k in ROUTE}


def reset(spy):
    for k in spy:
        spy[k] = 0


def N(t):
    return t.detach().cpu().numpy()


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def fixtures(nfa):
    """The three fixtures, loaded once and left unchanged."""
    return {name: cases.load_case(name) for name in cases.FIXTURES}


def step(layer, d, x, cz, cl, which="both", context=None):
    """[z, ld, gx, every parameter gradient] of loss = sum(z cz) + sum(ld cl) through layer.inverse (d = "inv": density) or
    layer.forward ("fwd": sampling); which = "z" | "ld": one cotangent absent."""
    layer.zero_grad(set_to_none=True)
    xx = x.clone().requires_grad_(True)
    fn = layer.inverse if d == "inv" else layer.forward
    z, ld = fn(xx) if context is None else fn(xx, context)
    loss = (z * cz).sum() if which == "z" else ((ld * cl).sum() if which == "ld" else (z * cz).sum() + (ld * cl).sum())
    loss.backward()
    return [z.detach(), ld.detach(), xx.grad] + [torch.zeros_like(p) if p.grad is None else p.grad.clone() for p in layer.parameters()]


def eager(nfa, layer, *a, **k):
    """The same step with the switch off: eager torch modules for the conditioner, nf_rqs_coupling_bwd_ft for the spline."""
    nfa.config.set_nsf_circular_train(False)
    try:
        return step(layer, *a, **k)
    finally:
        nfa.config.set_nsf_circular_train(True)


def compare(layer, D, got, ref, what=""):
    """The bars against the eager route: z 1e-4 / 1e-4, ld by ld_bar(D), every gradient 2e-4 of scale."""
    assert_close(N(got[0]), N(ref[0]), what=what + " z", rtol=1e-4, atol=1e-4)
    assert_close(N(got[1]), N(ref[1]), what=what + " ld", **ld_bar(D))
    names = ["gx"] + [k for k, _ in layer.named_parameters()]
    worst = 0.0
    for k, a, b in zip(names, got[2:], ref[2:]):
        assert a.shape == b.shape, (what, k)
        e = float((a - b).abs().max()) / max(1.0, float(b.abs().max()))
        worst = max(worst, e)
        assert e <= 2e-4, (what, k, e)
    return worst


def full_bound(layer, D):
    p = layer.prqct
    tb = torch.zeros(D)
    for idx, b in ((p.transform_features, p.tail_bound), (p.identity_features, p.unconditional_transform.tail_bound)):
        tb[idx.cpu()] = b.detach().cpu().float() if torch.is_tensor(b) else torch.full((len(idx),), float(b))
    return tb


def batch(layer, D, B, seed):
    """x uniform within 0.98 x bound, with two entries far outside their intervals when there is room; cz, cl."""
    gen = torch.Generator().manual_seed(seed)
    x = (2 * torch.rand(B, D, generator=gen) - 1) * full_bound(layer, D) * 0.98
    if B > 8:
        x[1, 0], x[B - 1, D - 1] = 50.0, -60.0
    return x.to(DEV), torch.randn(B, D, generator=gen).to(DEV), torch.randn(B, generator=gen).to(DEV)


@pytest.mark.parametrize("name,d", [(n, d) for n, ds in cases.FIXTURES.items() for d in ds])
def test_fixtures_vs_reference_autograd(nfa, spy, fixtures, name, d):
    """layer.inverse(x) / layer.forward(x) + backward of the fixtures: the four MADE training ops and (8 bins) the wave-private spline
    backward exactly once each, never an eager Linear; for 5 bins the wave kernel is not called and the spline's backward goes the
    old way.  (The sampling direction has a second spline backward, of the identity half alone: it has no conditioner rows to stage
    and stays on nf_rqs_coupling_bwd_ft.)  Bars of tests/test_gpu_arnsf_train_ft.py: outputs, gx and the strided gradient samples
    within 1e-3 of scale of the reference's float32 leg, sums within 1e-4 max(1, abs-sum), q90 of the errors against the float64 leg
    <= 4 x the reference's own (floor 1e-7).  At the `outside` positions the output is exactly 0, and gx is exactly 0 wherever the
    reference's own is: a transform coordinate in either direction and an identity coordinate in the sampling direction (in the
    density direction the raw identity coordinate still feeds the conditioner, in the reference as here)."""
    g = fixtures[name]
    layer = cases.make_layer(nfa, name, g).to(DEV)
    x = T(g["x"]).requires_grad_(True)
    z, ld = (layer.inverse if d == "inv" else layer.forward)(x)
    ((z * T(g["cz"])).sum() + (ld * T(g["cl"])).sum()).backward()
    k8 = layer.prqct.num_bins == 8
    assert route_counts(spy) == dict(ROUTE, **{WAVE: 1 if k8 else 0}), spy
    assert spy["linear"] == 0 and spy["rqs_coupling_bwd"] == (2 if d == "fwd" else 1), spy
    stride = int(g["stride"])

    def err(a, ref):
        return np.abs(a.astype(np.float64) - ref) / max(1.0, float(np.abs(ref).max()))
    ours = {"z": N(z), "ld": N(ld), "gx": N(x.grad)}
    own, got = [], []
    for k, a in ours.items():
        r32, r64 = g["%s_%s_f32" % (k, d)], g["%s_%s_f64" % (k, d)]
        print("%s %s %s: %.3e of scale vs the float32 leg" % (name, d, k, err(a, r32).max()))
        assert err(a, r32).max() < 1e-3, (k, err(a, r32).max())
        own.append(err(r32, r64).max())
        got.append(err(a, r64).max())
    for k, p in layer.named_parameters():
        key = k.replace(".", "__")
        flat = N(p.grad).reshape(-1)
        ref32, ref64 = g["g_%s_f32__%s" % (d, key)], g["g_%s_f64__%s" % (d, key)]
        assert err(flat[::stride], ref32).max() < 1e-3, (k, err(flat[::stride], ref32).max())
        chk = g["chk_%s_f64__%s" % (d, key)]
        assert abs(float(flat.astype(np.float64).sum()) - chk[0]) < 1e-4 * max(1.0, chk[1]), k
        own.append(err(ref32, ref64).max())
        got.append(err(flat[::stride], ref64).max())
    print("%s %s: q90 vs float64 %.3e, the reference's own %.3e" % (name, d, np.quantile(got, 0.9), np.quantile(own, 0.9)))
    assert np.quantile(got, 0.9) <= 4 * max(np.quantile(own, 0.9), 1e-7), (np.quantile(got, 0.9), np.quantile(own, 0.9))
    zeros = 0
    for r, c in g["outside"]:
        assert float(ours["z"][r, c]) == 0.0
        if float(g["gx_%s_f32" % d][r, c]) == 0.0:
            zeros += 1
            assert float(ours["gx"][r, c]) == 0.0, (r, c)
    assert zeros == {"inv": 2, "fwd": 4}[d] if len(g["outside"]) else zeros == 0


def with_bias(nfa, layer):
    net = layer.prqct.transform_net
    old = net.preprocessing
    pre = nfa.nets.PeriodicFeaturesElementwise(old.ndim, old.ind, old.scale, bias=True)
    with torch.no_grad():
        pre.weights.copy_(old.weights)
        pre.bias.copy_(torch.linspace(-0.4, 0.5, len(old.ind)))
    net.preprocessing = pre
    return layer


# (fixture, rows, periodic bias, seed of the batch).  The seeds were chosen on the CPU against the reference alone: at them the
# reference's own float32 leg is within 3e-5 (z, ld) / 6e-5 of scale (gradients) of its float64 leg in both directions, a third of the
# bars below, so that two float32 routes can meet them.  (Seed 7 with the periodic bias does not qualify: the reference's float32
# log-det of row 28 is 1.8e-4 off its float64 value, the layer is that steep there.)
ROUTES = [("grad_circ_cpl_d7_h40", 1, False, 7), ("grad_circ_cpl_d7_h40", 63, False, 7), ("grad_circ_cpl_d7_h40", 64, False, 7),
          ("grad_circ_cpl_d7_h40", 65, False, 7), ("grad_circ_cpl_d7_h40", 65, True, 8), ("grad_circ_cpl_d21_h260", 130, False, 7),
          ("grad_circ_cpl_d6_k5", 70, False, 7)]


@pytest.mark.parametrize("name,B,bias,seed", ROUTES)
def test_new_route_matches_the_eager_route(nfa, spy, fixtures, name, B, bias, seed):
    """The fixtures' states (one with a PeriodicFeaturesElementwise(bias=True) swapped in) at one row, around the 64-row tile and at
    three tiles, both directions, both cotangents and each one alone, against the same weights with the switch off."""
    layer = cases.make_layer(nfa, name, fixtures[name])
    layer = (with_bias(nfa, layer) if bias else layer).to(DEV)
    D = layer.prqct.identity_features.numel() + layer.prqct.transform_features.numel()
    k8 = layer.prqct.num_bins == 8
    x, cz, cl = batch(layer, D, B, seed)
    for d in ("inv", "fwd"):
        for which in ("both", "z", "ld"):
            reset(spy)
            got = step(layer, d, x, cz, cl, which)
            assert route_counts(spy) == dict(ROUTE, **{WAVE: 1 if k8 else 0}) and spy["linear"] == 0, spy
            reset(spy)
            ref = eager(nfa, layer, d, x, cz, cl, which)
            assert all(spy[k] == 0 for k in ROUTE) and spy["linear"] >= 1, spy
            worst = compare(layer, D, got, ref, "%s B=%d %s %s" % (name, B, d, which))
            print("%s B=%d %s %s: max|dz| %.3e max|dld| %.3e worst gradient %.3e of scale" % (
                name, B, d, which, float((got[0] - ref[0]).abs().max()), float((got[1] - ref[1]).abs().max()), worst))
        if B > 8:          # list tails: 0 beyond the interval (utils/splines.py:48-57)
            assert float(got[0][1, 0]) == 0.0 and float(got[0][B - 1, D - 1]) == 0.0
    if bias:
        pre = layer.prqct.transform_net.preprocessing
        assert pre.bias.grad is not None and float(pre.bias.grad.abs().max()) > 0.0


def kernel_inputs(nI, nT, B, seed, spread=1.5):
    """Random operands of the spline backward: conditioner rows spread x N(0, 1) (divided by wh_div = 3 in the kernel), batch-shared
    parameters spread / 1.5 x N(0, 1)."""
    D = nI + nT
    gen = torch.Generator().manual_seed(seed)
    perm = torch.randperm(D, generator=gen)
    r = lambda *s: torch.randn(*s, generator=gen)      # noqa: E731
    bound = 1.5 + 2.0 * torch.rand(D, generator=gen)
    codes = torch.randint(1, 3, (D,), generator=gen, dtype=torch.int32)
    x = (2 * torch.rand(B, D, generator=gen) - 1) * bound * 1.1          # (about one entry in eleven outside its interval)
    iidx, tidx = perm[:nI].sort().values, perm[nI:].sort().values
    u = spread / 1.5
    t = dict(x=x, gy=r(B, D), gld=r(B), cond=spread * r(B, nT * 25) if nT else None, uw=u * r(nI, 8) if nI else None,
             uh=u * r(nI, 8) if nI else None, ud=u * r(nI, 9) if nI else None, iidx=iidx, tidx=tidx, tails_t=codes[tidx], bound_t=bound[tidx],
             tails_i=codes[iidx], bound_i=bound[iidx])
    return {k: (None if v is None else v.to(DEV).contiguous()) for k, v in t.items()}


# (nI, nT, rows, spread of the random parameters).  The two multi-pass cases use milder splines than the small ones.  With spread 1.5
# and thousands of rows the float32 element-wise kernel ITSELF is 3e-4 to 5e-3 of scale away from its own float64 evaluation on the
# steepest elements (measured: 5.2e-3 on gx of the inverse at 32 + 32 features / 9 029 rows, where this kernel is 1.9e-3 away), so
# no float32 kernel could be held to 2e-4 against it there.  The test therefore checks its own premise on those cases: the
# element-wise kernel's float32 results lie within a third of the bar of its float64 results on the same inputs.
KERNEL_CASES = [(nI, nT, B, 1.5) for nI, nT in ((4, 3), (0, 7), (7, 0), (66, 4), (3, 70)) for B in (1, 67)] + [
    (3, 70, 4613, 0.4), (32, 32, 9029, 0.4)]


@pytest.mark.parametrize("nI,nT,B,spread", KERNEL_CASES)
def test_wave_kernel_vs_elementwise_kernel(nfa, nI, nT, B, spread):
    """nf_rqs_coupling_bwd_ft_wave alone on the inputs of nf_rqs_coupling_bwd_ft, the three modes: nI = 0, nT = 0, both halves, more
    identity features than a wave has lanes (their sums go straight to workgroup LDS) and more transform features than a wave pass.
    The launch has at most 2 048 waves: 73 features at 4 613 rows (one sample per pass) and 64 features at 9 029 rows (two per pass,
    the lane-private sums) make every wave take a second and a third pass, the last one ragged -- the staging buffers are reused,
    gx is zeroed again and the lane-private sums carry over (milder random splines there, and the premise checked: KERNEL_CASES).
    Against the element-wise kernel every output within 2e-4 of scale, the bar this suite holds two float32 routes through one layer
    to (the two kernels differ in evaluation order and in hardware exp2 / rcp against libm).  One exception, which has to prove
    itself: the log-det's x-derivative jumps at a spline knot, and the two kernels round the knots differently, so an element whose
    x lies within knot rounding (tools/circ_coupled_train_bench.KNOT_ROUNDING, 4e-6 of its bound, derived there) of a knot of ITS OWN
    spline may take the other one-sided value.  Such elements are counted (at most 2 + 2e-5 of all), each must be that close to a
    knot in a float64 evaluation, their rows leave the gx / gcond comparison, and the batch-shared sums are compared only when none
    of them is an identity element.  Over two runs of the new kernel gx and gcond are bit-identical and the batch-shared parameters'
    gradients, which come through atomics, agree to 1e-5 of scale.  Canary words around every output buffer stay untouched."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import circ_coupled_train_bench as tool
    L, ops = nfa._lib, nfa.ops
    D, pad, C = nI + nT, 256, 1234.5
    t = kernel_inputs(nI, nT, B, 11 + nI, spread)
    kw = dict(tails="feature", tail_bound=1.0, wh_div=3.0, tails_t=t["tails_t"], bound_t=t["bound_t"], tails_i=t["tails_i"],
              bound_i=t["bound_i"])
    dbl = lambda v: None if v is None else v.double()      # noqa: E731

    def scale_err(a, b):
        return float((a.double() - b.double()).abs().max()) / max(1.0, float(b.abs().max())) if a.numel() else 0.0
    for mode in (L.RQS_DENSITY, L.RQS_SAMPLE_IDENTITY, L.RQS_SAMPLE_TRANSFORM):
        old = ops.rqs_coupling_bwd(t["x"], t["gy"], t["gld"], t["cond"], t["uw"], t["uh"], t["ud"], t["iidx"], t["tidx"], 8, mode, **kw)
        if B > 1000:          # the premise of the multi-pass cases (see KERNEL_CASES)
            o64 = ops.rqs_coupling_bwd(*[dbl(t[k]) for k in ("x", "gy", "gld", "cond", "uw", "uh", "ud")], t["iidx"], t["tidx"], 8, mode,
                                       **dict(kw, bound_t=dbl(t["bound_t"]), bound_i=dbl(t["bound_i"])))
            own = max(scale_err(a, b) for i, (a, b) in enumerate(zip(old, o64)) if a is not None and not (i == 1 and mode == 1))
            print("nI %d nT %d B %d mode %d: the element-wise kernel's own float32 error %.3e of scale" % (nI, nT, B, mode, own))
            assert own <= 2e-4 / 3, (mode, own)
        runs = []
        for _ in range(2):
            bufs, outs = [], []
            for n, fill in ((B * D, 0.0), (B * nT * 25, 0.0), (nI * 8, 0.0), (nI * 8, 0.0), (nI * 9, 0.0)):
                buf = torch.full((pad + n + pad,), C, device=DEV)
                buf[pad:pad + n] = fill
                bufs.append((buf, n))
                outs.append(buf[pad:pad + n] if n else None)
            L.call("nf_rqs_coupling_bwd_ft_wave", L.ptr(t["x"]), L.ptr(t["gy"]), L.ptr(t["gld"]), L.ptr(t["cond"]), L.ptr(t["uw"]),
                   L.ptr(t["uh"]), L.ptr(t["ud"]), L.ptr(t["iidx"]), nI, L.ptr(t["tidx"]), nT, B, D, 8, 3, 1.0, 1e-3, 1e-3, 1e-3, 3.0,
                   mode, *[L.ptr(o) for o in outs], 0, L.ptr(t["tails_t"]), L.ptr(t["bound_t"]), L.ptr(t["tails_i"]),
                   L.ptr(t["bound_i"]), L.stream())
            torch.cuda.synchronize()
            for buf, n in bufs:
                assert bool((buf[:pad] == C).all()) and bool((buf[pad + n:] == C).all())
            runs.append(outs)
        # elements on the other side of a knot: few, and each one shown to be within knot rounding of a knot of its own spline
        rows, cols, gaps, ident = tool.far_elements(runs[0][0].view(B, D), old[0], t["x"], t["cond"], t["uw"], t["uh"], t["iidx"],
                                                    t["tidx"], t["bound_i"], t["bound_t"], 3.0, mode != L.RQS_DENSITY, bar=2e-4)
        if rows.numel():
            print("nI %d nT %d B %d mode %d: %d element(s) beyond the bar, knot gaps %s of the bound" % (
                nI, nT, B, mode, rows.numel(), ["%.1e" % float(g) for g in gaps]))
        assert rows.numel() <= 2 + 2e-5 * B * D, rows.numel()
        assert bool((gaps <= tool.KNOT_ROUNDING).all()), (mode, rows.tolist(), cols.tolist(), gaps.tolist())
        keep = torch.ones(B, dtype=torch.bool, device=DEV)
        keep[rows] = False
        shapes = [(B, D), (B, nT * 25), (nI, 8), (nI, 8), (nI, 9)]
        for i, (a, b, ref, sh) in enumerate(zip(runs[0], runs[1], old, shapes)):
            if a is None or (i == 1 and mode == L.RQS_SAMPLE_IDENTITY):      # (gcond is not an output of the identity half's mode:
                continue                                                     # neither kernel writes it; the canaries still hold)
            assert torch.isfinite(a).all()
            if i < 2:
                assert torch.equal(a, b), (mode, i)
                e = scale_err(a.view(sh)[keep], ref.view(sh)[keep])
            else:
                assert scale_err(a, b) <= 1e-5, (mode, i, scale_err(a, b))
                if bool(ident.any()):
                    continue
                e = scale_err(a.view(sh), ref.view(sh))
            print("nI %d nT %d B %d mode %d output %d: %.3e of scale vs the element-wise kernel" % (nI, nT, B, mode, i, e))
            assert e <= 2e-4, (mode, i, e)
    # the op itself: the same results as the raw call, None never (the shapes fit)
    got = ops.rqs_coupling_bwd_ft_wave(t["x"], t["gy"], t["gld"], t["cond"], t["uw"], t["uh"], t["ud"], t["iidx"], t["tidx"], 8, 0,
                                       1.0, 1e-3, 1e-3, 1e-3, 3.0, t["tails_t"], t["bound_t"], t["tails_i"], t["bound_i"])
    assert got is not None and torch.isfinite(got[0]).all()


def test_live_parameters_and_higher_order(nfa, spy, fixtures):
    """After one fused-Adam step the next forward equals the eager route's on the CURRENT weights within 2e-4 (no stale pack, no stale
    periodic weights); inside config.higher_order_gradients() the torch modules run and create_graph=True works."""
    name = "grad_circ_cpl_d7_h40"
    layer = cases.make_layer(nfa, name, fixtures[name]).to(DEV)
    x, cz, cl = batch(layer, 7, 65, 8)
    pre = layer.prqct.transform_net.preprocessing
    opt = torch.optim.Adam(layer.parameters(), lr=3e-3, fused=True)
    before = pre.weights.detach().clone()
    step(layer, "inv", x, cz, cl)
    opt.step()
    assert not torch.equal(before, pre.weights.detach())
    for d in ("inv", "fwd"):
        got = step(layer, d, x, cz, cl)
        ref = eager(nfa, layer, d, x, cz, cl)
        assert_close(N(got[0]), N(ref[0]), what="z after the step, " + d, rtol=2e-4, atol=2e-4)
        assert_close(N(got[1]), N(ref[1]), what="ld after the step, " + d, rtol=2e-4, atol=2e-4)
        assert all(torch.isfinite(a).all() for a in got)
    reset(spy)
    with nfa.config.higher_order_gradients():
        xx = x.clone().requires_grad_(True)
        z, ld = layer.inverse(xx)
        (gx,) = torch.autograd.grad((z * cz).sum() + (ld * cl).sum(), xx, create_graph=True)
        gx.pow(2).sum().backward()
        assert torch.isfinite(xx.grad).all() and float(xx.grad.abs().max()) > 0.0
    assert all(spy[k] == 0 for k in MADE_OPS) and spy["linear"] >= 1, spy


@pytest.mark.parametrize("case", ["context", "cpu", "float64", "nI_1"])
def test_declined_calls_keep_the_eager_path(nfa, spy, fixtures, case):
    """A context, a CPU tensor, float64 and a one-column identity half each leave the four MADE training ops at zero and run the
    eager modules, with the results of the switch-off route (float64: of the reference's float64 leg)."""
    C = nfa.flows.CircularCoupledRationalQuadraticSpline
    name = "grad_circ_cpl_d7_h40"
    g = fixtures[name]
    if case == "cpu":          # the conditioner alone: the layer itself has no CPU path
        net = cases.make_layer(nfa, name, g).prqct.transform_net
        xi = torch.from_numpy(g["x"][:, ::2].copy()).requires_grad_(True)
        out = net(xi)
        out.sum().backward()
        twin = cases.make_layer(nfa, name, g).prqct.transform_net.double()
        ref = twin(xi.detach().double())
        assert_close(N(out), N(ref), rtol=1e-4, atol=1e-4, what="cpu conditioner")
        assert torch.isfinite(xi.grad).all()
    elif case == "float64":
        layer = cases.make_layer(nfa, name, g).double().to(DEV)
        got = step(layer, "inv", T(g["x"]).double(), T(g["cz"]).double(), T(g["cl"]).double())
        for k, a in zip(("z", "ld", "gx"), got):
            ref = g["%s_inv_f64" % k]
            assert float(np.abs(N(a) - ref).max()) <= 1e-9 * max(1.0, float(np.abs(ref).max())), k
        assert spy[WAVE] == 0
    else:
        torch.manual_seed(19)
        if case == "context":
            layer = C(7, 2, 40, ind_circ=[0, 2, 3, 6], num_context_channels=3, num_bins=8, tail_bound=3.0, init_identity=False).to(DEV)
            ctx, D = torch.randn(33, 3, device=DEV), 7
        else:
            layer = C(3, 2, 24, ind_circ=[1], num_bins=8, tail_bound=2.5, reverse_mask=True, init_identity=False).to(DEV)
            assert layer.prqct.identity_features.numel() == 1 and layer.prqct.transform_net.preprocessing is not None
            ctx, D = None, 3
        x, cz, cl = batch(layer, D, 33, 3)
        got = step(layer, "inv", x, cz, cl, context=ctx)
        assert spy["linear"] >= 1
        ref = eager(nfa, layer, "inv", x, cz, cl, context=ctx)
        compare(layer, D, got, ref, case)
    assert all(spy[k] == 0 for k in MADE_OPS), spy
