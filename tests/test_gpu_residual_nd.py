"""The d-dimensional Residual route on the GPU (flows/lipmlp_nd_pack.py, csrc/lipmlp_nd.hip, config.residual_nd): every density and
sampling fixture of the reference through the kernels with the fixture's own noise, the route against the torch formulas on the
same device under one seed pair at the tile edges, the router's segment boundaries, what stays on the torch formulas, and cache
invalidation.  Every test looks at which route ran (spies on the ops' calls and on the layers' torch-formula method).

Bars: z within TOL[float32]; a log-det within conftest.ld_tol(float32), with 4 x the fixture's recorded ld_floor as the absolute part
where that floor exceeds a quarter of the bar's (residual_nd_cases.ld_bar): the kernels sum forward-mode tangents, autograd
vector-Jacobian products, and the reference's own float32 error is the floor nobody can beat."""
import contextlib
import copy

import numpy as np
import pytest
import torch

import residual_nd_cases as cases
from conftest import TOL, assert_close, golden_state, ld_tol

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.dtype("float32")


@pytest.fixture(scope="module")
def nfa():
    import normflows_amd
    assert torch.cuda.is_available()
    return normflows_amd


@pytest.fixture
def calls(nfa, monkeypatch):
    """Counts of the ops' calls (with the K of every chain call) and of the layers' torch-formula method."""
    n = {"chain": 0, "apply": 0, "torch": 0, "K": [], "nres": [], "draws": []}

    def counted(key, fn, note=None):
        def wrapper(*a, **k):
            n[key] += 1
            if note is not None:
                note(a, k)
            return fn(*a, **k)
        return wrapper

    def note_chain(a, k):
        n["K"].append(a[3])
        n["nres"].append(a[4])
    monkeypatch.setattr(nfa.ops, "lipmlp_nd_chain", counted("chain", nfa.ops.lipmlp_nd_chain, note_chain))
    monkeypatch.setattr(nfa.ops, "lipmlp_nd_apply", counted("apply", nfa.ops.lipmlp_nd_apply))
    monkeypatch.setattr(nfa.flows.Residual, "_torch_pass",
                        counted("torch", nfa.flows.Residual._torch_pass, lambda a, k: n["draws"].append(a[3] if len(a) > 3 else k.get("truncation"))))
    return n


@contextlib.contextmanager
def switch(nfa, on):
    before = nfa.config.residual_nd
    nfa.config.set_residual_nd(on)
    try:
        yield
    finally:
        nfa.config.set_residual_nd(before)


@pytest.fixture(autouse=True)
def route_on(nfa):
    """config.residual_nd on (it ships off) and residual_chain on for every test of this file."""
    before = nfa.config.residual_chain
    nfa.config.set_residual_chain(True)
    with switch(nfa, True):
        yield
    nfa.config.set_residual_chain(before)


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def N(t):
    return t.detach().cpu().numpy()


_models = {}


def fixture_stack(nfa, name):
    """The fixture's model on the device (loaded once and shared: the tests that change a model build their own)."""
    if name not in _models:
        g = cases.load(name)
        m = cases.stack(nfa, name)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in golden_state(g).items()}, strict=True)
        _models[name] = (m.to(DEV), g)
    return _models[name]


def small_stack(nfa, channels=(3, 16, 3), n=1, actnorm=False, seed=77, **kw):
    """A model of its own, at the Lipschitz cap like the fixtures."""
    torch.manual_seed(seed)
    flows = []
    for _ in range(n):
        flows.append(nfa.flows.Residual(nfa.nets.LipschitzMLP(list(channels), init_zeros=False, lipschitz_const=0.9), **kw))
        if actnorm:
            flows.append(nfa.flows.ActNorm(channels[0]))
    m = nfa.NormalizingFlow(nfa.distributions.DiagGaussian(channels[0], trainable=False), flows).eval()
    cases.at_the_cap(nfa, m, torch.Generator().manual_seed(seed + 1))
    return m.to(DEV)


def rows(B, d=3, seed=5):
    return (torch.randn(B, d, generator=torch.Generator().manual_seed(seed)) * 1.5).to(DEV)


def both_close(a, b, layers=1):
    """z within TOL; the log-det within conftest.ld_tol, which is the bar of ONE layer's log-det: a SUM over `layers` Residual
    layers is held to `layers` times its absolute part (as tests/test_gpu_residual.py holds its summed log-dets), the relative
    part unchanged.  The single-layer tests -- every tile-edge case among them -- use the bar as it stands (layers = 1)."""
    assert_close(N(a[0]), N(b[0]), what="z", **TOL[F32])
    t = ld_tol(F32)
    assert_close(N(a[1]), N(b[1]), what="ld", rtol=t["rtol"], atol=layers * t["atol"])


def seeded(fn, seed=3):
    """(fn(), the next draw of both generators) after np.random.seed(seed); torch.manual_seed(seed)."""
    np.random.seed(seed)
    torch.manual_seed(seed)
    out = fn()
    return out, (np.random.rand(), float(torch.rand(1)), float(torch.rand(1, device=DEV)))


def density(m, x, inverse=True):
    with torch.no_grad():
        return m.inverse_and_log_det(x) if inverse else m.forward_and_log_det(x)


# ---- 1. the reference's fixtures through the kernels, on the fixtures' own noise ----------------------------------------------------
@pytest.mark.parametrize("name", list(cases.DENSITY))
def test_density_fixture_vs_reference(nfa, calls, name):
    from normflows_amd.flows import lipmlp_nd_pack as lp
    m, g = fixture_stack(nfa, name)
    inverse = cases.density_is_inverse(name)
    run = list(reversed(m.flows)) if inverse else list(m.flows)
    draws = cases.draws(g)
    x = T(g["x"])
    bar = cases.ld_bar(g, ld_tol(F32))
    print("%s: ld_floor %.3g, bar %s" % (name, float(g["ld_floor"]), bar))
    with torch.no_grad():
        assert lp.eligible(run, x)
        z, ld = lp.run_density_noise(run, x, T(np.stack([v for _, _, v in draws])), [t for t, _, _ in draws], [c for _, c, _ in draws],
                                     inverse=inverse)
    assert calls["chain"] == 1 and calls["K"] == [len(run)] and calls["torch"] == 0 and calls["apply"] == 0       # ONE launch
    print("  z max err %.3g, summed ld max err %.3g" % (np.abs(N(z) - g["z"]).max(), np.abs(N(ld) - g["ld"]).max()))
    assert_close(N(z), g["z"], what="z", **TOL[F32])
    assert_close(N(ld), g["ld"], what="summed ld", **bar)
    if inverse:
        with torch.no_grad():
            lp_ = m.q0.log_prob(z) + ld
        assert_close(N(lp_), g["log_prob"], what="log_prob", **bar)
    cur, k = x, 0
    with torch.no_grad():       # layer by layer: every Residual is a launch of its own (K = 1), ActNorm its own kernel
        for i, f in enumerate(run):
            if isinstance(f, nfa.flows.Residual):
                t, c, v = draws[k]
                cur, l = f._density_nd(cur, T(v), t, c)
                k += 1
            else:
                cur, l = f.inverse(cur) if inverse else f(cur)
            l = N(l * torch.ones(x.shape[0], device=DEV))
            print("  layer %d ld max err %.3g" % (i, np.abs(l - g["ld_layers"][i]).max()))
            assert_close(l, g["ld_layers"][i], what="ld of layer %d" % i, **bar)
    assert calls["K"] == [len(run)] + [1] * k and calls["torch"] == 0
    assert_close(N(cur), g["z"], what="z (layer by layer)", **TOL[F32])


@pytest.mark.parametrize("name", list(cases.SAMPLING))
def test_sampling_fixture_vs_reference(nfa, calls, name):
    from normflows_amd.flows import lipmlp_nd_pack as lp
    m, g = fixture_stack(nfa, name)
    draws = cases.draws(g)
    bar = cases.ld_bar(g, ld_tol(F32, root_finding=True))
    cur, total = T(g["x"]), 0
    with torch.no_grad():
        for k, f in enumerate(m.flows):         # reverse=True: the model's forward pass is the fixed-point direction
            t, c, v = draws[k]
            assert lp.eligible([f], cur, sampling=True)
            before = (calls["apply"], calls["chain"])
            cur, l = lp.run_sampling(f, cur, noise=(T(v), t, c))
            iters = int(g["iters"][k])
            assert lp.last_iterations == iters
            assert (calls["apply"] - before[0], calls["chain"] - before[1]) == (iters + 1, 1)       # iterations + 2 launches
            print("%s: layer %d ld max err %.3g" % (name, k, np.abs(N(l) - g["ld_layers"][k]).max()))
            assert_close(N(l), g["ld_layers"][k], what="ld of layer %d" % k, **bar)
            total = total + l
    assert calls["torch"] == 0
    assert_close(N(cur), g["z"], what="z", **TOL[F32])
    assert_close(N(total), g["ld"], what="summed ld", **bar)
    # through the model, on noise of its own: the same route, the same number of launches
    n0 = (calls["apply"], calls["chain"])
    with torch.no_grad():
        z, _ = m.forward_and_log_det(T(g["x"]))
    assert (calls["apply"] - n0[0], calls["chain"] - n0[1]) == (int(g["iters"].sum()) + len(draws), len(draws)) and calls["torch"] == 0
    assert_close(N(z), g["z"], what="z (model)", **TOL[F32])


# ---- 2. the route against the formulas on the device, one seed pair -----------------------------------------------------------------
_edge = {}


def edge_model(nfa, shape):
    if shape not in _edge:
        _edge[shape] = small_stack(nfa, channels=shape, n=1, seed=31)
    return _edge[shape]


@pytest.mark.parametrize("which", ["1", "R-1", "R", "R+1", "second tile"])
@pytest.mark.parametrize("shape", [(3, 32, 3), (64, 128, 128, 64)])
def test_route_vs_torch_formulas_at_the_tile_edges(nfa, calls, shape, which):
    m = edge_model(nfa, shape)
    d, hp = shape[0], max(shape[1:-1])
    R = nfa.ops.lipmlp_nd_rows(hp, d)
    assert R == {(3, 32): 128, (64, 128): 32}[(d, hp)]
    B = {"1": 1, "R-1": R - 1, "R": R, "R+1": R + 1,
         "second tile": nfa._lib.lib().nf_persistent_workgroups() * R + R + 3}[which]
    x = rows(B, d=d)
    got, after = seeded(lambda: density(m, x))
    assert calls["chain"] == 1 and calls["K"] == [1] and calls["torch"] == 0
    with switch(nfa, False):
        want, after_formulas = seeded(lambda: density(m, x))
    assert calls["chain"] == 1 and calls["torch"] == 1
    assert after == after_formulas                      # both generators left in the same state
    print("d %d hp %d B %d: z max err %.3g, ld max err %.3g" % (d, hp, B, (got[0] - want[0]).abs().max(), (got[1] - want[1]).abs().max()))
    both_close(got, want)


@pytest.mark.parametrize("d", [40, 41])
def test_route_vs_torch_formulas_where_the_lds_budget_halves_the_tile(nfa, calls, d):
    """hp 32: d = 40 is the last d whose 128-row tile fits the 160 KiB of LDS (exactly), d = 41 the first on 64 rows."""
    m = small_stack(nfa, channels=(d, 32, d), n=1, seed=33)
    R = nfa.ops.lipmlp_nd_rows(32, d)
    assert R == {40: 128, 41: 64}[d]
    x = rows(2 * R + 1, d=d)
    got, after = seeded(lambda: density(m, x))
    assert calls["chain"] == 1 and calls["torch"] == 0
    with switch(nfa, False):
        want, after_formulas = seeded(lambda: density(m, x))
    assert after == after_formulas and calls["torch"] == 1
    both_close(got, want)


def test_sampling_route_vs_torch_formulas(nfa, calls):
    m = edge_model(nfa, (3, 32, 3))
    x = rows(200)
    with torch.no_grad():
        (got, after) = seeded(lambda: m.forward_and_log_det(x))
        assert calls["chain"] == 1 and calls["apply"] >= 2 and calls["torch"] == 0
        with switch(nfa, False):
            (want, after_formulas) = seeded(lambda: m.forward_and_log_det(x))
    assert after == after_formulas and calls["torch"] == 1
    assert_close(N(got[0]), N(want[0]), what="z", **TOL[F32])
    assert_close(N(got[1]), N(want[1]), what="ld", **ld_tol(F32, root_finding=True))


# ---- 3. the router's segment boundaries ---------------------------------------------------------------------------------------------
def test_nine_residual_layers_split_8_and_1(nfa, calls):
    m = small_stack(nfa, channels=(5, 16, 5), n=9, seed=41)
    x = rows(70, d=5)
    got, after = seeded(lambda: density(m, x))
    assert calls["K"] == [8, 1] and calls["nres"] == [8, 1] and calls["torch"] == 0
    with switch(nfa, False):
        want, after_formulas = seeded(lambda: density(m, x))
    assert after == after_formulas and calls["torch"] == 9
    both_close(got, want, layers=9)


def test_runs_with_actnorm_and_the_cut_at_an_uninitialised_one(nfa, calls):
    m = small_stack(nfa, channels=(5, 40, 24, 5), n=2, actnorm=True, seed=42)
    x = rows(70, d=5)
    got, after = seeded(lambda: density(m, x))
    assert calls["K"] == [4] and calls["nres"] == [2] and calls["torch"] == 0
    with switch(nfa, False):
        want, after_formulas = seeded(lambda: density(m, x))
    assert after == after_formulas
    both_close(got, want, layers=2)
    calls["K"].clear()
    fresh = small_stack(nfa, channels=(5, 40, 24, 5), n=2, actnorm=True, seed=43)
    fresh.flows[1].data_dep_init_done.fill_(0.0)
    fresh.flows[1]._init_known = None
    twin = copy.deepcopy(fresh)
    got, _ = seeded(lambda: density(fresh, x))
    assert calls["K"] == [2, 1] and fresh.flows[1].initialised()       # [ActNorm, Residual], the fresh ActNorm alone, [Residual]
    with switch(nfa, False):
        want, _ = seeded(lambda: density(twin, x))
    both_close(got, want, layers=2)
    calls["K"].clear()
    density(fresh, x)
    assert calls["K"] == [4]


def test_a_stochastic_layer_is_a_boundary(nfa, calls):
    m = small_stack(nfa, channels=(4, 16, 4), n=2, seed=44, reverse=False)
    target = torch.distributions.MultivariateNormal(torch.zeros(4, device=DEV), torch.eye(4, device=DEV))
    mh = nfa.flows.MetropolisHastings(target, nfa.distributions.DiagGaussianProposal((4,), 0.1), 2).to(DEV)
    mixed = nfa.NormalizingFlow(m.q0, [m.flows[0], mh, m.flows[1]])
    x = rows(50, d=4)
    got, after = seeded(lambda: density(mixed, x, inverse=False))
    assert calls["K"] == [1, 1] and calls["torch"] == 0
    with switch(nfa, False):
        want, after_formulas = seeded(lambda: density(mixed, x, inverse=False))
    assert after == after_formulas and calls["torch"] == 2
    both_close(got, want, layers=2)


# ---- 4. what stays on the torch formulas --------------------------------------------------------------------------------------------
def test_the_switch_decides(nfa, calls):
    """With the switch on a d = 3 layer runs the new op; with it off (the default) it keeps the formulas."""
    m = small_stack(nfa)
    x = rows(40)
    assert nfa.config.residual_nd is True
    density(m, x)
    assert (calls["chain"], calls["torch"]) == (1, 0)
    with switch(nfa, False):
        density(m, x)
    assert (calls["chain"], calls["torch"]) == (1, 1)
    nfa.config.set_residual_chain(False)                # the route needs residual_chain as well
    density(m, x)
    assert (calls["chain"], calls["torch"]) == (1, 2)


def test_what_stays_on_the_torch_formulas(nfa, calls, monkeypatch):
    """Each of these takes the torch route with the switch on and gives the switch-off route's bits under the same seeds."""
    x = rows(40)

    def same_route(m, xx, grad=False, inverse=True):
        out = []
        for on in (True, False):
            np.random.seed(3)
            torch.manual_seed(3)
            with switch(nfa, on), (contextlib.nullcontext() if grad else torch.no_grad()):
                out.append(m.inverse_and_log_det(xx) if inverse else m.forward_and_log_det(xx))
        assert calls["chain"] == 0 and calls["apply"] == 0 and calls["torch"] > 0
        assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])

    same_route(small_stack(nfa).train(), x)                                                     # training mode
    same_route(small_stack(nfa, exact_trace=True), x)                                           # exact_trace
    same_route(small_stack(nfa, channels=(65, 16, 65)), rows(40, d=65))                         # d = 65
    same_route(small_stack(nfa).double(), x.double())                                           # float64
    same_route(small_stack(nfa), rows(40, d=6)[:, ::2])                                         # a strided view
    same_route(small_stack(nfa), x, grad=True)                                                  # a parameter needs a gradient
    same_route(small_stack(nfa, channels=(3, 130, 3)), x)                                       # wider than the kernels take

    class Sub(nfa.flows.Residual):
        pass
    m = small_stack(nfa)
    sub = Sub(m.flows[0].iresblock.nnet).eval().to(DEV)
    same_route(nfa.NormalizingFlow(m.q0, [sub]), x)                                             # a subclass
    frozen = small_stack(nfa)
    nfa.utils.set_requires_grad(frozen, False)
    with nfa.config.higher_order_gradients():
        same_route(frozen, x)                                                                   # higher_order_gradients()
    same_route(frozen, x.clone().requires_grad_(True), grad=True)                               # the input needs a gradient
    z, ld = frozen.inverse_and_log_det(x)                      # grad enabled, but nothing requires one: the kernels
    assert calls["chain"] == 1 and not z.requires_grad and not ld.requires_grad
    calls["chain"] = calls["torch"] = 0
    calls["draws"].clear()
    from normflows_amd.flows import residual
    monkeypatch.setattr(residual, "geometric_sample", lambda p, n_samples: np.full(n_samples, 29))
    same_route(small_stack(nfa), x)                                                             # a forced 49-term draw
    assert calls["draws"][0] is not None and calls["draws"][0][0] == 49 and calls["draws"][1] is None


# ---- 5. live parameters and buffers -------------------------------------------------------------------------------------------------
def test_cache_follows_weights_and_buffers(nfa, calls):
    from normflows_amd.flows import lipmlp_nd_pack as lp
    m = small_stack(nfa, channels=(5, 40, 24, 5), n=2, actnorm=True, seed=51)
    x = rows(70, d=5)
    run = list(reversed(m.flows))

    def check():
        got, _ = seeded(lambda: density(m, x))
        with switch(nfa, False):
            want, _ = seeded(lambda: density(m, x))
        both_close(got, want, layers=2)

    check()
    first = lp._cached_pack(run, True)
    density(m, x)
    assert lp._cached_pack(run, True) is first                                  # cached
    with torch.no_grad():
        m.flows[0].iresblock.nnet.net[1].weight.data[0, 0] += 0.5               # a .data update: invisible to the key
    nfa.invalidate_caches(m)
    check()
    second = lp._cached_pack(run, True)
    assert second is not first and not torch.equal(second[0], first[0])
    nfa.utils.update_lipschitz(m, 5)                                            # u, v change in place: no parameter is touched
    check()
    assert lp._cached_pack(run, True) is not second
