"""Residual flows on the GPU (flows/residual.py, flows/lipmlp_pack.py, csrc/lipmlp.hip): every chain and sampling fixture of the
reference through the kernels, the route against the torch formulas on the same device at the tile edges, what stays on the torch
formulas, the router's segment boundaries, cache invalidation and views.  Every test looks at which route ran (spies on the ops'
calls and on the layers' torch-formula method)."""
import contextlib
import copy

import numpy as np
import pytest
import torch

import residual_cases as cases
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
    n = {"chain": 0, "apply": 0, "torch": 0, "K": []}

    def counted(key, fn, note=None):
        def wrapper(*a, **k):
            n[key] += 1
            if note is not None:
                note(a)
            return fn(*a, **k)
        return wrapper
    monkeypatch.setattr(nfa.ops, "lipmlp_chain", counted("chain", nfa.ops.lipmlp_chain, lambda a: n["K"].append(a[2])))
    monkeypatch.setattr(nfa.ops, "lipmlp_apply", counted("apply", nfa.ops.lipmlp_apply))
    monkeypatch.setattr(nfa.flows.Residual, "_torch_pass", counted("torch", nfa.flows.Residual._torch_pass))
    return n


@pytest.fixture
def formulas(nfa):
    """Context manager factory: the torch-formula route (the switch off) for the `with` body, whatever the default is."""
    @contextlib.contextmanager
    def off():
        before = nfa.config.residual_chain
        nfa.config.set_residual_chain(False)
        try:
            yield
        finally:
            nfa.config.set_residual_chain(before)
    return off


@pytest.fixture(autouse=True)
def route_on(nfa):
    before = nfa.config.residual_chain
    nfa.config.set_residual_chain(True)
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


def small_stack(nfa, channels=(2, 32, 2), n=2, actnorm=True, seed=77, **kw):
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


def rows(B, d=2, seed=5):
    return (torch.randn(B, d, generator=torch.Generator().manual_seed(seed)) * 1.5).to(DEV)


def both_close(a, b):
    assert_close(N(a[0]), N(b[0]), what="z", **TOL[F32])
    assert_close(N(a[1]), N(b[1]), what="ld", **ld_tol(F32))


# ---- 1. the reference's fixtures through the kernels -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.CHAIN))
def test_chain_fixture_vs_reference(nfa, calls, name):
    m, g = fixture_stack(nfa, name)
    inverse = cases.density_is_inverse(name)
    x = T(g["x"])
    K = len(m.flows)
    with torch.no_grad():
        z, ld = m.inverse_and_log_det(x) if inverse else m.forward_and_log_det(x)
    assert calls["chain"] == 1 and calls["K"] == [K] and calls["torch"] == 0 and calls["apply"] == 0      # ONE launch
    assert_close(N(z), g["z"], what="z", **TOL[F32])
    # the sum of K per-layer log-dets, each held at ld_tol: K times its absolute part
    t = ld_tol(F32)
    assert_close(N(ld), g["ld"], what="summed ld", rtol=t["rtol"], atol=K * t["atol"])
    with torch.no_grad():       # layer by layer: every Residual is a launch of its own (K = 1), ActNorm its own kernel
        zz, lds = cases.walk(list(m.flows), x, inverse)
    assert calls["K"] == [K] + [1] * cases.STACKS[name][1] and calls["torch"] == 0
    assert_close(N(zz), g["z"], what="z (layer by layer)", **TOL[F32])
    for i, l in enumerate(lds):
        assert_close(N(l), g["ld_layers"][i], what="ld of layer %d" % i, **ld_tol(F32))
    if inverse:
        with torch.no_grad():
            lp = N(m.log_prob(x))
        err = np.max(np.abs(lp - g["log_prob"]) / np.maximum(1.0, np.abs(g["log_prob"])))
        print("%s: log_prob max rel err %.3e" % (name, err))
        assert err < 1e-4 and calls["torch"] == 0


@pytest.mark.parametrize("name", list(cases.SAMPLING))
def test_sampling_fixture_vs_reference(nfa, calls, name):
    from normflows_amd.flows import lipmlp_pack as lp
    m, g = fixture_stack(nfa, name)
    x = T(g["x"])
    iters, k = [], 0
    cur = x
    with torch.no_grad():
        for f in m.flows:                # reverse=True: the model's forward pass is the fixed-point direction
            y = cur
            cur, l = f(cur)
            if isinstance(f, nfa.flows.Residual):
                iters.append(lp.last_iterations)
                # the point found solves x + g(x) = y to the stop rule's tolerance, judged in float64
                f64 = copy.deepcopy(f).double()
                with formulas_off(nfa):
                    back = cur.double() + f64.iresblock.nnet(cur.double())
                res = ((back - y.double()) ** 2).sum(1)
                bound = (lp.ATOL + y.double().abs() * lp.RTOL).sum(1)
                assert bool((res < bound).all()), float((res / bound).max())
            assert_close(N(l * torch.ones(x.shape[0], device=DEV)), g["ld_layers"][k], what="ld of layer %d" % k, **ld_tol(F32))
            k += 1
    nres = cases.STACKS[name][1]
    assert iters == g["iters"].tolist()
    assert calls["torch"] == 0 and calls["apply"] == sum(iters) + nres and calls["K"] == [1] * nres
    assert_close(N(cur), g["z"], what="z", **TOL[F32])
    calls["K"].clear()
    with torch.no_grad():                # through the container: the same route
        z, ld = m.forward_and_log_det(x)
    assert calls["torch"] == 0 and calls["K"] == [1] * nres
    assert torch.equal(z, cur)
    t = ld_tol(F32)
    assert_close(N(ld), g["ld"], what="summed ld", rtol=t["rtol"], atol=len(m.flows) * t["atol"])


@contextlib.contextmanager
def formulas_off(nfa):
    before = nfa.config.residual_chain
    nfa.config.set_residual_chain(False)
    try:
        yield
    finally:
        nfa.config.set_residual_chain(before)


# ---- 2. route on against route off at the tile edges --------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [0, 1, 128, 129, 256 * 128 + 128 + 5])
def test_route_vs_torch_formulas_at_the_tile_edges(nfa, calls, formulas, B):
    """hp = 32: 128 rows per tile; the last size gives 258 tiles to at most 256 persistent workgroups (a second round)."""
    assert nfa._lib.lib().nf_lipmlp_rows(32) == 128 and nfa._lib.lib().nf_persistent_workgroups() == 256
    m = small_stack(nfa, n=1)
    x = rows(B)
    with torch.no_grad():
        got = m.inverse_and_log_det(x)
    assert calls["K"] == [2] and calls["torch"] == 0
    with formulas(), torch.no_grad():
        want = m.inverse_and_log_det(x)
    assert calls["torch"] == 1 and calls["chain"] == 1
    assert got[0].shape == (B, 2) and got[1].shape == (B,)
    both_close(got, want)
    if B in (1, 129):                  # the fixed-point direction at a ragged tile
        with torch.no_grad():
            s_got = m.forward_and_log_det(x)
        with formulas(), torch.no_grad():
            s_want = m.forward_and_log_det(x)
        assert calls["apply"] >= 1 and calls["torch"] == 2
        both_close(s_got, s_want)


@pytest.mark.parametrize("channels", [(2, 64, 2), (2, 128, 2), (2, 96, 7, 2)])
def test_other_widths_vs_torch_formulas(nfa, calls, formulas, channels):
    """One full tile plus one row at hp = 64 (64 rows) and hp = 128 (32 rows), and a network whose widths differ."""
    hp = 64 if max(channels[1:-1]) <= 64 else 128
    B = 4096 // hp + 1
    m = small_stack(nfa, channels=channels, n=2)
    x = rows(B)
    with torch.no_grad():
        got = m.inverse_and_log_det(x)
    with formulas(), torch.no_grad():
        want = m.inverse_and_log_det(x)
    assert calls["K"] == [4] and calls["torch"] == 2
    both_close(got, want)


# ---- 3. segment boundaries and what stays on the torch formulas --------------------------------------------------------------------
def test_runs_around_other_layers_and_the_cut_at_32(nfa, calls, formulas):
    torch.manual_seed(11)
    m = small_stack(nfa, n=2)
    planar = nfa.flows.Planar((2,), act="leaky_relu").to(DEV)
    mixed = nfa.NormalizingFlow(m.q0, list(m.flows[:2]) + [planar] + list(m.flows[2:]))
    x = rows(70)
    with torch.no_grad():
        got = mixed.inverse_and_log_det(x)
    assert calls["K"] == [2, 2] and calls["torch"] == 0
    with formulas(), torch.no_grad():
        want = mixed.inverse_and_log_det(x)
    assert calls["torch"] == 2
    both_close(got, want)
    calls["K"].clear()
    long = small_stack(nfa, n=17, seed=12)             # 34 records: 32 and 2
    with torch.no_grad():
        got = long.inverse_and_log_det(x)
    assert calls["K"] == [32, 2]
    with formulas(), torch.no_grad():
        want = long.inverse_and_log_det(x)
    assert_close(N(got[0]), N(want[0]), what="z", **TOL[F32])
    t = ld_tol(F32)
    assert_close(N(got[1]), N(want[1]), what="ld", rtol=t["rtol"], atol=34 * t["atol"])
    calls["K"].clear()
    fresh = small_stack(nfa, n=2, seed=13)             # an ActNorm that still has to initialise itself from the batch cuts the run
    fresh.flows[1].data_dep_init_done.fill_(0.0)
    fresh.flows[1]._init_known = None
    twin = copy.deepcopy(fresh)
    with torch.no_grad():
        got = fresh.inverse_and_log_det(x)
    assert calls["K"] == [2, 1] and fresh.flows[1].initialised()       # [ActNorm, Residual], the fresh ActNorm alone, [Residual]
    with formulas(), torch.no_grad():
        want = twin.inverse_and_log_det(x)
    both_close(got, want)


def test_what_stays_on_the_torch_formulas(nfa, calls, formulas):
    """Each of these takes the torch route and gives the torch route's numbers (bit for bit: it IS the same route; the stochastic
    ones under the same seeds)."""
    x = rows(40)

    def same_route(m, xx, grad=False, seeded=False):
        out = []
        for off in (False, True):
            if seeded:
                np.random.seed(3)
                torch.manual_seed(3)
            with (formulas() if off else contextlib.nullcontext()), (contextlib.nullcontext() if grad else torch.no_grad()):
                out.append(m.inverse_and_log_det(xx))
        assert calls["chain"] == 0 and calls["apply"] == 0 and calls["torch"] > 0
        assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])

    same_route(small_stack(nfa, channels=(3, 16, 3), n=1, actnorm=False), rows(40, d=3), seeded=True)     # d = 3
    same_route(small_stack(nfa, n=1).train(), x, seeded=True)                                         # training, no brute_force
    same_route(small_stack(nfa, n=1), x, grad=True)                                                   # a parameter needs a gradient
    wide = small_stack(nfa, channels=(2, 130, 2), n=1)                                                # wider than the kernels take
    same_route(wide, x)

    class Sub(nfa.flows.Residual):
        pass
    m = small_stack(nfa, n=1)
    sub = Sub(m.flows[0].iresblock.nnet).eval().to(DEV)
    same_route(nfa.NormalizingFlow(m.q0, [sub, m.flows[1]]), x)                                       # a subclass
    m64 = small_stack(nfa, n=1).double()
    same_route(m64, x.double())                                                                       # float64
    frozen = small_stack(nfa, n=1)
    nfa.utils.set_requires_grad(frozen, False)
    z, ld = frozen.inverse_and_log_det(x)                      # grad enabled, but nothing requires one: the kernels
    assert calls["chain"] == 1 and not z.requires_grad
    xg = x.clone().requires_grad_(True)
    frozen.inverse_and_log_det(xg)                             # the input does
    assert calls["chain"] == 1
    with nfa.config.higher_order_gradients(), torch.no_grad():
        frozen.inverse_and_log_det(x)
    assert calls["chain"] == 1


# ---- 4. live parameters and buffers ------------------------------------------------------------------------------------------------
def test_cache_follows_buffers_optimizer_steps_and_state_dicts(nfa, calls, formulas):
    m = small_stack(nfa, channels=(2, 40, 24, 2), n=2)
    x = rows(70)

    def routed_equals_formulas():
        with torch.no_grad():
            got = m.inverse_and_log_det(x)
        with formulas(), torch.no_grad():
            want = m.inverse_and_log_det(x)
        both_close(got, want)
        return got

    a = routed_equals_formulas()
    with torch.no_grad():
        assert torch.equal(m.inverse_and_log_det(x)[0], a[0])
        for mod in m.modules():            # off the cap's fixed point: the next power iterations move u, v and sigma
            if isinstance(mod, nfa.nets.InducedNormLinear):
                mod.u.copy_(torch.nn.functional.normalize(mod.u + 0.5 * torch.randn_like(mod.u), dim=0))
    b0 = routed_equals_formulas()
    nfa.utils.update_lipschitz(m, 5)       # buffers only
    b = routed_equals_formulas()
    assert not torch.equal(b[0], b0[0]) and not torch.equal(b0[0], a[0])
    opt = torch.optim.Adam(m.parameters(), lr=0.05, fused=True)
    z, ld = m.inverse_and_log_det(x)       # grad enabled: the torch formulas, differentiable
    (z.sum() + ld.sum()).backward()
    opt.step()                             # fused: Tensor._version stays
    c = routed_equals_formulas()
    assert not torch.equal(c[0], b[0])
    other = small_stack(nfa, channels=(2, 40, 24, 2), n=2, seed=78)
    m.load_state_dict(other.state_dict())
    d = routed_equals_formulas()
    with torch.no_grad():
        assert torch.equal(d[0], other.inverse_and_log_det(x)[0])
    assert calls["torch"] > 0 and calls["chain"] > 0


# ---- 5. views -----------------------------------------------------------------------------------------------------------------------
def test_views(nfa, calls):
    m = small_stack(nfa, n=1, actnorm=False)
    x = rows(70)
    with torch.no_grad():
        want = m.inverse_and_log_det(x)
    assert calls["chain"] == 1
    big = torch.zeros(70, 5, device=DEV)
    big[:, 1:3] = x
    strided = big[:, 1:3]                                      # rows 20 bytes apart: the torch formulas
    flat = torch.zeros(2 * 70 + 3, device=DEV)
    flat[3:] = x.reshape(-1)
    offset = flat[3:].view(70, 2)                              # contiguous, 12 bytes into its storage: the kernels
    with torch.no_grad():
        got_s = m.inverse_and_log_det(strided)
        assert calls["chain"] == 1 and calls["torch"] == 1
        got_o = m.inverse_and_log_det(offset)
        assert calls["chain"] == 2 and calls["torch"] == 1
    both_close(got_s, want)
    assert torch.equal(got_o[0], want[0]) and torch.equal(got_o[1], want[1])
    assert torch.equal(strided, x) and torch.equal(offset, x)


def test_a_blob_off_a_16_byte_boundary_gives_the_same_bits(nfa):
    """The packer's blobs are 16-byte aligned; a blob that is a view 4 bytes into a larger buffer takes the kernels' 4-byte weight
    loads: the same arithmetic, the same bits, at every padded width."""
    from normflows_amd.flows import lipmlp_pack as lp
    for channels in ((2, 32, 2), (2, 40, 24, 2), (2, 128, 128, 128, 2)):
        m = small_stack(nfa, channels=channels, n=1)
        run = list(reversed(m.flows))
        blob, hp, nres = lp.pack(run, True)
        moved = torch.zeros(blob.numel() + 1, device=DEV)
        moved[1:] = blob
        assert blob.data_ptr() % 16 == 0 and moved[1:].data_ptr() % 16 == 4
        x = rows(4096 // hp + 3)
        a = nfa.ops.lipmlp_chain(x, blob, 2, nres, hp)
        b = nfa.ops.lipmlp_chain(x, moved[1:], 2, nres, hp)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        one, _, _ = lp.pack([m.flows[0]], False)
        moved = torch.zeros(one.numel() + 1, device=DEV)
        moved[1:] = one
        cnt = torch.zeros(2, dtype=torch.int32, device=DEV)
        c = nfa.ops.lipmlp_apply(x, x, one, hp, 1, cnt[0:1])
        d = nfa.ops.lipmlp_apply(x, x, moved[1:], hp, 1, cnt[1:2])
        assert torch.equal(c, d) and int(cnt[0]) == int(cnt[1]) > 0
        assert torch.equal(nfa.ops.lipmlp_apply(x, None, one, hp, 0), nfa.ops.lipmlp_apply(x, None, moved[1:], hp, 0))


def test_capture_and_replay(nfa, calls):
    """The density launch is capturable (a cached pack: no allocation from host memory, no synchronisation); the fixed-point route
    synchronises and is not taken during capture."""
    m = small_stack(nfa, n=2)
    x = rows(300)
    with torch.no_grad():
        want = m.inverse_and_log_det(x)
        static = x.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            m.inverse_and_log_det(static)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = m.inverse_and_log_det(static)
        static.copy_(x.flip(0))
        graph.replay()
        torch.cuda.synchronize()
    assert torch.equal(out[0], want[0].flip(0)) and torch.equal(out[1], want[1].flip(0))
    assert calls["torch"] == 0
