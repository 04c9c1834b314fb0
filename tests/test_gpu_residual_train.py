"""Training of 2-D Residual layers on the GPU (csrc/lipmlp_train.hip, autograd.LipMlpTrainFn, flows/lipmlp_pack.py): every training
fixture of the reference and the eight d = 2 estimator fixtures through the kernels, the route against the torch formulas under one
seed, the second tile of a persistent workgroup, repeatability, frozen networks, what stays on the formulas, and a captured step.
Every test looks at which route ran (spies on the ops' calls and on the layers' torch-formula method).

The fixtures were drawn on the CPU: `cpu_noise` makes torch.randn_like draw from the CPU generator on both routes."""
import contextlib

import numpy as np
import pytest
import torch

import residual_cases as cases
import residual_train_cases as tc
from conftest import TOL, assert_close, ld_tol
from test_host_rank1 import grads_close
from test_host_residual_train import EST_2D

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
    """Counts of the new ops' calls (with the backward's slab request) and of the layers' torch-formula method."""
    n = {"fwd": 0, "bwd": 0, "want": [], "torch": 0}
    fwd, bwd, tp = nfa.ops.lipmlp_train_fwd, nfa.ops.lipmlp_train_bwd, nfa.flows.Residual._torch_pass

    def cfwd(*a, **k):
        n["fwd"] += 1
        return fwd(*a, **k)

    def cbwd(x, gy, jhat, w, blob, hp, want_gblob, want_gx=True):
        n["bwd"] += 1
        n["want"].append(bool(want_gblob))
        return bwd(x, gy, jhat, w, blob, hp, want_gblob, want_gx)

    def ctp(self, z, density, *a):
        n["torch"] += 1
        return tp(self, z, density, *a)
    monkeypatch.setattr(nfa.ops, "lipmlp_train_fwd", cfwd)
    monkeypatch.setattr(nfa.ops, "lipmlp_train_bwd", cbwd)
    monkeypatch.setattr(nfa.flows.Residual, "_torch_pass", ctp)
    return n


@pytest.fixture(autouse=True)
def route_on(nfa):
    before = nfa.config.residual_train, nfa.config.residual_chain
    nfa.config.set_residual_train(True)
    nfa.config.set_residual_chain(True)
    yield
    nfa.config.set_residual_train(before[0])
    nfa.config.set_residual_chain(before[1])


@pytest.fixture
def formulas(nfa):
    """Context manager factory: the switch off (the parent's behaviour, the reference's arithmetic) for the `with` body."""
    @contextlib.contextmanager
    def off():
        nfa.config.set_residual_train(False)
        try:
            yield
        finally:
            nfa.config.set_residual_train(True)
    return off


@pytest.fixture
def cpu_noise(monkeypatch):
    monkeypatch.setattr(torch, "randn_like", lambda x: torch.randn(x.shape, dtype=x.dtype).to(x.device))


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def N(t):
    return t.detach().cpu().numpy()


def step(f, g, dtype=torch.float32):
    """One seeded step of layer f on fixture g's inputs: {z, ld, gx, every parameter gradient, the three buffers}."""
    seed = int(g["seed"])
    f.zero_grad(set_to_none=True)
    xx = T(g["x"]).to(dtype).requires_grad_(True)
    np.random.seed(seed)
    torch.manual_seed(seed)
    z, ld = tc.density(f, xx)
    ((z * T(g["cz"]).to(dtype)).sum() + (ld * T(g["cl"]).to(dtype)).sum()).backward()
    out = {"z": N(z), "ld": N(ld), "gx": N(xx.grad)}
    out.update({"g__" + k.replace(".", "__"): N(p.grad) for k, p in f.named_parameters() if p.grad is not None})
    out.update({b: N(getattr(f.iresblock, b)) for b in ("last_n_samples", "last_firmom", "last_secmom")})
    return out


def same_step(got, ref, min_grads):
    """The bars of this file: z to TOL, ld and the moment buffers to ld_tol, every gradient to grads_close, the drawn n equal."""
    assert got["ld"].shape == (got["z"].shape[0],)
    assert_close(got["z"], ref["z"], what="z", **TOL[F32])
    assert_close(got["ld"], ref["ld"], what="ld", **ld_tol(F32))
    keys = sorted(k for k in got if k == "gx" or k.startswith("g__"))
    assert keys == sorted(k for k in ref if k == "gx" or k.startswith("g__"))
    assert len(keys) >= 1 + min_grads
    for k in keys:
        grads_close(got[k], ref[k], k)
    assert np.array_equal(got["last_n_samples"], ref["last_n_samples"])
    for b in ("last_firmom", "last_secmom"):
        assert_close(got[b], ref[b], what=b, **ld_tol(F32))


def fixture_layer(nfa, name, est=False):
    g = cases.load("est_" + name) if est else tc.load(name)
    f = cases.estimator_layer(nfa, name) if est else tc.layer(nfa, name).flows[0]
    f.load_state_dict(tc.state(g), strict=True)
    return f.to(DEV), g


def small_layer(nfa, channels=(2, 32, 2), seed=77, **kw):
    torch.manual_seed(seed)
    f = nfa.flows.Residual(nfa.nets.LipschitzMLP(list(channels), init_zeros=False, lipschitz_const=0.9), **kw)
    m = nfa.NormalizingFlow(nfa.distributions.DiagGaussian(2, trainable=False), [f])
    cases.at_the_cap(nfa, m, torch.Generator().manual_seed(seed + 1))
    return f.to(DEV).train()


def rows(B, d=2, seed=5):
    return (torch.randn(B, d, generator=torch.Generator().manual_seed(seed)) * 1.5).to(DEV)


# ---- 1. the reference's fixtures through the kernels, and the two routes under one seed -----------------------------------------------
def both_routes(nfa, calls, formulas, f, g, min_grads):
    got = step(f, g)
    assert calls["fwd"] == 1 and calls["bwd"] == 1 and calls["want"] == [True] and calls["torch"] == 0
    same_step(got, g, min_grads)
    with formulas():
        off = step(f, g)
    assert calls["fwd"] == 1 and calls["bwd"] == 1 and calls["torch"] == 1
    same_step(got, off, min_grads)


@pytest.mark.parametrize("name", list(tc.LAYERS))
def test_training_fixture_vs_reference(nfa, calls, formulas, cpu_noise, name):
    f, g = fixture_layer(nfa, name)
    both_routes(nfa, calls, formulas, f, g, 3 * (len(tc.LAYERS[name][0]) - 1))


@pytest.mark.parametrize("name", EST_2D)
def test_estimator_fixture_vs_reference(nfa, calls, formulas, cpu_noise, name):
    f, g = fixture_layer(nfa, name, est=True)
    both_routes(nfa, calls, formulas, f, g, 9)


def test_stack_through_forward_kld_vs_reference(nfa, calls, cpu_noise):
    """3 x [Residual, ActNorm] in training mode: the loss (six per-layer log-dets, each at ld_tol) and every parameter's gradient."""
    g = tc.load(tc.STACK)
    m = tc.stack(nfa)
    m.load_state_dict(tc.state(g), strict=True)
    m = m.to(DEV)
    np.random.seed(int(g["seed"]))
    torch.manual_seed(int(g["seed"]))
    loss = m.forward_kld(T(g["x"]))
    loss.backward()
    assert calls["fwd"] == 3 and calls["bwd"] == 3 and calls["want"] == [True] * 3 and calls["torch"] == 0
    t = ld_tol(F32)
    assert_close(N(loss), g["loss"], what="loss", rtol=t["rtol"], atol=6 * t["atol"])
    n = 0
    for k, p in m.named_parameters():
        key = "g__" + k.replace(".", "__")
        assert (p.grad is None) == (key not in g), k
        if p.grad is not None:
            grads_close(N(p.grad), g[key], k)
            n += 1
    assert n == 3 * 6 + 3 * 2


# ---- 2. tiles ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [(2, 32, 2), (2, 128, 128, 2)])
def test_second_tile_of_a_persistent_workgroup(nfa, calls, formulas, channels):
    """More row tiles than workgroups, the last one ragged, against the formulas in float64 on the same device."""
    f = small_layer(nfa, channels, brute_force=True)
    hp = nfa.ops.lipmlp_width(max(channels[1:-1]))
    r = nfa.ops.lipmlp_train_rows(hp)
    B = nfa._lib.query("nf_persistent_workgroups") * r + r + 3
    x = rows(B)
    gen = torch.Generator().manual_seed(9)
    cz, cl = torch.randn(B, 2, generator=gen).to(DEV), torch.randn(B, generator=gen).to(DEV)

    def run(layer, dt):
        layer.zero_grad(set_to_none=True)
        xx = x.detach().clone().to(dt).requires_grad_(True)
        z, ld = layer.inverse(xx)
        ((z * cz.to(dt)).sum() + (ld * cl.to(dt)).sum()).backward()
        out = {"z": N(z), "ld": N(ld), "gx": N(xx.grad)}
        out.update({k: N(p.grad) for k, p in layer.named_parameters() if p.grad is not None})
        return out
    got = run(f, torch.float32)
    assert calls["fwd"] == 1 and calls["bwd"] == 1 and calls["torch"] == 0
    import copy
    with formulas():
        ref = run(copy.deepcopy(f).double(), torch.float64)
    assert calls["torch"] == 1
    assert_close(got["z"], ref["z"], what="z", **TOL[F32])
    assert_close(got["ld"], ref["ld"], what="ld", **ld_tol(F32))
    assert sorted(got) == sorted(ref) and len(got) == 3 + 3 * (len(channels) - 1)
    for k in got:
        if k not in ("z", "ld"):
            grads_close(got[k], ref[k], k)


@pytest.mark.parametrize("name", ["brute_h32", "neumann_h128x2", "basic_h40x24"])
def test_expanded_and_strided_cotangents(nfa, calls, formulas, cpu_noise, name):
    """loss = z.sum() + ld.sum() hands the backward stride-0 cotangents; z.t() a transposed one: both routes, one seed.  The
    kernel must see every copied cotangent's own values (the copies live until the launch is enqueued)."""
    f, g = fixture_layer(nfa, name)
    wt = T(g["cz"]).t().contiguous()

    def run(loss):
        f.zero_grad(set_to_none=True)
        xx = T(g["x"]).requires_grad_(True)
        np.random.seed(int(g["seed"]))
        torch.manual_seed(int(g["seed"]))
        z, ld = tc.density(f, xx)
        loss(z, ld).backward()
        out = {"gx": N(xx.grad)}
        out.update({k: N(p.grad) for k, p in f.named_parameters() if p.grad is not None})
        return out
    row = torch.tensor([[2.0, -3.0]], device=DEV)
    for loss in (lambda z, ld: z.sum() + ld.sum(), lambda z, ld: (z.t() * wt).sum() + ld.sum(),
                 lambda z, ld: (z * row).sum() + 0.5 * ld.sum()):       # (two expanded cotangents of different values)
        before = calls["bwd"], calls["torch"]
        got = run(loss)
        assert (calls["bwd"], calls["torch"]) == (before[0] + 1, before[1])
        with formulas():
            ref = run(loss)
        assert (calls["bwd"], calls["torch"]) == (before[0] + 1, before[1] + 1)
        assert sorted(got) == sorted(ref) and len(got) >= 7
        for k in got:
            grads_close(got[k], ref[k], k)


def test_the_same_step_twice_gives_the_same_bits(nfa, calls, cpu_noise):
    f, g = fixture_layer(nfa, "neumann_h128x2")
    a, b = step(f, g), step(f, g)
    assert calls["fwd"] == 2 and calls["bwd"] == 2
    for k in a:
        assert np.array_equal(a[k], b[k]), k


# ---- 3. frozen networks ------------------------------------------------------------------------------------------------------------------
def test_frozen_network_and_frozen_beta(nfa, calls, formulas, cpu_noise):
    f, g = fixture_layer(nfa, "basic_h40x24")
    with formulas():
        ref = step(f, g)
    for p in f.parameters():
        p.requires_grad_(False)
    got = step(f, g)
    assert calls["fwd"] == 1 and calls["bwd"] == 1 and calls["want"] == [False]           # no slab, no reduction
    assert all(p.grad is None for p in f.parameters())
    grads_close(got["gx"], ref["gx"], "gx")
    assert_close(got["ld"], ref["ld"], what="ld", **ld_tol(F32))
    for k, p in f.named_parameters():
        p.requires_grad_(not k.endswith("beta"))
    got = step(f, g)
    assert calls["want"] == [False, True]
    for k, p in f.named_parameters():
        key = "g__" + k.replace(".", "__")
        if k.endswith("beta") or key not in ref:
            assert p.grad is None, k
        else:
            grads_close(got[key], ref[key], k)
    grads_close(got["gx"], ref["gx"], "gx")


# ---- 4. what stays on the torch formulas ---------------------------------------------------------------------------------------------------
def test_what_takes_the_formulas(nfa, calls):
    f = small_layer(nfa)
    x = rows(9)
    f.inverse(x)
    assert (calls["fwd"], calls["torch"]) == (1, 0)
    # B = 0 (on the exact determinant: the series estimators' formulas refuse an empty batch, in the reference too)
    small_layer(nfa, brute_force=True).inverse(rows(0).requires_grad_(True))
    f.inverse(rows(9, 4)[:, ::2])                                       # a strided view
    assert (calls["fwd"], calls["torch"]) == (1, 2)
    f.forward(x)                                                        # the fixed-point direction (reverse=True)
    assert (calls["fwd"], calls["torch"]) == (1, 3)
    with nfa.config.higher_order_gradients():
        f.inverse(x)
    assert (calls["fwd"], calls["torch"]) == (1, 4)
    import copy
    copy.deepcopy(f).double().inverse(x.double())                       # float64
    assert (calls["fwd"], calls["torch"]) == (1, 5)
    torch.manual_seed(1)
    f3 = nfa.flows.Residual(nfa.nets.LipschitzMLP([3, 16, 3], init_zeros=False)).to(DEV).train()
    f3.inverse(rows(9, 3))                                              # d = 3
    assert (calls["fwd"], calls["torch"]) == (1, 6)

    class Sub(nfa.flows.Residual):
        pass
    sub = Sub(nfa.nets.LipschitzMLP([2, 16, 2], init_zeros=False)).to(DEV).train()
    sub.inverse(x)
    assert (calls["fwd"], calls["bwd"], calls["torch"]) == (1, 0, 7)


def test_with_the_switch_off_nothing_calls_the_new_ops(nfa, calls, formulas, cpu_noise):
    assert nfa.config.residual_train is True        # (this file's fixture; the package's default is off:)
    import importlib
    src = open(importlib.import_module("normflows_amd.config").__file__).read()
    assert "\nresidual_train = False\n" in src
    f, g = fixture_layer(nfa, "neumann_h128x2")
    with formulas():
        step(f, g)
        f.eval()
        step(f, g)
        with torch.no_grad():
            f.train().inverse(T(g["x"]))
    assert calls["fwd"] == 0 and calls["bwd"] == 0 and calls["torch"] >= 2


# ---- 5. a captured step ----------------------------------------------------------------------------------------------------------------------
def test_a_captured_brute_force_step_replays_the_eager_bits(nfa, calls):
    f = small_layer(nfa, (2, 40, 24, 2), brute_force=True)
    params = [p for k, p in f.named_parameters() if "nnet" in k]
    x = rows(300)

    def fwd_bwd(xx):
        z, ld = f.inverse(xx)
        return (z, ld) + torch.autograd.grad((z * z).sum() + ld.sum(), [xx] + params)
    want = [t.detach().clone() for t in fwd_bwd(x.flip(0).requires_grad_(True))]
    static = x.clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fwd_bwd(static)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fwd_bwd(static)
    with torch.no_grad():
        static.copy_(x.flip(0))
    graph.replay()
    torch.cuda.synchronize()
    assert calls["fwd"] == 3 and calls["bwd"] == 3 and calls["torch"] == 0
    for a, b in zip(out, want):
        assert torch.equal(a, b)
