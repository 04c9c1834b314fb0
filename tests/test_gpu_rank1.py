"""GPU tests of the Planar / Radial flows on the rank-1 chain kernels (csrc/rank1_chain.hip, flows/rank1_pack.py,
autograd.Rank1ChainFn): against the reference's fixtures (tests/golden/rank1_*.npz), against the torch-formula route with the switch
off, and the route's own contracts (persistent loop, determinism, frozen parameters, accumulation, live parameters, router
boundaries, views, capture)."""
import contextlib
import math

import numpy as np
import pytest
import torch

import rank1_cases as cases
from conftest import TOL, assert_close, golden_state, ld_tol, load_golden

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
    """Counts of the ops' calls (with the K of every call and the backward's flags) and of the layers' torch-formula methods."""
    n = {"chain": 0, "fwd": 0, "bwd": 0, "torch": 0, "K": [], "bwd_flags": []}

    def counted(key, fn, note=None):
        def wrapper(*a, **k):
            n[key] += 1
            if note is not None:
                note(a)
            return fn(*a, **k)
        return wrapper
    monkeypatch.setattr(nfa.ops, "rank1_chain", counted("chain", nfa.ops.rank1_chain, lambda a: n["K"].append(a[1].shape[0])))
    monkeypatch.setattr(nfa.ops, "rank1_chain_train_fwd",
                        counted("fwd", nfa.ops.rank1_chain_train_fwd, lambda a: n["K"].append(a[1].shape[0])))
    monkeypatch.setattr(nfa.ops, "rank1_chain_bwd",
                        counted("bwd", nfa.ops.rank1_chain_bwd, lambda a: n["bwd_flags"].append((bool(a[7]), bool(a[8])))))
    for cls, names in ((nfa.flows.Planar, ("_torch_forward", "_torch_inverse")), (nfa.flows.Radial, ("_torch_forward",))):
        for name in names:
            monkeypatch.setattr(cls, name, counted("torch", getattr(cls, name)))
    return n


def counts(n):
    return {k: n[k] for k in ("chain", "fwd", "bwd", "torch")}


@pytest.fixture
def formulas(nfa):
    """Context manager factory: the torch-formula route (the switch off) for the `with` body."""
    @contextlib.contextmanager
    def off():
        nfa.config.set_rank1_chain(False)
        try:
            yield
        finally:
            nfa.config.set_rank1_chain(True)
    return off


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def N(t):
    return t.detach().cpu().numpy()


def fixture_model(nfa, name):
    g = load_golden("rank1_" + name)
    m = cases.model(nfa, name)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in golden_state(g).items()}, strict=True)
    return m.to(DEV), g


def random_model(nfa, codes, shape, seed=5):
    """Layers `codes` (rank1_cases) on `shape`, perturbed like the fixtures: p += 0.3 randn except Radial's beta."""
    torch.manual_seed(seed)
    flows = cases.layers(nfa, codes, shape)
    m = nfa.NormalizingFlow(nfa.distributions.DiagGaussian(math.prod(shape), trainable=False), flows)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for k, p in m.named_parameters():
            if not k.endswith(".beta"):
                p.add_(0.3 * torch.randn(p.shape, generator=g))
    return m.to(DEV)


def batch(B, shape, seed=11):
    """x, and cotangents of one sign (0.5 .. 1.5), as a likelihood gives: with random signs a gradient summed over many rows can
    cancel to float32 noise, and "of scale" then measures the noise of either route."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn((B,) + tuple(shape), generator=g) * 1.2).to(DEV)
    return x, (0.5 + torch.rand(x.shape, generator=g)).to(DEV), (0.5 + torch.rand(B, generator=g)).to(DEV)


def step(m, x, inverse=False, cz=None, cl=None, zero=True, x_grad=True):
    """One pass + backward of sum(z * cz) + sum(ld * cl) (ones by default): (z, ld, gx, [gradient or None of every flow parameter])."""
    if zero:
        m.zero_grad(set_to_none=True)
    xx = x.detach().clone().requires_grad_(x_grad) if x.is_contiguous() else x.detach().requires_grad_(x_grad)
    z, ld = m.inverse_and_log_det(xx) if inverse else m.forward_and_log_det(xx)
    ((z if cz is None else z * cz).sum() + (ld if cl is None else ld * cl).sum()).backward()
    return z.detach(), ld.detach(), xx.grad, [None if p.grad is None else p.grad.detach().clone() for p in m.flows.parameters()]


def of_scale(got, ref):
    got, ref = got.detach().double(), ref.detach().double()
    return float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)


def assert_grads_of_scale(got, ref, bar, what):
    assert len(got) == len(ref) > 0
    for k, (a, b) in enumerate(zip(got, ref)):
        assert (a is None) == (b is None), (what, k)
        if a is not None:
            e = of_scale(a, b)
            print("%s parameter %d: %.3e of scale (bar %.1e)" % (what, k, e, bar))
            assert e <= bar, (what, k, e)


# ---- 1. every fixture against the reference ---------------------------------------------------------------------------------------
FIXTURE_LEGS = [(name, d) for name in cases.CASES for d in cases.directions(name)]


@pytest.mark.parametrize("name,dname", FIXTURE_LEGS)
def test_fixture_vs_reference(nfa, calls, name, dname):
    """no_grad: z and log-det at the parity bars, the whole model ONE nf_rank1_chain call.  Autograd: gx and every parameter gradient
    within max(1e-3 of scale, 4 x the reference's own float32-vs-float64 error), one forward and one backward call.  No layer's
    torch formulas run."""
    m, g = fixture_model(nfa, name)
    x, inverse = T(g["x"]), dname == "inv"
    with torch.no_grad():
        z, ld = m.inverse_and_log_det(x) if inverse else m.forward_and_log_det(x)
    assert counts(calls) == {"chain": 1, "fwd": 0, "bwd": 0, "torch": 0} and calls["K"] == [len(m.flows)], calls
    assert z.shape == x.shape and ld.shape == (x.shape[0],)
    assert_close(N(z), g["z_" + dname], what="z", **TOL[F32])
    assert_close(N(ld), g["ld_" + dname], what="ld", **ld_tol(F32))
    z1, ld1, gx, _ = step(m, x, inverse, T(g["cz"]), T(g["cl"]))
    assert counts(calls) == {"chain": 1, "fwd": 1, "bwd": 1, "torch": 0} and calls["bwd_flags"] == [(True, True)], calls
    assert_close(N(z1), g["z_" + dname], what="z (autograd)", **TOL[F32])
    assert_close(N(ld1), g["ld_" + dname], what="ld (autograd)", **ld_tol(F32))
    items = [("x", gx, "gx_" + dname)] + [(k, p.grad, "g_%s__%s" % (dname, k.replace(".", "__"))) for k, p in m.flows.named_parameters()]
    for k, got, key in items:
        ref32, ref64 = g[key], g[key.replace("_" + dname, "_%s_f64" % dname, 1)]
        assert got is not None, k
        scale = float(np.abs(ref64).max())
        bar = max(1e-3 * scale, 4.0 * float(np.abs(ref32 - ref64).max()))
        err = float(np.abs(N(got) - ref32).max())
        print("%s %s %s: err %.3e bar %.3e (scale %.3e)" % (name, dname, k, err, bar, scale))
        assert err <= bar, (k, err, bar, scale)
    assert len(items) == 1 + 3 * len(m.flows)


def test_edge_fixture(nfa, calls):
    """|lin| = 0, 15, 50, 95 through one tanh layer: z and log-det against the reference's float32 leg (its sech^2 is 0 at 95 as
    well), finite gradients within 1e-3 of scale of its FLOAT64 leg (the float32 leg's gradients are NaN there: cosh overflows).
    lin == 0 through one leaky layer, both directions: the slope-1 side, against the float32 leg at the fixtures' bar."""
    g = load_golden("rank1_planar_edges")
    for key, (layer, x) in cases.edge_layers(nfa).items():
        layer, x = layer.to(DEV), x.to(DEV)
        cz, cl = T(g[key + "__cz"]), T(g[key + "__cl"])
        for dname in (("fwd", "inv") if key == "leaky" else ("fwd",)):
            layer.zero_grad(set_to_none=True)
            xx = x.clone().requires_grad_(True)
            z, ld = layer.inverse(xx) if dname == "inv" else layer(xx)
            ((z * cz).sum() + (ld * cl).sum()).backward()
            assert_close(N(z), g["%s__z_%s" % (key, dname)], what="z", **TOL[F32])
            assert_close(N(ld), g["%s__ld_%s" % (key, dname)], what="ld", **ld_tol(F32))
            items = [(xx.grad, "%s__gx_%s" % (key, dname))] + [(p.grad, "%s__g_%s__0__%s" % (key, dname, n_))
                                                                for n_, p in layer.named_parameters()]
            for got, ref_key in items:
                assert torch.isfinite(got).all(), ref_key
                ref64 = g[ref_key.replace("_" + dname, "_%s_f64" % dname, 1)]
                scale = float(np.abs(ref64).max())
                if key == "tanh":
                    bar, ref = 1e-3 * scale, ref64
                else:
                    bar, ref = max(1e-3 * scale, 4.0 * float(np.abs(g[ref_key] - ref64).max())), g[ref_key]
                err = float(np.abs(N(got) - ref).max())
                print("%s: err %.3e bar %.3e" % (ref_key, err, bar))
                assert err <= bar, (ref_key, err, bar)
    assert calls["torch"] == 0 and calls["fwd"] == calls["bwd"] == 3


# ---- 2. route against route -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [2, 16, 17, 128])
def test_route_vs_torch_formulas(nfa, calls, formulas, d):
    m = random_model(nfa, cases.MIXED, (d,), seed=20 + d)
    x, cz, cl = batch(70, (d,))
    z, ld, gx, gp = step(m, x, False, cz, cl)
    with torch.no_grad():
        zi, ldi = m.forward_and_log_det(x)
    assert counts(calls) == {"chain": 1, "fwd": 1, "bwd": 1, "torch": 0}
    assert torch.equal(z, zi) and torch.equal(ld, ldi)            # the training forward is the inference kernel with saves
    with formulas():
        z0, ld0, gx0, gp0 = step(m, x, False, cz, cl)
    assert counts(calls) == {"chain": 1, "fwd": 1, "bwd": 1, "torch": len(m.flows)}
    assert_close(N(z), N(z0), what="z", **TOL[F32])
    assert_close(N(ld), N(ld0), what="ld", **ld_tol(F32))
    print("gx: %.3e of scale" % of_scale(gx, gx0))
    assert of_scale(gx, gx0) <= 1e-5
    assert_grads_of_scale(gp, gp0, 1e-5, "d=%d" % d)


@pytest.mark.parametrize("d", [3, 40])
def test_inverse_route_vs_torch_formulas(nfa, calls, formulas, d):
    m = random_model(nfa, "LLL", (d,), seed=40 + d)
    x, cz, cl = batch(70, (d,))
    z, ld, gx, gp = step(m, x, True, cz, cl)
    assert counts(calls) == {"chain": 0, "fwd": 1, "bwd": 1, "torch": 0}
    with formulas():
        z0, ld0, gx0, gp0 = step(m, x, True, cz, cl)
    assert calls["torch"] == 3
    assert_close(N(z), N(z0), what="z", **TOL[F32])
    assert_close(N(ld), N(ld0), what="ld", **ld_tol(F32))
    assert of_scale(gx, gx0) <= 1e-5
    assert_grads_of_scale(gp, gp0, 1e-5, "inverse d=%d" % d)
    with torch.no_grad():      # and back: the forward direction undoes it
        x1, ld1 = m.forward_and_log_det(z)
    assert_close(N(x1), N(x), rtol=1e-4, atol=1e-4, what="round trip")
    assert_close(N(ld1), -N(ld), rtol=1e-4, atol=1e-4, what="round trip ld")


# ---- 3. second round of the persistent loop ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [2, 17])
def test_second_round_of_the_persistent_loop(nfa, calls, formulas, d):
    """B = cap x rows + rows + 1: the first workgroup walks a second tile and a last, one-row tile follows.  The first and the last
    `rows` rows equal fresh calls on those rows alone bit for bit, two calls give identical bits, the gradients match the formulas."""
    rows, cap = nfa.ops.rank1_rows(d), nfa._lib.lib().nf_persistent_workgroups()
    B = cap * rows + rows + 1
    assert B == (65793 if d == 2 else 4113)
    m = random_model(nfa, "PR", (d,), seed=60 + d)
    x, cz, cl = batch(B, (d,))
    z, ld, gx, gp = step(m, x, False, cz, cl)
    assert calls["K"] == [2]
    for sl in (slice(0, rows), slice(B - rows, B)):
        z1, ld1, gx1, _ = step(m, x[sl].contiguous(), False, cz[sl].contiguous(), cl[sl].contiguous())
        assert torch.equal(z[sl], z1) and torch.equal(ld[sl], ld1) and torch.equal(gx[sl], gx1), sl
        with torch.no_grad():
            z2, ld2 = m.forward_and_log_det(x[sl].contiguous())
        assert torch.equal(z[sl], z2) and torch.equal(ld[sl], ld2), sl
    zb, ldb, gxb, gpb = step(m, x, False, cz, cl)
    assert torch.equal(z, zb) and torch.equal(ld, ldb) and torch.equal(gx, gxb)
    assert all(torch.equal(a, b) for a, b in zip(gp, gpb))
    assert calls["torch"] == 0
    with formulas():
        z0, ld0, gx0, gp0 = step(m, x, False, cz, cl)
    assert_close(N(z), N(z0), what="z", **TOL[F32])
    assert_close(N(ld), N(ld0), what="ld", **ld_tol(F32))
    assert of_scale(gx, gx0) <= 1e-5
    assert_grads_of_scale(gp, gp0, 1e-5, "second round d=%d" % d)


# ---- 4. determinism ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [2, 40])
def test_gradients_are_bit_identical_from_run_to_run(nfa, d):
    m = random_model(nfa, cases.MIXED, (d,), seed=70 + d)
    x, cz, cl = batch(1000, (d,))
    a = step(m, x, False, cz, cl)
    b = step(m, x, False, cz, cl)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert len(a[3]) == 18 and all(torch.equal(p, q) for p, q in zip(a[3], b[3]))


# ---- 5. frozen parameters ---------------------------------------------------------------------------------------------------------
def test_frozen_parameters_and_no_input_gradient(nfa, calls, formulas):
    m = random_model(nfa, cases.MIXED, (17,), seed=81)
    x, cz, cl = batch(70, (17,))
    _, _, gx_ref, gp_ref = step(m, x, False, cz, cl)
    for p in m.parameters():
        p.requires_grad_(False)
    calls["bwd_flags"].clear()
    z, ld, gx, gp = step(m, x, False, cz, cl)
    assert calls["bwd_flags"] == [(False, True)]              # need_gP == 0: one backward launch, no slabs, no reduction
    assert torch.equal(gx, gx_ref) and all(g is None for g in gp)
    for p in m.parameters():
        p.requires_grad_(True)
    calls["bwd_flags"].clear()
    _, _, gx2, gp2 = step(m, x, False, cz, cl, x_grad=False)
    assert calls["bwd_flags"] == [(True, False)] and gx2 is None      # gz is NULL
    assert all(torch.equal(a, b) for a, b in zip(gp2, gp_ref))
    assert calls["torch"] == 0


# ---- 6. accumulation --------------------------------------------------------------------------------------------------------------
def test_two_micro_batches_accumulate(nfa):
    m = random_model(nfa, cases.MIXED, (2,), seed=91)
    x1, cz1, cl1 = batch(300, (2,), seed=1)
    x2, cz2, cl2 = batch(200, (2,), seed=2)
    g1 = step(m, x1, False, cz1, cl1)[3]
    g2 = step(m, x2, False, cz2, cl2)[3]
    step(m, x1, False, cz1, cl1)
    both = step(m, x2, False, cz2, cl2, zero=False)[3]
    for a, b, c in zip(g1, g2, both):
        assert of_scale(c, a + b) <= 1e-6 and of_scale(c, 2 * b) > 1e-3


# ---- 7. live parameters -----------------------------------------------------------------------------------------------------------
def test_an_optimizer_step_reaches_the_next_forward(nfa, calls):
    """Fused Adam does not bump Tensor._version: the no_grad pack is keyed through _keys' optimizer hook, the autograd pack is
    built from the live parameters."""
    m = random_model(nfa, "PRL", (2,), seed=95)
    x, cz, cl = batch(64, (2,))
    opt = torch.optim.Adam(m.parameters(), lr=0.05, fused=True)
    with torch.no_grad():
        z0, ld0 = m.forward_and_log_det(x)
        z0b, _ = m.forward_and_log_det(x)
    assert torch.equal(z0, z0b)
    za = step(m, x, False, cz, cl)[0]
    assert torch.equal(za, z0)
    opt.step()
    zb = step(m, x, False, cz, cl)[0]
    with torch.no_grad():
        z1, ld1 = m.forward_and_log_det(x)
    assert not torch.equal(zb, za) and not torch.equal(z1, z0) and not torch.equal(ld1, ld0)
    assert torch.equal(z1, zb) and calls["torch"] == 0


# ---- 8. router boundaries ---------------------------------------------------------------------------------------------------------
def test_runs_around_another_layer_and_the_cut_at_64(nfa, calls, formulas):
    P, R = nfa.flows.Planar, nfa.flows.Radial
    torch.manual_seed(3)
    an = nfa.flows.ActNorm(2)
    an.data_dep_init_done.fill_(1.0)
    with torch.no_grad():
        an.s.fill_(0.3)
        an.t.fill_(-0.2)
    m = nfa.NormalizingFlow(nfa.distributions.DiagGaussian(2), [P((2,)), P((2,)), an, R((2,)), R((2,))]).to(DEV)
    x = batch(70, (2,))[0]
    with torch.no_grad():
        z, ld = m.forward_and_log_det(x)
    assert calls["chain"] == 2 and calls["K"] == [2, 2] and calls["torch"] == 0
    with formulas(), torch.no_grad():
        z0, ld0 = m.forward_and_log_det(x)
    assert calls["torch"] == 4
    assert_close(N(z), N(z0), what="z", **TOL[F32])
    assert_close(N(ld), N(ld0), what="ld", **ld_tol(F32))
    calls["K"].clear()
    torch.manual_seed(4)
    long = nfa.NormalizingFlow(nfa.distributions.DiagGaussian(2), [P((2,)) if i % 3 else R((2,)) for i in range(65)]).to(DEV)
    with torch.no_grad():
        z, ld = long.forward_and_log_det(x)
    assert calls["K"] == [64, 1]
    z1, ld1, gx, gp = step(long, x)
    assert calls["K"] == [64, 1, 64, 1] and torch.equal(z, z1)
    with formulas():
        z0, ld0, gx0, gp0 = step(long, x)
    assert_close(N(z), N(z0), what="z", rtol=1e-4, atol=1e-4)
    assert_close(N(ld), N(ld0), what="ld", rtol=1e-4, atol=1e-4)
    assert of_scale(gx, gx0) <= 1e-4


def test_what_stays_on_the_torch_formulas(nfa, calls):
    P = nfa.flows.Planar
    x = batch(70, (2,))[0]

    class MyPlanar(P):
        pass
    torch.manual_seed(6)
    sub, plain = MyPlanar((2,)).to(DEV), P((2,)).to(DEV)
    plain.load_state_dict(sub.state_dict())
    msub = nfa.NormalizingFlow(nfa.distributions.DiagGaussian(2), [sub]).to(DEV)
    with torch.no_grad():
        z_s, ld_s = msub.forward_and_log_det(x)          # a subclass, through the container and directly
        z_s2, _ = sub(x)
    assert counts(calls) == {"chain": 0, "fwd": 0, "bwd": 0, "torch": 2}
    with torch.no_grad():
        z_k, ld_k = plain(x)
    assert calls["chain"] == 1 and calls["torch"] == 2
    assert_close(N(z_s), N(z_k), what="subclass z", **TOL[F32])
    assert_close(N(ld_s), N(ld_k), what="subclass ld", **ld_tol(F32))
    assert torch.equal(z_s, z_s2)
    n = dict(counts(calls))
    p64 = P((2,)).to(DEV)
    p64.load_state_dict(plain.state_dict())
    p64 = p64.double()
    with torch.no_grad():
        z64, ld64 = p64(x.double())                      # float64
    assert calls["chain"] == n["chain"] and calls["torch"] == n["torch"] + 1 and z64.dtype == torch.float64
    assert_close(N(z_k), N(z64), what="float64 z", **TOL[F32])
    assert_close(N(ld_k), N(ld64), what="float64 ld", **ld_tol(F32))
    wide = nfa.NormalizingFlow(nfa.distributions.DiagGaussian(129), [P((129,)), nfa.flows.Radial((129,))]).to(DEV)
    x129 = batch(8, (129,))[0]
    z, ld, gx, gp = step(wide, x129)                     # d = 129
    assert calls["chain"] == n["chain"] and calls["fwd"] == 0 and calls["torch"] == n["torch"] + 3      # (float64's one, these two)
    assert torch.isfinite(z).all() and torch.isfinite(gx).all() and all(torch.isfinite(g).all() for g in gp)
    with nfa.config.higher_order_gradients():            # double backward needs the formulas
        xx = x.clone().requires_grad_(True)
        z, ld = plain(xx)
        (g1,) = torch.autograd.grad(z.sum() + ld.sum(), xx, create_graph=True)
        g1.sum().backward()
    assert calls["fwd"] == 0 and xx.grad is not None and torch.isfinite(xx.grad).all()


def test_inverse_over_a_tanh_layer_raises_and_launches_nothing(nfa, calls):
    P = nfa.flows.Planar
    m = nfa.NormalizingFlow(nfa.distributions.DiagGaussian(2), [P((2,)), P((2,), act="leaky_relu")]).to(DEV)
    x = batch(8, (2,))[0]
    for ctx in (torch.no_grad(), torch.enable_grad()):
        with ctx, pytest.raises(NotImplementedError, match="This flow has no algebraic inverse."):
            m.inverse_and_log_det(x)
    with pytest.raises(NotImplementedError, match="This flow has no algebraic inverse."):
        m.flows[0].inverse(x)
    with pytest.raises(NotImplementedError, match="This flow has no algebraic inverse."):
        nfa.flows.Radial((2,)).to(DEV).inverse(x)
    assert counts(calls) == {"chain": 0, "fwd": 0, "bwd": 0, "torch": 1}      # (the direct call reaches _torch_inverse, which raises)


# ---- 9. views ---------------------------------------------------------------------------------------------------------------------
def test_views(nfa, calls):
    m = random_model(nfa, cases.MIXED, (3,), seed=33)
    big = batch(40, (6,))[0]
    strided = big[:, ::2]
    assert not strided.is_contiguous()
    with torch.no_grad():
        z0, ld0 = m.forward_and_log_det(strided)
        # the first layer meets the strided input and falls back; its output is contiguous, so the other five are one launch
        assert counts(calls) == {"chain": 1, "fwd": 0, "bwd": 0, "torch": 1} and calls["K"] == [5]
        z1, ld1 = m.forward_and_log_det(strided.contiguous())
        assert calls["chain"] == 2 and calls["K"] == [5, 6]
        assert_close(N(z0), N(z1), what="z", **TOL[F32])
        assert_close(N(ld0), N(ld1), what="ld", **ld_tol(F32))
        rows = strided.contiguous()
        view = rows[3:]
        assert view.is_contiguous() and view.data_ptr() != rows.data_ptr() and view.data_ptr() % 16 != 0
        z2, ld2 = m.forward_and_log_det(view)
        assert calls["chain"] == 3 and calls["torch"] == 1
        assert torch.equal(z2, z1[3:]) and torch.equal(ld2, ld1[3:])
    za, lda, gxa, _ = step(m, view)
    assert calls["fwd"] == 1 and torch.equal(za, z1[3:])


# ---- 10. capture ------------------------------------------------------------------------------------------------------------------
def test_capture_and_replay(nfa, calls):
    """forward_and_log_det of a K = 4 model recorded with torch.cuda.graph on one stream and replayed with new input contents: no
    host synchronisation on the route, the eager bits."""
    m = random_model(nfa, "PRLP", (2,), seed=44)
    xs = [batch(500, (2,), seed=s)[0] for s in (1, 2, 3)]
    static = xs[0].clone()
    with torch.no_grad():
        eager = [m.forward_and_log_det(x) for x in xs]
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            m.forward_and_log_det(static)
        torch.cuda.current_stream().wait_stream(s)
        n = calls["chain"]
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = m.forward_and_log_det(static)
        assert calls["chain"] == n + 1 and calls["torch"] == 0
        for x, (z, ld) in list(zip(xs, eager))[1:]:
            static.copy_(x)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out[0], z) and torch.equal(out[1], ld)
