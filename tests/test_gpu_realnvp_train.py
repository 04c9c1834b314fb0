"""GPU tests of the RealNVP training route: runs of MaskedAffineFlow(MLP s, MLP t) / ActNorm / AffineConstFlow layers under autograd
as one forward and one backward launch (csrc/realnvp_train.hip, autograd.RealNVPChainFn) -- against the reference's autograd
(tests/golden/grad_realnvp_train_*.npz, grad_realnvp.npz), against the layer-by-layer route, and the route's own contracts
(persistent loop, determinism, accumulation, frozen parameters, live parameters, views, capture, what stays outside)."""
import numpy as np
import pytest
import torch

import realnvp_train_cases as cases
import realnvp_train_emulator as emu
from conftest import assert_close, golden_state, ld_tol
from test_gpu_training import _check_grads, load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def nfa():
    import normflows_amd
    assert torch.cuda.is_available()
    return normflows_amd


@pytest.fixture
def calls(nfa, monkeypatch):
    """Counts of the new ops' calls and of what the layer-by-layer route runs instead."""
    n = {"fwd": 0, "bwd": 0, "maf": 0, "lin": 0}

    def counted(key, fn):
        def wrapper(*a, **k):
            n[key] += 1
            return fn(*a, **k)
        return wrapper
    monkeypatch.setattr(nfa.ops, "realnvp_chain_train_fwd", counted("fwd", nfa.ops.realnvp_chain_train_fwd))
    monkeypatch.setattr(nfa.ops, "realnvp_chain_bwd", counted("bwd", nfa.ops.realnvp_chain_bwd))
    monkeypatch.setattr(nfa.autograd.MaskedAffineFn, "apply", counted("maf", nfa.autograd.MaskedAffineFn.apply))
    monkeypatch.setattr(torch.nn.Linear, "forward", counted("lin", torch.nn.Linear.forward))
    return n


@pytest.fixture
def eager(nfa):
    """Context manager factory: the layer-by-layer route for the `with` body."""
    import contextlib

    @contextlib.contextmanager
    def off():
        nfa.config.set_realnvp_train(False)
        try:
            yield
        finally:
            nfa.config.set_realnvp_train(True)
    return off


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def N(t):
    return t.detach().cpu().numpy()


def fixture_model(nfa, name):
    g = load_golden("grad_realnvp_train_" + name)
    m = cases.model(nfa, name)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in golden_state(g).items()}, strict=True)
    return m.to(DEV), g


def small_model(nfa, d=2, widths=(8,), n=2, seed=3, actnorm=True, dtype=torch.float32):
    """n x [MaskedAffineFlow(MLP s, MLP t), ActNorm (initialised) or AffineConstFlow], every parameter random."""
    g = torch.Generator().manual_seed(seed)
    b = torch.tensor([1.0, 0.0] * ((d + 1) // 2))[:d]
    flows = []
    for i in range(n):
        flows += [nfa.flows.MaskedAffineFlow(b if i % 2 == 0 else 1 - b, nfa.nets.MLP([d] + list(widths) + [d]),
                                             nfa.nets.MLP([d] + list(widths) + [d], leaky=0.05)),
                  nfa.flows.ActNorm(d) if actnorm else nfa.flows.AffineConstFlow(d)]
    m = nfa.NormalizingFlow(nfa.distributions.DiagGaussian(d, trainable=False), flows)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(0.3 * torch.randn(p.shape, generator=g))
        for f in flows:
            if hasattr(f, "data_dep_init_done"):
                f.data_dep_init_done.fill_(1.0)
    return m.to(dtype).to(DEV)


def step(m, x, inverse=True, cz=None, cl=None, zero=True):
    """One pass + backward of sum(z * cz) + sum(ld * cl) (ones by default); (z, ld, gx, [gradient or None of every parameter of m.flows])."""
    if zero:
        m.zero_grad(set_to_none=True)
    xx = x.detach().clone().requires_grad_(True) if x.is_contiguous() else x.detach().requires_grad_(True)
    z, ld = m.inverse_and_log_det(xx) if inverse else m.forward_and_log_det(xx)
    ((z if cz is None else z * cz).sum() + (ld if cl is None else ld * cl).sum()).backward()
    return z.detach(), ld.detach(), xx.grad, [None if p.grad is None else p.grad.detach().clone() for p in m.flows.parameters()]


def of_scale(got, ref):
    got, ref = got.detach().double(), ref.detach().double()
    return float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)


def assert_grads_of_scale(got, ref, bar, what):
    for k, (a, b) in enumerate(zip(got, ref)):
        assert (a is None) == (b is None), (what, k)
        if a is not None:
            assert of_scale(a, b) <= bar, (what, k, of_scale(a, b))


# ---- 1. against the reference's autograd ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dname", ["fwd", "inv"])
@pytest.mark.parametrize("name", list(cases.CASES))
def test_fixture_gradients_vs_reference_autograd(nfa, calls, name, dname):
    """z and log-det at the parity bars, gx and every parameter gradient within max(1e-3 of scale, 4 x the reference's own
    float32-vs-float64 error): one forward and one backward call for the whole model, no MaskedAffineFn, no Linear.forward."""
    m, g = fixture_model(nfa, name)
    z, ld, gx, _ = step(m, T(g["x"]), dname == "inv", T(g["cz"]), T(g["cl"]))
    assert calls == {"fwd": 1, "bwd": 1, "maf": 0, "lin": 0}, calls
    assert_close(N(z), g["z_" + dname], rtol=1e-4, atol=1e-4, what="z")
    assert_close(N(ld), g["ld_" + dname], what="ld", **ld_tol(np.float32))
    items = [("x", gx, "gx_" + dname)] + [(k, p.grad, "g_%s__%s" % (dname, k.replace(".", "__"))) for k, p in m.named_parameters()]
    for k, got, key in items:
        ref32, ref64 = g[key], g[key.replace("_" + dname, "_%s_f64" % dname, 1)]
        assert got is not None, k
        scale = float(np.abs(ref64).max())
        bar = max(1e-3 * scale, 4.0 * float(np.abs(ref32 - ref64).max()))
        err = float(np.abs(N(got) - ref32).max())
        print("%s %s %s: err %.3e bar %.3e (scale %.3e)" % (name, dname, k, err, bar, scale))
        assert err <= bar, (k, err, bar, scale)
    assert len(items) > 4


@pytest.mark.parametrize("name", ["realnvp"] + list(cases.CASES))
def test_forward_kld_step_vs_reference(nfa, calls, name):
    """loss = forward_kld(x); loss.backward() on the new fixtures and on the existing grad_realnvp.npz (4 x [MaskedAffineFlow(MLP
    [2, 8, 2]) + ActNorm], its ActNorms initialised by a no_grad pass first, as its generator did)."""
    if name == "realnvp":
        g = load_golden("grad_realnvp")
        b = torch.tensor([1.0, 0.0])
        flows = []
        for i in range(4):
            flows += [nfa.flows.MaskedAffineFlow(b if i % 2 == 0 else 1 - b, nfa.nets.MLP([2, 8, 2], init_zeros=True),
                                                 nfa.nets.MLP([2, 8, 2], init_zeros=True)), nfa.flows.ActNorm(2)]
        m = nfa.NormalizingFlow(nfa.distributions.DiagGaussian(2), flows)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in golden_state(g).items()}, strict=True)
        m = m.to(DEV)
        with torch.no_grad():
            m.log_prob(T(g["x"]))
    else:
        m, g = fixture_model(nfa, name)
    loss = m.forward_kld(T(g["x"]))
    loss.backward()
    assert calls == {"fwd": 1, "bwd": 1, "maf": 0, "lin": 0}, calls
    assert abs(float(loss.detach()) - float(g["loss"])) < 2e-4 * abs(float(g["loss"]))
    _check_grads(m, g, min_checked=len(list(m.flows.parameters())))
    if name == "realnvp":      # the other direction of that model: against the float64 restatement of the formulas on the CPU
        x = T(g["x"])
        z, ld, gx, gp = step(m, x, inverse=False)
        m64 = m.double().cpu()
        z64, ld64, gx64, gp64 = emu.grads(list(m64.flows), x.double().cpu(), torch.ones(x.shape, dtype=torch.float64),
                                          torch.ones(x.shape[0], dtype=torch.float64), False)
        assert_close(N(z), z64.numpy(), rtol=1e-4, atol=1e-4, what="z fwd")
        assert_close(N(ld), ld64.numpy(), what="ld fwd", **ld_tol(np.float32))
        assert of_scale(gx.cpu(), gx64) < 1e-3
        for got, p in zip(gp, m64.flows.parameters()):
            assert of_scale(got.cpu(), gp64[id(p)]) < 1e-3


# ---- 2. route against route ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("name", list(cases.CASES))
def test_route_vs_layer_by_layer(nfa, calls, eager, name, inverse):
    m, g = fixture_model(nfa, name)
    x, cz, cl = T(g["x"]), T(g["cz"]), T(g["cl"])
    z, ld, gx, gp = step(m, x, inverse, cz, cl)
    assert calls["fwd"] == 1 and calls["bwd"] == 1
    with eager():
        z0, ld0, gx0, gp0 = step(m, x, inverse, cz, cl)
    assert calls["fwd"] == 1 and calls["bwd"] == 1 and calls["lin"] > 0
    assert_close(N(z), N(z0), rtol=1e-4, atol=1e-4, what="z")
    assert_close(N(ld), N(ld0), rtol=1e-4, atol=1e-4, what="ld")
    assert of_scale(gx, gx0) <= 2e-4
    assert_grads_of_scale(gp, gp0, 2e-4, name)


# ---- 3. second round of the persistent loop --------------------------------------------------------------------------------------
def test_second_round_of_the_persistent_loop(nfa, calls, eager):
    m = small_model(nfa, d=2, widths=(8,), n=2)
    rows = nfa.ops.realnvp_rows(8, 10)          # hmax 8; one MLP's Linear inputs: 2 + 8
    assert rows in (64, 128, 256)
    wg = nfa._lib.lib().nf_persistent_workgroups()
    B = wg * rows + rows + 3
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, 2, generator=g).to(DEV)
    # cotangents of one sign (0.5 .. 1.5), as a likelihood gives: with random signs a gradient summed over 65 795 rows can cancel to
    # float32 noise (a bias gradient of -0.012 from terms of size 1), and "of scale" then measures the noise of either route
    cz, cl = (0.5 + torch.rand(B, 2, generator=g)).to(DEV), (0.5 + torch.rand(B, generator=g)).to(DEV)
    for inverse in (True, False):
        z, ld, gx, gp = step(m, x, inverse, cz, cl)
        for sl in (slice(0, rows + 3), slice(B - rows - 3, B)):
            z1, ld1, gx1, _ = step(m, x[sl].contiguous(), inverse, cz[sl].contiguous(), cl[sl].contiguous())
            assert torch.equal(z[sl], z1) and torch.equal(ld[sl], ld1) and torch.equal(gx[sl], gx1), (inverse, sl)
        n = calls["fwd"]
        with eager():
            _, _, gx0, gp0 = step(m, x, inverse, cz, cl)
        assert calls["fwd"] == n
        assert of_scale(gx, gx0) <= 2e-4
        assert_grads_of_scale(gp, gp0, 2e-4, "second round")


# ---- 4. determinism --------------------------------------------------------------------------------------------------------------
def test_gradients_are_bit_identical_from_run_to_run(nfa):
    m, g = fixture_model(nfa, "d2_w64")
    x = torch.randn(3000, 2, generator=torch.Generator().manual_seed(5)).to(DEV)
    a = step(m, x)
    b = step(m, x)
    assert torch.equal(a[2], b[2]) and all(torch.equal(p, q) for p, q in zip(a[3], b[3])) and len(a[3]) > 0


# ---- 5. accumulation -------------------------------------------------------------------------------------------------------------
def test_accumulation_over_micro_batches(nfa):
    m, g = fixture_model(nfa, "d5_mixed")
    x1 = T(g["x"])
    x2 = torch.randn(50, 5, generator=torch.Generator().manual_seed(6)).to(DEV)
    g1, g2 = step(m, x1)[3], step(m, x2)[3]
    step(m, x1)
    acc = step(m, x2, zero=False)[3]
    assert all(torch.equal(a, p + q) for a, p, q in zip(acc, g1, g2))
    m.zero_grad(set_to_none=True)
    (m.forward_kld(x1) * x1.shape[0] + m.forward_kld(x2) * x2.shape[0]).backward()
    k1 = [p.grad.clone() for p in m.parameters()]
    m.zero_grad(set_to_none=True)
    (m.forward_kld(x1) * x1.shape[0]).backward()
    (m.forward_kld(x2) * x2.shape[0]).backward()
    assert all(torch.equal(a, p.grad) for a, p in zip(k1, m.parameters()))


# ---- 6. frozen and partial -------------------------------------------------------------------------------------------------------
def test_frozen_and_partially_frozen_parameters(nfa, calls):
    m, g = fixture_model(nfa, "d16")
    x = T(g["x"])
    _, _, gx, gp = step(m, x)
    for p in m.parameters():
        p.requires_grad_(False)
    n = dict(calls)
    z, ld, gx_f, gp_f = step(m, x)
    assert calls["fwd"] == n["fwd"] + 1 and calls["bwd"] == n["bwd"] + 1 and calls["lin"] == 0
    assert torch.equal(gx_f, gx) and all(q is None for q in gp_f)
    for p in m.parameters():
        p.requires_grad_(True)
    frozen = list(m.flows[0].s.parameters())
    for p in frozen:
        p.requires_grad_(False)
    _, _, gx_p, gp_p = step(m, x)
    assert torch.equal(gx_p, gx)
    ids = {id(p) for p in frozen}
    for p, a, b in zip(m.parameters(), gp_p, gp):
        if id(p) in ids:
            assert a is None and p.grad is None
        else:
            assert torch.equal(a, b)
    # frozen parameters and an input without gradient: nothing to train, the inference route
    for p in m.parameters():
        p.requires_grad_(False)
    n = dict(calls)
    z2, _ = m.inverse_and_log_det(x)
    assert calls == n and not z2.requires_grad
    assert_close(N(z2), N(z), rtol=1e-5, atol=1e-5, what="inference route")


# ---- 7. live parameters ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["fused_adam", "data_update"])
def test_the_blob_follows_the_live_parameters(nfa, calls, eager, how):
    m, g = fixture_model(nfa, "d5_mixed")
    x = T(g["x"])
    loss0 = m.forward_kld(x)
    loss0.backward()
    if how == "fused_adam":
        torch.optim.Adam(m.parameters(), lr=5e-2, fused=True).step()
    else:
        for p in m.parameters():
            p.data.add_(0.05 * torch.sign(p.grad))
        nfa.invalidate_caches(m)
    n = calls["fwd"]
    loss1 = m.forward_kld(x)
    assert calls["fwd"] == n + 1
    with eager():
        loss2 = m.forward_kld(x)
    assert calls["fwd"] == n + 1
    assert abs(float(loss1) - float(loss0)) > 1e-3 * abs(float(loss0))
    assert abs(float(loss1) - float(loss2)) < 2e-4 * abs(float(loss2))


# ---- 8. views --------------------------------------------------------------------------------------------------------------------
def test_offset_strided_input_view(nfa, calls):
    m, g = fixture_model(nfa, "d5_mixed")
    wide = torch.randn(40, 9, generator=torch.Generator().manual_seed(8)).to(DEV)
    view = wide[3:36, 2:7]
    assert not view.is_contiguous() and view.storage_offset() > 0
    a = step(m, view)
    b = step(m, view.contiguous())
    assert calls["fwd"] == 2
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert all(torch.equal(p, q) for p, q in zip(a[3], b[3]))


# ---- 9. outside the route --------------------------------------------------------------------------------------------------------
def _check_vs_formulas(m, x, inverse, got, bar):
    z, ld, gx, gp = got
    flows = list(m.flows)
    z0, ld0, gx0, gp0 = emu.grads(flows, x, torch.ones_like(x), torch.ones(x.shape[0], dtype=x.dtype, device=x.device), inverse)
    assert of_scale(z, z0) <= bar and of_scale(ld, ld0) <= bar and of_scale(gx, gx0) <= bar
    for a, p in zip(gp, m.parameters()):
        assert of_scale(a, gp0[id(p)]) <= bar


@pytest.mark.parametrize("case", ["width65", "d17", "float64"])
def test_outside_the_route_shapes(nfa, calls, case):
    if case == "width65":
        m = small_model(nfa, d=2, widths=(65,))
    elif case == "d17":
        m = small_model(nfa, d=17, widths=(8,))
    else:
        m = small_model(nfa, d=2, widths=(8,), dtype=torch.float64)
    d = 17 if case == "d17" else 2
    x = torch.randn(37, d, generator=torch.Generator().manual_seed(9)).to(m.flows[1].s.dtype).to(DEV)
    for inverse in (True, False):
        got = step(m, x, inverse)
        assert calls["fwd"] == 0 and calls["bwd"] == 0 and calls["maf"] > 0
        _check_vs_formulas(m, x, inverse, got, 1e-9 if case == "float64" else 2e-4)


def test_pending_actnorm_keeps_the_layer_by_layer_path_once(nfa, calls):
    m = small_model(nfa, d=2, widths=(8,), n=1)
    m.flows[1].data_dep_init_done.fill_(0.0)
    m.flows[1]._init_known = None
    x = torch.randn(37, 2, generator=torch.Generator().manual_seed(10)).to(DEV)
    got = step(m, x)
    assert calls["fwd"] == 0 and calls["maf"] == 1 and float(m.flows[1].data_dep_init_done) > 0
    _check_vs_formulas(m, x, True, got, 2e-4)          # (the initialised layer applied to the batch it was initialised on)
    got = step(m, x)
    assert calls["fwd"] == 1 and calls["bwd"] == 1 and calls["maf"] == 1
    _check_vs_formulas(m, x, True, got, 2e-4)


def test_higher_order_gradients_stay_outside(nfa, calls):
    m = small_model(nfa, d=2, widths=(8,), n=2)
    x = torch.randn(37, 2, generator=torch.Generator().manual_seed(12)).to(DEV)
    with nfa.config.higher_order_gradients():
        got = step(m, x)
        assert calls["fwd"] == 0 and calls["bwd"] == 0
        _check_vs_formulas(m, x, True, got, 2e-4)
        # a gradient penalty: d/dtheta |d log_det / dx|^2, against the same thing through the restated formulas
        m.zero_grad(set_to_none=True)
        xx = x.clone().requires_grad_(True)
        z, ld = m.inverse_and_log_det(xx)
        gx, = torch.autograd.grad(ld.sum() + (z * z).sum(), xx, create_graph=True)
        assert gx.requires_grad
        gx.pow(2).sum().backward()
        got2 = [p.grad.clone() for p in m.parameters()]
    assert calls["fwd"] == 0 and calls["bwd"] == 0
    m.zero_grad(set_to_none=True)
    xx = x.clone().requires_grad_(True)
    z, ld = emu.chain(list(m.flows), xx, True)
    gx0, = torch.autograd.grad(ld.sum() + (z * z).sum(), xx, create_graph=True)
    gx0.pow(2).sum().backward()
    assert of_scale(gx, gx0) <= 2e-4
    for a, p in zip(got2, m.parameters()):
        assert float(p.grad.abs().max()) > 0 and of_scale(a, p.grad) <= 2e-4
    step(m, x)
    assert calls["fwd"] == 1          # and the route is back outside the context


# ---- 10. capture -----------------------------------------------------------------------------------------------------------------
def _captured_step(m, static_x, x_new):
    """(loss, gradients) of one forward_kld + backward captured on static_x after the usual side-stream warm-up, replayed on x_new."""
    def one_step():
        m.zero_grad(set_to_none=True)
        loss = m.forward_kld(static_x)
        loss.backward()
        return loss

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            one_step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    m.zero_grad(set_to_none=True)
    with torch.cuda.graph(graph):
        loss = m.forward_kld(static_x)
        loss.backward()
    captured = [p.grad for p in m.parameters()]
    static_x.copy_(x_new)
    graph.replay()
    torch.cuda.synchronize()
    return loss.clone(), [t.clone() for t in captured]


def test_training_step_captures_into_a_graph(nfa, calls):
    """From config.realnvp_train_capture_min_batch rows on a captured step takes the route: replayed on new input it gives the bits
    of an uncaptured step.  Below that size the capture records the layer-by-layer route (faster when replayed:
    profiles/realnvp_train_bench.json), and the replay agrees with an uncaptured step at the route-vs-route bar."""
    m, g = fixture_model(nfa, "d2_w64")
    gen = torch.Generator().manual_seed(13)
    B = nfa.config.realnvp_train_capture_min_batch
    assert 1024 < B <= 65536
    static_x, x_new = torch.randn(B, 2, generator=gen).to(DEV), torch.randn(B, 2, generator=gen).to(DEV)
    n = calls["fwd"]
    got_loss, got = _captured_step(m, static_x, x_new)
    assert calls["fwd"] == n + 3 and calls["lin"] == 0           # two warm-up steps and the captured one
    m.zero_grad(set_to_none=True)
    ref_loss = m.forward_kld(x_new)
    ref_loss.backward()
    assert calls["fwd"] == n + 4
    assert torch.equal(got_loss, ref_loss.detach())
    assert all(torch.equal(a, p.grad) for a, p in zip(got, m.parameters())) and len(got) > 0
    # below the threshold
    static_x, x_new = torch.randn(300, 2, generator=gen).to(DEV), torch.randn(300, 2, generator=gen).to(DEV)
    n = calls["fwd"]
    got_loss, got = _captured_step(m, static_x, x_new)
    assert calls["fwd"] == n + 2 and calls["lin"] > 0            # the warm-up steps only
    m.zero_grad(set_to_none=True)
    ref_loss = m.forward_kld(x_new)
    ref_loss.backward()
    assert calls["fwd"] == n + 3
    assert abs(float(got_loss) - float(ref_loss)) <= 2e-4 * abs(float(ref_loss))
    assert_grads_of_scale(got, [p.grad for p in m.parameters()], 2e-4, "captured below the threshold")


# ---- 11. reverse_kld -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("score_fn", [True, False])
def test_reverse_kld(nfa, calls, eager, score_fn):
    m, g = fixture_model(nfa, "d2_w64")
    m.p = nfa.distributions.DiagGaussian(2, trainable=False).to(DEV)

    eps = torch.randn(256, 2, generator=torch.Generator().manual_seed(14)).to(DEV)

    def grads_of():
        m.zero_grad(set_to_none=True)
        loss = m.reverse_kld(num_samples=256, score_fn=score_fn, eps=eps)
        loss.backward()
        return loss.detach(), [None if p.grad is None else p.grad.clone() for p in m.flows.parameters()]

    loss, gp = grads_of()
    assert calls["fwd"] >= 1 and calls["bwd"] >= 1 and calls["lin"] == 0
    live = [a for a in gp if a is not None]
    assert live and all(torch.isfinite(a).all() for a in live) and sum(float(a.abs().sum()) for a in live) > 0
    with eager():
        loss0, gp0 = grads_of()
    assert abs(float(loss) - float(loss0)) <= 2e-4 * max(1.0, abs(float(loss0)))
    assert_grads_of_scale(gp, gp0, 2e-4, "reverse_kld")
