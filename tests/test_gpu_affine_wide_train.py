"""GPU tests (-m gpu) of the wide RealNVP coupling layers UNDER AUTOGRAD on HIP kernels (config.affine_wide_train, opt-in:
autograd.AffineWideFn = nf_pack_gather + nf_made_forward_train in plain-MLP mode + nf_affine_wide_apply; nf_affine_wide_apply_bwd +
nf_made_backward + nf_made_wgrad) -- against the reference's autograd (tests/golden/grad_affine_wide_*.npz), against the layer-wise
route (switch off) on the same weights, with one cotangent absent, a frozen conditioner, a frozen input, batches around the tile edge,
live parameters under an optimizer, a stacked model, outside the route, and captured into a graph.  Every test sets the switch on and
restores it.  Shapes: the 130-row fixtures of tests/affine_wide_cases.py (two 64-row tiles + 2 rows)."""
import copy

import numpy as np
import pytest
import torch

import affine_wide_cases as cases
import affine_wide_train_ref as ref
from conftest import assert_close, ld_tol

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAMES = sorted(cases.CASES)
ROUTE_OPS = ("made_forward_train", "affine_wide_apply", "affine_wide_apply_bwd", "made_backward", "made_wgrad")
ROUTE = {k: 1 for k in ROUTE_OPS}
LAYERWISE_OPS = ("masked_affine", "affine_coupling", "masked_affine_bwd", "affine_coupling_bwd")


@pytest.fixture(scope="module")
def nfa():
    import normflows_amd
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    assert normflows_amd.native_library_path().endswith("normalizing-flows_amd/lib/libnf_mi355x.so")
    normflows_amd._lib.lib()
    return normflows_amd


@pytest.fixture(autouse=True)
def _switch_on(nfa):
    gate = nfa.config.affine_wide_train_capture_min_batch
    nfa.config.set_affine_wide_train(True)
    yield
    nfa.config.set_affine_wide_train(False, capture_min_batch=gate)
    assert nfa.config.affine_wide_train is False


@pytest.fixture
def spy(nfa, monkeypatch):
    """Counts of the calls that tell the two routes apart."""
    calls = {k: 0 for k in ROUTE_OPS + LAYERWISE_OPS + ("linear",)}

    def wrap(real, key):
        def f(*a, **k):
            calls[key] += 1
            return real(*a, **k)
        return f
    for k in ROUTE_OPS + LAYERWISE_OPS:
        monkeypatch.setattr(nfa.ops, k, wrap(getattr(nfa.ops, k), k))
    monkeypatch.setattr(torch.nn.functional, "linear", wrap(torch.nn.functional.linear, "linear"))
    monkeypatch.setattr(torch.nn.Linear, "forward", wrap(torch.nn.Linear.forward, "linear"))
    return calls


def route_counts(spy):
    return {k: spy[k] for k in ROUTE_OPS}


def layerwise_counts(spy):
    return sum(spy[k] for k in LAYERWISE_OPS)


def reset(spy):
    for k in spy:
        spy[k] = 0


def N(t):
    return t.detach().cpu().numpy()


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


_FIX = {}


def fixture(nfa, name):
    """(layer on the GPU, x, cz, cl on the GPU, training fixture): built once per module, never modified by the tests that share it."""
    if name not in _FIX:
        layer, g, gold = ref.load_layer(nfa, name)
        _FIX[name] = (layer.to(DEV), T(g["x"]), T(gold["cz"]), T(gold["cl"]), gold)
    return _FIX[name]


def fresh(nfa, name):
    return copy.deepcopy(fixture(nfa, name)[0])


def step(layer, direction, x, cz, cl, which="both", x_grad=True):
    """[z, ld, gx, every parameter gradient] of loss = sum(z cz) + sum(ld cl) through layer.forward (direction 0) / layer.inverse (1);
    which = "z" | "ld": one cotangent absent."""
    layer.zero_grad(set_to_none=True)
    xx = x.clone().requires_grad_(x_grad)
    z, ld = (layer.inverse if direction else layer.forward)(xx)
    loss = (z * cz).sum() if which == "z" else ((ld * cl).sum() if which == "ld" else (z * cz).sum() + (ld * cl).sum())
    loss.backward()
    gx = xx.grad if x_grad else torch.zeros_like(x)
    return [z.detach(), ld.detach(), gx] + [torch.zeros_like(p) if p.grad is None else p.grad.clone() for p in layer.parameters()]


def layerwise(nfa, layer, *a, **k):
    """The same step with the switch off: the parent's route."""
    nfa.config.set_affine_wide_train(False)
    try:
        return step(layer, *a, **k)
    finally:
        nfa.config.set_affine_wide_train(True)


def of_scale(a, b):
    return float((a - b).abs().max()) / max(1.0, float(b.abs().max()))


def compare(layer, got, want, what=""):
    """The bars against the layer-wise route: z 1e-4 / 1e-4, ld by ld_tol(float32), every element of every gradient 2e-4 of scale."""
    assert_close(N(got[0]), N(want[0]), what=what + " z", rtol=1e-4, atol=1e-4)
    assert_close(N(got[1]), N(want[1]), what=what + " ld", **ld_tol(np.float32))
    names = ["gx"] + [k for k, _ in layer.named_parameters()]
    assert len(names) == len(got) - 2 == len(want) - 2
    for k, a, b in zip(names, got[2:], want[2:]):
        assert a.shape == b.shape, (what, k)
        assert of_scale(a, b) <= 2e-4, (what, k, of_scale(a, b))


def exact_zeros_hold(layer, name, grads):
    by_name = dict(zip([k for k, _ in layer.named_parameters()], grads))
    zeros = ref.exact_zero_entries(layer, name)
    for k, m in zeros:
        assert m.any() and not N(by_name[k])[m].any(), k
    return len(zeros)


# ---- 1. against the reference's autograd ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("direction", (0, 1))
@pytest.mark.parametrize("name", NAMES)
def test_fixtures_vs_reference_autograd(nfa, spy, name, direction):
    """The five ops of the route exactly once each, never a Linear nor a layer-wise coupling kernel.  Bars of
    tests/test_gpu_circ_coupled_train.py: z, ld, gx and the strided gradient samples within 1e-3 of scale of the reference's float32
    leg, sums within 1e-4 max(1, abs-sum), q90 of the errors against the float64 leg <= 4 x max(the reference's own, the layer-wise
    route's in this same test, 1e-7)."""
    layer, x, cz, cl, g = fixture(nfa, name)
    d = "inv" if direction else "fwd"
    got = step(layer, direction, x, cz, cl)
    assert route_counts(spy) == ROUTE and spy["linear"] == 0 and layerwise_counts(spy) == 0, spy
    reset(spy)
    base = layerwise(nfa, layer, direction, x, cz, cl)
    assert sum(route_counts(spy).values()) == 0 and spy["linear"] >= 3 and layerwise_counts(spy) == 2, spy
    stride = int(g["stride"])

    def err(a, r):
        return np.abs(a.astype(np.float64) - r) / max(1.0, float(np.abs(r).max()))
    own, ours, theirs = [], [], []
    for i, k in enumerate(("z", "ld", "gx")):
        r32, r64 = g["%s_%s_f32" % (k, d)], g["%s_%s_f64" % (k, d)]
        e = err(N(got[i]), r32).max()
        print("%s %s %s: %.3e of scale vs the float32 leg" % (name, d, k, e))
        assert e < 1e-3, (k, e)
        own.append(err(r32, r64).max())
        ours.append(err(N(got[i]), r64).max())
        theirs.append(err(N(base[i]), r64).max())
    for i, (k, p) in enumerate(layer.named_parameters()):
        key = k.replace(".", "__")
        flat, flat0 = N(got[3 + i]).reshape(-1), N(base[3 + i]).reshape(-1)
        r32, r64 = g["g_%s_f32__%s" % (d, key)], g["g_%s_f64__%s" % (d, key)]
        e = err(flat[::stride], r32).max()
        assert e < 1e-3, (k, e)
        chk = g["chk_%s_f64__%s" % (d, key)]
        assert abs(float(flat.astype(np.float64).sum()) - chk[0]) < 1e-4 * max(1.0, chk[1]), k
        own.append(err(r32, r64).max())
        ours.append(err(flat[::stride], r64).max())
        theirs.append(err(flat0[::stride], r64).max())
    q, q_own, q_lw = np.quantile(ours, 0.9), np.quantile(own, 0.9), np.quantile(theirs, 0.9)
    print("%s %s: q90 vs float64 %.3e, the reference's own %.3e, the layer-wise route's %.3e" % (name, d, q, q_own, q_lw))
    assert q <= 4 * max(q_own, q_lw, 1e-7), (q, q_own, q_lw)


# ---- 2. against the layer-wise route -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_route_matches_the_layerwise_route(nfa, spy, name):
    layer, x, cz, cl, _ = fixture(nfa, name)
    for direction in (0, 1):
        reset(spy)
        got = step(layer, direction, x, cz, cl)
        assert route_counts(spy) == ROUTE, spy
        want = layerwise(nfa, layer, direction, x, cz, cl)
        compare(layer, got, want, "%s %d" % (name, direction))
        n = exact_zeros_hold(layer, name, got[3:])
        assert n == exact_zeros_hold(layer, name, want[3:]) and (n > 0) == (cases.CASES[name]["kind"] == "masked")
        idt = np.nonzero(N(got[0] == x).all(0))[0]
        assert idt.size >= 1                                             # identity columns leave bit for bit


# ---- 3. one cotangent absent ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ("z", "ld"))
@pytest.mark.parametrize("name", ("a", "e"))
def test_one_cotangent_absent(nfa, spy, name, which):
    layer, x, cz, cl, _ = fixture(nfa, name)
    for direction in (0, 1):
        reset(spy)
        got = step(layer, direction, x, cz, cl, which=which)
        assert route_counts(spy) == ROUTE, spy
        compare(layer, got, layerwise(nfa, layer, direction, x, cz, cl, which=which), "%s %d only %s" % (name, direction, which))


# ---- 4. / 5. frozen conditioner, frozen input ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("b", "g"))
def test_frozen_conditioner_and_frozen_input(nfa, spy, name):
    _, x, cz, cl, _ = fixture(nfa, name)
    layer = fresh(nfa, name)
    full = step(layer, 1, x, cz, cl)
    assert route_counts(spy) == ROUTE
    reset(spy)
    frozen_in = step(layer, 1, x, cz, cl, x_grad=False)
    assert route_counts(spy) == ROUTE
    assert all(torch.equal(a, b) for a, b in zip(frozen_in[3:], full[3:])) and len(full) > 3
    for p in layer.parameters():
        p.requires_grad_(False)
    reset(spy)
    frozen = step(layer, 1, x, cz, cl)
    assert route_counts(spy) == dict(ROUTE, made_wgrad=0) and spy["linear"] == 0, spy
    assert torch.equal(frozen[2], full[2]) and torch.equal(frozen[0], full[0]) and torch.equal(frozen[1], full[1])
    assert all(p.grad is None for p in layer.parameters())


# ---- 6. batches ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", (1, 63, 64, 65))
def test_batches_around_the_tile_edge(nfa, spy, B):
    layer, x, cz, cl, _ = fixture(nfa, "a")
    for direction in (0, 1):
        reset(spy)
        got = step(layer, direction, x[:B], cz[:B], cl[:B])
        assert route_counts(spy) == ROUTE, spy
        compare(layer, got, layerwise(nfa, layer, direction, x[:B], cz[:B], cl[:B]), "B %d direction %d" % (B, direction))


def test_two_runs_are_bit_identical(nfa):
    layer, x, cz, cl, _ = fixture(nfa, "a")
    for direction in (0, 1):
        one, two = step(layer, direction, x, cz, cl), step(layer, direction, x, cz, cl)
        assert all(torch.equal(a, b) for a, b in zip(one, two))


# ---- 7. live parameters --------------------------------------------------------------------------------------------------------------
def test_three_adam_steps_follow_the_live_parameters(nfa, spy):
    """The pack is gathered from the parameters of THIS call: three fused-Adam steps from the same start, route on against off."""
    _, x, _, _, _ = fixture(nfa, "b")

    def train(on):
        nfa.config.set_affine_wide_train(on)
        layer = fresh(nfa, "b")
        opt = torch.optim.Adam(layer.parameters(), lr=1e-3, fused=True)
        losses = []
        for _ in range(3):
            opt.zero_grad(set_to_none=True)
            z, ld = layer.inverse(x)
            loss = (0.5 * (z * z).sum(1) - ld).mean()
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
        return losses
    try:
        on = train(True)
        assert route_counts(spy) == {k: 3 for k in ROUTE_OPS} and spy["linear"] == 0, spy
        off = train(False)
    finally:
        nfa.config.set_affine_wide_train(True)
    assert on[0] != on[2]
    for a, b in zip(on, off):
        assert abs(a - b) <= 1e-5 * abs(b), (on, off)


# ---- 8. a stacked model --------------------------------------------------------------------------------------------------------------
def test_stacked_model_forward_kld(nfa, spy):
    first = fresh(nfa, "a")
    torch.manual_seed(77)
    b2 = 1.0 - torch.from_numpy(cases.mask(cases.CASES["a"]))
    second = nfa.flows.MaskedAffineFlow(b2, nfa.nets.MLP([17, 72, 72, 17], init_zeros=False), nfa.nets.MLP([17, 80, 72, 17], init_zeros=False))
    model = nfa.NormalizingFlow(nfa.distributions.DiagGaussian(17), [first, nfa.flows.ActNorm(17), second]).to(DEV)
    x = fixture(nfa, "a")[1]
    with torch.no_grad():
        model.log_prob(x)                     # (ActNorm's data-dependent initialisation)

    def grads():
        model.zero_grad(set_to_none=True)
        loss = model.forward_kld(x)
        loss.backward()
        return float(loss.detach()), [p.grad.clone() for p in model.parameters() if p.grad is not None]
    reset(spy)
    loss, got = grads()
    assert route_counts(spy) == {k: 2 for k in ROUTE_OPS} and spy["linear"] == 0 and layerwise_counts(spy) == 0, spy
    nfa.config.set_affine_wide_train(False)
    try:
        loss0, want = grads()
    finally:
        nfa.config.set_affine_wide_train(True)
    assert abs(loss - loss0) <= 1e-5 * abs(loss0), (loss, loss0)
    assert len(got) == len(want) > 12
    for a, b in zip(got, want):
        assert of_scale(a, b) <= 2e-4, of_scale(a, b)


# ---- 9. outside the route ------------------------------------------------------------------------------------------------------------
def test_declined_layers_and_the_switch(nfa, spy):
    MLP, MAF = nfa.nets.MLP, nfa.flows.MaskedAffineFlow
    alt = lambda d: torch.tensor([1.0 if i % 2 == 0 else 0.0 for i in range(d)])      # noqa: E731
    gen = torch.Generator().manual_seed(5)
    torch.manual_seed(6)
    declined = [(MAF(alt(17), MLP([17, 72, 72, 17], init_zeros=False), MLP([17, 72, 72, 17], init_zeros=False)).double(), torch.float64),
                (MAF(alt(16), MLP([16, 64, 64, 16], init_zeros=False), MLP([16, 64, 64, 16], init_zeros=False)), torch.float32),
                (MAF(alt(17), MLP([17, 72, 17], init_zeros=False), None), torch.float32)]
    for layer, dt in declined:
        layer = layer.to(DEV)
        d = layer.b.numel()
        x = torch.randn(20, d, generator=gen).to(DEV, dt).requires_grad_(True)
        z, ld = layer.inverse(x)
        (z.sum() + ld.sum()).backward()
        assert sum(route_counts(spy).values()) == 0, spy
        assert x.grad is not None and all(p.grad is not None for p in layer.parameters())
    # inside higher_order_gradients() the torch modules run, and a double backward succeeds
    layer, x, cz, cl, _ = fixture(nfa, "a")
    layer = copy.deepcopy(layer)
    reset(spy)
    with nfa.config.higher_order_gradients():
        xx = x.clone().requires_grad_(True)
        z, ld = layer.inverse(xx)
        gx, = torch.autograd.grad((z * cz).sum() + (ld * cl).sum(), xx, create_graph=True)
        assert gx.requires_grad
        gx.pow(2).sum().backward()
    assert sum(route_counts(spy).values()) == 0 and spy["linear"] >= 3, spy
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in layer.parameters())
    # the route is once-differentiable: a double backward through it raises instead of returning a wrong number
    xx = x.clone().requires_grad_(True)
    z, ld = layer.inverse(xx)
    gx, = torch.autograd.grad((z * cz).sum(), xx, create_graph=True)
    with pytest.raises(RuntimeError):
        gx.pow(2).sum().backward()
    # with the switch off the route's ops are never called
    nfa.config.set_affine_wide_train(False)
    reset(spy)
    step(layer, 1, x, cz, cl)
    nfa.config.set_affine_wide_train(True)
    assert sum(route_counts(spy).values()) == 0 and spy["linear"] >= 3 and layerwise_counts(spy) == 2, spy


# ---- 10. captured and replayed -------------------------------------------------------------------------------------------------------
def _captured(layer, x, cz, cl, replays=2):
    """The gradients of `replays` replays of one training step captured after the usual side-stream warm-up."""
    def one_step():
        layer.zero_grad(set_to_none=True)
        z, ld = layer.inverse(x)
        ((z * cz).sum() + (ld * cl).sum()).backward()

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            one_step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    layer.zero_grad(set_to_none=True)
    with torch.cuda.graph(graph):
        z, ld = layer.inverse(x)
        ((z * cz).sum() + (ld * cl).sum()).backward()
    captured = [p.grad for p in layer.parameters()]
    out = []
    for _ in range(replays):
        graph.replay()
        torch.cuda.synchronize()
        out.append([t.clone() for t in captured])
    return out


def test_training_step_captured_and_replayed(nfa, spy):
    _, x, cz, cl, _ = fixture(nfa, "b")
    layer = fresh(nfa, "b")
    B = x.shape[0]
    eager = step(layer, 1, x, cz, cl, x_grad=False)[3:]
    layerwise(nfa, layer, 1, x, cz, cl, x_grad=False)                    # (the library GEMMs of this shape have run before a capture)
    nfa.config.set_affine_wide_train(True, capture_min_batch=B)          # at the gate: the route is captured
    reset(spy)
    one, two = _captured(layer, x, cz, cl)
    assert route_counts(spy) == {k: 3 for k in ROUTE_OPS} and spy["linear"] == 0, spy      # two warm-up steps and the captured one
    assert len(one) == len(eager) and all(torch.equal(a, b) for a, b in zip(one, two))
    for a, b in zip(one, eager):
        assert of_scale(a, b) <= 2e-4
    nfa.config.set_affine_wide_train(True, capture_min_batch=B + 1)      # below the gate: the layer-wise launches are captured
    reset(spy)
    one, two = _captured(layer, x, cz, cl)
    assert route_counts(spy) == {k: 2 for k in ROUTE_OPS}, spy            # the eager warm-up steps only
    assert spy["linear"] >= 3 and layerwise_counts(spy) == 2, spy
    assert all(torch.equal(a, b) for a, b in zip(one, two))
    for a, b in zip(one, eager):
        assert of_scale(a, b) <= 2e-4
