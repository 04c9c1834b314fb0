"""GPU tests of the gated ResidualNet conditioner under autograd (autograd.ResNetCtxFn, csrc/resnet_ctx_train.hip): the route (one
training forward and one backward per conditional coupling layer, no eager GLU), the differential against the eager conditioner
(config.set_nsf_context_train(False)) over batches, depths, widths and both directions, bit properties (run-to-run, row
permutation, stride-0 context), gradient accumulation, hipGraph capture, and unchanged context-free models."""
import numpy as np
import pytest
import torch

from conftest import load_golden as load_fixture

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def nfa():
    import normflows_amd
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    normflows_amd._lib.lib()
    return normflows_amd


@pytest.fixture
def eager(nfa):
    """A context manager that switches the new route off for its body."""
    class _Off:
        def __enter__(self):
            nfa.config.set_nsf_context_train(False)

        def __exit__(self, *exc):
            nfa.config.set_nsf_context_train(True)
            return False
    return _Off


def _layer(nfa, D, C, H, NB=2, K=8, seed=0, sigma=0.05):
    torch.manual_seed(seed)
    layer = nfa.flows.CoupledRationalQuadraticSpline(D, NB, H, num_context_channels=C, num_bins=K, init_identity=False)
    with torch.no_grad():
        for p in layer.parameters():
            p.add_(sigma * torch.randn_like(p))
    return layer.to(DEV)


def _rows(B, D, C, seed):
    g = torch.Generator().manual_seed(seed)
    return (1.5 * torch.randn(B, D, generator=g)).to(DEV), torch.randn(B, C, generator=g).to(DEV)


def _step(layer, x, c, sample=False, ctx_grad=False):
    """loss of one direction of the layer, backward; (loss, x.grad, context.grad, {name: grad})."""
    layer.zero_grad(set_to_none=True)
    x = x.clone().requires_grad_(True)
    c = c.clone().requires_grad_(ctx_grad)
    z, ld = (layer.forward if sample else layer.inverse)(x, c)
    loss = (0.5 * z.pow(2).sum(1) - ld).mean()
    loss.backward()
    return (loss.detach(), x.grad, c.grad if ctx_grad else None,
            {k: p.grad.detach().clone() for k, p in layer.named_parameters() if p.grad is not None})


def _close(a, b, what, bar=2e-4):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    scale = max(float(b.abs().max()), 1e-6)
    err = float((a - b).abs().max()) / scale
    assert err <= bar, (what, err)


def _close_rows(a, b, what, bar=2e-4):
    """Per-row gradients (g_x, g_context): every row within the bar except rows on a kink of the network -- a ReLU input or a spline
    input within float32 rounding of its switch point, where the two evaluation orders land on opposite sides and the row's gradient
    takes the other one-sided value.  At most one such row in 10 000 (and 2 in any batch)."""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    scale = max(float(b.abs().max()), 1e-6)
    row = (a - b).abs().amax(1) / scale
    bad = int((row > bar).sum())
    assert bad <= max(2, a.shape[0] // 10000), (what, bad, float(row.max()))


def _net_keys(grads):
    """The conditioner's parameters (the batch-shared spline parameters of the unconditional transform are reduced elsewhere)."""
    return [k for k in grads if ".transform_net." in k]


class _Spy:
    def __init__(self, nfa, monkeypatch):
        self.fwd = self.bwd = 0
        rf, rb = nfa.ops.resnet_ctx_forward_train, nfa.ops.resnet_ctx_backward

        def f(*a, **k):
            self.fwd += 1
            return rf(*a, **k)

        def b(*a, **k):
            self.bwd += 1
            return rb(*a, **k)
        monkeypatch.setattr(nfa.ops, "resnet_ctx_forward_train", f)
        monkeypatch.setattr(nfa.ops, "resnet_ctx_backward", b)
        self.glu = 0
        real_glu = torch.nn.functional.glu

        def glu(*a, **k):
            self.glu += 1
            return real_glu(*a, **k)
        monkeypatch.setattr(torch.nn.functional, "glu", glu)
        self.ctx_linear = 0
        real_lin = torch.nn.Linear.forward

        def lin(mod, *a, **k):
            self.ctx_linear += 1
            return real_lin(mod, *a, **k)
        monkeypatch.setattr(torch.nn.Linear, "forward", lin)


def _model(nfa, seed=0, n=4, D=2, C=4, H=128):
    torch.manual_seed(seed)
    flows = []
    for _ in range(n):
        flows += [nfa.flows.CoupledRationalQuadraticSpline(D, 2, H, num_context_channels=C, init_identity=False),
                  nfa.flows.LULinearPermute(D)]
    m = nfa.ConditionalNormalizingFlow(nfa.distributions.DiagGaussian(D), flows)
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.05 * torch.randn_like(p))
    return m.to(DEV)


def test_route_spy(nfa, monkeypatch, eager):
    """The notebook's model: one forward_kld + backward runs the new forward and backward once per coupling layer; neither F.glu nor
    the blocks' context_layer (torch.nn.Linear) runs.  With the switch off the eager modules run again."""
    m = _model(nfa)
    x, c = _rows(1000, 2, 4, 1)
    spy = _Spy(nfa, monkeypatch)
    m.forward_kld(x, c).backward()
    assert (spy.fwd, spy.bwd, spy.glu, spy.ctx_linear) == (4, 4, 0, 0)
    with eager():
        m.zero_grad()
        m.forward_kld(x, c).backward()
    assert (spy.fwd, spy.bwd) == (4, 4) and spy.glu == 8 and spy.ctx_linear == 8


def test_model_step_matches_eager(nfa, eager):
    m = _model(nfa)
    x, c = _rows(1000, 2, 4, 2)
    loss = m.forward_kld(x, c)
    loss.backward()
    got = {k: p.grad.clone() for k, p in m.named_parameters()}
    m.zero_grad(set_to_none=True)
    with eager():
        ref_loss = m.forward_kld(x, c)
        ref_loss.backward()
    assert abs(float(loss.detach()) - float(ref_loss.detach())) <= 1e-5 * abs(float(ref_loss)) + 1e-6
    for k, p in m.named_parameters():
        _close(got[k], p.grad, k)


SHAPES = [(6, 3, 40, 2), (64, 16, 136, 1), (17, 33, 200, 3), (16, 4, 128, 4), (64, 16, 256, 2)]


@pytest.mark.parametrize("B,D,C,H,NB", [(B,) + s for B in (1, 63, 64, 1000) for s in SHAPES] + [(65537, 64, 16, 256, 2)])
def test_layer_vs_eager(nfa, eager, monkeypatch, B, D, C, H, NB):
    from normflows_amd.flows import ctx_train_pack
    monkeypatch.setattr(ctx_train_pack, "MAX_ROWS", 1 << 30)       # (the kernels at every batch, above the route's limit too)
    layer = _layer(nfa, D, C, H, NB, seed=D + H)
    x, c = _rows(B, D, C, B + D)
    for sample in (False, True):
        got = _step(layer, x, c, sample, ctx_grad=True)
        with eager():
            ref = _step(layer, x, c, sample, ctx_grad=True)
        what = "B%d D%d C%d H%d NB%d %s" % (B, D, C, H, NB, "sample" if sample else "density")
        assert abs(float(got[0]) - float(ref[0])) <= 1e-5 * abs(float(ref[0])) + 1e-6, what
        _close_rows(got[1], ref[1], what + " g_x")
        _close_rows(got[2], ref[2], what + " g_context")
        assert set(got[3]) == set(ref[3])
        for k in ref[3]:
            _close(got[3][k], ref[3][k], what + " " + k, bar=1e-3)


def test_context_with_requires_grad_through_embedding(nfa, eager):
    layer = _layer(nfa, 8, 5, 64)
    emb = torch.nn.Linear(3, 5).to(DEV)
    x, _ = _rows(300, 8, 5, 3)
    raw = torch.randn(300, 3, device=DEV)

    def run():
        layer.zero_grad(set_to_none=True)
        emb.zero_grad(set_to_none=True)
        z, ld = layer.inverse(x, emb(raw))
        (z.square().sum() - ld.sum()).backward()
        return [p.grad.clone() for p in list(emb.parameters()) + list(layer.parameters())]
    got = run()
    with eager():
        ref = run()
    for a, b in zip(got, ref):
        _close(a, b, "embedding net")


def test_bits_determinism_permutation_stride0(nfa):
    layer = _layer(nfa, 64, 16, 256)
    x, c = _rows(3000, 64, 16, 4)
    a, b = _step(layer, x, c, ctx_grad=True), _step(layer, x, c, ctx_grad=True)
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    for k in _net_keys(a[3]):
        assert torch.equal(a[3][k], b[3][k]), k
    perm = torch.randperm(3000, generator=torch.Generator().manual_seed(0)).to(DEV)
    p = _step(layer, x[perm], c[perm], ctx_grad=True)
    assert torch.equal(p[1], a[1][perm]) and torch.equal(p[2], a[2][perm])
    # a stride-0 context gives the same forward bits as the materialised one
    c1 = torch.randn(1, 16, device=DEV)
    xr = x.clone().requires_grad_(True)
    z0, l0 = layer.inverse(xr, c1.expand(3000, 16))
    z1, l1 = layer.inverse(xr, c1.expand(3000, 16).contiguous())
    assert torch.equal(z0, z1) and torch.equal(l0, l1)


def test_accumulation_two_batches_and_two_losses(nfa):
    layer = _layer(nfa, 16, 4, 128)
    x1, c1 = _rows(700, 16, 4, 5)
    x2, c2 = _rows(900, 16, 4, 6)
    g1 = _step(layer, x1, c1)[3]
    g2 = _step(layer, x2, c2)[3]
    layer.zero_grad(set_to_none=True)
    for x, c in ((x1, c1), (x2, c2)):
        z, ld = layer.inverse(x, c)
        (0.5 * z.pow(2).sum(1) - ld).mean().backward()
    for k, p in layer.named_parameters():
        if k in _net_keys(g1):
            assert torch.equal(p.grad, g1[k] + g2[k]), k
        else:
            _close(p.grad, g1[k] + g2[k], k, bar=1e-6)
    # two losses in one graph
    layer.zero_grad(set_to_none=True)
    za, la = layer.inverse(x1, c1)
    zb, lb = layer.inverse(x2, c2)
    ((0.5 * za.pow(2).sum(1) - la).mean() + (0.5 * zb.pow(2).sum(1) - lb).mean()).backward()
    for k, p in layer.named_parameters():
        _close(p.grad, g1[k] + g2[k], "two losses " + k, bar=1e-6)


def test_accumulation_flat_parameters(nfa):
    from normflows_amd import dp
    m = _model(nfa, n=2, D=8, C=4, H=64)
    x1, c1 = _rows(500, 8, 4, 7)
    x2, c2 = _rows(600, 8, 4, 8)
    flat = dp.FlatParameters(m)
    gs = []
    for x, c in ((x1, c1), (x2, c2)):
        flat.zero_grad()
        m.forward_kld(x, c).backward()
        flat.sync()
        gs.append(flat.param.grad.clone())
    flat.zero_grad()
    m.forward_kld(x1, c1).backward()
    m.forward_kld(x2, c2).backward()
    flat.sync()
    _close(flat.param.grad, gs[0] + gs[1], "two micro-batches", bar=1e-6)
    flat.zero_grad()
    (m.forward_kld(x1, c1) + m.forward_kld(x2, c2)).backward()
    flat.sync()
    _close(flat.param.grad, gs[0] + gs[1], "two losses", bar=1e-6)


def test_graph_capture_replay_matches_eager_step(nfa):
    layer = _layer(nfa, 16, 4, 128)
    x, c = _rows(1024, 16, 4, 9)
    xs, cs = x.clone(), c.clone()
    ref = _step(layer, x, c)
    for p in layer.parameters():
        p.grad = torch.zeros_like(p)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            for p in layer.parameters():
                p.grad.zero_()
            z, ld = layer.inverse(xs, cs)
            (0.5 * z.pow(2).sum(1) - ld).mean().backward()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    for p in layer.parameters():
        p.grad.zero_()
    with torch.cuda.graph(g):
        z, ld = layer.inverse(xs, cs)
        (0.5 * z.pow(2).sum(1) - ld).mean().backward()
    for p in layer.parameters():
        p.grad.zero_()
    g.replay()
    torch.cuda.synchronize()
    for k, p in layer.named_parameters():
        if k in _net_keys(ref[3]):
            assert torch.equal(p.grad, ref[3][k]), k
        else:
            _close(p.grad, ref[3][k], k, bar=1e-6)


def test_context_free_unchanged(nfa, eager, monkeypatch):
    torch.manual_seed(0)
    layer = nfa.flows.CoupledRationalQuadraticSpline(16, 2, 160, init_identity=False).to(DEV)
    x = torch.randn(512, 16, device=DEV)

    def run():
        layer.zero_grad(set_to_none=True)
        xr = x.clone().requires_grad_(True)
        z, ld = layer.inverse(xr)
        loss = (z.square().sum(1) - ld).mean()
        loss.backward()
        return [loss.detach(), xr.grad] + [p.grad.clone() for p in layer.prqct.transform_net.parameters()]
    spy = _Spy(nfa, monkeypatch)
    a = run()
    with eager():
        b = run()
    assert spy.fwd == 0 and spy.bwd == 0
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def test_higher_order_gradients_take_the_eager_path(nfa, monkeypatch):
    layer = _layer(nfa, 6, 3, 40)
    x, c = _rows(50, 6, 3, 10)
    spy = _Spy(nfa, monkeypatch)
    with nfa.config.higher_order_gradients():
        xr = x.clone().requires_grad_(True)
        z, ld = layer.inverse(xr, c)
        (g,) = torch.autograd.grad(z.square().sum() - ld.sum(), xr, create_graph=True)
        g.square().sum().backward()
    assert spy.fwd == 0 and spy.glu > 0


def test_route_declines_large_batches(nfa, monkeypatch):
    """Above ctx_train_pack.MAX_ROWS rows the eager conditioner runs (the kernels are slower there)."""
    from normflows_amd.flows import ctx_train_pack
    layer = _layer(nfa, 16, 4, 64)
    spy = _Spy(nfa, monkeypatch)
    x, c = _rows(ctx_train_pack.MAX_ROWS, 16, 4, 11)
    _step(layer, x, c)
    assert spy.fwd == 1 and spy.bwd == 1
    x, c = _rows(ctx_train_pack.MAX_ROWS + 1, 16, 4, 12)
    _step(layer, x, c)
    assert spy.fwd == 1 and spy.bwd == 1 and spy.glu == 2


# ---- parity with the reference's autograd (tests/golden/grad_ctx_*.npz, tests/golden/make_golden_ctx_train.py) ----------------------
REF_LAYERS = {"grad_ctx_d6_c3_h40": ("ctx_d6_c3_h40", 6, 3, 40, 2, 8), "grad_ctx_d64_c16_h136": ("ctx_d64_c16_h136", 64, 16, 136, 1, 4),
              "grad_ctx_d17_c33_h200": ("ctx_d17_c33_h200", 17, 33, 200, 1, 16)}


@pytest.mark.parametrize("name", sorted(REF_LAYERS))
@pytest.mark.parametrize("direction", ["inv", "fwd"])
def test_layer_gradients_vs_reference(nfa, monkeypatch, name, direction):
    """One conditional coupling layer, density (inv) and sampling (fwd) direction, loss sum(z cz) + sum(log_det cl), against the
    reference's autograd: loss within 1e-4 relative, then g_x, g_context and every parameter gradient on the bars of _ref_bars --
    through the new kernels (spy)."""
    g = load_fixture(name)
    src, D, C, H, NB, K = REF_LAYERS[name]
    w = load_fixture(src)
    layer = nfa.flows.CoupledRationalQuadraticSpline(D, NB, H, num_context_channels=C, num_bins=K, init_identity=False)
    layer.load_state_dict({k[4:].replace("__", "."): torch.from_numpy(v) for k, v in w.items() if k.startswith("sd__")}, strict=True)
    layer = layer.to(DEV)
    spy = _Spy(nfa, monkeypatch)
    x = torch.from_numpy(g["x"]).to(DEV).requires_grad_(True)
    c = torch.from_numpy(g["context"]).to(DEV).requires_grad_(True)
    z, ld = (layer.inverse if direction == "inv" else layer.forward)(x, c)
    loss = (z * torch.from_numpy(g["cz"]).to(DEV)).sum() + (ld * torch.from_numpy(g["cl"]).to(DEV)).sum()
    loss.backward()
    assert (spy.fwd, spy.bwd, spy.glu) == (1, 1, 0)
    _check_against(g, "_" + direction, layer, x.grad, c.grad, float(loss.detach()), name + " " + direction)


def _check_against(g, sfx, module, gx, gc, loss, what):
    ref = float(g["loss_f32" + sfx])
    assert abs(loss - ref) <= 1e-4 * abs(ref), (what, loss, ref)
    stride = int(g["stride"])
    items, bad = [], []
    for nm, ours, key in (("g_x", gx, "gx"), ("g_context", gc, "gc")):
        items.append((nm, ours.detach().cpu().numpy(), key))
    for k, p in module.named_parameters():
        key = k.replace(".", "__")
        flat = np.zeros(p.numel(), np.float32) if p.grad is None else p.grad.detach().cpu().numpy().reshape(-1)
        chk = g["chk_f64%s__%s" % (sfx, key)]
        assert abs(float(flat.astype(np.float64).sum()) - chk[0]) <= 1e-4 * max(chk[1], 1e-6), (what, k, float(flat.sum()), chk)
        items.append((k, flat[::stride], None))
    own, got = [], []
    for nm, ours, key in items:
        r32 = g[("%s_f32%s" % (key, sfx)) if key else ("g_f32%s__%s" % (sfx, nm.replace(".", "__")))]
        r64 = g[("%s_f64%s" % (key, sfx)) if key else ("g_f64%s__%s" % (sfx, nm.replace(".", "__")))]
        scale = max(float(np.abs(r64).max()), 1e-6)
        ours = np.asarray(ours, dtype=np.float64).reshape(r32.shape)
        e32 = float(np.abs(ours - r32).max()) / scale
        if not e32 <= 3e-3:
            bad.append((nm, e32))
        own.append(float(np.abs(r32 - r64).max()) / scale)
        got.append(float(np.abs(ours - r64).max()) / scale)
    assert not bad, (what, bad)
    assert np.quantile(got, 0.9) <= 4 * max(np.quantile(own, 0.9), 1e-7), (what, np.quantile(got, 0.9), np.quantile(own, 0.9))


def _notebook_model(nfa, seed=11):
    """tests/golden/make_golden_ctx_train.py build_model: the same seeded construction gives the reference's weights."""
    torch.manual_seed(seed)
    flows = []
    for _ in range(4):
        flows += [nfa.flows.CoupledRationalQuadraticSpline(2, 2, 128, num_context_channels=4, init_identity=False),
                  nfa.flows.LULinearPermute(2)]
    m = nfa.ConditionalNormalizingFlow(nfa.distributions.DiagGaussian(2), flows)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.05 * torch.randn(p.shape, generator=g, dtype=p.dtype))
    return m


def test_notebook_model_gradients_vs_reference(nfa, monkeypatch):
    """examples/conditional_flow.ipynb's model, forward_kld(x, context) + backward, against the reference's autograd: the weights are
    the fixture's (checksums), the loss within 1e-4, g_x, g_context and every parameter gradient on the bars; 4 new forwards and
    backwards, no GLU."""
    g = load_fixture("grad_ctx_model_nsf")
    m = _notebook_model(nfa)
    for k, p in m.named_parameters():
        chk = g["w__" + k.replace(".", "__")]
        assert abs(float(p.detach().double().sum()) - chk[0]) <= 1e-6 * max(chk[1], 1.0), k
    m = m.to(DEV)
    spy = _Spy(nfa, monkeypatch)
    x = torch.from_numpy(g["x"]).to(DEV).requires_grad_(True)
    c = torch.from_numpy(g["context"]).to(DEV).requires_grad_(True)
    loss = m.forward_kld(x, c)
    loss.backward()
    assert (spy.fwd, spy.bwd, spy.glu, spy.ctx_linear) == (4, 4, 0, 0)
    _check_against(g, "_kld", m, x.grad, c.grad, float(loss.detach()), "notebook model")


def test_empty_batch_gives_zero_gradients(nfa, monkeypatch):
    """B = 0 through the new route: nothing is launched and every parameter gradient is zero (as autograd through the eager
    modules gives), not the contents of an uninitialised buffer."""
    layer = _layer(nfa, 16, 4, 64)
    net = layer.prqct.transform_net
    spy = _Spy(nfa, monkeypatch)
    for _ in range(2):
        junk = torch.full((1 << 20,), float("nan"), device=DEV)      # (freed memory the caching allocator hands out again)
        del junk
        net.zero_grad(set_to_none=True)
        x = torch.zeros(0, 8, device=DEV, requires_grad=True)
        c = torch.zeros(0, 4, device=DEV, requires_grad=True)
        net(x, c).sum().backward()
        for k, p in net.named_parameters():
            assert p.grad is not None and torch.equal(p.grad, torch.zeros_like(p)), k
        assert x.grad.shape == (0, 8) and c.grad.shape == (0, 4)
    assert spy.fwd == 2 and spy.bwd == 2
