"""GPU tests of the one-launch wide RealNVP coupling layer (nf_affine_wide; run with -m gpu on an MI355X): every fixture of
tests/affine_wide_cases.py in both directions against the REFERENCE's stored outputs and against the layer-wise route
(config.affine_wide off) at the bars of the other one-launch-vs-reference tests (outputs rtol = atol = 1e-4, log-det
conftest.ld_tol), with spies on the launches; identity columns, non-finite rows, batch sizes, accumulation modes, the second tile of
a persistent workgroup, views, stacked models eager and graph-replayed, the pack cache, and the autograd route."""
import numpy as np
import pytest
import torch

import affine_wide_cases as cases
from conftest import assert_close, golden_state, ld_tol, load_golden

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = dict(rtol=1e-4, atol=1e-4)
NAMES = sorted(cases.CASES)


@pytest.fixture(scope="module")
def nfa():
    import normflows_amd
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    assert normflows_amd.native_library_path().endswith("normalizing-flows_amd/lib/libnf_mi355x.so")
    normflows_amd._lib.lib()
    return normflows_amd


@pytest.fixture(autouse=True)
def _inference(nfa):
    with torch.no_grad():
        yield
    nfa.config.set_affine_wide(True)


@pytest.fixture
def spy(nfa, monkeypatch):
    """Counts of the calls that tell the two routes apart."""
    log = {"affine_wide": 0, "masked_affine": 0, "affine_coupling": 0, "linear": 0}

    def counted(key, fn):
        def f(*a, **k):
            log[key] += 1
            return fn(*a, **k)
        return f
    for k in ("affine_wide", "masked_affine", "affine_coupling"):
        monkeypatch.setattr(nfa.ops, k, counted(k, getattr(nfa.ops, k)))
    monkeypatch.setattr(torch.nn.functional, "linear", counted("linear", torch.nn.functional.linear))
    monkeypatch.setattr(torch.nn.Linear, "forward", counted("linear", torch.nn.Linear.forward))
    return log


_LAYERS = {}


def layer_of(nfa, name):
    """(layer on the GPU, fixture, x on the GPU): built once per module, never modified by the tests that share it."""
    if name not in _LAYERS:
        g = load_golden("affine_wide_" + name)
        layer = cases.build(nfa, name)
        layer.load_state_dict({k: torch.from_numpy(v) for k, v in golden_state(g).items()})
        _LAYERS[name] = (layer.to(DEV), g, torch.from_numpy(g["x"]).to(DEV))
    return _LAYERS[name]


def fresh_layer(nfa, name):
    g = load_golden("affine_wide_" + name)
    layer = cases.build(nfa, name)
    layer.load_state_dict({k: torch.from_numpy(v) for k, v in golden_state(g).items()})
    return layer.to(DEV), torch.from_numpy(g["x"]).to(DEV)


def N(t):
    return t.detach().cpu().numpy()


def run(layer, x, direction):
    return layer.inverse(x) if direction else layer.forward(x)


def identity_columns(nfa, name):
    from normflows_amd.flows import affine_wide_pack as awp
    layer = layer_of(nfa, name)[0]
    return np.nonzero(awp.slot_layers(layer, cases.CASES[name]["d"])["modes"] == 0)[0]


@pytest.mark.parametrize("direction", (0, 1))
@pytest.mark.parametrize("name", NAMES)
def test_one_launch_against_the_reference_and_the_layerwise_route(nfa, spy, name, direction):
    layer, g, x = layer_of(nfa, name)
    leg = "inv" if direction else "fwd"
    y, ld = run(layer, x, direction)
    assert spy == {"affine_wide": 1, "masked_affine": 0, "affine_coupling": 0, "linear": 0}, spy
    assert_close(N(y), g["y_" + leg], what="y vs reference", **TOL)
    assert_close(N(ld), g["ld_" + leg], what="ld vs reference", **ld_tol(np.float32))
    nfa.config.set_affine_wide(False)
    y0, ld0 = run(layer, x, direction)
    nfa.config.set_affine_wide(True)
    assert spy["affine_wide"] == 1 and spy["masked_affine"] + spy["affine_coupling"] == 1 and spy["linear"] >= 3, spy
    assert_close(N(y0), g["y_" + leg], what="layer-wise y vs reference", **TOL)
    assert_close(N(ld0), g["ld_" + leg], what="layer-wise ld vs reference", **ld_tol(np.float32))
    assert_close(N(y), N(y0), what="y vs layer-wise", **TOL)
    assert_close(N(ld), N(ld0), what="ld vs layer-wise", **ld_tol(np.float32))
    idt = identity_columns(nfa, name)
    assert idt.size and torch.equal(y[:, idt], x[:, idt])                   # identity columns: z bit for bit
    if name in ("d", "h"):                                                  # no scale parameter: exactly 0 (h: shift only)
        assert not bool(ld.any())


@pytest.mark.parametrize("name", ("a", "c", "d", "e", "f"))
def test_non_finite_rows_land_where_the_layerwise_route_puts_them(nfa, name):
    """inf in a transformed column, inf in an identity column, NaN in a transformed column, and a last-layer bias of each net forced
    to inf: NaN / inf in the same places as the layer-wise route, every untouched row as before."""
    layer, x0 = fresh_layer(nfa, name)
    idt = identity_columns(nfa, name)
    tr = np.setdiff1d(np.arange(x0.shape[1]), idt)
    x = x0[:40].clone()
    x[3, int(tr[1])] = float("inf")
    x[7, int(idt[1])] = float("inf")
    x[11, int(tr[0])] = float("nan")
    x[13, int(tr[-1])] = float("-inf")

    def both(direction):
        nfa.config.set_affine_wide(True)
        a = run(layer, x, direction)
        nfa.config.set_affine_wide(False)
        b = run(layer, x, direction)
        nfa.config.set_affine_wide(True)
        return a, b
    for direction in (0, 1):
        (y, ld), (y0, ld0) = both(direction)
        assert torch.equal(torch.isnan(y), torch.isnan(y0)) and torch.equal(torch.isinf(y), torch.isinf(y0)), direction
        assert torch.equal(torch.isnan(ld), torch.isnan(ld0)) and torch.equal(torch.isinf(ld), torch.isinf(ld0)), direction
        assert int(torch.isnan(y0).sum()) + int(torch.isinf(y0).sum()) >= 4
        assert_close(N(y), N(y0), what="y", **TOL)
        assert_close(N(ld), N(ld0), what="ld", **ld_tol(np.float32))
    lasts = [[m for m in net.net if isinstance(m, torch.nn.Linear)][-1] for net in layer.modules() if type(net).__name__ == "MLP"]
    for lin in lasts:                                                   # (a masked flow: s and t in turn; a block: its param_map)
        for row in (0, lin.out_features - 1):
            old = float(lin.bias[row])
            lin.bias[row] = float("inf")
            for direction in (0, 1):
                (y, ld), (y0, ld0) = both(direction)
                assert torch.equal(torch.isnan(y), torch.isnan(y0)) and torch.equal(torch.isinf(y), torch.isinf(y0)), (row, direction)
                assert torch.equal(torch.isnan(ld), torch.isnan(ld0)) and torch.equal(torch.isinf(ld), torch.isinf(ld0)), (row, direction)
                assert bool((torch.isnan(y0) | torch.isinf(y0)).any())
                assert_close(N(y), N(y0), what="y, bias inf", **TOL)
            lin.bias[row] = old


@pytest.mark.parametrize("name", NAMES)
def test_batches_repeat_bit_for_bit_and_the_accumulation_modes_agree(nfa, spy, name):
    layer, g, x = layer_of(nfa, name)
    for direction in (0, 1):
        full = run(layer, x, direction)
        for B in (1, 64, 129):
            y, ld = run(layer, x[:B], direction)
            y2, ld2 = run(layer, x[:B], direction)
            assert torch.equal(y, full[0][:B]) and torch.equal(ld, full[1][:B]), (direction, B)
            assert torch.equal(y, y2) and torch.equal(ld, ld2)
            base = torch.linspace(-1.0, 1.0, B, device=DEV)
            add, sub = base.clone(), base.clone()
            ya = layer._run(x[:B], bool(direction), add, 1)
            ys = layer._run(x[:B], bool(direction), sub, -1)
            assert torch.equal(ya, y) and torch.equal(ys, y)
            assert torch.equal(add, base + ld) and torch.equal(sub, base - ld)
    assert spy["masked_affine"] == 0 and spy["affine_coupling"] == 0 and spy["linear"] == 0 and spy["affine_wide"] == 2 * (1 + 3 * 4)


@pytest.mark.parametrize("name", ("a", "b"))
def test_second_tile_of_a_persistent_workgroup(nfa, spy, name):
    """B = 256 x 64 + 64 + 1 rows: workgroups 0 and 1 walk a second tile (the ring wraps into it) and the last tile holds one row; rows
    [16 384, B) and [0, 64) equal fresh calls on those rows alone bit for bit."""
    layer, g, x = layer_of(nfa, name)
    B = 256 * 64 + 64 + 1
    big = x[torch.arange(B, device=DEV) % x.shape[0]] + 0.001 * torch.arange(B, device=DEV, dtype=torch.float32)[:, None] / B
    for direction in (0, 1):
        y, ld = run(layer, big, direction)
        for lo, hi in ((16384, B), (0, 64)):
            ys, lds = run(layer, big[lo:hi].clone(), direction)
            assert torch.equal(y[lo:hi], ys) and torch.equal(ld[lo:hi], lds), (direction, lo)
    assert spy["affine_wide"] == 6 and spy["linear"] == 0


@pytest.mark.parametrize("kind", ("elem1", "elem2", "elem3", "row1", "cols", "rows2", "tr"))
@pytest.mark.parametrize("name", ("a", "b"))
def test_views_of_z(nfa, spy, name, kind):
    """z as an offset / strided / misaligned view inside NaN-filled storage (tests/test_gpu_views.py): the result on a clone bit for
    bit, the storage around the view untouched."""
    from test_gpu_views import bits, embed
    layer, g, x = layer_of(nfa, name)
    for direction in (0, 1):
        want = run(layer, x.clone(), direction)
        view, base = embed(x, kind)
        before = bits(base).clone()
        got = run(layer, view, direction)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (kind, direction)
        assert torch.equal(bits(base), before)
    assert spy["affine_wide"] == 4 and spy["linear"] == 0


def _model(nfa, kind, seed=5):
    """4 x [MaskedAffineFlow(wide), ActNorm] (d 20) or 4 x [AffineCouplingBlock(wide), Permute] (d 21), last layers small."""
    torch.manual_seed(seed)
    flows = []
    if kind == "masked":
        d = 20
        b = torch.tensor([1.0 if i % 2 == 0 else 0.0 for i in range(d)])
        for i in range(4):
            flows += [nfa.flows.MaskedAffineFlow(b if i % 2 == 0 else 1 - b, nfa.nets.MLP([d, 72, 80, d], init_zeros=False),
                                                 nfa.nets.MLP([d, 96, 96, d], init_zeros=False)), nfa.flows.ActNorm(d)]
    else:
        d = 21
        for i in range(4):
            flows += [nfa.flows.AffineCouplingBlock(nfa.nets.MLP([11, 130, 130, 20], init_zeros=False), scale_map=("exp", "sigmoid")[i % 2]),
                      nfa.flows.Permute(d, mode="shuffle")]
    m = nfa.NormalizingFlow(nfa.distributions.DiagGaussian(d, trainable=False), flows).to(DEV)
    m.log_prob(torch.randn(256, d, device=DEV))          # ActNorm's data-dependent initialisation
    return m, d


@pytest.mark.parametrize("kind", ("masked", "block"))
def test_stacked_models_eager_and_graph_replayed(nfa, spy, kind):
    m, d = _model(nfa, kind)
    gen = torch.Generator().manual_seed(11)
    x, eps = torch.randn(300, d, generator=gen).to(DEV), torch.randn(300, d, generator=gen).to(DEV)
    for k in spy:
        spy[k] = 0
    lp = m.log_prob(x)
    xs, lq = m.sample_from_noise(eps)
    assert spy == {"affine_wide": 8, "masked_affine": 0, "affine_coupling": 0, "linear": 0}, spy
    nfa.config.set_affine_wide(False)
    lp0 = m.log_prob(x)
    xs0, lq0 = m.sample_from_noise(eps)
    nfa.config.set_affine_wide(True)
    assert spy["affine_wide"] == 8 and spy["masked_affine"] + spy["affine_coupling"] == 8
    assert_close(N(lp), N(lp0), what="log_prob", **ld_tol(np.float32))
    assert_close(N(xs), N(xs0), what="samples", **TOL)
    assert_close(N(lq), N(lq0), what="log q", **ld_tol(np.float32))
    # recorded for graph replay, a batch below config.affine_wide_graph_min_batch keeps the layer-wise launches (the warm-up call and
    # the capture alike); from that size on, or with the gate at 0, the replay is the one launch and equals the eager call bit for bit
    gate = nfa.config.affine_wide_graph_min_batch
    assert 300 < gate <= 65536
    big, big_eps = x[torch.arange(gate, device=DEV) % 300] * 1.01, eps[torch.arange(gate, device=DEV) % 300] * 1.01
    lp_big, (xs_big, lq_big) = m.log_prob(big), m.sample_from_noise(big_eps)
    before = dict(spy)
    m.use_graphs(True)
    try:
        for _ in range(2):
            assert_close(N(m.log_prob(x)), N(lp0), what="gated replay", **ld_tol(np.float32))
        assert spy["affine_wide"] == before["affine_wide"] and spy["masked_affine"] + spy["affine_coupling"] > 8
        for _ in range(2):
            assert torch.equal(m.log_prob(big), lp_big)
            out = m.sample_from_noise(big_eps)
            assert torch.equal(out[0], xs_big) and torch.equal(out[1], lq_big)
        assert spy["affine_wide"] == before["affine_wide"] + 2 * 8       # (the warm-up call and the capture of either pass)
        nfa.config.set_affine_wide(True, graph_min_batch=0)
        m.refresh_graphs()
        for _ in range(2):
            assert torch.equal(m.log_prob(x), lp)
            out = m.sample_from_noise(eps)
            assert torch.equal(out[0], xs) and torch.equal(out[1], lq)
    finally:
        m.use_graphs(False)
        nfa.config.set_affine_wide(True, graph_min_batch=gate)


@pytest.mark.parametrize("name", ("a", "e"))
def test_pack_follows_parameter_updates(nfa, spy, name):
    """An in-place update and a fused-optimizer step (which leaves Tensor._version alone: _keys.py) each change the output: the pack is
    rebuilt; an unchanged layer reuses it."""
    from normflows_amd.flows import affine_wide_pack as awp
    layer, x = fresh_layer(nfa, name)
    built = []
    real = awp.pack

    def counting(*a, **k):
        built.append(1)
        return real(*a, **k)
    awp.pack = counting
    try:
        y1, ld1 = layer.forward(x)
        y1b, _ = layer.forward(x)
        assert len(built) == 1 and torch.equal(y1, y1b)
        lin = [m for m in layer.modules() if isinstance(m, torch.nn.Linear)][0]
        lin.weight.mul_(1.5)
        y2, ld2 = layer.forward(x)
        assert len(built) == 2 and float((y2 - y1).abs().max()) > 1e-3
        with torch.enable_grad():
            opt = torch.optim.Adam(layer.parameters(), lr=5e-2, fused=True)
            for p in layer.parameters():
                p.grad = torch.ones_like(p)
            opt.step()
        y3, ld3 = layer.forward(x)
        assert len(built) == 3 and float((y3 - y2).abs().max()) > 1e-3
        nfa.config.set_affine_wide(False)
        y3w, ld3w = layer.forward(x)
        nfa.config.set_affine_wide(True)
        assert_close(N(y3), N(y3w), what="after the updates", **TOL)
        assert_close(N(ld3), N(ld3w), what="after the updates", **ld_tol(np.float32))
    finally:
        awp.pack = real
    assert spy["affine_wide"] == 4


@pytest.mark.parametrize("name", ("a", "e"))
def test_route_is_not_taken_under_autograd(nfa, spy, name):
    layer, x = fresh_layer(nfa, name)
    cz = torch.randn(x.shape, generator=torch.Generator().manual_seed(3)).to(DEV)

    def grads():
        layer.zero_grad(set_to_none=True)
        xx = x.clone().requires_grad_(True)
        y, ld = layer.forward(xx)
        ((y * cz).sum() + ld.sum()).backward()
        return [xx.grad.clone()] + [p.grad.clone() for p in layer.parameters()]
    with torch.enable_grad():
        g1 = grads()
        assert spy["affine_wide"] == 0 and spy["linear"] >= 3
        nfa.config.set_affine_wide(False)
        g0 = grads()
        nfa.config.set_affine_wide(True)
    assert len(g1) == len(g0) and all(torch.equal(a, b) for a, b in zip(g1, g0))
    for p in layer.parameters():                 # frozen parameters, gradient-free input: inference, although grad mode is on
        p.requires_grad_(False)
    with torch.enable_grad():
        layer.forward(x)
    assert spy["affine_wide"] == 1


def test_declined_layers_keep_the_layerwise_launches(nfa, spy):
    """A layer of the chain kernels' shape, a float64 layer and a one-hidden-layer net never reach nf_affine_wide."""
    b = torch.tensor([1.0, 0.0] * 8)
    small = nfa.flows.MaskedAffineFlow(b, nfa.nets.MLP([16, 64, 64, 16], init_zeros=False), nfa.nets.MLP([16, 64, 64, 16], init_zeros=False)).to(DEV)
    shallow = nfa.flows.MaskedAffineFlow(torch.tensor([1.0, 0.0] * 10), nfa.nets.MLP([20, 96, 20]), None).to(DEV)
    dbl, x = fresh_layer(nfa, "a")
    dbl(x)
    assert spy["affine_wide"] == 1
    dbl = dbl.double()                           # `.double()` after the first call
    small(torch.randn(9, 16, device=DEV))
    shallow(torch.randn(9, 20, device=DEV))
    y, ld = dbl(x.double())
    assert y.dtype == torch.float64 and spy["affine_wide"] == 1 and spy["masked_affine"] == 3
