"""GPU tests of the conditional NSF coupling layer in one launch (nf_nsf_wide_ctx, csrc/nsf_ctx.hip): parity with the reference
(tests/golden/ctx_*.npz, tests/golden/make_golden_context.py), the route (one launch per conditional coupling layer, no eager
conditioner), the differential against the layer-wise path at full size, and bit-level properties (expanded context, row permutation,
run-to-run, NaN containment, hipGraph replay)."""
import numpy as np
import pytest
import torch

from conftest import assert_close, golden_state, ld_tol, load_golden

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LAYERS = {"ctx_d6_c3_h40": (6, 3, 40, 2, 8), "ctx_d64_c16_h136": (64, 16, 136, 1, 4), "ctx_d17_c33_h200": (17, 33, 200, 1, 16)}
# tools/context_bench.py's shapes that the kernel builds (hidden 512 is declined: the layer-wise path runs it): D, C, hidden
BENCH_SHAPES = ((64, 16, 128), (64, 16, 256), (16, 4, 128), (64, 64, 256))


@pytest.fixture(autouse=True)
def _inference_mode():
    with torch.no_grad():
        yield


@pytest.fixture(scope="module")
def nfa():
    import normflows_amd
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    assert normflows_amd.native_library_path().endswith("normalizing-flows_amd/lib/libnf_mi355x.so")
    normflows_amd._lib.lib()
    return normflows_amd


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def N(t):
    return t.detach().cpu().numpy()


class _Spy:
    def __init__(self, nfa, monkeypatch, forbid_eager=False):
        self.calls = 0
        real = nfa.ops.nsf_wide_ctx

        def spy(*a, **k):
            self.calls += 1
            return real(*a, **k)
        monkeypatch.setattr(nfa.ops, "nsf_wide_ctx", spy)
        if forbid_eager:
            def boom(*a, **k):
                raise AssertionError("the layer-wise path ran")
            monkeypatch.setattr(nfa.nets.ResidualNet, "forward", boom)
            monkeypatch.setattr(nfa.ops, "rqs_coupling", boom)


def _layer(nfa, D, C, H, NB=2, K=8, seed=0, sigma=0.05):
    torch.manual_seed(seed)
    layer = nfa.flows.CoupledRationalQuadraticSpline(D, NB, H, num_context_channels=C, num_bins=K, init_identity=False)
    with torch.no_grad():
        for p in layer.parameters():
            p.add_(sigma * torch.randn_like(p))
    return layer.eval().to(DEV)


def _rows(B, D, C, seed):
    g = torch.Generator().manual_seed(seed)
    x = 1.5 * torch.randn(B, D, generator=g)
    x[: B // 8] *= 3.0                                   # some rows beyond the tail bound
    return x.to(DEV), torch.randn(B, C, generator=g).to(DEV)


@pytest.mark.parametrize("name", sorted(LAYERS))
def test_context_layer_vs_reference(nfa, monkeypatch, name):
    """Each fixture layer, both directions, against the reference's float32 and float64 outputs; through the new launch."""
    D, C, H, NB, K = LAYERS[name]
    g = load_golden(name)
    layer = nfa.flows.CoupledRationalQuadraticSpline(D, NB, H, num_context_channels=C, num_bins=K, init_identity=False)
    layer.load_state_dict({k: torch.from_numpy(v) for k, v in golden_state(g).items()}, strict=True)
    layer = layer.eval().to(DEV)
    spy = _Spy(nfa, monkeypatch, forbid_eager=True)
    x, c = T(g["x"]), T(g["context"])
    zi, ldi = layer.inverse(x, c)
    zf, ldf = layer.forward(x, c)
    assert spy.calls == 2
    for leg in ("f32", "f64"):
        assert_close(N(zi), g["z_inv_" + leg], rtol=1e-4, atol=1e-4, what=name + " z density " + leg)
        assert_close(N(zf), g["z_fwd_" + leg], rtol=1e-4, atol=1e-4, what=name + " z sampling " + leg)
    assert_close(N(ldi), g["ld_inv_f32"], what=name + " ld density", **ld_tol(np.float32))
    assert_close(N(ldf), g["ld_fwd_f32"], what=name + " ld sampling", **ld_tol(np.float32, root_finding=True))


def test_conditional_model_vs_reference_and_route(nfa, monkeypatch):
    """2 x [CoupledRQS(8, 2, 64, C = 4) + LULinearPermute(8)] over ConditionalDiagGaussian: log_prob, both directions, and
    log_prob(sample(n, c)) = the sampler's log_q -- with the eager conditioner and the layer-wise coupling patched to raise, and
    exactly one new launch per coupling layer and call."""
    g = load_golden("ctx_model_nsf")
    flows = []
    for _ in range(2):
        flows += [nfa.flows.CoupledRationalQuadraticSpline(8, 2, 64, num_context_channels=4, num_bins=8, init_identity=False),
                  nfa.flows.LULinearPermute(8)]
    q0 = nfa.distributions.ConditionalDiagGaussian(8, torch.nn.Linear(4, 16))
    m = nfa.ConditionalNormalizingFlow(q0, flows)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in golden_state(g).items()}, strict=True)
    m = m.eval().to(DEV)
    spy = _Spy(nfa, monkeypatch, forbid_eager=True)
    x, c = T(g["x"]), T(g["context"])
    lp = m.log_prob(x, c)
    assert spy.calls == 2
    assert_close(N(lp), g["log_prob_f64"], rtol=1e-4, atol=1e-4, what="log_prob")
    z, ld = m.inverse_and_log_det(x, c)
    assert_close(N(z), g["z_inv_f64"], rtol=1e-4, atol=1e-4, what="z_inv")
    assert_close(N(ld), g["ld_inv_f32"], what="ld_inv", **ld_tol(np.float32))
    xf, ldf = m.forward_and_log_det(x, c)
    assert_close(N(xf), g["z_fwd_f64"], rtol=1e-4, atol=1e-4, what="z_fwd")
    assert_close(N(ldf), g["ld_fwd_f32"], what="ld_fwd", **ld_tol(np.float32, root_finding=True))
    spy.calls = 0
    torch.manual_seed(4)
    xs, lq = m.sample(300, context=c[:1].expand(300, 4))
    assert spy.calls == 2
    assert_close(N(m.log_prob(xs, c[:1].expand(300, 4))), N(lq), rtol=1e-3, atol=1e-3, what="log_prob(sample)")
    assert spy.calls == 4


def _differential(nfa, layer, x, c, direction):
    run = layer.inverse if direction == 0 else layer.forward
    y, ld = run(x, c)
    nfa.config.set_nsf_context(False)
    try:
        y0, ld0 = run(x, c)
    finally:
        nfa.config.set_nsf_context(True)
    return y, ld, y0, ld0


@pytest.mark.parametrize("D,C,H", BENCH_SHAPES)
def test_context_layer_vs_layerwise_full_size(nfa, monkeypatch, D, C, H):
    """The new launch against set_nsf_context(False) (eager conditioner + nf_rqs_coupling) at ragged and full batches (one row,
    partial tiles, exactly one / two 64- and 128-row tiles, 65 536 and 65 537 rows: persistent workgroups over several tiles), both
    directions; and the round trip inverse(forward(z)) = z."""
    layer = _layer(nfa, D, C, H, seed=D + C + H)
    spy = _Spy(nfa, monkeypatch)
    xa, ca = _rows(65537, D, C, 5)
    for B in (1, 63, 127, 128, 129, 65536, 65537):
        x, c = xa[:B], ca[:B]
        for direction in (0, 1):
            n0 = spy.calls
            y, ld, y0, ld0 = _differential(nfa, layer, x, c, direction)
            assert spy.calls == n0 + 1
            what = "D%d C%d H%d B%d dir%d" % (D, C, H, B, direction)
            assert_close(N(y), N(y0), rtol=2e-4, atol=2e-4, what=what + " y")
            assert_close(N(ld), N(ld0), rtol=2e-4, atol=1e-3, what=what + " ld")
    xf, ldf = layer.forward(xa, ca)
    xb, ldb = layer.inverse(xf, ca)
    assert float((xb - xa).abs().max()) < 2e-3
    assert float((ldf + ldb).abs().max()) < 2e-3


def test_context_bit_properties(nfa):
    """Expanded context (row stride 0) = the materialised repeat, bit for bit; permuting the rows permutes the outputs bitwise; two
    runs give the same bits; a NaN in one row's context or in one transform element leaves every other row / element unchanged."""
    for D, C, H in ((16, 4, 128), (64, 16, 256)):
        layer = _layer(nfa, D, C, H, seed=3)
        x, c = _rows(4099, D, C, 9)
        for run in (layer.inverse, layer.forward):
            ce = c[5:6].expand(4099, C)
            assert ce.stride(0) == 0
            ye, lde = run(x, ce)
            yr, ldr = run(x, c[5:6].repeat(4099, 1))
            assert torch.equal(ye, yr) and torch.equal(lde, ldr)
            y, ld = run(x, c)
            y2, ld2 = run(x, c)
            assert torch.equal(y, y2) and torch.equal(ld, ld2)
            perm = torch.randperm(4099, generator=torch.Generator().manual_seed(1)).to(DEV)
            yp, ldp = run(x[perm], c[perm])
            assert torch.equal(yp, y[perm]) and torch.equal(ldp, ld[perm])
            # strided context rows (a column slice of a wider tensor) = the contiguous copy
            wide = torch.cat([c, torch.randn(4099, 3, device=DEV)], 1)[:, :C]
            assert wide.stride(0) == C + 3
            yw, ldw = run(x, wide)
            assert torch.equal(yw, y) and torch.equal(ldw, ld)
            # NaN in one row's context: that row only
            cn = c.clone()
            cn[3077, C - 1] = float("nan")
            yn, ldn = run(x, cn)
            keep = torch.ones(4099, dtype=torch.bool, device=DEV)
            keep[3077] = False
            assert torch.equal(yn[keep], y[keep]) and torch.equal(ldn[keep], ld[keep])
            assert torch.isnan(ldn[3077])
            # NaN in one transform element: that element (and its row's log-det) only
            tcol = int(layer.prqct.transform_features[1])
            xn = x.clone()
            xn[3200, tcol] = float("nan")
            yn, ldn = run(xn, c)
            assert torch.isnan(yn[3200, tcol])
            mask = torch.ones_like(y, dtype=torch.bool)
            mask[3200, tcol] = False
            assert torch.equal(yn[mask], y[mask])
            keep = torch.ones(4099, dtype=torch.bool, device=DEV)
            keep[3200] = False
            assert torch.equal(ldn[keep], ld[keep])


def test_context_free_layer_unchanged_by_switch(nfa, monkeypatch):
    """A context-free layer never takes the new launch: its outputs are bit-identical with set_nsf_context True and False."""
    torch.manual_seed(2)
    layer = nfa.flows.CoupledRationalQuadraticSpline(64, 2, 256, num_bins=8, init_identity=False).eval().to(DEV)
    spy = _Spy(nfa, monkeypatch)
    x = torch.randn(1000, 64, device=DEV)
    outs = []
    for mode in (True, False):
        nfa.config.set_nsf_context(mode)
        try:
            outs.append(layer.inverse(x) + layer.forward(x))
        finally:
            nfa.config.set_nsf_context(True)
    assert all(torch.equal(a, b) for a, b in zip(*outs)) and spy.calls == 0


def test_conditional_log_prob_graph_replay(nfa):
    """A captured conditional log_prob (hipGraph) replays the eager bits."""
    torch.manual_seed(5)
    flows = []
    for _ in range(2):
        flows += [nfa.flows.CoupledRationalQuadraticSpline(16, 2, 128, num_context_channels=4, num_bins=8, init_identity=False),
                  nfa.flows.LULinearPermute(16)]
    q0 = nfa.distributions.ConditionalDiagGaussian(16, torch.nn.Linear(4, 32))
    m = nfa.ConditionalNormalizingFlow(q0, flows).eval().to(DEV)
    x, c = _rows(1000, 16, 4, 11)
    eager = m.log_prob(x, c)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            m.log_prob(x, c)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = m.log_prob(x, c)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
