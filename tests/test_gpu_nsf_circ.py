"""GPU tests (-m gpu) of the circular NSF coupling layer in one launch (nf_nsf_wide_ft, csrc/nsf_circ.hip): the fixture layers of
tests/golden/circ_wide_*.npz (five at 8 bins, one each at 4 and 16) against the reference's stored outputs and against the project's
own layer-wise path, the layers the packer declines on that path, coordinates
outside their interval, batch sizes around the tiles, the log-det accumulation modes, and a whole circular model on a UniformGaussian
base against the reference's log_prob."""
import numpy as np
import pytest
import torch

import circ_wide_cases as cw
from conftest import assert_close, ld_tol

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def nfa():
    import normflows_amd
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    assert normflows_amd.native_library_path().endswith("normalizing-flows_amd/lib/libnf_mi355x.so")
    normflows_amd._lib.lib()
    return normflows_amd


@pytest.fixture
def spy(nfa, monkeypatch):
    """Counts the launches of the new kernel and of the layer-wise path's coupling kernel."""
    calls = {"ft": 0, "layerwise": 0}
    ft, lw = nfa.ops.nsf_wide_ft, nfa.ops.rqs_coupling

    def ft_(*a, **k):
        calls["ft"] += 1
        return ft(*a, **k)

    def lw_(*a, **k):
        calls["layerwise"] += 1
        return lw(*a, **k)
    monkeypatch.setattr(nfa.ops, "nsf_wide_ft", ft_)
    monkeypatch.setattr(nfa.ops, "rqs_coupling", lw_)
    return calls


def N(t):
    return t.detach().cpu().numpy()


_layers = {}


def gpu_layer(nfa, name):
    if name not in _layers:
        _layers[name] = cw.layer(nfa, name).to(DEV)
    return _layers[name]


def run(layer, x, direction):
    """direction 1 = layer.forward (sampling, prqct.inverse), 0 = layer.inverse (density)."""
    with torch.no_grad():
        return layer.forward(x) if direction == 1 else layer.inverse(x)


@pytest.mark.parametrize("name", sorted(cw.LAYERS))
@pytest.mark.parametrize("direction", [0, 1])
def test_parity_with_reference_and_layerwise(nfa, spy, name, direction):
    """One launch of nf_nsf_wide_ft per call; outputs within 1e-4 relative of the reference's float32 leg -- the largest error is at
    most 1e-4 of the largest output, and every element is within 1e-4 relative + the 1e-4 absolute term of the existing fixture
    tests (an output crosses zero inside every interval, |y| <= 3.5) --, log-det within
    conftest.ld_tol (root-finding allowance in the sampling direction); the layer-wise path (use_fused = False) on the same rows at
    the same bars; the four outside coordinates exactly 0 with log-det contributions 0 (the rows' log-dets still match)."""
    layer, g = gpu_layer(nfa, name), cw.golden(name)
    x = torch.from_numpy(g["x"]).to(DEV)
    zk, lk = ("z_fwd", "ld_fwd") if direction == 1 else ("z_inv", "ld_inv")
    y, ld = run(layer, x, direction)
    assert spy["ft"] == 1 and spy["layerwise"] == 0
    layer.prqct.use_fused = False
    try:
        y2, ld2 = run(layer, x, direction)
    finally:
        layer.prqct.use_fused = True
    assert spy["ft"] == 1 and spy["layerwise"] >= 1
    tol = ld_tol(np.float32, root_finding=direction == 1)
    scale = np.abs(g[zk]).max()
    print("%s dir %d: one-launch vs reference  y %.3e (rel to max %.3e)  ld %.3e | layer-wise vs reference  y %.3e  ld %.3e" % (
        name, direction, np.abs(N(y) - g[zk]).max(), np.abs(N(y) - g[zk]).max() / scale, np.abs(N(ld) - g[lk]).max(),
        np.abs(N(y2) - g[zk]).max(), np.abs(N(ld2) - g[lk]).max()))
    for got_y, got_ld, what in ((y, ld, "one launch"), (y2, ld2, "layer-wise")):
        assert np.abs(N(got_y) - g[zk]).max() <= 1e-4 * scale, "%s %s dir %d outputs against the largest" % (what, name, direction)
        assert_close(N(got_y), g[zk], what="%s %s dir %d outputs" % (what, name, direction), rtol=1e-4, atol=1e-4)
        assert_close(N(got_ld), g[lk], what="%s %s dir %d log-det" % (what, name, direction), **tol)
    assert_close(N(y), N(y2), what="one launch vs layer-wise outputs", rtol=1e-4, atol=1e-4)
    assert_close(N(ld), N(ld2), what="one launch vs layer-wise log-det", **tol)
    for r, c in g["outside"]:
        assert float(y[r, c]) == 0.0 and float(y2[r, c]) == 0.0


def test_outside_coordinates_contribute_nothing(nfa, spy):
    """Layer (a): a row whose every coordinate is outside its interval comes out as zeros with log-det exactly 0, in both directions."""
    layer = gpu_layer(nfa, "a")
    x = (torch.tensor(cw.TB_A) + 0.5).repeat(3, 1) * torch.tensor([[1.0], [-1.0], [1.0]])
    for direction in (0, 1):
        y, ld = run(layer, x.to(DEV), direction)
        assert not N(y).any() and not N(ld).any()
    assert spy["ft"] == 2


@pytest.mark.parametrize("name,B", [("a", 1), ("a", 64), ("a", 129), ("c", 129), ("d", 1), ("d", 64), ("d", 129)])
def test_batches_accumulation_and_determinism(nfa, spy, name, B):
    """Batches of 1, 64 and 129 rows on 128-row tiles (a, d: Hp 128) and 64-row tiles (c: Hp 256): every row equals the same row of
    a full-fixture call bit for bit (rows are independent), two consecutive calls give identical bits, and the three log-det
    accumulation modes write, add and subtract the same values."""
    layer, g = gpu_layer(nfa, name), cw.golden(name)
    p = layer.prqct
    reps = (B + len(g["x"]) - 1) // len(g["x"])
    x = torch.from_numpy(np.tile(g["x"], (reps, 1))[:B]).to(DEV)
    L = nfa._lib
    with torch.no_grad():
        for direction in (0, 1):
            y, ld = p._route(x, None, direction, None, None)
            y_again, ld_again = p._route(x, None, direction, None, None)
            assert torch.equal(y, y_again) and torch.equal(ld, ld_again)
            full_y, full_ld = p._route(torch.from_numpy(g["x"]).to(DEV), None, direction, None, None)
            n = min(B, len(g["x"]))
            assert torch.equal(y[:n], full_y[:n]) and torch.equal(ld[:n], full_ld[:n])
            base = torch.linspace(-1.0, 1.0, B, device=DEV)
            for acc, want in ((L.LD_WRITE, ld), (L.LD_ADD, base + ld), (L.LD_SUB, base - ld)):
                buf = base.clone()
                y3, out = p._route(x, None, direction, buf, acc)
                assert out.data_ptr() == buf.data_ptr() and torch.equal(y3, y) and torch.equal(buf, want)
    assert spy["ft"] == 2 * 6 and spy["layerwise"] == 0


@pytest.mark.parametrize("what", cw.DECLINED)
def test_declined_layers_keep_the_layerwise_path(nfa, spy, what):
    """Each layer the packer declines (context, a non-alternating mask, 5 bins, a Tanh in the preprocessing, no unconditional
    transform) still evaluates in both directions: no launch of nf_nsf_wide_ft, the layer-wise path's coupling kernel instead, finite
    outputs, and the sampling direction undoes the density direction."""
    layer = cw.declined_layer(nfa, what).to(DEV)
    torch.manual_seed(4)
    x = ((torch.rand(40, 8) * 2 - 1) * 2.9).to(DEV)
    ctx = (torch.randn(40, cw.DECLINED_CONTEXT).to(DEV),) if what == "context" else ()
    assert layer.prqct._circ_pack(x, *(ctx or (None,))) is None
    with torch.no_grad():
        y, ld = layer.inverse(x, *ctx)
        assert spy["ft"] == 0 and spy["layerwise"] >= 1
        n = spy["layerwise"]
        back, ld_back = layer.forward(y, *ctx)
    assert spy["ft"] == 0 and spy["layerwise"] > n
    for t in (y, ld, back, ld_back):
        assert bool(torch.isfinite(t).all())
    assert y.shape == x.shape and ld.shape == (40,) and bool((y != x).any())
    assert_close(N(back), N(x), what="round trip", rtol=1e-4, atol=1e-4)
    assert_close(N(ld_back), -N(ld), what="round trip log-det", **ld_tol(np.float32, root_finding=True))


def test_switches_keep_the_layerwise_path(nfa, spy):
    """config.nsf_circular = False sends a supported layer to the layer-wise path too (use_fused = False:
    test_parity_with_reference_and_layerwise)."""
    layer, g = gpu_layer(nfa, "a"), cw.golden("a")
    xa = torch.from_numpy(g["x"]).to(DEV)
    assert nfa.config.nsf_circular is True
    nfa.config.set_nsf_circular(False)
    try:
        run(layer, xa, 0)
        assert spy["ft"] == 0 and spy["layerwise"] >= 1
    finally:
        nfa.config.set_nsf_circular(True)
    run(layer, xa, 0)
    assert spy["ft"] == 1


def test_circular_model_end_to_end(nfa, spy):
    """UniformGaussian(6, [1, 3, 4], scale) + 3 x [circular coupling, PeriodicShift]: log_prob(x) against the reference's stored
    values at the README's 1e-4 relative bar, and log_prob(sample) against the log_q that forward of the base + chain returns."""
    m, g = cw.model(nfa)
    m = m.to(DEV)
    with torch.no_grad():
        lp = m.log_prob(torch.from_numpy(g["x"]).to(DEV))
    assert spy["ft"] == 3 and spy["layerwise"] == 0
    print("model log_prob vs reference: max rel %.3e" % np.max(np.abs(N(lp) - g["log_prob"]) / np.abs(g["log_prob"])))
    np.testing.assert_allclose(N(lp), g["log_prob"], rtol=1e-4, atol=0)
    torch.manual_seed(11)
    bound = torch.tensor(cw.TB_A).to(DEV)
    with torch.no_grad():
        x, log_q = m.q0(257)                             # forward of the base, then of the chain (core.py:167-180)
        inside = (x.abs() <= bound).all(1)               # list tails send a coordinate outside its interval to 0: not invertible there
        for flow in m.flows:
            x, ld = flow(x)
            log_q = log_q - ld
        x, log_q = x[inside], log_q[inside]
        lp2 = m.log_prob(x)
    assert spy["ft"] == 9 and int(inside.sum()) >= 250
    assert bool((x.abs()[:, [1, 3, 4]] <= bound[[1, 3, 4]] * (1 + 1e-6)).all())
    print("model log_prob(sample) vs log_q: max rel %.3e" % np.max(np.abs(N(lp2) - N(log_q)) / np.abs(N(log_q))))
    np.testing.assert_allclose(N(lp2), N(log_q), rtol=1e-4, atol=0)
