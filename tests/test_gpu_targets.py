"""GPU tests of the target, prior and mixture densities on their kernels (csrc/density2d.hip, csrc/gmm.hip, dist_route.py,
dist_mixture.py, autograd.Density2dFn / GmmLogProbFn): against the reference's fixtures (tests/golden/targets_*.npz), against the
torch-formula route with the switch off, and the route's own contracts (which route is taken, shapes at the edges, the second sweep
of the grid loops, determinism, absent cotangents, frozen parameters, live parameters, accumulation, canaries, capture).

Bars.  log_prob: 1e-4 relative to max(1, |reference float64|), the README's parity bar.  Gradients: the error as a fraction of the
tensor's largest reference magnitude, against the larger of 1e-3 and four times the reference's own float32-to-float64 error on
that tensor (tests/test_gpu_training.py's rule), with a floor on the scale for tensors that are exactly zero."""
import contextlib

import numpy as np
import pytest
import torch

import target_cases as cases
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY = 12345.0


@pytest.fixture(scope="module")
def nfa():
    import normflows_amd
    assert torch.cuda.is_available()
    return normflows_amd


@pytest.fixture(autouse=True)
def route_on(nfa):
    """Every test runs with the switch on, whatever the default is; `formulas()` turns it off for a `with` body."""
    old = nfa.config.target_density
    nfa.config.set_target_density(True)
    yield
    nfa.config.set_target_density(old)


@pytest.fixture
def formulas(nfa):
    @contextlib.contextmanager
    def off():
        nfa.config.set_target_density(False)
        try:
            yield
        finally:
            nfa.config.set_target_density(True)
    return off


@pytest.fixture
def calls(nfa, monkeypatch):
    """Counts of the ops' calls (the mixture backward's flags noted) and of the classes' torch-formula methods."""
    n = {"d2": 0, "d2_grad": 0, "gmm": 0, "gmm_bwd": 0, "torch": 0, "bwd_flags": []}

    def counted(key, fn, note=None):
        def wrapper(*a, **k):
            n[key] += 1
            if note is not None:
                note(a, k)
            return fn(*a, **k)
        return wrapper

    def note_d2(a, k):
        if k.get("want_grad"):
            n["d2_grad"] += 1
    monkeypatch.setattr(nfa.ops, "density2d", counted("d2", nfa.ops.density2d, note_d2))
    monkeypatch.setattr(nfa.ops, "gmm_log_prob", counted("gmm", nfa.ops.gmm_log_prob))
    monkeypatch.setattr(nfa.ops, "gmm_log_prob_bwd",
                        counted("gmm_bwd", nfa.ops.gmm_log_prob_bwd, lambda a, k: n["bwd_flags"].append((bool(a[5]), int(a[6])))))
    D = nfa.distributions
    for cls in (D.TwoMoons, D.CircularGaussianMixture, D.RingMixture, D.TwoModes, D.Sinusoidal, D.Sinusoidal_gap, D.Sinusoidal_split,
                D.Smiley, D.GaussianMixture):
        monkeypatch.setattr(cls, "_log_prob_torch", counted("torch", cls._log_prob_torch))
    return n


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def N(t):
    return t.detach().cpu().numpy()


def lp_error(got, ref64):
    return float(np.max(np.abs(N(got).astype(np.float64) - ref64) / np.maximum(1.0, np.abs(ref64))))


def grad_error(got, ref64, ref32=None):
    scale = max(float(np.abs(ref64).max()), 1e-6)
    own = 0.0 if ref32 is None else float(np.abs(np.asarray(ref32, dtype=np.float64) - ref64).max()) / scale
    return float(np.abs(N(got).astype(np.float64) - ref64).max()) / scale, max(1e-3, 4 * own)


def build(nfa, name):
    p = cases.build_2d(nfa.distributions, name)
    return p.to(DEV) if isinstance(p, torch.nn.Module) else p


def gmm(nfa, name, g, trainable=True):
    M, d = cases.GMM[name]
    return nfa.distributions.GaussianMixture(M, d, loc=g["loc0"], scale=g["scale0"], weights=g["weights0"],
                                             trainable=trainable).float().to(DEV)


def random_gmm(nfa, M, d, seed, trainable=True):
    rs = np.random.RandomState(seed)
    return nfa.distributions.GaussianMixture(M, d, loc=1.5 * rs.randn(M, d), scale=0.5 + rs.rand(M, d), weights=0.2 + rs.rand(M),
                                             trainable=trainable).float().to(DEV)


def rows(B, d, seed, scale=2.5):
    g = torch.Generator().manual_seed(seed)
    return (scale * torch.randn(B, d, generator=g)).to(DEV), torch.randn(B, generator=g).to(DEV)


def step_2d(p, z, c):
    z = z.detach().clone().requires_grad_(True)
    lp = p.log_prob(z)
    (lp * c).sum().backward()
    return lp.detach(), z.grad


def step_gmm(m, z, c, z_grad=True):
    m.zero_grad(set_to_none=True)
    z = z.detach().clone().requires_grad_(z_grad)
    lp = m.log_prob(z)
    (lp * c).sum().backward()
    return lp.detach(), z.grad, {k: p.grad for k, p in m.named_parameters()}


def f64_2d(nfa, name, z, c, formulas):
    """The switch-off route in float64: the reference of the generated cases."""
    p = build(nfa, name)
    if isinstance(p, torch.nn.Module):
        p = p.double()
    with formulas():
        lp, gz = step_2d(p, z.double(), c.double())
    return N(lp), N(gz)


def f64_gmm(m, z, c, formulas):
    import copy
    m64 = copy.deepcopy(m).double()
    with formulas():
        lp, gz, gp = step_gmm(m64, z.double(), c.double())
    return N(lp), N(gz), {k: N(v) for k, v in gp.items()}


def check_gmm(got, ref, what):
    lp, gz, gp = got
    rlp, rgz, rgp = ref
    assert lp_error(lp, rlp) < 1e-4, (what, lp_error(lp, rlp))
    for key, a, b in [("gz", gz, rgz)] + [(k, gp[k], rgp[k]) for k in rgp]:
        err, bar = grad_error(a, b)
        assert err <= bar, (what, key, err, bar)


# ---- 1. the kernel route against the reference's fixtures -------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.CASES_2D))
def test_2d_fixture(nfa, calls, name):
    g = load_golden("targets_" + name)
    p = build(nfa, name)
    z, c = T(g["z"]), T(g["c"])
    with torch.no_grad():
        lp0 = p.log_prob(z)
    lp, gz = step_2d(p, z, c)
    assert (calls["d2"], calls["d2_grad"], calls["torch"]) == (2, 1, 0)
    assert torch.equal(lp0, lp) and lp.dtype == torch.float32 and tuple(gz.shape) == (cases.ROWS_2D, 2)
    e = lp_error(lp, g["lp_f64"])
    err, bar = grad_error(gz, g["gz_f64"], g["gz"])
    print("%s: log_prob %.2e; gz %.2e of scale (bar %.1e)" % (name, e, err, bar))
    assert e < 1e-4, (name, e)
    assert err <= bar, (name, err, bar)
    # rows exactly on a kink: the reference's float32 leg, the same conventions.  The scale is the tensor's largest reference
    # magnitude WITHOUT the far row (30, -30), whose gradient is 10^2 .. 10^4 times everybody else's: stricter than the bar above.
    # (Not the kink rows' own magnitude: on row (0, 1) RingMixture(3)'s gradient is two terms of 48 that cancel to float32 noise.)
    kink = list(cases.KINK_ROWS)
    near = [r for r in range(cases.ROWS_2D) if r != len(cases.EDGE_ROWS) - 1]
    scale = max(float(np.abs(g["gz"][near]).max()), 1e-6)
    err = float(np.abs(N(gz[kink]).astype(np.float64) - g["gz"][kink]).max()) / scale
    assert err <= 1e-3, (name, "kink rows", err, N(gz[kink]), g["gz"][kink])


@pytest.mark.parametrize("name", list(cases.GMM))
def test_mixture_fixture(nfa, calls, name):
    g = load_golden("targets_gmm_" + name)
    m = gmm(nfa, name, g)
    z, c = T(g["z"]), T(g["c"])
    with torch.no_grad():
        lp0 = m.log_prob(z)
    lp, gz, gp = step_gmm(m, z, c)
    assert (calls["gmm"], calls["gmm_bwd"], calls["torch"]) == (2, 1, 0) and calls["bwd_flags"] == [(True, 7)]
    assert torch.equal(lp0, lp)
    e = lp_error(lp, g["lp_f64"])
    print("gmm %s: log_prob %.2e" % (name, e))
    assert e < 1e-4, (name, e)
    for key, got in [("gz", gz)] + [("g__" + k, v) for k, v in gp.items()]:
        assert tuple(got.shape) == g[key].shape, key
        err, bar = grad_error(got, g[key + "_f64"], g[key])
        print("gmm %s: %s %.2e of scale (bar %.1e)" % (name, key, err, bar))
        assert err <= bar, (name, key, err, bar)


# ---- 2. which route is taken ------------------------------------------------------------------------------------------------------
def test_2d_routes(nfa, calls, formulas):
    D = nfa.distributions
    z, c = rows(64, 2, 1)
    for name in cases.CASES_2D:
        p = build(nfa, name)
        before = dict(calls)
        with torch.no_grad():
            on = p.log_prob(z)
        assert calls["d2"] == before["d2"] + 1 and calls["torch"] == before["torch"], name
        with formulas(), torch.no_grad():
            off = p.log_prob(z)
        assert calls["d2"] == before["d2"] + 1 and calls["torch"] == before["torch"] + 1, name
        assert lp_error(on, N(off).astype(np.float64)) < 1e-4, name

    def torch_route(p, zz, **ctx):
        a, b = calls["d2"], calls["torch"]
        out = p.log_prob(zz)
        assert calls["d2"] == a and calls["torch"] == b + 1, (type(p).__name__, tuple(zz.shape), zz.dtype)
        return out
    p = D.TwoModes(2, 0.1)
    n = calls["d2"]
    assert tuple(p.log_prob(z[:0]).shape) == (0,) and calls["d2"] == n + 1        # an empty batch: no launch, no fault
    torch_route(p, z.double())                                             # float64
    wide = torch.cat([z, z], 1)
    assert not wide[:, 1:3].is_contiguous()
    torch_route(p, wide[:, 1:3])                                           # a (B, 2) column-sliced view
    out = torch_route(D.Sinusoidal(0.4, 4), z[:32].reshape(4, 8, 2))       # (4, 8, 2) input to a prior
    assert tuple(out.shape) == (4, 8)
    torch_route(D.CircularGaussianMixture(8), z)                           # its `scale` buffer is on the CPU
    torch_route(D.CircularGaussianMixture(257).to(DEV), z)                 # more modes than the LDS table holds

    class Mine(D.TwoModes):
        pass
    torch_route(Mine(2, 0.1), z)                                           # a subclass
    with nfa.config.higher_order_gradients():
        zz = z.clone().requires_grad_(True)
        lp = torch_route(p, zz)
        (gz,) = torch.autograd.grad(lp.sum(), zz, create_graph=True)
        gz.square().sum().backward()                                       # double backward works on the formulas
        assert zz.grad is not None and torch.isfinite(zz.grad).all()


def test_mixture_routes(nfa, calls, formulas):
    import copy
    m = random_gmm(nfa, 3, 2, seed=2)
    z, c = rows(40, 2, 3)

    def torch_route(mm, zz):
        a, b = calls["gmm"], calls["torch"]
        out = mm.log_prob(zz)
        assert calls["gmm"] == a and calls["torch"] == b + 1
        return out
    with torch.no_grad():
        on = m.log_prob(z)
        assert calls["gmm"] == 1 and calls["torch"] == 0
        with formulas():
            off = torch_route(m, z)
        assert lp_error(on, N(off).astype(np.float64)) < 1e-4
        assert tuple(m.log_prob(z[:0]).shape) == (0,) and calls["gmm"] == 2    # an empty batch: no launch, no fault
        torch_route(copy.deepcopy(m).double(), z.double())                 # float64, the constructor's dtype
        torch_route(nfa.distributions.GaussianMixture(3, 2).to(DEV), z.double())
        torch_route(m, torch.cat([z, z], 1)[:, 1:3])                       # a column-sliced view
        # d = 129, M = 65, M x d = 4097 (= 17 x 241: no shape within the other two limits has it), and 64 x 65 = 4160, which
        # breaks the product limit alone
        for M, d in ((2, 129), (65, 2), (17, 241), (64, 65)):
            assert (M, d) != (17, 241) or M * d == 4097
            torch_route(random_gmm(nfa, M, d, seed=4), rows(8, d, 5)[0])
        sub = type("Mine", (nfa.distributions.GaussianMixture,), {})(3, 2).float().to(DEV)
        torch_route(sub, z)                                                # a subclass
    with nfa.config.higher_order_gradients():
        zz = z.clone().requires_grad_(True)
        lp = torch_route(m, zz)
        (gz,) = torch.autograd.grad(lp.sum(), zz, create_graph=True)
        gz.square().sum().backward()
        assert torch.isfinite(zz.grad).all()
    with formulas():                                                       # the switch off, under autograd: the same numbers
        ref = step_gmm(m, z, c)
    assert calls["gmm_bwd"] == 0
    got = step_gmm(m, z, c)
    assert calls["gmm_bwd"] == 1
    check_gmm(got, (N(ref[0]).astype(np.float64), N(ref[1]).astype(np.float64), {k: N(v).astype(np.float64) for k, v in ref[2].items()}),
              "switch off")


# ---- 3. shapes at the edges -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 255, 257, 1027])
def test_2d_batch_edges(nfa, calls, formulas, B):
    z, c = rows(B, 2, 10 + B)
    for name in ("two_moons", "sinusoidal_gap", "sinusoidal_split", "smiley", "ring_3", "circ_gmm_8"):
        p = build(nfa, name)
        lp, gz = step_2d(p, z, c)
        rlp, rgz = f64_2d(nfa, name, z, c, formulas)
        assert lp_error(lp, rlp) < 1e-4, (name, B)
        err, bar = grad_error(gz, rgz)
        assert err <= bar, (name, B, err)
    assert calls["d2_grad"] == 6


@pytest.mark.parametrize("d", [1, 2, 16, 17, 64, 128])
def test_mixture_shape_edges(nfa, calls, formulas, d):
    n = 0
    for M in (1, 3, 64):
        if M * d > 4096:
            continue
        m = random_gmm(nfa, M, d, seed=100 + M + d)
        for B in ((1, 15, 16, 17, 1027) if M == 3 else (17,)):
            z, c = rows(B, d, 7 * B + d)
            check_gmm(step_gmm(m, z, c), f64_gmm(m, z, c, formulas), (M, d, B))
            n += 1
    assert M * d == 4096 or d != 64              # (64, 64): M x d = 4096, the largest record
    assert calls["gmm_bwd"] == n


def test_second_sweep_of_the_grid_loops(nfa, calls, formulas):
    """Batches sized from the launches' own grids so that EVERY workgroup takes a second sweep."""
    B = 2 * 256 * nfa.ops.density2d_grid(1 << 40) + 3
    assert nfa.ops.density2d_grid(B) * 256 * 2 < B
    z, c = rows(B, 2, 21)
    for name in ("two_modes_m15_02", "circ_gmm_3"):
        lp, gz = step_2d(build(nfa, name), z, c)
        rlp, rgz = f64_2d(nfa, name, z, c, formulas)
        assert lp_error(lp, rlp) < 1e-4, name
        err, bar = grad_error(gz, rgz)
        assert err <= bar, (name, err)
    W = nfa._lib.query("nf_persistent_workgroups")
    for M, d in ((3, 2), (5, 17)):
        B = 2 * W * nfa.ops.gmm_rows(d) + 5
        m = random_gmm(nfa, M, d, seed=31 + d)
        z, c = rows(B, d, 22 + d)
        check_gmm(step_gmm(m, z, c), f64_gmm(m, z, c, formulas), (M, d, B))


# ---- 4. contracts -----------------------------------------------------------------------------------------------------------------
def test_same_input_same_bits(nfa):
    z, c = rows(3000, 2, 40)
    for name in ("two_moons", "ring_2", "circ_gmm_8"):
        p = build(nfa, name)
        a, b = step_2d(p, z, c), step_2d(p, z, c)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), name
    for M, d in ((10, 2), (5, 17)):
        m = random_gmm(nfa, M, d, seed=41)
        z, c = rows(70000 if d == 2 else 5000, d, 42)
        a, b = step_gmm(m, z, c), step_gmm(m, z, c)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        assert all(torch.equal(a[2][k], b[2][k]) for k in a[2]), (M, d)


def test_absent_cotangent_gives_none(nfa):
    from normflows_amd.autograd import Density2dFn, GmmLogProbFn
    z = rows(16, 2, 50)[0].requires_grad_(True)
    lp = nfa.distributions.TwoModes(2, 0.1).log_prob(z)
    assert "Density2dFn" in type(lp.grad_fn).__name__ and Density2dFn is not None
    assert lp.grad_fn.apply(None)[0] is None
    m = random_gmm(nfa, 3, 2, seed=51)
    lp = m.log_prob(z)
    assert "GmmLogProbFn" in type(lp.grad_fn).__name__ and GmmLogProbFn is not None
    assert all(o is None for o in lp.grad_fn.apply(None))
    (lp.sum() * 0 + z.sum()).backward()          # a graph in which lp's cotangent is zero but present still works
    assert torch.equal(z.grad, torch.ones_like(z))


def test_nothing_saved_without_a_gradient(nfa, calls):
    z, _ = rows(16, 2, 52)
    p = nfa.distributions.TwoModes(2, 0.1)
    lp = p.log_prob(z)                                         # grad mode on, nothing requires a gradient
    with torch.no_grad():
        lp2 = p.log_prob(z.clone().requires_grad_(True))
    assert calls["d2"] == 2 and calls["d2_grad"] == 0 and lp.grad_fn is None and lp2.grad_fn is None


def test_buffer_and_frozen_variants_make_no_slab_launch(nfa, calls, formulas):
    z, c = rows(100, 2, 60)
    buf = random_gmm(nfa, 3, 2, seed=61, trainable=False)
    lp, gz, gp = step_gmm(buf, z, c)
    assert calls["bwd_flags"] == [(True, 0)] and gp == {}
    frozen = random_gmm(nfa, 3, 2, seed=61)
    for p in frozen.parameters():
        p.requires_grad_(False)
    lp2, gz2, gp2 = step_gmm(frozen, z, c)
    assert calls["bwd_flags"][-1] == (True, 0) and all(v is None for v in gp2.values())
    assert torch.equal(lp, lp2) and torch.equal(gz, gz2)
    with torch.no_grad():                                      # ... and with nothing to differentiate, no Function at all
        n = calls["gmm_bwd"]
        assert buf.log_prob(z).grad_fn is None and calls["gmm_bwd"] == n


def test_gz_alone_and_parameter_gradients_alone(nfa, calls, formulas):
    m = random_gmm(nfa, 5, 17, seed=62)
    z, c = rows(333, 17, 63)
    full = step_gmm(m, z, c)
    only_p = step_gmm(m, z, c, z_grad=False)
    assert calls["bwd_flags"][-1] == (False, 7) and only_p[1] is None
    assert all(torch.equal(full[2][k], only_p[2][k]) for k in full[2])
    m.log_scale.requires_grad_(False)                          # one section switched off: the others keep their bits
    part = step_gmm(m, z, c)
    assert calls["bwd_flags"][-1] == (True, 5) and part[2]["log_scale"] is None
    assert torch.equal(part[1], full[1]) and torch.equal(part[2]["loc"], full[2]["loc"])
    assert torch.equal(part[2]["weight_scores"], full[2]["weight_scores"])


@pytest.mark.parametrize("fused", [False, True])
def test_an_optimizer_step_reaches_the_next_call(nfa, calls, formulas, fused):
    m = random_gmm(nfa, 3, 2, seed=64)
    z, c = rows(50, 2, 65)
    opt = torch.optim.Adam(m.parameters(), lr=0.1, fused=fused)
    with torch.no_grad():
        before = m.log_prob(z)                                 # fills the no_grad record cache
    step_gmm(m, z, c)
    opt.step()
    with torch.no_grad():
        after = m.log_prob(z)
        with formulas():
            ref = m.log_prob(z)
    assert not torch.equal(before, after) and lp_error(after, N(ref).astype(np.float64)) < 1e-4
    with torch.no_grad():
        m.loc.add_(1.0)                                        # an in-place change through the parameter itself
        moved = m.log_prob(z)
        with formulas():
            ref = m.log_prob(z)
    assert not torch.equal(moved, after) and lp_error(moved, N(ref).astype(np.float64)) < 1e-4
    p = nfa.distributions.TwoModes(2, 0.1)                     # the 2-D record is read from the attributes at call time
    a = p.log_prob(z)
    p.scale = 0.2
    b = p.log_prob(z)
    with formulas():
        ref = p.log_prob(z)
    assert not torch.equal(a, b) and lp_error(b, N(ref).astype(np.float64)) < 1e-4


def test_accumulate_form(nfa, calls):
    m = random_gmm(nfa, 10, 2, seed=66)
    z, _ = rows(300, 2, 67)
    base = torch.randn(300, device=DEV)
    with torch.no_grad():
        lp = m.log_prob(z)
        R = m._record_nograd()
        for acc, want in ((+1, base + lp), (-1, base - lp)):
            out = base.clone()
            assert nfa.ops.gmm_log_prob(z, R, 10, out=out, acc=acc) is out
            assert torch.equal(out, want)
            out = base.clone()
            assert m._log_prob_acc(z, out, acc) is out and torch.equal(out, want)
        out = base.clone()
        nfa.ops.gmm_log_prob(z, R, 10, out=out)                # `out` without `acc`: added
        assert torch.equal(out, base + lp)
    zz = z.clone().requires_grad_(True)                        # under autograd: the Function, then the addition
    out = m._log_prob_acc(zz, base.clone(), +1)
    assert out.requires_grad and torch.equal(out.detach(), base + lp)


def test_normalizing_flow_uses_the_accumulate_hook(nfa, calls, monkeypatch):
    q0 = random_gmm(nfa, 3, 2, seed=68)
    seen = []
    hook = type(q0)._log_prob_acc
    monkeypatch.setattr(type(q0), "_log_prob_acc", lambda self, z, log_q, acc=+1: (seen.append(acc), hook(self, z, log_q, acc))[1])
    torch.manual_seed(0)
    flows = [nfa.flows.Planar((2,), act="leaky_relu") for _ in range(3)]
    model = nfa.NormalizingFlow(q0, flows).to(DEV)
    x, _ = rows(200, 2, 69, scale=1.0)
    with torch.no_grad():
        lp = model.log_prob(x)
        log_q = torch.zeros(200, device=DEV)
        z = x
        for f in reversed(flows):
            z, ld = f.inverse(z)
            log_q = log_q + ld
        want = log_q + q0.log_prob(z)
    assert seen == [+1] and calls["gmm"] >= 2 and calls["torch"] == 0
    assert lp_error(lp, N(want).astype(np.float64)) < 1e-5


def test_canaries_around_every_output(nfa, monkeypatch):
    """Every output of the kernels is a slice of a larger buffer of canaries: nothing outside the slice changes."""
    bufs = []

    def padded(shape, dtype, device):
        n = int(np.prod(shape))
        big = torch.full((n + 128,), CANARY, dtype=dtype, device=device)
        bufs.append((big, n))
        return big[64:64 + n].view(shape)

    class PaddedTorch:
        """`torch` as ops.py sees it, with empty / empty_like handing out the padded slices."""

        def __getattr__(self, name):
            return getattr(torch, name)

        @staticmethod
        def empty(*s, dtype=None, device=None):
            return padded(tuple(s[0]) if isinstance(s[0], (tuple, list, torch.Size)) else s, dtype, device)

        @staticmethod
        def empty_like(t):
            return padded(tuple(t.shape), t.dtype, t.device)
    from normflows_amd import ops
    monkeypatch.setattr(ops, "torch", PaddedTorch())
    z, c = rows(77, 2, 70)
    for name in ("two_moons", "ring_2", "circ_gmm_3", "sinusoidal_gap", "smiley"):
        step_2d(build(nfa, name), z, c)
    for M, d in ((3, 2), (5, 17)):
        step_gmm(random_gmm(nfa, M, d, seed=71), *rows(77, d, 72))
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert len(bufs) == 5 * 2 + 2 * 4          # 2-D: lp and gz; mixture: lp, then gz, the slabs and gR
    for big, n in bufs:
        assert bool((big[:64] == CANARY).all()) and bool((big[64 + n:] == CANARY).all())
        assert not bool((big[64:64 + n] == CANARY).any())      # ... and every element inside was written


def test_capture_and_replay(nfa, calls):
    """log_prob recorded with torch.cuda.graph and replayed with new input contents: no host synchronisation and no allocation
    beyond the outputs on the route, the eager bits."""
    for make, d in ((lambda: nfa.distributions.CircularGaussianMixture(8).to(DEV), 2), (lambda: random_gmm(nfa, 10, 64, seed=80), 64)):
        warm, p = make(), make()
        xs = [rows(500, d, s)[0] for s in (1, 2, 3)]
        static = xs[0].clone()
        with torch.no_grad():
            eager = [warm.log_prob(x) for x in xs]
            p.log_prob(static)                 # (the mixture's record is packed and cached here, outside the capture)
            torch.cuda.synchronize()
            n = calls["d2"] + calls["gmm"]
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                out = p.log_prob(static)
            assert calls["d2"] + calls["gmm"] == n + 1 and calls["torch"] == 0
            for x, want in list(zip(xs, eager))[1:]:
                static.copy_(x)
                graph.replay()
                torch.cuda.synchronize()
                assert torch.equal(out, want)


# ---- 5. end to end ----------------------------------------------------------------------------------------------------------------
def realnvp(nfa, q0, p, seed):
    torch.manual_seed(seed)
    flows = []
    for _ in range(4):
        flows.append(nfa.flows.AffineCouplingBlock(nfa.nets.MLP([1, 16, 16, 2], init_zeros=False)))
        flows.append(nfa.flows.Permute(2, mode="swap"))
    return nfa.NormalizingFlow(q0, flows, p).to(DEV)


def grads_agree(model, loss_fn, formulas, what):
    out = []
    for off in (True, False):
        model.zero_grad(set_to_none=True)
        with (formulas() if off else contextlib.nullcontext()):
            loss = loss_fn()
            loss.backward()
        out.append((float(loss.detach()), {k: p.grad.clone() for k, p in model.named_parameters()}))
    (l0, g0), (l1, g1) = out
    assert abs(l0 - l1) <= 1e-4 * max(1.0, abs(l0)), (what, l0, l1)
    for k in g0:
        err, bar = grad_error(g1[k], N(g0[k]).astype(np.float64))
        assert err <= bar, (what, k, err)


def test_reverse_kld_of_a_realnvp_model_against_two_modes(nfa, calls, formulas):
    model = realnvp(nfa, nfa.distributions.DiagGaussian(2), nfa.distributions.TwoModes(2, 0.1), seed=90)
    eps = torch.randn(512, 2, generator=torch.Generator().manual_seed(91)).to(DEV)
    grads_agree(model, lambda: model.reverse_kld(eps=eps), formulas, "reverse_kld")
    assert calls["d2_grad"] == 1 and calls["torch"] == 1


def test_forward_kld_with_a_mixture_base(nfa, calls, formulas):
    model = realnvp(nfa, random_gmm(nfa, 3, 2, seed=92), None, seed=93)
    x, _ = rows(512, 2, 94, scale=1.0)
    grads_agree(model, lambda: model.forward_kld(x), formulas, "forward_kld")
    assert calls["gmm_bwd"] == 1 and calls["bwd_flags"] == [(True, 7)] and calls["torch"] == 1


# ---- 6. samples on the GPU: properties --------------------------------------------------------------------------------------------
def test_samples_on_the_gpu(nfa):
    D = nfa.distributions
    torch.manual_seed(0)
    for t in (D.TwoMoons().to(DEV), D.RingMixture(2).to(DEV)):
        s = t.sample(100)
        assert tuple(s.shape) == (100, 2) and s.dtype == torch.float32 and s.device.type == "cuda"
        assert torch.isfinite(s).all() and float(s.min()) >= -3.0 and float(s.max()) <= 3.0
    s = D.CircularGaussianMixture(8).to(DEV).sample(100)
    assert tuple(s.shape) == (100, 2) and s.dtype == torch.float32 and s.device.type == "cuda" and torch.isfinite(s).all()
    z, lp = random_gmm(nfa, 5, 17, seed=95)(100)
    assert tuple(z.shape) == (100, 17) and tuple(lp.shape) == (100,) and z.dtype == torch.float32 and z.device.type == "cuda"
    assert torch.isfinite(z).all() and torch.isfinite(lp).all() and z.requires_grad and lp.requires_grad
    s = D.TwoIndependent(D.TwoMoons().to(DEV), D.RingMixture(2).to(DEV)).sample(10)
    assert tuple(s.shape) == (10, 4) and s.device.type == "cuda"
