"""GPU tests of the stochastic flow layers on their kernels (csrc/hmc2d.hip, stochastic_route.py, autograd.Hmc2dFn / Mh2dFn): the
kernels against the float64 emulator (tests/stochastic_emulator.py) on explicit noise, the accept decisions with real uniforms, the
layers, HAIS and a NormalizingFlow with the switch off and on under one seed, and the route's contracts (canaries, determinism,
frozen parameters, absent cotangents, live parameters, views and float64 inputs, capture).

Bars.  z_out, log_det and the tangents: the error relative to max(1, |float64|), against the larger of 1e-4 (the README's parity
bar) and four times the torch-formula route's own float32-to-float64 error on that tensor -- the second term absorbs what a
trajectory does to rounding (tests/test_gpu_training.py's rule, as tests/test_gpu_targets.py restates it).  Gradients: the error as
a fraction of the tensor's largest reference magnitude, against the larger of 1e-3 and four times that own error.  Decisions: a row
is decided when |log u - log prob (float64)| exceeds four times 1e-4 max(1, largest of the four terms of the log-ratio)."""
import contextlib
import copy

import numpy as np
import pytest
import torch

import stochastic_cases as cases
import stochastic_emulator as emu

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY = 12345.0
LSS, LM = (-2.6, -2.9), (0.1, -0.2)
LSS_WIDE = (-1.7, -1.9)      # the decision tests: steps wide enough that a good part of the rows is rejected


@pytest.fixture(scope="module")
def nfa():
    import normflows_amd
    assert torch.cuda.is_available()
    return normflows_amd


@pytest.fixture(autouse=True)
def route_on(nfa):
    """Every test runs with the switch on, whatever the default is; `formulas()` turns it off for a `with` body."""
    old = nfa.config.stochastic_kernels
    nfa.config.set_stochastic_kernels(True)
    yield
    nfa.config.set_stochastic_kernels(old)


@pytest.fixture
def formulas(nfa):
    @contextlib.contextmanager
    def off():
        nfa.config.set_stochastic_kernels(False)
        try:
            yield
        finally:
            nfa.config.set_stochastic_kernels(True)
    return off


@pytest.fixture
def calls(nfa, monkeypatch):
    """Counts of the ops' calls (the backward's `want` noted) and of the layers' torch-formula transitions."""
    n = {"hmc2d": 0, "hmc2d_bwd": 0, "mh2d": 0, "torch": 0, "want": []}

    def counted(key, fn, note=None):
        def wrapper(*a, **k):
            n[key] += 1
            if note is not None:
                note(a, k)
            return fn(*a, **k)
        return wrapper
    monkeypatch.setattr(nfa.ops, "hmc2d", counted("hmc2d", nfa.ops.hmc2d))
    monkeypatch.setattr(nfa.ops, "mh2d", counted("mh2d", nfa.ops.mh2d))
    monkeypatch.setattr(nfa.ops, "hmc2d_bwd", counted("hmc2d_bwd", nfa.ops.hmc2d_bwd, lambda a, k: n["want"].append(int(a[5]))))
    for cls in (nfa.flows.HamiltonianMonteCarlo, nfa.flows.MetropolisHastings):
        monkeypatch.setattr(cls, "_transition_torch", counted("torch", cls._transition_torch))
    return n


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def N(t):
    return t.detach().cpu().numpy().astype(np.float64)


def gauss(nfa):
    return cases.set_gauss(nfa.distributions.DiagGaussian(2, trainable=False), torch.float32).to(DEV)


def make_target(nfa, name):
    """Every kind as a single term, and two mixed pairs (one with the Gaussian term, one with the mixture's LDS centres)."""
    D = nfa.distributions
    single = {"two_modes": lambda: D.TwoModes(2.0, 0.1), "two_moons": D.TwoMoons, "sinusoidal": lambda: D.Sinusoidal(0.4, 4),
              "sinusoidal_gap": lambda: D.Sinusoidal_gap(0.4, 4), "sinusoidal_split": lambda: D.Sinusoidal_split(0.4, 4),
              "smiley": lambda: D.Smiley(0.15), "ring_2": lambda: D.RingMixture(2), "circ_gmm_8": lambda: D.CircularGaussianMixture(8),
              "gauss": lambda: gauss(nfa)}
    if name == "pair_two_modes_gauss":
        return D.LinearInterpolation(D.TwoModes(2.0, 0.1), gauss(nfa), 0.3)
    if name == "pair_circ_gmm_sinusoidal":
        return D.LinearInterpolation(D.CircularGaussianMixture(8).to(DEV), D.Sinusoidal(0.4, 4), torch.tensor(0.6))
    t = single[name]()
    return t.to(DEV) if isinstance(t, torch.nn.Module) else t


TARGETS = ["two_modes", "two_moons", "sinusoidal", "sinusoidal_gap", "sinusoidal_split", "smiley", "ring_2", "circ_gmm_8", "gauss",
           "pair_two_modes_gauss", "pair_circ_gmm_sinusoidal"]


def to64(target):
    """The same target with its tensors in float64 (for the formula route's float64 leg)."""
    t = copy.deepcopy(target)
    if isinstance(t, torch.nn.Module):
        return t.double()
    for k in ("dist1", "dist2"):
        if hasattr(t, k) and isinstance(getattr(t, k), torch.nn.Module):
            setattr(t, k, getattr(t, k).double())
    if hasattr(t, "alpha") and torch.is_tensor(t.alpha):
        t.alpha = t.alpha.double()
    return t


def terms_of(target):
    from normflows_amd import stochastic_route as route
    with torch.no_grad():
        terms = route.target_terms(target, torch.device(DEV))
    assert terms is not None
    return terms


def emu_terms(terms):
    return [(w, k, n, rec, None if a0 is None else N(a0), None if a1 is None else N(a1)) for w, k, n, rec, a0, a1 in terms]


def rows(B, seed, steps=None):
    """z (B, 2) near and around the modes (kink rows first when there is room), standard-normal noise, uniforms, cotangents."""
    g = torch.Generator().manual_seed(seed)
    z = 1.2 * torch.randn(B, 2, generator=g)
    m = B // 2
    phi = 6.2831853 * torch.rand(m, generator=g)
    z[:m] = 2.0 * torch.stack([torch.cos(phi), torch.sin(phi)], 1) + 0.15 * torch.randn(m, 2, generator=g)
    if B >= 16:
        z[:len(cases.KINK_ROWS)] = torch.tensor(cases.KINK_ROWS)
    shape = (B,) if steps is None else (steps, B)
    eps = torch.randn(shape + (2,), generator=g)
    u = torch.rand(shape, generator=g)
    return z.to(DEV), eps.to(DEV), u.to(DEV), torch.randn(B, 2, generator=g).to(DEV), torch.randn(B, generator=g).to(DEV)


def hmc_layer(nfa, target, steps, clip=None, dtype=torch.float32, lss=LSS):
    return nfa.flows.HamiltonianMonteCarlo(target, steps, torch.tensor(lss, dtype=dtype), torch.tensor(LM, dtype=dtype), clip).to(DEV)


def mh_layer(nfa, target, steps, scale=(0.05, 0.08), dtype=torch.float32):
    return nfa.flows.MetropolisHastings(target, nfa.distributions.DiagGaussianProposal((2,), scale).to(dtype), steps).to(DEV)


def rel_error(got, ref64):
    return float(np.max(np.abs(np.asarray(got, np.float64) - ref64) / np.maximum(1.0, np.abs(ref64)))) if ref64.size else 0.0


def check_value(what, got, ref64, f32, f64, rows_ok=None):
    """got against the emulator's float64 under the bar max(1e-4, 4 x the formula route's own float32-to-float64 error)."""
    sel = slice(None) if rows_ok is None else rows_ok
    err, own = rel_error(N(got)[sel], ref64[sel]), rel_error(N(f32)[sel], N(f64)[sel])
    bar = max(1e-4, 4 * own)
    print("%s: error %.3e, own %.3e, bar %.3e" % (what, err, own, bar))
    assert err <= bar, (what, err, bar)


def grad_error(what, got, ref64, ref32):
    ref64 = np.asarray(ref64, np.float64)
    scale = max(float(np.abs(ref64).max()), 1e-6)
    own = float(np.abs(np.asarray(ref32, np.float64) - ref64).max()) / scale
    err, bar = float(np.abs(N(got) - ref64).max()) / scale, max(1e-3, 4 * own)
    print("%s: error %.3e, own %.3e, bar %.3e" % (what, err, own, bar))
    assert err <= bar, (what, err, bar)


def zeros_for(g, like):
    return torch.zeros_like(like) if g is None else g


def formula_hmc(nfa, target, steps, clip, z, eps, u, cz, c, dtype, lss=LSS):
    """The torch-formula transition in `dtype` with per-row copies of the parameters, so that the gradient of sum(z_out) is the per-row
    tangent: (z_out, log_det, tan_lss, tan_lm) and, with the shared parameters, (gz, g log_step_size, g log_mass) of the loss."""
    tgt = target if dtype == torch.float32 else to64(target)
    B = len(z)
    layer = hmc_layer(nfa, tgt, steps, clip, dtype, lss)
    layer.log_step_size = torch.nn.Parameter(layer.log_step_size.detach().expand(B, 2).clone())
    layer.log_mass = torch.nn.Parameter(layer.log_mass.detach().expand(B, 2).clone())
    z_out, _ = layer._transition_torch(z.to(dtype), eps.to(dtype), u.to(dtype))
    if z_out.requires_grad:         # (steps = 0: z_out is z, no parameter is used)
        z_out.sum().backward()
    tan = (zeros_for(layer.log_step_size.grad, layer.log_step_size), zeros_for(layer.log_mass.grad, layer.log_mass))
    layer = hmc_layer(nfa, tgt, steps, clip, dtype, lss)
    zz = z.to(dtype).clone().requires_grad_(True)
    z_out, log_det = layer._transition_torch(zz, eps.to(dtype), u.to(dtype))
    ((z_out * cz.to(dtype)).sum() + (log_det * c.to(dtype)).sum()).backward()
    return (z_out.detach(), log_det.detach(), tan[0], tan[1], zz.grad, zeros_for(layer.log_step_size.grad, layer.log_step_size),
            zeros_for(layer.log_mass.grad, layer.log_mass))


def kernel_hmc(nfa, target, steps, clip, z, eps, u, cz, c):
    layer = hmc_layer(nfa, target, steps, clip)
    zz = z.clone().requires_grad_(True)
    z_out, log_det = layer._transition(zz, eps, u)
    ((z_out * cz).sum() + (log_det * c).sum()).backward()
    return z_out.detach(), log_det.detach(), zz.grad, layer.log_step_size.grad, layer.log_mass.grad


# ---- 1. the kernels against the emulator on explicit noise: the continuous part (every row accepts) -------------------------------
def hmc_continuous(nfa, formulas, calls, name, B, steps, clip, seed):
    from normflows_amd import ops
    target = make_target(nfa, name)
    z, eps, _, cz, c = rows(B, seed)
    u = torch.zeros(B, device=DEV)
    terms = terms_of(target)
    lss, lm = T(np.array(LSS, np.float32)), T(np.array(LM, np.float32))
    z_out, log_det, accept, side = ops.hmc2d(z, eps, u, lss, lm, terms, steps, clip or 0.0, want_side=True)
    plain = ops.hmc2d(z, eps, u, lss, lm, terms, steps, clip or 0.0)
    assert torch.equal(plain[0], z_out) and torch.equal(plain[1], log_det) and plain[3] is None    # the two instantiations agree
    f = emu.hmc2d(emu_terms(terms), N(z), N(eps), N(u), LSS, LM, steps, clip or 0.0)
    with formulas():
        f32 = formula_hmc(nfa, target, steps, clip, z, eps, u, cz, c, torch.float32)
        f64 = formula_hmc(nfa, target, steps, clip, z, eps, u, cz, c, torch.float64)
    assert bool(accept.all()) and f["accept"].all()
    what = "%s B=%d steps=%d clip=%s" % (name, B, steps, clip)
    check_value(what + " z_out", z_out, f["z_out"], f32[0], f64[0])
    check_value(what + " log_det", log_det, f["log_det"], f32[1], f64[1])
    check_value(what + " tan_lss", side[:, 0:2], f["tan_lss"], f32[2], f64[2])
    check_value(what + " tan_lm", side[:, 2:4], f["tan_lm"], f32[3], f64[3])
    got = kernel_hmc(nfa, target, steps, clip, z, eps, u, cz, c)
    for key, a, r64, r32 in (("gz", got[2], f64[4], f32[4]), ("g_lss", got[3], f64[5], f32[5]), ("g_lm", got[4], f64[6], f32[6])):
        grad_error(what + " " + key, a, N(r64), N(r32))
    gz, gs, gm = emu.hmc2d_bwd(f, N(cz), N(c))
    grad_error(what + " gz vs emulator", got[2], gz, N(f32[4]))
    grad_error(what + " g_lss vs emulator", got[3], gs, N(f32[5]))
    grad_error(what + " g_lm vs emulator", got[4], gm, N(f32[6]))
    return f


@pytest.mark.parametrize("name", TARGETS)
def test_hmc_kernel_every_target(nfa, formulas, calls, name):
    hmc_continuous(nfa, formulas, calls, name, 257, 5, None, seed=100 + TARGETS.index(name))


@pytest.mark.parametrize("B,steps", [(1, 5), (257, 0), (257, 1)])
def test_hmc_kernel_shape_edges(nfa, formulas, calls, B, steps):
    for name in ("two_modes", "pair_two_modes_gauss"):
        f = hmc_continuous(nfa, formulas, calls, name, B, steps, None, seed=130 + steps)
        if steps == 0:              # no trajectory: z_out is z, the log-det and the tangents are zero
            assert not f["log_det"].any() and not f["tan_lss"].any() and not f["tan_lm"].any()


def test_hmc_kernel_with_clipping_that_binds(nfa, formulas, calls):
    f = hmc_continuous(nfa, formulas, calls, "two_modes", 257, 5, 4.0, seed=140)
    assert (np.abs(f["g_in"]) > 4.0).any(1).mean() > 0.5
    hmc_continuous(nfa, formulas, calls, "pair_circ_gmm_sinusoidal", 257, 5, 1.5, seed=141)


def test_second_sweep_of_the_grid_loops(nfa, formulas, calls):
    """grid x 256 + 3 rows: the rows of the second sweep of every kernel, forward and backward."""
    from normflows_amd import ops
    B = ops.hmc2d_grid(1 << 40) * 256 + 3
    assert ops.hmc2d_grid(B) * 256 < B and ops.mh2d_grid(B) * 256 < B and ops.hmc2d_bwd_grid(B) * 256 < B
    hmc_continuous(nfa, formulas, calls, "two_moons", B, 2, None, seed=150)
    target = make_target(nfa, "two_moons")
    terms = terms_of(target)
    z, eps, u, _, _ = rows(B, 151, steps=2)
    z_out, log_det, gs = ops.mh2d(z, eps, u, T(np.array([0.05], np.float32)), terms, 2, want_side=True)
    m = emu.mh2d(emu_terms(terms), N(z), N(eps), N(u), [np.float32(0.05)], 2)
    decided = mh_decided(m, N(u))
    tail = np.arange(B) >= B - 259
    assert decided[tail].mean() >= 0.9
    for sel in (decided, decided & tail):
        assert rel_error(N(z_out)[sel], m["z_out"][sel]) <= 1e-4 and rel_error(N(log_det)[sel], m["log_det"][sel]) <= 1e-4
        assert rel_error(N(gs)[sel][:, 2:], m["g_out"][sel]) <= 1e-4 * max(1.0, float(np.abs(m["g_out"]).max()))


def mh_decided(m, u):
    """Rows whose every step is decided: |log u - log ratio| beyond four times 1e-4 max(1, |log p|, |log p'|), or a ratio that far
    above one (it accepts whatever u is)."""
    thr = 4e-4 * np.maximum.reduce([np.ones_like(m["lp_cur"]), np.abs(m["lp_cur"]), np.abs(m["lp_prop"])])
    with np.errstate(divide="ignore"):
        return ((np.abs(np.log(u) - m["log_ratio"]) > thr) | (m["log_ratio"] > thr)).all(0) if len(u) else np.ones(u.shape[1], bool)


def mh_formula(nfa, target, steps, scale, z, eps, u, cz, c, dtype):
    layer = mh_layer(nfa, target if dtype == torch.float32 else to64(target), steps, scale, dtype)
    zz = z.to(dtype).clone().requires_grad_(True)
    z_out, log_det = layer._transition_torch(zz, eps.to(dtype), u.to(dtype))
    ((z_out * cz.to(dtype)).sum() + (log_det * c.to(dtype)).sum()).backward()
    return z_out.detach(), log_det.detach(), zz.grad


@pytest.mark.parametrize("name", TARGETS)
def test_mh_kernel_every_target(nfa, formulas, calls, name):
    """The random-walk steps with real uniforms: rows whose every step is decided agree with the emulator's float64."""
    target = make_target(nfa, name)
    steps, scale, B = 5, (0.05, 0.08), 257
    z, eps, u, cz, c = rows(B, 200 + TARGETS.index(name), steps=steps)
    terms = terms_of(target)
    m = emu.mh2d(emu_terms(terms), N(z), N(eps), N(u), np.array(scale, np.float32), steps)
    layer = mh_layer(nfa, target, steps, scale)
    zz = z.clone().requires_grad_(True)
    z_out, log_det = layer._transition(zz, eps, u)
    ((z_out * cz).sum() + (log_det * c).sum()).backward()
    assert calls["mh2d"] == 1 and calls["torch"] == 0
    with formulas():
        f32 = mh_formula(nfa, target, steps, scale, z, eps, u, cz, c, torch.float32)
        f64 = mh_formula(nfa, target, steps, scale, z, eps, u, cz, c, torch.float64)
    decided = mh_decided(m, N(u))
    print("%s: %d of %d rows decided" % (name, decided.sum(), B))
    assert decided.mean() >= 0.95             # (five steps of at most 1 % undecided each; test_mh_decisions holds the 1 % itself)
    assert np.array_equal((N(z_out) != N(z)).any(1)[decided], m["accept"].any(0)[decided])
    check_value(name + " mh z_out", z_out, m["z_out"], f32[0], f64[0], decided)
    check_value(name + " mh log_det", log_det, m["log_det"], f32[1], f64[1], decided)
    gz = emu.mh2d_bwd(m, N(cz), N(c))
    grad_error(name + " mh gz", zz.grad[T(decided)], gz[decided], N(f32[2])[decided])
    rejected = T(~m["accept"].any(0) & decided)
    assert torch.equal(z_out[rejected], z[rejected]) and bool((log_det[rejected] == 0.0).all())


@pytest.mark.parametrize("B,steps", [(1, 5), (257, 0), (257, 1)])
def test_mh_kernel_shape_edges(nfa, B, steps):
    from normflows_amd import ops
    target = make_target(nfa, "pair_two_modes_gauss")
    z, eps, u, _, _ = rows(B, 230 + steps, steps=steps)
    terms = terms_of(target)
    for scale in ([0.4], [0.4, 0.2]):       # (wide enough that a good part of the proposals is rejected)
        z_out, log_det, gs = ops.mh2d(z, eps, u, T(np.array(scale, np.float32)), terms, steps, want_side=True)
        m = emu.mh2d(emu_terms(terms), N(z), N(eps), N(u), np.array(scale, np.float32), steps)
        decided = mh_decided(m, N(u))
        assert rel_error(N(z_out)[decided], m["z_out"][decided]) <= 1e-4 and rel_error(N(log_det)[decided], m["log_det"][decided]) <= 1e-4
        assert rel_error(N(gs)[decided][:, :2], m["g_in"][decided]) <= 1e-3 * max(1.0, float(np.abs(m["g_in"]).max()))
        rejected = T(~m["accept"].any(0) & decided) if steps else torch.ones(B, dtype=torch.bool, device=DEV)
        assert torch.equal(z_out[rejected], z[rejected]) and not bool(log_det[rejected].any())
        assert torch.equal(gs[rejected][:, :2], gs[rejected][:, 2:])
        if B > 1 and steps == 1:
            assert 0.1 < float(rejected.float().mean()) < 0.9


# ---- 2. the decisions, with real uniforms ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["two_modes", "circ_gmm_8", "pair_two_modes_gauss"])
def test_hmc_decisions(nfa, formulas, name):
    from normflows_amd import ops
    target = make_target(nfa, name)
    B, steps = 1024, 5
    z, eps, u, cz, c = rows(B, 300 + TARGETS.index(name))
    terms = terms_of(target)
    lss, lm = T(np.array(LSS_WIDE, np.float32)), T(np.array(LM, np.float32))
    z_out, log_det, accept, _ = ops.hmc2d(z, eps, u, lss, lm, terms, steps, 0.0)
    f = emu.hmc2d(emu_terms(terms), N(z), N(eps), N(u), N(lss), N(lm), steps)
    largest = np.maximum.reduce([np.abs(f["lp_in"]), np.abs(f["lp_new"]), f["kin_in"], f["kin_new"], np.ones(B)])
    with np.errstate(divide="ignore"):
        decided = np.abs(np.log(N(u)) - f["log_ratio"]) > 4 * 1e-4 * largest
    print("%s: %d of %d rows undecided, %d accepted" % (name, (~decided).sum(), B, f["accept"].sum()))
    assert (~decided).sum() <= 0.01 * B
    assert 0 < f["accept"].sum() < B
    assert np.array_equal(N(accept)[decided] == 1.0, f["accept"][decided])
    with formulas():
        f32 = formula_hmc(nfa, target, steps, None, z, eps, u, cz, c, torch.float32, LSS_WIDE)
        f64 = formula_hmc(nfa, target, steps, None, z, eps, u, cz, c, torch.float64, LSS_WIDE)
    ok = decided & ((N(f32[0]) != N(z)).any(1) == f["accept"]) & ((N(f64[0]) != N(z)).any(1) == f["accept"])
    check_value(name + " z_out", z_out, f["z_out"], f32[0], f64[0], ok)
    check_value(name + " log_det", log_det, f["log_det"], f32[1], f64[1], ok)
    rejected = accept == 0.0
    assert torch.equal(z_out[rejected], z[rejected]) and bool((log_det[rejected] == 0.0).all())
    assert bool(((accept == 0.0) | (accept == 1.0)).all())


@pytest.mark.parametrize("name", ["two_modes", "circ_gmm_8", "pair_two_modes_gauss"])
def test_mh_decisions(nfa, formulas, name):
    """The decisions of every step of every decided row: the kernel on the first k steps' noise gives the state after step k, and
    step k was accepted exactly when that state moved."""
    from normflows_amd import ops
    target = make_target(nfa, name)
    B, steps, scale = 1024, 3, (0.4, 0.2)           # (wide enough that a good part of the proposals is rejected)
    z, eps, u, cz, c = rows(B, 350 + TARGETS.index(name), steps=steps)
    terms = terms_of(target)
    sc = T(np.array(scale, np.float32))
    m = emu.mh2d(emu_terms(terms), N(z), N(eps), N(u), np.array(scale, np.float32), steps)
    decided = mh_decided(m, N(u))
    print("%s: %d of %d rows undecided, accepted per step %s" % (name, (~decided).sum(), B, m["accept"].sum(1).tolist()))
    assert (~decided).sum() <= 0.01 * B
    assert all(0 < int(a) < B for a in m["accept"].sum(1))
    states = [z] + [ops.mh2d(z, eps[:k].contiguous(), u[:k].contiguous(), sc, terms, k)[0] for k in range(1, steps + 1)]
    flags = np.stack([(N(states[k + 1]) != N(states[k])).any(1) for k in range(steps)])
    assert np.array_equal(flags[:, decided], m["accept"][:, decided])
    z_out, log_det, _ = ops.mh2d(z, eps, u, sc, terms, steps)
    assert torch.equal(z_out, states[-1])
    with formulas():
        f32 = mh_formula(nfa, target, steps, scale, z, eps, u, cz, c, torch.float32)
        f64 = mh_formula(nfa, target, steps, scale, z, eps, u, cz, c, torch.float64)
    check_value(name + " mh z_out", z_out, m["z_out"], f32[0], f64[0], decided)
    check_value(name + " mh log_det", log_det, m["log_det"], f32[1], f64[1], decided)
    rejected = T(~m["accept"].any(0) & decided)
    assert bool(rejected.any())
    assert torch.equal(z_out[rejected], z[rejected]) and bool((log_det[rejected] == 0.0).all())


# ---- 3. the layers, same seed, switch off and on ----------------------------------------------------------------------------------
def own_bars(f32, f64, rows_ok):
    """The bars of a (z_out, log_det) pair: max(1e-4, 4 x the formula route's own float32-to-float64 error on that tensor), the own
    error taken over the rows on which both legs of the formula route took the same decisions."""
    return tuple(max(1e-4, 4 * rel_error(N(a)[rows_ok], N(b)[rows_ok])) for a, b in zip(f32, f64))


def rows_agree(a, b, bars=(1e-4, 1e-4)):
    """Fraction of the rows of two (z_out, log_det) pairs that agree within the bars, relative to max(1, |value|); a flipped decision
    makes a row differ grossly.  Without measured bars: the 1e-4 floor alone."""
    za, la, zb, lb = N(a[0]), N(a[1]), N(b[0]), N(b[1])
    ok = (np.abs(za - zb) <= bars[0] * np.maximum(1.0, np.abs(zb))).all(1) & (np.abs(la - lb) <= bars[1] * np.maximum(1.0, np.abs(lb)))
    return float(ok.mean())


def moved(out, z):
    return (N(out[0]) != N(z)).any(1)


def hais_prior_cpu(dtype):
    return cases.set_gauss(cases.TorchDiagGaussian(2).to(dtype), dtype)


def test_cpu_draws_float32_against_float64_formulas(nfa):
    """What the 98 % of the layer-level tests allows for: with CPU draws, the float32 formulas against the float64 formulas stay well
    inside it, within the 1e-4 floor alone -- for one layer and for the three-layer HAIS chain (the Gaussian as torch statements:
    this package's runs on the device only)."""
    z = rows(512, 400)[0].cpu()
    g = torch.Generator().manual_seed(401)
    prior_eps = torch.randn(512, 2, generator=g)
    noise = [(torch.randn(512, 2, generator=g), torch.rand(512, generator=g)) for _ in range(3)]
    single, chain = [], []
    for dtype in (torch.float32, torch.float64):
        layer = nfa.flows.HamiltonianMonteCarlo(nfa.distributions.TwoModes(2.0, 0.1), 5, torch.tensor(LSS, dtype=dtype),
                                                torch.tensor(LM, dtype=dtype))
        h = nfa.HAIS(torch.tensor(cases.HAIS_BETAS, dtype=dtype), hais_prior_cpu(dtype), nfa.distributions.TwoModes(2.0, 0.1), 3,
                     torch.tensor([0.08, 0.06], dtype=dtype), torch.tensor(LM, dtype=dtype))
        with torch.no_grad():
            single.append(layer._transition(z.to(dtype), noise[0][0].to(dtype), noise[0][1].to(dtype)))
            s = h.prior.loc + torch.exp(h.prior.log_scale) * prior_eps.to(dtype)
            lw = -h.prior.log_prob(s)
            for hl, (eps, u) in zip(h.layers, noise):
                s, d = hl._transition(s, eps.to(dtype), u.to(dtype))
                lw = lw + d
            chain.append((s, lw + h.target.log_prob(s)))
    frac, frac3 = rows_agree(single[0], single[1]), rows_agree(chain[0], chain[1])
    print("float32 against float64 formulas: %.4f of 512 rows agree for one layer, %.4f for the three-layer chain" % (frac, frac3))
    assert frac >= 0.99 and frac3 >= 0.99


@pytest.mark.parametrize("kind", ["hmc", "mh"])
@pytest.mark.parametrize("name", ["two_modes", "circ_gmm_8", "pair_two_modes_gauss"])
def test_layer_same_seed_off_and_on(nfa, formulas, calls, kind, name):
    target = make_target(nfa, name)
    layer = hmc_layer(nfa, target, 5) if kind == "hmc" else mh_layer(nfa, target, 5)
    z = rows(512, 410)[0]
    with torch.no_grad():
        torch.manual_seed(411)
        on = layer(z)
        assert (calls["hmc2d"], calls["mh2d"]) == ((1, 0) if kind == "hmc" else (0, 1)) and calls["torch"] == 0
        with formulas():
            torch.manual_seed(411)
            off = layer(z)
        assert calls["torch"] == 1 and calls["hmc2d"] + calls["mh2d"] == 1
        torch.manual_seed(411)
        again = layer.inverse(z)            # inverse is forward
        # the formula route's float64 leg on the same draws (replayed in the layer's order), for the bars
        torch.manual_seed(411)
        if kind == "hmc":
            eps, u = torch.randn_like(z), torch.rand(len(z), device=DEV)
            l64 = hmc_layer(nfa, to64(target), 5, dtype=torch.float64)
        else:
            draws = [(torch.randn(len(z), 2, device=DEV), torch.rand(len(z), device=DEV)) for _ in range(5)]
            eps, u = torch.stack([d[0] for d in draws]), torch.stack([d[1] for d in draws])
            l64 = mh_layer(nfa, to64(target), 5, dtype=torch.float64)
        assert torch.equal(layer._transition_torch(z, eps, u)[0], off[0])          # the replayed draws are the layer's
        f64 = l64._transition_torch(z.double(), eps.double(), u.double())
    assert torch.equal(again[0], on[0]) and torch.equal(again[1], on[1])
    if kind == "hmc":
        same = moved(off, z) == moved(f64, z)
    else:
        m = emu.mh2d(emu_terms(terms_of(target)), N(z), N(eps), N(u), N(layer.proposal.scale), 5)
        same = mh_decided(m, N(u))
    bars = own_bars(off, f64, same)
    frac = rows_agree(on, off, bars)
    print("%s %s: %.4f of 512 rows agree within %.1e (z_out), %.1e (log_det)" % ((kind, name, frac) + bars))
    assert frac >= 0.98
    assert 0.02 < float((on[0] != z).any(1).float().mean())


def test_layer_under_autograd_off_and_on(nfa, formulas, calls):
    target = make_target(nfa, "pair_two_modes_gauss")
    z, eps, u, cz, c = rows(512, 420)
    u = torch.zeros_like(u)
    got = kernel_hmc(nfa, target, 3, None, z, eps, u, cz, c)
    assert calls["hmc2d"] == 1 and calls["hmc2d_bwd"] == 1 and calls["want"] == [3] and calls["torch"] == 0
    with formulas():
        f32 = formula_hmc(nfa, target, 3, None, z, eps, u, cz, c, torch.float32)
        f64 = formula_hmc(nfa, target, 3, None, z, eps, u, cz, c, torch.float64)
    for key, a, r64, r32 in (("gz", got[2], f64[4], f32[4]), ("g_lss", got[3], f64[5], f32[5]), ("g_lm", got[4], f64[6], f32[6])):
        grad_error("layer " + key, a, N(r64), N(r32))


def test_hais_sample_off_and_on(nfa, formulas, calls):
    prior = gauss(nfa)
    h = nfa.HAIS(torch.tensor(cases.HAIS_BETAS), prior, nfa.distributions.TwoModes(2.0, 0.1), 3, torch.tensor([0.08, 0.06], device=DEV),
                 torch.tensor(LM, device=DEV))
    assert len(h.layers) == 3
    with torch.no_grad():
        torch.manual_seed(430)
        on = h.sample(512)
        assert calls["hmc2d"] == 3 and calls["torch"] == 0
        with formulas():
            torch.manual_seed(430)
            off = h.sample(512)
        assert calls["torch"] == 3 and calls["hmc2d"] == 3
        # the formula route's float64 leg on the same draws (replayed in the chain's order), for the bars
        torch.manual_seed(430)
        prior_eps = torch.randn(512, 2, device=DEV)
        noise = [(torch.randn(512, 2, device=DEV), torch.rand(512, device=DEV)) for _ in h.layers]
        legs = []
        for dtype in (torch.float32, torch.float64):
            pr = prior if dtype == torch.float32 else copy.deepcopy(prior).double()
            s = pr.loc + torch.exp(pr.log_scale) * prior_eps.to(dtype)
            lw, same = -pr.log_prob(s), []
            for hl, (eps, u) in zip(h.layers, noise):
                tgt = nfa.distributions.LinearInterpolation(h.target, pr, hl.target.alpha.to(dtype))
                l = nfa.flows.HamiltonianMonteCarlo(tgt, 3, hl.log_step_size.detach().to(dtype), hl.log_mass.detach().to(dtype))
                s2, d = l._transition_torch(s, eps.to(dtype), u.to(dtype))
                same.append(moved((s2,), s))
                s, lw = s2, lw + d
            legs.append(((s, lw + h.target.log_prob(s)), np.stack(same)))
    assert rel_error(N(legs[0][0][0]), N(off[0])) <= 1e-6          # the replayed draws are the chain's
    bars = own_bars(legs[0][0], legs[1][0], (legs[0][1] == legs[1][1]).all(0))
    frac = rows_agree(on, off, bars)
    print("HAIS: %.4f of 512 rows agree within %.1e (samples), %.1e (log_weights)" % ((frac,) + bars))
    assert frac >= 0.98
    assert np.isfinite(N(on[1])).all()


def test_normalizing_flow_with_an_hmc_layer(nfa, calls, monkeypatch):
    """A stochastic layer is a segment boundary for the chain routers: the [MaskedAffineFlow, ActNorm] runs on either side keep their
    one launch each (nf_realnvp_chain), and the model's pass equals the layer-by-layer calls."""
    F = nfa.flows
    chain = []
    real_chain = nfa.ops.realnvp_chain
    monkeypatch.setattr(nfa.ops, "realnvp_chain", lambda *a, **k: (chain.append(a[0].shape), real_chain(*a, **k))[1])
    torch.manual_seed(440)

    def coupling(i):
        b = torch.tensor([1.0, 0.0]) if i % 2 else torch.tensor([0.0, 1.0])
        return F.MaskedAffineFlow(b, nfa.nets.MLP([2, 16, 2], init_zeros=False), nfa.nets.MLP([2, 16, 2], init_zeros=False))
    target = nfa.distributions.TwoModes(2.0, 0.1)
    layers = [coupling(0), F.ActNorm((2,)), hmc_layer(nfa, target, 3), coupling(1), F.ActNorm((2,))]
    model = nfa.NormalizingFlow(nfa.distributions.DiagGaussian(2, trainable=False), layers, target).to(DEV)
    x = rows(512, 441)[0]
    with torch.no_grad():
        model.log_prob(x)                   # (ActNorm's data-dependent initialisation)
        calls["hmc2d"] = 0
        del chain[:]
        torch.manual_seed(442)
        lp = model.log_prob(x)
        assert calls["hmc2d"] == 1 and calls["torch"] == 0
        assert len(chain) == 2, chain         # one chain launch in front of the stochastic layer, one behind it
        torch.manual_seed(442)
        z, ld = x, torch.zeros(len(x), device=DEV)
        for f in reversed(layers):
            z, d = f.inverse(z)
            ld = ld + d
        want = ld + model.q0.log_prob(z)
    err = np.abs(N(lp) - N(want)) / np.maximum(1.0, np.abs(N(want)))
    print("model against layer by layer: worst %.3e" % err.max())
    assert (err <= 1e-4).mean() >= 0.98


# ---- 4. contracts -----------------------------------------------------------------------------------------------------------------
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
    z, eps, u, cz, c = rows(77, 500)
    _, eps5, u5, _, _ = rows(77, 501, steps=5)
    target = make_target(nfa, "pair_circ_gmm_sinusoidal")
    monkeypatch.setattr(ops, "torch", PaddedTorch())
    kernel_hmc(nfa, target, 3, None, z, eps, u, cz, c)
    layer = mh_layer(nfa, target, 5)
    zz = z.clone().requires_grad_(True)
    z_out, log_det = layer._transition(zz, eps5, u5)
    (z_out.sum() + log_det.sum()).backward()
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert len(bufs) == 4 + 3 + 3       # hmc: z_out, log_det, accept, side; its backward: gz, slabs, gpar; mh: z_out, log_det, gside
    for big, n in bufs:
        assert bool((big[:64] == CANARY).all()) and bool((big[64 + n:] == CANARY).all())
        assert not bool((big[64:64 + n] == CANARY).any())      # ... and every element inside was written


def test_backward_is_deterministic(nfa):
    target = make_target(nfa, "circ_gmm_8")
    z, eps, u, cz, c = rows(3001, 510)
    a = kernel_hmc(nfa, target, 4, None, z, eps, u, cz, c)
    b = kernel_hmc(nfa, target, 4, None, z, eps, u, cz, c)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_frozen_parameters_make_no_reduction_launch(nfa, calls):
    target = make_target(nfa, "two_modes")
    z, eps, u, cz, c = rows(300, 520)
    full = kernel_hmc(nfa, target, 3, None, z, eps, u, cz, c)
    for freeze, want in ((("log_step_size",), 2), (("log_mass",), 1), (("log_step_size", "log_mass"), 0)):
        layer = hmc_layer(nfa, target, 3)
        for k in freeze:
            getattr(layer, k).requires_grad_(False)
        zz = z.clone().requires_grad_(True)
        z_out, log_det = layer._transition(zz, eps, u)
        ((z_out * cz).sum() + (log_det * c).sum()).backward()
        assert calls["want"][-1] == want and calls["torch"] == 0
        assert torch.equal(zz.grad, full[2])
        for k, ref in (("log_step_size", full[3]), ("log_mass", full[4])):
            g = getattr(layer, k).grad
            assert (g is None) if k in freeze else torch.equal(g, ref)
    # nobody wants a gradient: the inference launch, nothing saved
    layer = hmc_layer(nfa, target, 3)
    for p in layer.parameters():
        p.requires_grad_(False)
    n = calls["hmc2d_bwd"]
    z_out, log_det = layer._transition(z, eps, u)
    assert z_out.grad_fn is None and log_det.grad_fn is None and calls["hmc2d_bwd"] == n
    assert torch.equal(z_out, full[0]) and torch.equal(log_det, full[1])


def test_absent_cotangents(nfa, calls):
    """Only z_out used, or only log_det used: the missing cotangent is a zero (the ops-level backward on explicit zeros, same bits)."""
    from normflows_amd import ops
    target = make_target(nfa, "two_modes")
    z, eps, u, cz, c = rows(300, 530)
    lss, lm = T(np.array(LSS, np.float32)), T(np.array(LM, np.float32))
    _, _, accept, side = ops.hmc2d(z, eps, u, lss, lm, terms_of(target), 3, 0.0, want_side=True)
    for use_z in (True, False):
        layer = hmc_layer(nfa, target, 3)
        zz = z.clone().requires_grad_(True)
        z_out, log_det = layer._transition(zz, eps, u)
        ((z_out * cz).sum() if use_z else (log_det * c).sum()).backward()
        gz, gpar = ops.hmc2d_bwd(cz if use_z else torch.zeros_like(cz), torch.zeros_like(c) if use_z else c, accept, side, True, 3)
        assert torch.equal(zz.grad, gz) and torch.equal(layer.log_step_size.grad, gpar[:2]) and torch.equal(layer.log_mass.grad, gpar[2:])
        assert bool(gz.any()) and bool(gpar.any())
    # neither used: no backward launch at all
    layer = hmc_layer(nfa, target, 3)
    zz = z.clone().requires_grad_(True)
    z_out, log_det = layer._transition(zz, eps, u)
    n = calls["hmc2d_bwd"]
    (z_out.sum() * 0 + zz.sum()).backward()
    assert calls["hmc2d_bwd"] == n + 1         # (a zero cotangent that is present still runs)
    # mh: only z_out used -> the cotangent passes through; only log_det used -> the telescoped expression
    _, eps5, u5, _, _ = rows(300, 531, steps=4)
    layer = mh_layer(nfa, target, 4)
    zz = z.clone().requires_grad_(True)
    (layer._transition(zz, eps5, u5)[0] * cz).sum().backward()
    assert torch.equal(zz.grad, cz)
    zz = z.clone().requires_grad_(True)
    z_out, log_det = layer._transition(zz, eps5, u5)
    (log_det * c).sum().backward()
    gs = ops.mh2d(z, eps5, u5, layer.proposal.scale.reshape(-1), terms_of(target), 4, want_side=True)[2]
    assert torch.equal(zz.grad, c.unsqueeze(1) * (gs[:, :2] - gs[:, 2:]))
    assert calls["torch"] == 0


def test_live_parameters(nfa, calls):
    """An in-place change of log_mass, and of the proposal's scale, is seen by the next call (the kernels read them on the device)."""
    target = make_target(nfa, "two_modes")
    z, eps, u, _, _ = rows(300, 540)
    u = torch.zeros_like(u)
    layer = hmc_layer(nfa, target, 3)
    with torch.no_grad():
        a = layer._transition(z, eps, u)
        layer.log_mass.add_(0.5)
        b = layer._transition(z, eps, u)
        other = nfa.flows.HamiltonianMonteCarlo(target, 3, torch.tensor(LSS), torch.tensor(LM) + 0.5).to(DEV)
        want = other._transition(z, eps, u)
    assert not torch.equal(a[0], b[0]) and torch.equal(b[0], want[0]) and torch.equal(b[1], want[1])
    _, eps5, u5, _, _ = rows(300, 541, steps=3)
    mh = mh_layer(nfa, target, 3, 0.05)
    with torch.no_grad():
        a = mh._transition(z, eps5, u5)
        mh.proposal.scale.mul_(2.0)
        b = mh._transition(z, eps5, u5)
        want = mh_layer(nfa, target, 3, 0.1)._transition(z, eps5, u5)
    assert not torch.equal(a[0], b[0]) and torch.equal(b[0], want[0]) and torch.equal(b[1], want[1])
    assert calls["torch"] == 0


def test_views_and_float64_inputs_take_the_formulas(nfa, calls):
    target = make_target(nfa, "two_modes")
    z, eps, u, _, _ = rows(64, 550)
    layer, mh = hmc_layer(nfa, target, 2), mh_layer(nfa, target, 2)
    wide = torch.zeros(64, 4, device=DEV)
    wide[:, :2] = z
    with torch.no_grad():
        base = layer._transition(z, eps, u)
        assert calls["hmc2d"] == 1 and calls["torch"] == 0
        view = layer._transition(wide[:, :2], eps, u)                   # a strided view
        assert calls["hmc2d"] == 1 and calls["torch"] == 1
        layer64 = hmc_layer(nfa, target, 2, dtype=torch.float64)
        out64 = layer64._transition(z.double(), eps.double(), u.double())
        assert calls["hmc2d"] == 1 and calls["torch"] == 2 and out64[0].dtype == torch.float64
        mh(wide[:, :2])
        mh_layer(nfa, target, 2, dtype=torch.float64)(z.double())
        assert calls["mh2d"] == 0 and calls["torch"] == 4
        with nfa.config.higher_order_gradients():
            layer._transition(z, eps, u)
        assert calls["hmc2d"] == 1 and calls["torch"] == 5
    assert rows_agree(base, view) >= 0.98        # (the 1e-4 floor alone)


def test_capture_and_replay(nfa, calls):
    """The explicit-noise ops recorded with torch.cuda.graph and replayed with new contents: no host synchronisation, the eager bits."""
    target = make_target(nfa, "pair_circ_gmm_sinusoidal")
    layer, mh = hmc_layer(nfa, target, 3), mh_layer(nfa, target, 3)
    sets = [rows(500, s) for s in (560, 561, 562)]
    sets5 = [rows(500, s, steps=3) for s in (560, 561, 562)]
    with torch.no_grad():
        eager = [layer._transition(z, eps, u) + mh._transition(z, e5, u5) for (z, eps, u, _, _), (_, e5, u5, _, _) in zip(sets, sets5)]
        static = [t.clone() for t in sets[0][:3]] + [t.clone() for t in sets5[0][1:3]]
        torch.cuda.synchronize()
        n = calls["hmc2d"] + calls["mh2d"]
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = layer._transition(*static[:3]) + mh._transition(static[0], static[3], static[4])
        assert calls["hmc2d"] + calls["mh2d"] == n + 2 and calls["torch"] == 0
        for (z, eps, u, _, _), (_, e5, u5, _, _), want in list(zip(sets, sets5, eager))[1:]:
            for dst, src in zip(static, (z, eps, u, e5, u5)):
                dst.copy_(src)
            graph.replay()
            torch.cuda.synchronize()
            for a, b in zip(out, want):
                assert torch.equal(a, b)
