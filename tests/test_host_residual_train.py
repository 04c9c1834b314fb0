"""Training of 2-D Residual layers on the kernels of csrc/lipmlp_train.hip, the parts that need no GPU: the kernels' arithmetic
(tests/residual_train_emulator.py) against the reference's fixtures through the route's own host code (lipmlp_pack.run_train with
ops' two entry points replaced by the emulator), pack_train's gradient, train_eligible's table, the C ABI's symbols and argument
checks, and the kernels' register budget."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import residual_cases as cases
import residual_train_cases as tc
import residual_train_emulator as emu
from conftest import TOL, assert_close, ld_tol
from test_host_rank1 import grads_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EST_2D = ["basic_geometric", "neumann_memsave_geometric", "neumann_plain_geometric", "basic_memsave_geometric", "basic_poisson",
          "neumann_memsave_poisson", "series5_basic", "series5_memsave"]


@pytest.fixture(scope="module")
def nfa():
    import __graft_entry__
    import normflows_amd
    if not os.path.exists(normflows_amd.native_library_path()):
        __graft_entry__.build()
    return normflows_amd


def check_layer(f, g, run, dtype="float32", leg=""):
    """One seeded step of layer `f` by `run(f, x)` against the legs `leg` of fixture g: outputs, every gradient, the buffers."""
    dt = getattr(torch, dtype)
    seed = int(g["seed"])
    x, cz, cl = (torch.from_numpy(g[k]).to(dt) for k in ("x", "cz", "cl"))
    xx = x.clone().requires_grad_(True)
    np.random.seed(seed)
    torch.manual_seed(seed)
    z, ld = run(f, xx)
    ((z * cz).sum() + (ld * cl).sum()).backward()
    assert ld.shape == (x.shape[0],)
    assert_close(z.detach().numpy(), g["z" + leg], what="z", **TOL[np.dtype(dtype)])
    assert_close(ld.detach().numpy(), g["ld" + leg], what="ld", **ld_tol(dtype))
    grads_close(xx.grad.numpy(), g["gx" + leg], "gx")
    n = 0
    for k, p in f.named_parameters():
        key = "g%s__%s" % (leg, k.replace(".", "__"))
        if leg and not any(q.startswith("g%s__" % leg) for q in g):
            continue        # (a large case keeps no float64 parameter gradients)
        assert (p.grad is None) == (key not in g), k
        if p.grad is not None:
            grads_close(p.grad.numpy(), g[key], k)
            n += 1
    blk = f.iresblock
    assert np.array_equal(blk.last_n_samples.numpy(), g["last_n_samples" + leg])
    assert_close(blk.last_firmom.numpy(), g["last_firmom" + leg], what="firmom", **ld_tol(dtype))
    assert_close(blk.last_secmom.numpy(), g["last_secmom" + leg], what="secmom", **ld_tol(dtype))
    return n


def emulated(calls):
    from normflows_amd.flows import lipmlp_pack as lp

    def run(f, x):
        before = calls["fwd"]
        out, drawn = lp.run_train(f, x)
        assert out is not None and drawn is None and calls["fwd"] == before + 1
        return out
    return run


@pytest.mark.parametrize("dtype,leg", [("float32", ""), ("float64", "_f64")])
@pytest.mark.parametrize("name", list(tc.LAYERS))
def test_emulator_reproduces_the_training_fixtures(nfa, monkeypatch, name, dtype, leg):
    """The kernels' formulas, run_train's draws and pack_train's graph together give the reference's numbers: z, ld, gx and every
    parameter gradient of a seeded step, in the kernels' float32 and -- the formulas themselves -- in float64."""
    calls = emu.patched(monkeypatch)
    g = tc.load(name)
    f = tc.layer(nfa, name).flows[0]
    f.load_state_dict(tc.state(g), strict=True)
    f = f.to(getattr(torch, dtype))
    n = check_layer(f, g, emulated(calls), dtype, leg)
    assert n >= 4 or (leg and n == 0)
    assert calls["bwd"] == 1 and calls["want"] == [True]


@pytest.mark.parametrize("name", EST_2D)
def test_emulator_reproduces_the_estimator_fixtures(nfa, monkeypatch, name):
    """The eight d = 2 fixtures of the stochastic branches (tests/golden/residual_est_*.npz), the memory-saving wrapper's
    first-row cotangent included."""
    calls = emu.patched(monkeypatch)
    g = cases.load("est_" + name)
    f = cases.estimator_layer(nfa, name)
    f.load_state_dict(tc.state(g), strict=True)
    assert check_layer(f, g, emulated(calls)) >= 6
    assert calls["bwd"] == 1


@pytest.mark.parametrize("dtype,leg", [("float32", ""), ("float64", "_f64")])
def test_emulator_reproduces_the_stack_fixture(nfa, monkeypatch, dtype, leg):
    """3 x [Residual, ActNorm] through forward_kld's own walk (the layers reversed, every one's inverse; ActNorm and the base
    density have kernels only, so their formulas -- affine/coupling.py:38-54, base.py:89-97 -- are written out): the loss and every
    parameter's gradient."""
    calls = emu.patched(monkeypatch)
    run = emulated(calls)
    dt = getattr(torch, dtype)
    g = tc.load(tc.STACK)
    m = tc.stack(nfa)
    m.load_state_dict(tc.state(g), strict=True)
    m = m.to(dt)
    z = torch.from_numpy(g["x"]).to(dt)
    np.random.seed(int(g["seed"]))
    torch.manual_seed(int(g["seed"]))
    log_q = torch.zeros(z.shape[0], dtype=dt)
    for f in reversed(m.flows):
        if hasattr(f, "iresblock"):
            z, ld = run(f, z)
        else:
            z, ld = (z - f.t) * torch.exp(-f.s), -f.s.sum()
        log_q = log_q + ld
    log_q = log_q - 0.5 * 2 * np.log(2 * np.pi) - 0.5 * (z * z).sum(1)         # DiagGaussian(2, trainable=False): loc 0, scale 1
    loss = -log_q.mean()
    loss.backward()
    assert calls["fwd"] == 3 and calls["bwd"] == 3 and calls["want"] == [True] * 3
    t = ld_tol("float32")       # (both legs: the reference's log_prob keeps a float32 accumulator whatever the model's dtype)
    assert_close(loss.detach().numpy(), g["loss" + leg], what="loss", rtol=t["rtol"], atol=6 * t["atol"])
    n = 0
    for k, p in m.named_parameters():
        key = "g%s__%s" % (leg, k.replace(".", "__"))
        assert (p.grad is None) == (key not in g), k
        if p.grad is not None:
            grads_close(p.grad.numpy(), g[key], k)
            n += 1
    assert n == 3 * 6 + 3 * 2


def test_torch_route_reproduces_the_training_fixtures(nfa):
    """The switch-off route (the GPU tests' other leg) gives the same fixtures: one case per estimator kind."""
    for name in ("brute_h32", "basic_h40x24", "poisson3_h32", "exact_h64"):
        g = tc.load(name)
        f = tc.layer(nfa, name).flows[0]
        f.load_state_dict(tc.state(g), strict=True)
        assert check_layer(f, g, lambda f_, x: tc.density(f_, x)) >= 4


def test_a_truncation_beyond_32_terms_goes_to_the_formulas_with_its_draw(nfa, monkeypatch):
    from normflows_amd.flows import lipmlp_pack as lp
    calls = emu.patched(monkeypatch)
    torch.manual_seed(3)
    f = nfa.flows.Residual(nfa.nets.LipschitzMLP([2, 8, 2], init_zeros=False)).train()
    x = torch.randn(5, 2)
    draws = []

    def forty(p, m):
        draws.append(m)
        return np.full(m, 40)
    monkeypatch.setattr(nfa.flows.residual, "geometric_sample", forty)
    out, drawn = lp.run_train(f, x)
    assert out is None and calls["fwd"] == 0 and drawn[0] == 42 and draws == [1]
    # the layer's own pass hands that draw to the formulas: nothing is drawn twice, and the result is the formulas' under one seed
    monkeypatch.setattr(lp, "train_eligible", lambda layer, z, density=True: True)
    torch.manual_seed(11)
    z, ld = f.inverse(x)
    assert draws == [1, 1] and calls["fwd"] == 0 and np.array_equal(f.iresblock.last_n_samples.numpy(), [40.0])
    monkeypatch.setattr(lp, "train_eligible", lambda layer, z, density=True: False)
    torch.manual_seed(11)
    z2, ld2 = f.inverse(x)
    assert draws == [1, 1, 1] and torch.equal(z, z2) and torch.equal(ld, ld2)


def test_pack_train_is_pack_and_its_gradient_reaches_every_parameter(nfa):
    """pack_train gives pack's blob, and a cotangent on the blob reaches weight (through sigma and the clamp), bias and beta with
    the values the modules' own compute_weight / softplus give."""
    from normflows_amd.flows import lipmlp_pack as lp
    for name in ("basic_h40x24", "slack_h32", "neumann_h128x3"):
        g = tc.load(name)
        f = tc.layer(nfa, name).flows[0]
        f.load_state_dict(tc.state(g), strict=True)
        hp = lp.width([f])
        blob = lp.pack_train(f, hp)
        # (pack sums sigma's <= 128 products batched over the layers of one shape, pack_train per layer: the order may differ)
        assert_close(blob.detach().numpy(), lp.pack([f], False)[0].numpy(), what="blob", rtol=1e-5, atol=1e-7)
        R = torch.randn(blob.shape, generator=torch.Generator().manual_seed(1))
        (blob * R).sum().backward()
        got = {k: p.grad.clone() for k, p in f.named_parameters() if p.grad is not None}
        f.zero_grad(set_to_none=True)
        pairs = lp.linears(f.iresblock.nnet)
        hdr, blk = R[:lp.HDR], R[lp.HDR:]
        n = len(pairs)
        loss = sum(torch.nn.functional.softplus(sw.beta)[0] * hdr[2 + i] for i, (sw, _) in enumerate(pairs))
        h1 = pairs[0][1].out_features
        loss = loss + (pairs[0][1].compute_weight(update=False).t() * blk[:2 * hp].view(2, hp)[:, :h1]).sum()
        loss = loss + (pairs[0][1].bias * blk[2 * hp:2 * hp + h1]).sum()
        for m in range(n - 2):
            lin = pairs[1 + m][1]
            o = 3 * hp + m * (hp * hp + hp)
            loss = loss + (lin.compute_weight(update=False).t() * blk[o:o + hp * hp].view(hp, hp)[:lin.in_features, :lin.out_features]).sum()
            loss = loss + (lin.bias * blk[o + hp * hp:o + hp * hp + lin.out_features]).sum()
        o = 3 * hp + 2 * (hp * hp + hp)
        last = pairs[-1][1]
        loss = loss + (last.compute_weight(update=False) * blk[o:o + 2 * hp].view(2, hp)[:, :last.in_features]).sum()
        loss = loss + (last.bias * blk[o + 2 * hp:o + 2 * hp + 2]).sum()
        loss.backward()
        want = {k: p.grad for k, p in f.named_parameters() if p.grad is not None}
        assert set(got) == set(want) and len(got) == 3 * n
        for k in got:
            assert_close(got[k].numpy(), want[k].numpy(), what=k, rtol=1e-5, atol=1e-6)
        for _, lin in pairs:        # every layer's `scale` holds its sigma
            assert float(lin.scale) == pytest.approx(float(torch.dot(lin.u, torch.mv(lin.weight.detach(), lin.v))), rel=1e-6)


def test_train_eligible_table(nfa, monkeypatch):
    from normflows_amd.flows import lipmlp_pack as lp
    on_device = lp._on_device

    class AsIfOnTheDevice:          # (the table, not the device: the one attribute a CPU tensor answers differently)
        def __init__(self, t):
            self.t = t
        is_cuda = True

        def __getattr__(self, k):
            return getattr(self.t, k)
    monkeypatch.setattr(torch, "is_tensor", lambda t, real=torch.is_tensor: real(t) or isinstance(t, AsIfOnTheDevice))
    monkeypatch.setattr(lp, "_on_device", lambda z: on_device(AsIfOnTheDevice(z)))
    capturing = [False]
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: capturing[0])
    torch.manual_seed(0)

    def layer(channels=(2, 16, 2), **kw):
        return nfa.flows.Residual(nfa.nets.LipschitzMLP(list(channels), init_zeros=False), **kw)

    f, x = layer().train(), torch.randn(6, 2)
    assert nfa.config.residual_train is False and not lp.train_eligible(f, x)                    # default OFF
    monkeypatch.setattr(nfa.config, "residual_train", True)
    assert lp.train_eligible(f, x)
    assert not lp.train_eligible(f, x, density=False)                                            # the fixed-point direction
    monkeypatch.setattr(nfa.config, "residual_chain", False)
    assert not lp.train_eligible(f, x)
    monkeypatch.setattr(nfa.config, "residual_chain", True)
    with nfa.config.higher_order_gradients():
        assert not lp.train_eligible(f, x)
    assert not lp.train_eligible(f, x.double()) and not lp.train_eligible(f, torch.randn(6, 3))
    assert not lp.train_eligible(f, torch.randn(0, 2)) and not lp.train_eligible(f, torch.randn(6, 4)[:, ::2])
    assert not lp.train_eligible(f, torch.randn(2, 6, 2))

    class Sub(nfa.flows.Residual):
        pass
    sub = Sub(nfa.nets.LipschitzMLP([2, 16, 2]))
    assert not lp.train_eligible(sub, x)
    assert not lp.train_eligible(layer((2, 16, 16, 16, 16, 2)), x)                               # four hidden layers
    assert not lp.train_eligible(layer((2, 200, 2)), x)                                          # wider than 128
    assert not lp.train_eligible(layer().double(), x)
    # what needs the route: a gradient, or a stochastic estimator in training mode
    ev = layer().eval()
    assert lp.train_eligible(ev, x)                                                              # parameters require a gradient
    with torch.no_grad():
        assert not lp.train_eligible(ev, x) and lp.train_eligible(f, x)                          # (inference route / stochastic)
    for p in ev.parameters():
        p.requires_grad_(False)
    assert not lp.train_eligible(ev, x) and lp.train_eligible(ev, x.clone().requires_grad_(True))
    brute = layer(brute_force=True).train()
    with torch.no_grad():
        assert not lp.train_eligible(brute, x)
    assert lp.train_eligible(brute, x)
    assert lp.train_eligible(layer(n_power_series=32).train(), x) and not lp.train_eligible(layer(n_power_series=33).train(), x)
    capturing[0] = True         # recorded: deterministic truncations only
    assert not lp.train_eligible(f, x) and lp.train_eligible(brute, x) and lp.train_eligible(layer(n_power_series=4).train(), x)
    assert lp.train_eligible(layer().eval(), x)


def test_symbols_are_declared_exported_bound_and_validate_their_arguments(nfa):
    from normflows_amd.flows import lipmlp_pack as lp
    lib = nfa._lib.lib()
    for sym in ("nf_lipmlp_train_rows", "nf_lipmlp_train_scratch_floats", "nf_lipmlp_train_fwd", "nf_lipmlp_train_bwd"):
        assert sym in nfa._lib.exported_symbols_declared() and hasattr(lib, sym), sym
    assert "nf_lipmlp_train_scratch_floats" in nfa._lib.int64_functions_declared()
    assert lib.nf_lipmlp_train_scratch_floats.restype is ctypes.c_int64
    for name in ("lipmlp_train_fwd", "lipmlp_train_bwd", "lipmlp_train_rows"):
        assert hasattr(nfa.ops, name)
    assert hasattr(nfa.autograd, "LipMlpTrainFn") and hasattr(nfa.config, "set_residual_train")
    EINVAL, ENOTSUP, EFAULT, ERANGE = -22, -95, -14, -34
    assert [lib.nf_lipmlp_train_rows(h) for h in (32, 64, 128)] == [64, 32, 16] and lib.nf_lipmlp_train_rows(48) == ENOTSUP
    W = lib.nf_persistent_workgroups()
    sf = lib.nf_lipmlp_train_scratch_floats
    nb = {hp: 16 + lp.rstride(hp) for hp in (32, 64, 128)}
    assert sf(1, 128) == nb[128] and sf(17, 128) == 2 * nb[128] and sf(10 ** 6, 128) == W * nb[128] and sf(0, 32) == 0
    assert sf(5, 48) == ENOTSUP and sf(-1, 32) == EINVAL
    vp = ctypes.c_void_p
    null, ok = vp(0), vp(4096)
    coef = (ctypes.c_float * 32)(*([1.0] * 32))

    def fwd(B=8, hp=32, kind=2, nterms=3, nblob=None, coef=coef, **p):
        a = dict(x=ok, vareps=ok, y=ok, ld=ok, jhat=ok, blob=ok)
        a.update(p)
        return lib.nf_lipmlp_train_fwd(a["x"], a["vareps"], a["y"], a["ld"], a["jhat"], a["blob"], nb[hp] if nblob is None else nblob,
                                       B, hp, kind, nterms, coef, None)

    def bwd(B=8, hp=32, want=1, nblob=None, **p):
        a = dict(x=ok, gy=ok, jhat=ok, w=ok, gx=ok, blob=ok, slabs=ok, gblob=ok)
        a.update(p)
        return lib.nf_lipmlp_train_bwd(a["x"], a["gy"], a["jhat"], a["w"], a["gx"], a["blob"], a["slabs"], a["gblob"],
                                       nb[hp] if nblob is None else nblob, B, hp, want, None)

    for call in (fwd, bwd):         # every one of these returns before any launch
        assert call(hp=48, nblob=100) == ENOTSUP and call(B=-1) == EINVAL and call(nblob=17) == EINVAL
        assert call(B=0) == 0 and call(blob=null) == EFAULT and call(x=null) == EFAULT and call(jhat=vp(4100)) == EINVAL
    assert fwd(kind=4) == EINVAL and fwd(kind=-1) == EINVAL and fwd(nterms=33) == ERANGE and fwd(nterms=0) == EINVAL
    assert fwd(kind=1, vareps=null) == EFAULT and fwd(kind=3, coef=None) == EFAULT
    for k in ("y", "ld", "jhat"):
        assert fwd(**{k: null}) == EFAULT, k
    assert fwd(B=0, x=null, vareps=null, y=null, ld=null, jhat=null, blob=null) == 0             # B == 0: no pointer is looked at
    assert bwd(B=0, x=null, gy=null, jhat=null, w=null, gx=null, blob=null, slabs=null, gblob=null) == 0
    assert bwd(want=2) == EINVAL and bwd(slabs=null) == EFAULT and bwd(gblob=null) == EFAULT and bwd(jhat=null) == EFAULT
    assert bwd(want=0, gx=null, slabs=null, gblob=null) == 0                                     # nothing asked for: no launch


def test_ops_refuse_bad_operands_before_any_launch(nfa, monkeypatch):
    from normflows_amd.flows import lipmlp_pack as lp
    called = []
    monkeypatch.setattr(nfa._lib, "call", lambda *a: called.append(a))
    monkeypatch.setattr(nfa._lib, "_require_device", lambda tensors: None)
    x, blob = torch.zeros(4, 2), torch.zeros(16 + lp.rstride(32))
    bad = [lambda: nfa.ops.lipmlp_train_fwd(torch.zeros(4, 3), blob, 32, 0),
           lambda: nfa.ops.lipmlp_train_fwd(x, blob[:-1], 32, 0),
           lambda: nfa.ops.lipmlp_train_fwd(x, blob, 32, 4),
           lambda: nfa.ops.lipmlp_train_fwd(x, blob, 32, 1, (1.0,)),                             # no vareps
           lambda: nfa.ops.lipmlp_train_fwd(x, blob, 32, 1, (1.0,), torch.zeros(5, 2)),
           lambda: nfa.ops.lipmlp_train_bwd(x, torch.zeros(5, 2), torch.zeros(4, 4), torch.zeros(4), blob, 32, True),
           lambda: nfa.ops.lipmlp_train_bwd(x, x, torch.zeros(4, 3), torch.zeros(4), blob, 32, True),
           lambda: nfa.ops.lipmlp_train_bwd(x, x, torch.zeros(4, 4), torch.zeros(5), blob, 32, True)]
    for call in bad:
        with pytest.raises(ValueError):
            call()
    with pytest.raises(TypeError):
        nfa.ops.lipmlp_train_fwd(x.double(), blob, 32, 0)
    with pytest.raises(TypeError):
        nfa.ops.lipmlp_train_bwd(x, x, torch.zeros(4, 4).double(), torch.zeros(4), blob, 32, True)
    with pytest.raises(NotImplementedError):
        nfa.ops.lipmlp_train_fwd(x, torch.zeros(100), 48, 0)
    assert not called


def test_kernels_use_no_scratch(nfa):
    """Zero scratch bytes and no spills for every kernel of lipmlp_train.hip cross-compiled for gfx950.  The backward holds one
    workgroup of four waves per CU (its LDS), one wave per SIMD: up to 512 registers per lane are there to be used."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    seen = 0
    for name, d in kr.resources(os.path.join(ROOT, "normalizing-flows_amd", "lib", "obj", "lipmlp_train.o")).items():
        if "lipmlp_train_" in name:
            seen += 1
            limit = 512 if "bwd" in name else 256
            assert d["vgpr_spill_count"] == 0 and d["private_segment_fixed_size"] == 0 and d["vgpr_count"] <= limit, (name, d)
    assert seen == 13, seen     # forward and backward at three padded widths, 16-byte and 4-byte weight loads; the reduction
