"""CPU-side tests of the Residual flows and their HIP route (flows/residual.py, nets.LipschitzMLP / InducedNormLinear / Swish,
utils/optim.py, flows/lipmlp_pack.py, csrc/lipmlp.hip): the classes against the reference's fixtures (tests/golden/residual_*.npz:
state dicts, seeded construction, both precisions of the torch route in both directions, every stochastic estimator under the
reference's seeds, the power iteration), a float32 NumPy emulator of the kernels' arithmetic on the packed blob
(tests/residual_emulator.py) against the same fixtures, the C ABI's argument checks and the kernels' code-object resources."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import residual_cases as cases
import residual_emulator as emu
from conftest import TOL, assert_close, golden_state, ld_tol
from test_host_rank1 import grads_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = [("float32", ""), ("float64", "_f64")]


@pytest.fixture(scope="module")
def nfa():
    import __graft_entry__
    import normflows_amd
    if not os.path.exists(normflows_amd.native_library_path()):
        __graft_entry__.build()
    return normflows_amd


def fixture_stack(nfa, name, dtype=torch.float32):
    g = cases.load(name)
    m = cases.stack(nfa, name)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in golden_state(g).items()}, strict=True)
    return m.to(dtype), g


def layer_on_cpu(f, x, inverse):
    """(z, log_det) of one layer on a CPU tensor.  ActNorm has kernels only (the package has no CPU path for it): its formulas
    (affine/coupling.py:38-54) are written out here."""
    if hasattr(f, "iresblock"):
        return f.inverse(x) if inverse else f(x)
    s, t = f.s.detach(), f.t.detach()
    if inverse:
        return (x - t) * torch.exp(-s), -s.sum()
    return x * torch.exp(s) + t, s.sum()


def walk_with_counts(flows, x, inverse, sampling):
    """cases.walk, and in the fixed-point direction the further steps every Residual layer's iteration takes."""
    counts, lds = [], []
    for f in (reversed(flows) if inverse else flows):
        if sampling and hasattr(f, "iresblock"):
            with torch.no_grad():
                f.iresblock._inverse_fixed_point(x, count=counts)
        x, l = layer_on_cpu(f, x, inverse)
        lds.append(l.detach() * torch.ones(x.shape[0], dtype=x.dtype))
        x = x.detach()
    return x, lds, counts


# ---- the classes against the reference ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.STACKS))
def test_state_dicts_load_both_ways_and_seeded_construction_is_bit_identical(nfa, name):
    g = cases.load(name)
    ref_sd = golden_state(g)
    m = cases.stack(nfa, name)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in ref_sd.items()}, strict=True)
    ours = m.state_dict()
    assert list(ours) == list(ref_sd)
    for k, v in ours.items():
        assert tuple(v.shape) == ref_sd[k].shape and v.numpy().dtype == ref_sd[k].dtype and np.array_equal(v.numpy(), ref_sd[k]), k
    keys = list(ours)
    assert keys[:7] == ["q0.loc", "q0.log_scale", "flows.0.iresblock.geom_p", "flows.0.iresblock.lamb",
                        "flows.0.iresblock.last_n_samples", "flows.0.iresblock.last_firmom", "flows.0.iresblock.last_secmom"]
    assert keys[7:13] == ["flows.0.iresblock.nnet.net.0.beta"] + ["flows.0.iresblock.nnet.net.1." + k
                                                                  for k in ("weight", "bias", "scale", "u", "v")]
    ref0 = golden_state(g, prefix="sd0__")
    if name in ("h128x2_k16", "h128x3_k3"):
        assert not ref0         # (too large to keep twice: the models of 128 x 128 layers have no seeded copy)
        return
    seeded = cases.stack(nfa, name, seed=int(g["seed"])).state_dict()      # (the generator may have moved on to a later seed)
    assert list(seeded) == list(ref0)
    for k, v in seeded.items():
        assert v.numpy().dtype == ref0[k].dtype and np.array_equal(v.numpy(), ref0[k]), k


@pytest.mark.parametrize("dtype,leg", LEGS)
@pytest.mark.parametrize("name", list(cases.STACKS))
def test_torch_route_reproduces_the_fixtures_on_the_cpu(nfa, name, dtype, leg):
    dt = getattr(torch, dtype)
    m, g = fixture_stack(nfa, name, dt)
    sampling = name in cases.SAMPLING
    inverse = cases.density_is_inverse(name) != sampling
    x = torch.from_numpy(g["x"]).to(dt)
    with torch.no_grad():
        z, lds, counts = walk_with_counts(list(m.flows), x, inverse, sampling)
    assert z.dtype == dt and not z.requires_grad and not x.requires_grad
    assert_close(z.numpy(), g["z" + leg], what="z", **TOL[np.dtype(dtype)])
    ref = g["ld_layers" + leg]
    assert len(lds) == ref.shape[0]
    for i, l in enumerate(lds):
        assert_close(l.numpy(), ref[i], what="ld of layer %d" % i, **ld_tol(ref.dtype))
    if sampling:
        assert counts == g["iters" + leg].tolist()
    if any(not hasattr(f, "iresblock") for f in m.flows):
        return
    # through the container (stacks without ActNorm; the base density has kernels only): the chain router leaves a CPU model on the
    # torch route
    zz, ld = m.inverse_and_log_det(x) if inverse else m.forward_and_log_det(x)
    assert_close(zz.detach().numpy(), g["z" + leg], what="z (container)", **TOL[np.dtype(dtype)])
    assert_close(ld.detach().numpy().astype(ref.dtype), g["ld" + leg], what="ld (container)", **ld_tol(ref.dtype))


@pytest.mark.parametrize("dtype,leg", LEGS)
@pytest.mark.parametrize("name", list(cases.ESTIMATORS))
def test_estimators_reproduce_the_seeded_fixtures(nfa, name, dtype, leg):
    """Every stochastic branch in training mode, under the reference's seeds: the draws come in the reference's order (NumPy's
    truncation draw, then one torch.randn_like), so outputs, all gradients and the moment buffers are the reference's."""
    dt = getattr(torch, dtype)
    g = cases.load("est_" + name)
    seed = int(g["seed"])
    f = cases.estimator_layer(nfa, name, seed=seed)
    for k, v in f.state_dict().items():
        assert np.array_equal(v.numpy(), g["sd0__" + k.replace(".", "__")]), k
    f.load_state_dict({k: torch.from_numpy(v) for k, v in golden_state(g).items()}, strict=True)
    f = f.to(dt)
    x, cz, cl = (torch.from_numpy(g[k]).to(dt) for k in ("x", "cz", "cl"))
    xx = x.clone().requires_grad_(True)
    np.random.seed(seed)
    torch.manual_seed(seed)
    z, ld = f.inverse(xx)
    ((z * cz).sum() + (ld * cl).sum()).backward()
    assert ld.shape == (x.shape[0],)
    assert_close(z.detach().numpy(), g["z" + leg], what="z", **TOL[np.dtype(dtype)])
    assert_close(ld.detach().numpy(), g["ld" + leg], what="ld", **ld_tol(dtype))
    grads_close(xx.grad.numpy(), g["gx" + leg], "gx")
    n = 0
    for k, p in f.named_parameters():
        key = "g%s__%s" % (leg, k.replace(".", "__"))
        assert (p.grad is None) == (key not in g), k
        if p.grad is not None:
            grads_close(p.grad.numpy(), g[key], k)
            n += 1
    assert n >= 6
    blk = f.iresblock
    assert np.array_equal(blk.last_n_samples.numpy(), g["last_n_samples" + leg])
    assert_close(blk.last_firmom.numpy(), g["last_firmom" + leg], what="firmom", **ld_tol(dtype))
    assert_close(blk.last_secmom.numpy(), g["last_secmom" + leg], what="secmom", **ld_tol(dtype))


def test_power_iteration_reproduces_the_stored_buffers(nfa):
    g = cases.load("lipschitz")
    torch.manual_seed(int(g["seed"]))
    net = nfa.nets.LipschitzMLP([2, 40, 24, 2], init_zeros=True, lipschitz_const=cases.LIPSCHITZ)
    sd0 = golden_state(g, prefix="sd0__")
    assert list(net.state_dict()) == list(sd0)
    for k, v in net.state_dict().items():
        assert np.array_equal(v.numpy(), sd0[k]), k             # weight / 1000 in the last layer, 200 iterations at construction
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(3.0)
    nfa.utils.update_lipschitz(net, 5)

    def same(prefix):
        for k, v in net.state_dict().items():
            ref = golden_state(g, prefix=prefix)[k]
            if k.endswith((".u", ".v", ".scale")):
                assert_close(v.numpy(), ref, what=prefix + k, rtol=1e-6, atol=1e-7)
            else:
                assert np.array_equal(v.numpy(), ref), k

    same("after5__")
    one = [float(net.net[2 * i + 1].compute_one_iter()) for i in range(3)]
    assert_close(np.asarray(one), g["one_iter"], what="compute_one_iter", rtol=1e-6, atol=1e-7)
    same("after5__")                                              # compute_one_iter leaves the buffers alone
    with torch.no_grad():
        w = net.net[3].compute_weight(update=True, n_iterations=None, atol=1e-3, rtol=1e-3)
    assert_close(w.numpy(), g["tol_weight"], what="weight", rtol=1e-6, atol=1e-7)
    same("tol__")
    u_before = net.net[1].u.clone()
    with torch.no_grad():
        y = net(torch.from_numpy(g["x"]))
    assert_close(y.numpy(), g["y"], what="net(x)", **TOL[np.dtype("float32")])
    same("end__")                                                 # update=False: scale written, u / v untouched
    assert torch.equal(net.net[1].u, u_before)
    lin = net.net[1]
    with pytest.raises(ValueError, match="Need one of n_iteration"):
        nfa.nets.InducedNormLinear(2, 3).compute_weight(update=True)
    # the reference's quirk: a given rtol is replaced by atol, and with atol None the given rtol alone is no tolerance at all
    with pytest.raises(ValueError, match="Need one of n_iteration"):
        nfa.nets.InducedNormLinear(2, 3).compute_weight(update=True, n_iterations=None, atol=None, rtol=1e-3)
    assert float(lin.scale) > 0


def test_errors_exports_and_the_detached_outputs(nfa):
    with pytest.raises(NotImplementedError, match="2 -> 2"):
        nfa.nets.InducedNormLinear(2, 3, domain=1)
    with pytest.raises(NotImplementedError, match="2 -> 2"):
        nfa.nets.InducedNormLinear(2, 3, codomain=float("inf"))
    import normflows_amd.flows.residual
    import normflows_amd.nets.lipschitz
    import normflows_amd.utils.optim
    assert normflows_amd.flows.residual.Residual is nfa.flows.Residual
    assert normflows_amd.nets.lipschitz.LipschitzMLP is nfa.nets.LipschitzMLP
    assert normflows_amd.nets.lipschitz.InducedNormLinear is nfa.nets.InducedNormLinear
    assert normflows_amd.utils.optim.update_lipschitz is nfa.utils.update_lipschitz
    for name in ("set_requires_grad", "clear_grad", "update_lipschitz"):
        assert hasattr(nfa.utils, name)
    sw = nfa.nets.Swish()
    assert float(sw.beta.detach()) == 0.5 and sw.beta.shape == (1,)
    x = torch.linspace(-3, 3, 7)
    assert torch.allclose(sw(x), x * torch.sigmoid(x * torch.nn.functional.softplus(torch.tensor(0.5))) / 1.1)
    f = nfa.flows.Residual(nfa.nets.LipschitzMLP([2, 8, 2], init_zeros=False)).eval()
    x = torch.randn(5, 2)
    with torch.no_grad():
        z, ld = f.inverse(x)
    assert not z.requires_grad and not ld.requires_grad and not x.requires_grad      # the reference leaks a graph here
    z, ld = f.inverse(x)                                                               # with grad enabled the graph is kept
    assert z.requires_grad and ld.requires_grad and not x.requires_grad
    nfa.utils.set_requires_grad(f, False)
    assert not any(p.requires_grad for p in f.parameters())
    nfa.utils.set_requires_grad(f, True)
    z.sum().backward()
    assert f.iresblock.nnet.net[1].weight.grad is not None
    nfa.utils.clear_grad(f)
    assert all(p.grad is None for p in f.parameters())
    blk = f.iresblock
    assert abs(float(torch.sigmoid(blk.geom_p.detach())) - 0.5) < 1e-7 and float(blk.lamb.detach()) == 2.0 and blk.geom_p.dim() == 0
    assert "dist=geometric" in blk.extra_repr() and "coeff=0.97" in f.iresblock.nnet.net[1].extra_repr()


def test_switch_row_wise_and_eligibility(nfa):
    from normflows_amd import core
    from normflows_amd.flows import lipmlp_pack as lp
    assert isinstance(nfa.config.residual_chain, bool)
    before = nfa.config.residual_chain
    nfa.config.set_residual_chain(not before)
    try:
        assert nfa.config.residual_chain is (not before)
    finally:
        nfa.config.set_residual_chain(before)
    f = nfa.flows.Residual(nfa.nets.LipschitzMLP([2, 8, 2])).eval()
    assert core._row_wise(f)

    class Sub(nfa.flows.Residual):
        pass
    assert not core._row_wise(Sub(nfa.nets.LipschitzMLP([2, 8, 2])))
    assert lp.residual_ok(f) and not lp.residual_ok(Sub(nfa.nets.LipschitzMLP([2, 8, 2])).eval())
    assert not lp.eligible([f], torch.zeros(4, 2))                                  # a CPU tensor
    assert not lp.residual_ok(f.train())                                            # a stochastic branch
    assert lp.residual_ok(nfa.flows.Residual(nfa.nets.LipschitzMLP([2, 8, 2]), brute_force=True).train())
    for channels in ([2, 2], [2, 129, 2], [2, 8, 8, 8, 8, 2], [3, 8, 3]):
        assert lp.linears(nfa.nets.LipschitzMLP(channels)) is None, channels
    assert len(lp.linears(nfa.nets.LipschitzMLP([2, 128, 128, 128, 2]))) == 4
    assert lp.MAX_RECORDS == 32 and lp.HMAX == 128


# ---- the kernels' arithmetic, emulated, on the packed blob -------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.CHAIN))
def test_emulator_reproduces_the_chain_fixtures(nfa, name):
    from normflows_amd.flows import lipmlp_pack as lp
    m, g = fixture_stack(nfa, name)
    inverse = cases.density_is_inverse(name)
    run = list(reversed(m.flows)) if inverse else list(m.flows)
    scales = [mod.scale.clone() for mod in m.modules() if isinstance(mod, nfa.nets.InducedNormLinear)]
    for mod in m.modules():
        if isinstance(mod, nfa.nets.InducedNormLinear):
            mod.scale.zero_()
    blob, hp, nres = lp.pack(run, inverse)
    channels = cases.STACKS[name][0]
    assert hp == {32: 32, 40: 64, 64: 64, 128: 128}[max(channels[1:-1])] and nres == cases.STACKS[name][1]
    assert blob.numel() == len(run) * 16 + nres * lp.rstride(hp) and blob.dtype == torch.float32
    for mod, s in zip([mod for mod in m.modules() if isinstance(mod, nfa.nets.InducedNormLinear)], scales):
        assert abs(float(mod.scale) - float(s)) <= 1e-6 * abs(float(s))          # building the pack writes `scale`
    z, lds, total = emu.chain(blob.numpy(), len(run), hp, g["x"])
    assert_close(z, g["z"], what="z", **TOL[np.dtype("float32")])
    for i, l in enumerate(lds):
        assert_close(l, g["ld_layers"][i], what="ld of layer %d" % i, **ld_tol("float32"))
    assert_close(total, g["ld"], what="ld", **ld_tol("float32"))


@pytest.mark.parametrize("name", list(cases.SAMPLING))
def test_emulator_reproduces_the_sampling_fixtures(nfa, name):
    from normflows_amd.flows import lipmlp_pack as lp
    m, g = fixture_stack(nfa, name)
    x = g["x"]
    iters, k = [], 0
    for f in m.flows:                      # reverse=True: the model's forward pass is the fixed-point direction
        if isinstance(f, nfa.flows.Residual):
            blob, hp, _ = lp.pack([f], False)
            x, i = emu.fixed_point(blob.numpy(), hp, x)
            iters.append(i)
            _, lds, _ = emu.chain(blob.numpy(), 1, hp, x)
            assert_close(-lds[0], g["ld_layers"][k], what="ld of layer %d" % k, **ld_tol("float32"))
        else:
            x = layer_on_cpu(f, torch.from_numpy(x), False)[0].numpy()
        k += 1
    assert iters == g["iters"].tolist()
    assert_close(x, g["z"], what="z", **TOL[np.dtype("float32")])


def test_pack_follows_the_buffers(nfa):
    """The cache key holds u and v: update_lipschitz changes the effective weights without touching a parameter."""
    from normflows_amd.flows import lipmlp_pack as lp
    m, _ = fixture_stack(nfa, "h40x24_k2")
    run = list(reversed(m.flows))
    first = lp._cached_pack(run, True)
    assert lp._cached_pack(run, True) is first
    with torch.no_grad():
        m.flows[0].iresblock.nnet.net[1].weight.mul_(1.5)
    second = lp._cached_pack(run, True)
    assert second is not first
    nfa.utils.update_lipschitz(m, 5)
    third = lp._cached_pack(run, True)
    assert third is not second and not torch.equal(third[0], second[0])
    assert lp._cached_pack(run, True) is third
    nfa.invalidate_caches(m)
    assert lp._cached_pack(run, True) is not third


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_bound_and_validate_their_arguments(nfa):
    lib = nfa._lib.lib()
    syms = ("nf_lipmlp_width", "nf_lipmlp_rows", "nf_lipmlp_blob_floats", "nf_lipmlp_chain", "nf_lipmlp_apply")
    for sym in syms:
        assert sym in nfa._lib.exported_symbols_declared() and hasattr(lib, sym), sym
    assert "nf_lipmlp_blob_floats" in nfa._lib.int64_functions_declared()
    assert lib.nf_lipmlp_blob_floats.restype is ctypes.c_int64
    for name in ("lipmlp_chain", "lipmlp_apply", "lipmlp_width"):
        assert hasattr(nfa.ops, name)
    EINVAL, ENOTSUP, EFAULT, ERANGE = -22, -95, -14, -34
    assert [lib.nf_lipmlp_width(h) for h in (1, 32, 33, 64, 65, 128)] == [32, 32, 64, 64, 128, 128]
    assert lib.nf_lipmlp_width(0) == ENOTSUP and lib.nf_lipmlp_width(129) == ENOTSUP and nfa.ops.lipmlp_width(129) == 0
    assert [lib.nf_lipmlp_rows(h) for h in (32, 64, 128)] == [128, 64, 32] and lib.nf_lipmlp_rows(48) == ENOTSUP
    bf = lib.nf_lipmlp_blob_floats
    assert bf(1, 1, 32) == 16 + 2 * 32 * 32 + 7 * 32 + 4 and bf(32, 16, 128) == 32 * 16 + 16 * (2 * 128 * 128 + 7 * 128 + 4)
    assert bf(1, 1, 48) == ENOTSUP and bf(33, 1, 32) == ERANGE and bf(0, 0, 32) == EINVAL and bf(2, 3, 32) == EINVAL and bf(2, 0, 32) == EINVAL
    from normflows_amd.flows import lipmlp_pack as lp
    assert bf(5, 2, 64) == 5 * lp.HDR + 2 * lp.rstride(64)
    vp = ctypes.c_void_p
    null, ok = vp(0), vp(4096)

    def chain(B=8, hp=32, K=2, nres=1, acc=0, nblob=None, **p):
        a = dict(z=ok, y=ok, logdet=ok, blob=ok)
        a.update(p)
        nblob = K * 16 + nres * lp.rstride(hp) if nblob is None else nblob
        return lib.nf_lipmlp_chain(a["z"], a["y"], a["logdet"], a["blob"], nblob, B, hp, K, nres, acc, None)

    def apply(B=8, hp=32, mode=1, nblob=None, atol=1e-5, rtol=1e-5, **p):
        a = dict(x=ok, yin=ok, out=ok, count=ok, blob=ok)
        a.update(p)
        nblob = 16 + lp.rstride(hp) if nblob is None else nblob
        return lib.nf_lipmlp_apply(a["x"], a["yin"], a["out"], a["count"], a["blob"], nblob, B, hp, mode, atol, rtol, None)

    for call in (chain, apply):
        assert call(hp=48, nblob=100) == ENOTSUP and call(hp=256, nblob=100) == ENOTSUP
        assert call(B=-1) == EINVAL and call(nblob=17) == EINVAL and call(B=0) == 0
        assert call(blob=null) == EFAULT
    assert chain(K=33, nres=1) == ERANGE and chain(K=0, nres=0, nblob=0) == EINVAL and chain(K=2, nres=3) == EINVAL
    assert chain(K=2, nres=0) == EINVAL and chain(acc=2) == EINVAL and chain(acc=-2) == EINVAL
    assert chain(B=0, z=null, y=null, logdet=null, blob=null) == 0               # B == 0: no pointer is looked at
    assert apply(B=0, x=null, yin=null, out=null, count=null, blob=null) == 0
    for k in ("z", "y", "logdet"):
        assert chain(**{k: null}) == EFAULT, k
    for k in ("x", "yin", "out", "count"):
        assert apply(**{k: null}) == EFAULT, k
    assert apply(mode=2) == EINVAL and apply(atol=-1.0) == EINVAL and apply(atol=0.0, rtol=0.0) == EINVAL


def test_ops_refuse_bad_operands_before_any_launch(nfa, monkeypatch):
    from normflows_amd.flows import lipmlp_pack as lp
    called = []
    monkeypatch.setattr(nfa._lib, "call", lambda *a: called.append(a))
    monkeypatch.setattr(nfa._lib, "_require_device", lambda tensors: None)
    z, blob = torch.zeros(4, 2), torch.zeros(16 + lp.rstride(32))
    with pytest.raises(ValueError):
        nfa.ops.lipmlp_chain(torch.zeros(4, 3), blob, 1, 1, 32)                  # rows of 3
    with pytest.raises(ValueError):
        nfa.ops.lipmlp_chain(z, blob[:-1], 1, 1, 32)                             # a blob of the wrong size
    with pytest.raises(ValueError):
        nfa.ops.lipmlp_chain(z, blob, 2, 1, 32)                                  # ... for this K
    with pytest.raises(ValueError):
        nfa.ops.lipmlp_chain(z, blob, 1, 1, 32, logdet=torch.zeros(5), acc=1)    # logdet is not (B)
    with pytest.raises(TypeError):
        nfa.ops.lipmlp_chain(z.double(), blob, 1, 1, 32)
    with pytest.raises(TypeError):
        nfa.ops.lipmlp_chain(z, blob.double(), 1, 1, 32)
    with pytest.raises(NotImplementedError):
        nfa.ops.lipmlp_chain(z, blob, 1, 1, 48)
    with pytest.raises(ValueError):
        nfa.ops.lipmlp_apply(z, torch.zeros(5, 2), blob, 32, 1, torch.zeros(1, dtype=torch.int32))
    with pytest.raises(ValueError):
        nfa.ops.lipmlp_apply(z, z, blob, 32, 1, torch.zeros(1, dtype=torch.int64))
    with pytest.raises(ValueError):
        nfa.ops.lipmlp_apply(z, z, blob, 32, 1, None)
    with pytest.raises(ValueError):
        nfa.ops.lipmlp_apply(z, z, blob, 32, 2, torch.zeros(1, dtype=torch.int32))
    assert not called


def test_kernels_use_no_scratch(nfa):
    """Accumulators and epilogue temporaries stay in registers (every index into them is static): zero scratch bytes for every
    kernel of lipmlp.hip cross-compiled for gfx950."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    seen = 0
    for name, d in kr.resources(os.path.join(ROOT, "normalizing-flows_amd", "lib", "obj", "lipmlp.o")).items():
        if "lipmlp_" in name:
            seen += 1
            assert d["vgpr_spill_count"] == 0 and d["private_segment_fixed_size"] == 0 and d["vgpr_count"] <= 256, (name, d)
    assert seen == 12, seen     # chain and apply at three padded widths, 16-byte and 4-byte weight loads
