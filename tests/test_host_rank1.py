"""CPU-side tests of the Planar / Radial flows and their rank-1 chain route (flows/planar.py, flows/radial.py, flows/rank1_pack.py,
csrc/rank1_chain.hip): the classes against the reference's fixtures (tests/golden/rank1_*.npz: state dicts, seeded construction,
both precisions of the torch-formula route, the errors), the record layout, a float32 NumPy emulator of the kernels' arithmetic
(tests/rank1_emulator.py) against the same fixtures, the C ABI's argument checks and the kernels' code-object resources."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

import rank1_cases as cases
import rank1_emulator as emu
from conftest import TOL, assert_close, golden_state, ld_tol, load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = [("float32", ""), ("float64", "_f64")]


@pytest.fixture(scope="module")
def nfa():
    import __graft_entry__
    import normflows_amd
    if not os.path.exists(normflows_amd.native_library_path()):
        __graft_entry__.build()
    return normflows_amd


def fixture_model(nfa, name, dtype=torch.float32):
    g = load_golden("rank1_" + name)
    m = cases.model(nfa, name)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in golden_state(g).items()}, strict=True)
    return m.to(dtype), g


def grads_close(got, ref, what, rel=3e-3):
    """test_gpu_training._check_grads' rule (error < rel * max(1e-3, max |ref|) + 1e-5) on the finite entries; NaN where and only
    where the reference has NaN."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (what, got, ref)
    fin = ~np.isnan(ref)
    if fin.any():
        scale = max(1e-3, float(np.abs(ref[fin]).max()))
        err = float(np.abs(got[fin] - ref[fin]).max())
        assert err < rel * scale + 1e-5, (what, err, scale)


def step(flows, x, cz, cl, inverse, runner):
    for f in flows:
        f.zero_grad(set_to_none=True)
    xx = x.clone().requires_grad_(True)
    z, ld = runner(xx, inverse)
    ((z * cz).sum() + (ld * cl).sum()).backward()
    return z.detach(), ld.detach(), xx.grad


# ---- the classes against the reference ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.CASES))
def test_state_dicts_load_both_ways_and_seeded_construction_is_bit_identical(nfa, name):
    g = load_golden("rank1_" + name)
    ref_sd = golden_state(g)
    m = cases.model(nfa, name)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in ref_sd.items()}, strict=True)
    ours = m.state_dict()
    assert list(ours) == list(ref_sd)
    for k, v in ours.items():
        assert tuple(v.shape) == ref_sd[k].shape and np.array_equal(v.numpy(), ref_sd[k]), k
    codes, shape, _ = cases.CASES[name]
    for f, c in zip(m.flows, codes):
        if c == "R":
            assert f.beta.shape == f.alpha.shape == (1,) and f.z_0.shape == (1,) + shape and int(f.d) == math.prod(shape)
        else:
            assert f.u.shape == f.w.shape == (1,) + shape and f.b.shape == (1,)
    seeded = cases.model(nfa, name, seed=int(g["seed"])).state_dict()
    ref0 = golden_state(g, prefix="sd0__")
    assert list(seeded) == list(ref0)
    for k, v in seeded.items():
        assert v.numpy().dtype == ref0[k].dtype and np.array_equal(v.numpy(), ref0[k]), k


@pytest.mark.parametrize("dtype,leg", LEGS)
@pytest.mark.parametrize("name", list(cases.CASES))
def test_torch_route_reproduces_the_fixtures_on_the_cpu(nfa, name, dtype, leg):
    dt = getattr(torch, dtype)
    m, g = fixture_model(nfa, name, dt)
    x, cz, cl = (torch.from_numpy(g[k]).to(dt) for k in ("x", "cz", "cl"))
    for dname in cases.directions(name):
        z, ld, gx = step(list(m.flows), x, cz, cl, dname == "inv",
                         lambda xx, inv: m.inverse_and_log_det(xx) if inv else m.forward_and_log_det(xx))
        assert z.dtype == dt and ld.dtype == dt
        assert_close(z.numpy(), g["z_%s%s" % (dname, leg)], what="z", **TOL[np.dtype(dtype)])
        # (the reference's leaky h' is a float32 tensor whatever the model's dtype -- (x < 0) * (slope - 1.0) + 1.0, planar.py:60 --
        # and a 0-dim float64 factor does not promote it: an all-leaky model's forward float64 leg has a float32 log-det, held at
        # that bar)
        ref_ld = g["ld_%s%s" % (dname, leg)]
        assert_close(ld.numpy(), ref_ld, what="ld", **ld_tol(ref_ld.dtype))
        grads_close(gx.numpy(), g["gx_%s%s" % (dname, leg)], "gx")
        n = 0
        for k, p in m.flows.named_parameters():
            grads_close(p.grad.numpy(), g["g_%s%s__%s" % (dname, leg, k.replace(".", "__"))], k)
            n += 1
        assert n == 3 * len(m.flows)


@pytest.mark.parametrize("dtype,leg", LEGS)
def test_torch_route_reproduces_the_edge_fixture(nfa, dtype, leg):
    """|lin| = 0 .. 95 through one tanh layer (float32: the reference's cosh overflows at 95 and its gradients are NaN, exactly as
    stored) and lin == 0 through one leaky layer (the slope-1 side), both directions of the latter."""
    dt = getattr(torch, dtype)
    g = load_golden("rank1_planar_edges")
    for key, (layer, x) in cases.edge_layers(nfa, dt).items():
        cz, cl = (torch.from_numpy(g["%s__%s" % (key, k)]).to(dt) for k in ("cz", "cl"))
        for dname in (("fwd", "inv") if key == "leaky" else ("fwd",)):
            z, ld, gx = step([layer], x, cz, cl, dname == "inv", lambda xx, inv: layer.inverse(xx) if inv else layer(xx))
            assert_close(z.numpy(), g["%s__z_%s%s" % (key, dname, leg)], what="z", **TOL[np.dtype(dtype)])
            ref_ld = g["%s__ld_%s%s" % (key, dname, leg)]
            assert ld.numpy().dtype == ref_ld.dtype         # (float32 from the leaky layer's forward in either leg: see above)
            assert (ref_ld.dtype == np.float32) == (dtype == "float32" or (key, dname) == ("leaky", "fwd"))
            assert_close(ld.numpy(), ref_ld, what="ld", **ld_tol(ref_ld.dtype))
            grads_close(gx.numpy(), g["%s__gx_%s%s" % (key, dname, leg)], "gx")
            for k, p in layer.named_parameters():
                grads_close(p.grad.numpy(), g["%s__g_%s%s__0__%s" % (key, dname, leg, k)], k)
    assert np.isnan(g["tanh__gx_fwd"]).any() and np.isfinite(g["tanh__gx_fwd_f64"]).all()


def test_errors(nfa):
    P, R = nfa.flows.Planar, nfa.flows.Radial
    with pytest.raises(NotImplementedError, match="Nonlinearity is not implemented."):
        P((2,), act="relu")
    with pytest.raises(NotImplementedError, match="This flow has no algebraic inverse."):
        P((2,)).inverse(torch.zeros(3, 2))
    with pytest.raises(NotImplementedError, match="This flow has no algebraic inverse."):
        R((2,)).inverse(torch.zeros(3, 2))
    assert "inverse" not in R.__dict__
    m = nfa.NormalizingFlow(nfa.distributions.DiagGaussian(2), [P((2,), act="leaky_relu"), P((2,))])
    with pytest.raises(NotImplementedError, match="This flow has no algebraic inverse."):
        m.inverse_and_log_det(torch.zeros(3, 2))
    z, ld = P((2,), act="leaky_relu").inverse(torch.zeros(3, 2))
    assert z.shape == (3, 2) and ld.shape == (3,)
    import normflows_amd.flows.planar
    import normflows_amd.flows.radial
    assert normflows_amd.flows.planar.Planar is P and normflows_amd.flows.radial.Radial is R


def test_switch_and_row_wise(nfa):
    from normflows_amd import core
    assert nfa.config.rank1_chain is True
    nfa.config.set_rank1_chain(False)
    try:
        assert nfa.config.rank1_chain is False
    finally:
        nfa.config.set_rank1_chain(True)
    assert core._row_wise(nfa.flows.Planar((2,))) and core._row_wise(nfa.flows.Radial((2,)))

    class Sub(nfa.flows.Planar):
        pass
    assert not core._row_wise(Sub((2,)))
    from normflows_amd.flows import rank1_pack
    assert not rank1_pack.eligible([nfa.flows.Planar((2,))], torch.zeros(4, 2), False)        # a CPU tensor


# ---- the records ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed_d17_k6", "planar_leaky_d3_k4", "radial_d2_k8", "planar_shape_1x4x4"])
def test_pack_layout_and_stacked_equals_layer_by_layer(nfa, name):
    from normflows_amd.flows import rank1_pack as rp
    m, _ = fixture_model(nfa, name)
    run = list(m.flows)
    d = math.prod(cases.CASES[name][1])
    P = rp.pack(run, d, "cpu")
    assert P.shape == (len(run), 2 * d + 4) and P.dtype == torch.float32 and P.is_contiguous() and P.requires_grad
    assert rp.kinds(run) == tuple({"P": 0, "L": 1, "R": 2}[c] for c in cases.CASES[name][0])
    single = torch.cat([rp.pack([f], d, "cpu") for f in run])
    assert torch.equal(P.detach(), single.detach())                       # row-wise arithmetic: the same bits
    for row, f, kind in zip(P.detach(), run, rp.kinds(run)):
        assert float(row[0]) == kind
        if kind == 2:
            beta = torch.log(1 + torch.exp(f.beta)) - torch.abs(f.alpha)
            assert float(row[1]) == float(f.alpha.abs()) and float(row[2]) == float(beta) and float(row[3]) == d - 1
            assert torch.equal(row[4:4 + d], f.z_0.detach().reshape(-1)) and not row[4 + d:].any()
        else:
            u_hat = f._u_hat().detach().reshape(-1)
            assert float(row[1]) == float(f.b) and float(row[3]) == np.float32(0.2)
            assert torch.equal(row[4:4 + d], f.w.detach().reshape(-1))
            assert torch.allclose(row[4 + d:], u_hat, rtol=1e-6, atol=1e-7)
            assert abs(float(row[2]) - float((f.w.detach().reshape(-1) * u_hat).sum())) < 1e-6
            assert float(row[2]) > -1.0                                   # the constraint the formula enforces
    assert rp.MAX_RECORDS == 64 and rp.DMAX == 128


# ---- the kernels' arithmetic, emulated ---------------------------------------------------------------------------------------------
def emulated_step(nfa, run, x, cz, cl, inverse):
    """One training step as the GPU route runs it: P from the live parameters, the emulated forward with its saved scalars, the
    emulated backward from the OUTPUT, gP through torch's autograd to the leaves."""
    from normflows_amd.flows import rank1_pack as rp
    for f in run:
        f.zero_grad(set_to_none=True)
    B, d = x.shape[0], math.prod(x.shape[1:])
    P = rp.pack(run, d, "cpu")
    direction = 1 if inverse else 0
    y, ld, save = emu.forward(P.detach().numpy(), x.reshape(B, d).numpy(), direction)
    gz, gP = emu.backward(P.detach().numpy(), y, save, cz.reshape(B, d).numpy(), cl.numpy(), direction)
    P.backward(torch.from_numpy(gP))
    return y.reshape(x.shape), ld, gz.reshape(x.shape)


@pytest.mark.parametrize("name", list(cases.CASES))
def test_emulator_reproduces_the_fixtures(nfa, name):
    m, g = fixture_model(nfa, name)
    x, cz, cl = (torch.from_numpy(g[k]) for k in ("x", "cz", "cl"))
    for dname in cases.directions(name):
        z, ld, gx = emulated_step(nfa, list(m.flows), x, cz, cl, dname == "inv")
        assert_close(z, g["z_" + dname], what="z", **TOL[np.dtype("float32")])
        assert_close(ld, g["ld_" + dname], what="ld", **ld_tol("float32"))
        grads_close(gx, g["gx_" + dname], "gx")
        for k, p in m.flows.named_parameters():
            grads_close(p.grad.numpy(), g["g_%s__%s" % (dname, k.replace(".", "__"))], k)
    if name == "radial_d2_k8":      # r == 0 in row 0 of the first record: saved as exactly 0, and the backward stays finite
        from normflows_amd.flows import rank1_pack as rp
        P = rp.pack(list(m.flows), 2, "cpu").detach().numpy()
        assert emu.forward(P, x.numpy())[2][0, 0] == 0.0 and np.isfinite(gx).all()


def test_emulator_on_the_edge_fixture(nfa):
    """The kernels' sech^2 goes to 0 without an overflow: finite gradients at |lin| = 95, where the reference's float32 leg is NaN --
    compared with the reference's float64 leg there; z and log-det with the float32 leg."""
    g = load_golden("rank1_planar_edges")
    for key, (layer, x) in cases.edge_layers(nfa).items():
        cz, cl = (torch.from_numpy(g["%s__%s" % (key, k)]) for k in ("cz", "cl"))
        for dname in (("fwd", "inv") if key == "leaky" else ("fwd",)):
            z, ld, gx = emulated_step(nfa, [layer], x, cz, cl, dname == "inv")
            assert_close(z, g["%s__z_%s" % (key, dname)], what="z", **TOL[np.dtype("float32")])
            assert_close(ld, g["%s__ld_%s" % (key, dname)], what="ld", **ld_tol("float32"))
            leg = "_f64" if key == "tanh" else ""
            assert np.isfinite(gx).all()
            grads_close(gx, g["%s__gx_%s%s" % (key, dname, leg)], "gx")
            for k, p in layer.named_parameters():
                assert torch.isfinite(p.grad).all()
                grads_close(p.grad.numpy(), g["%s__g_%s%s__0__%s" % (key, dname, leg, k)], k)
    assert float(g["tanh__ld_fwd"][5]) == 0.0      # sech^2(95) is 0 in the reference's float32 as well


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_bound_and_validate_their_arguments(nfa):
    lib = nfa._lib.lib()
    syms = ("nf_rank1_rows", "nf_rank1_train_scratch_floats", "nf_rank1_chain", "nf_rank1_chain_train_fwd", "nf_rank1_chain_bwd")
    for sym in syms:
        assert sym in nfa._lib.exported_symbols_declared() and hasattr(lib, sym), sym
    assert "nf_rank1_train_scratch_floats" in nfa._lib.int64_functions_declared()
    assert lib.nf_rank1_train_scratch_floats.restype is ctypes.c_int64
    for name in ("rank1_chain", "rank1_chain_train_fwd", "rank1_chain_bwd", "rank1_rows"):
        assert hasattr(nfa.ops, name)
    assert hasattr(nfa.autograd, "Rank1ChainFn")
    EINVAL, ENOTSUP, EFAULT, ERANGE = -22, -95, -14, -34
    assert lib.nf_rank1_rows(1) == 256 and lib.nf_rank1_rows(16) == 256 and lib.nf_rank1_rows(17) == 16 and lib.nf_rank1_rows(128) == 16
    assert lib.nf_rank1_rows(129) == ENOTSUP and lib.nf_rank1_rows(0) == ENOTSUP
    assert nfa.ops.rank1_rows(16) == 256 and nfa.ops.rank1_rows(129) == 0
    wg = lib.nf_persistent_workgroups()
    sf = lib.nf_rank1_train_scratch_floats
    assert sf(1024, 2, 32) == 4 * 4 * 32 * 8 and sf(10 ** 6, 2, 32) == wg * 4 * 32 * 8      # one slab per wave of 4 per workgroup
    assert sf(35, 128, 4) == 3 * 4 * 4 * 260 and sf(10 ** 6, 128, 64) <= 1 << 24            # the 64 MiB bound lowers the grid
    assert sf(8, 129, 4) == ENOTSUP and sf(8, 2, 65) == ERANGE and sf(-1, 2, 4) == EINVAL and sf(8, 2, 0) == EINVAL
    vp = ctypes.c_void_p
    null, ok = vp(0), vp(4096)

    def inf(B=8, d=2, K=4, direction=0, acc=0, **p):
        a = dict(z=ok, y=ok, logdet=ok, P=ok)
        a.update(p)
        return lib.nf_rank1_chain(a["z"], a["y"], a["logdet"], a["P"], B, d, K, direction, acc, None)

    def fwd(B=8, d=2, K=4, direction=0, **p):
        a = dict(z=ok, y=ok, logdet=ok, save=ok, P=ok)
        a.update(p)
        return lib.nf_rank1_chain_train_fwd(a["z"], a["y"], a["logdet"], a["save"], a["P"], B, d, K, direction, None)

    def bwd(B=8, d=2, K=4, direction=0, need_gP=1, **p):
        a = dict(y=ok, save=ok, gy=ok, gld=ok, gz=ok, P=ok, slabs=ok, gP=ok)
        a.update(p)
        return lib.nf_rank1_chain_bwd(a["y"], a["save"], a["gy"], a["gld"], a["gz"], a["P"], a["slabs"], a["gP"], B, d, K, direction,
                                      need_gP, None)

    for call in (inf, fwd, bwd):
        assert call(d=0) == ENOTSUP and call(d=129) == ENOTSUP
        assert call(K=65) == ERANGE and call(K=0) == EINVAL and call(B=-1) == EINVAL and call(direction=2) == EINVAL
        assert call(B=0) == 0
    assert inf(B=0, z=null, y=null, logdet=null, P=null) == 0                 # B == 0: no pointer is looked at
    assert fwd(B=0, z=null, y=null, logdet=null, save=null, P=null) == 0
    assert bwd(B=0, y=null, save=null, P=null, slabs=null, gP=null) == 0
    assert inf(acc=2) == EINVAL and inf(acc=-2) == EINVAL
    for k in ("z", "y", "logdet", "P"):
        assert inf(**{k: null}) == EFAULT, k
    for k in ("z", "y", "logdet", "save", "P"):
        assert fwd(**{k: null}) == EFAULT, k
    for k in ("y", "save", "P", "slabs", "gP"):
        assert bwd(**{k: null}) == EFAULT, k
    assert bwd(need_gP=0, gz=null, slabs=null, gP=null) == 0                  # nothing asked for: nothing launched


def test_ops_refuse_bad_operands_before_any_launch(nfa, monkeypatch):
    """Direction 1 over a tanh or Radial record is refused on the host (P lives in device memory: the C side cannot look), as are
    operands of the wrong size; nothing reaches the library."""
    called = []
    monkeypatch.setattr(nfa._lib, "call", lambda *a: called.append(a))
    monkeypatch.setattr(nfa._lib, "_require_device", lambda tensors: None)
    z, P = torch.zeros(4, 2), torch.zeros(3, 8)
    with pytest.raises(ValueError, match="kind 1"):
        nfa.ops.rank1_chain(z, P, (1, 0, 1), 1)
    with pytest.raises(ValueError, match="kind 1"):
        nfa.ops.rank1_chain_train_fwd(z, P, (1, 2, 1), 1)
    with pytest.raises(ValueError):
        nfa.ops.rank1_chain(z, torch.zeros(3, 9), (1, 1, 1), 0)             # P is not (K, 2 d + 4)
    with pytest.raises(ValueError):
        nfa.ops.rank1_chain(z, P, (1, 1), 0)                                # two kinds for three records
    with pytest.raises(TypeError):
        nfa.ops.rank1_chain(z.double(), P, (1, 1, 1), 0)
    with pytest.raises(ValueError):
        nfa.ops.rank1_chain_bwd(z, torch.zeros(2, 4), None, None, P, (1, 1, 1), 0, True, True)      # save is not (K, B)
    assert not called


def test_kernels_use_no_scratch(nfa):
    """Rows, cotangents and the per-record temporaries stay in registers (every index into them is static): zero scratch bytes for
    every kernel of rank1_chain.hip cross-compiled for gfx950."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    seen = 0
    for name, d in kr.resources(os.path.join(ROOT, "normalizing-flows_amd", "lib", "obj", "rank1_chain.o")).items():
        if "rank1_" in name:
            seen += 1
            assert d["vgpr_spill_count"] == 0 and d["private_segment_fixed_size"] == 0 and d["vgpr_count"] <= 256, (name, d)
    assert seen == 5, seen      # forward and backward in two row layouts, the slab reduction
