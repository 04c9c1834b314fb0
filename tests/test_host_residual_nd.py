"""CPU-side tests of the d-dimensional Residual route (flows/lipmlp_nd_pack.py, csrc/lipmlp_nd.hip, config.residual_nd): a NumPy
emulator of the kernels' arithmetic on the packed blob (tests/residual_nd_emulator.py) against the reference's fixtures
(tests/golden/residual_nd_*.npz), the switch and the eligibility table, the C ABI's argument checks, the run-cutting rules and the
order of the random draws with the launch stubbed out, and the kernels' code-object resources."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import residual_nd_cases as cases
import residual_nd_emulator as emu
from conftest import TOL, assert_close, golden_state, ld_tol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.dtype("float32")


@pytest.fixture(scope="module")
def nfa():
    import __graft_entry__
    import normflows_amd
    if not os.path.exists(normflows_amd.native_library_path()):
        __graft_entry__.build()
    return normflows_amd


@pytest.fixture
def nd_on(nfa):
    before = nfa.config.residual_nd
    nfa.config.set_residual_nd(True)
    yield nfa
    nfa.config.set_residual_nd(before)


def fixture_stack(nfa, name):
    g = cases.load(name)
    m = cases.stack(nfa, name)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in golden_state(g).items()}, strict=True)
    return m, g


def test_fixtures_carry_what_the_tests_need():
    for name in cases.STACKS:
        g = cases.load(name)
        nres = cases.STACKS[name][1]
        d = cases.dim(name)
        assert g["x"].shape == (cases.ROWS, d) and g["vareps"].shape == (nres, cases.ROWS, d) and g["vareps"].dtype == F32
        assert g["terms"].shape == (nres,) and g["n"].shape[0] == nres and g["coef"].shape == (nres, g["terms"].max())
        assert (g["terms"] == g["n"].max(1) + 20).all() and (g["terms"] <= 48).all()
        assert (g["coef"][:, :20] == 1.0).all()             # the always-included terms carry weight 1
        for leg in ("", "_f64"):
            assert g["z" + leg].shape == (cases.ROWS, d) and g["ld" + leg].shape == (cases.ROWS,)
            assert g["ld_layers" + leg].shape == (nres * (2 if cases.STACKS[name][2] else 1), cases.ROWS)
        assert 0 < float(g["ld_floor"]) < 1e-5
        if name in cases.SAMPLING:
            assert g["iters"].shape == (nres,) and (g["iters"] >= 1).all()
        path = os.path.join(cases.GOLDEN, "residual_nd_%s.npz" % name)
        assert os.path.getsize(path) < 700 * 1024


# ---- the kernels' arithmetic, emulated, on the packed blob -------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.DENSITY))
def test_emulator_reproduces_the_density_fixtures(nfa, name):
    from normflows_amd.flows import lipmlp_nd_pack as lp
    m, g = fixture_stack(nfa, name)
    inverse = cases.density_is_inverse(name)
    run = list(reversed(m.flows)) if inverse else list(m.flows)
    lins = [mod for mod in m.modules() if isinstance(mod, nfa.nets.InducedNormLinear)]
    scales = [mod.scale.clone() for mod in lins]
    for mod in lins:
        mod.scale.zero_()
    blob, hp, nres, d = lp.pack(run, inverse)
    channels = cases.STACKS[name][0]
    assert hp == {16: 32, 32: 32, 40: 64, 128: 128}[max(channels[1:-1])] and nres == cases.STACKS[name][1] and d == channels[0]
    assert blob.dtype == torch.float32 and blob.numel() == lp.blob_floats(len(run), nres, hp, d) == emu.blob_floats(len(run), nres, hp, d)
    assert blob.numel() == nfa._lib.lib().nf_lipmlp_nd_blob_floats(len(run), nres, hp, d)
    for mod, s in zip(lins, scales):
        assert abs(float(mod.scale) - float(s)) <= 1e-6 * abs(float(s))          # building the pack writes `scale`
    draws = cases.draws(g)
    z, lds = emu.chain(blob.numpy(), len(run), nres, hp, d, g["x"], [v for _, _, v in draws], [t for t, _, _ in draws],
                       [c for _, c, _ in draws])
    bar = cases.ld_bar(g, ld_tol("float32"))
    assert_close(z, g["z"], what="z", **TOL[F32])
    for i, l in enumerate(lds):
        assert_close(l, g["ld_layers"][i], what="ld of layer %d" % i, **bar)
    assert_close(np.sum(lds, axis=0, dtype=np.float32), g["ld"], what="ld", **bar)


@pytest.mark.parametrize("name", list(cases.SAMPLING))
def test_emulator_reproduces_the_sampling_fixtures(nfa, name):
    from normflows_amd.flows import lipmlp_nd_pack as lp
    m, g = fixture_stack(nfa, name)
    draws = cases.draws(g)
    x, iters = g["x"], []
    bar = cases.ld_bar(g, ld_tol("float32", root_finding=True))
    for k, f in enumerate(m.flows):             # reverse=True: the model's forward pass is the fixed-point direction
        blob, hp, _, d = lp.pack([f], False)
        x, i = emu.sample(blob.numpy(), hp, d, x)
        iters.append(i)
        t, c, v = draws[k]
        _, lds = emu.chain(blob.numpy(), 1, 1, hp, d, x, [v], [t], [c])
        assert_close(-lds[0], g["ld_layers"][k], what="ld of layer %d" % k, **bar)
    assert iters == g["iters"].tolist()
    assert_close(x, g["z"], what="z", **TOL[F32])


def test_pack_pads_with_zeros_and_follows_the_buffers(nfa):
    from normflows_amd.flows import lipmlp_nd_pack as lp
    m, _ = fixture_stack(nfa, "d5_h40x24_k2")
    run = list(reversed(m.flows))
    blob, hp, nres, d = lp.pack(run, True)
    K, dp = len(run), 8
    assert (hp, nres, d) == (64, 2, 5) and emu.dpad(5) == 8 and emu.dpad(64) == 64 and emu.dpad(3) == 4
    hdr = blob[:K * 16].view(K, 16).numpy()
    assert hdr[:, 0].tolist() == [2.0, 0.0, 2.0, 0.0] and hdr[:, 11].tolist() == [0.0, 0.0, 0.0, 1.0] and hdr[1, 1] == 1.0
    aff = blob[K * 16:K * 16 + K * 2 * dp].view(K, 2, dp).numpy()
    assert not aff[:, :, d:].any() and not aff[1].any() and aff[0, 0, :d].all()
    assert_close(hdr[0, 10], -float(run[0].s.detach().sum()), what="affine log-det", **TOL[F32])
    blk = emu.block(blob.numpy(), K, 1, hp, d)
    assert not blk["W0"][d:].any() and not blk["W0"][:, 40:].any() and not blk["W1"][40:].any() and not blk["W1"][:, 24:].any()
    assert not blk["W2"].any() and not blk["Wl"][24:].any() and not blk["Wl"][:, d:].any() and not blk["bl"][d:].any()
    first = lp._cached_pack(run, True)
    assert lp._cached_pack(run, True) is first
    nfa.utils.update_lipschitz(m, 5)
    second = lp._cached_pack(run, True)
    assert second is not first and not torch.equal(second[0], first[0])
    nfa.invalidate_caches(m)
    assert lp._cached_pack(run, True) is not second


# ---- the switch and the eligibility table ------------------------------------------------------------------------------------------
def test_switch_default_and_eligibility(nfa, monkeypatch):
    from normflows_amd.flows import lipmlp_nd_pack as lp
    from normflows_amd.flows import lipmlp_pack as lp2
    assert nfa.config.residual_nd is False                  # ships off
    Res, MLP = nfa.flows.Residual, nfa.nets.LipschitzMLP
    f = Res(MLP([3, 8, 3])).eval()
    monkeypatch.setattr(lp, "on_device", lambda z: torch.is_tensor(z) and z.dtype == torch.float32 and z.dim() == 2
                        and 3 <= z.shape[1] <= 64 and z.shape[0] > 0 and z.is_contiguous())
    z = torch.zeros(4, 3)
    with torch.no_grad():
        assert not lp.eligible([f], z)                      # off: declines
        nfa.config.set_residual_nd(True)
        try:
            assert lp.eligible([f], z)
            nfa.config.set_residual_chain(False)
            assert not lp.eligible([f], z)                  # residual_chain must be on as well
            nfa.config.set_residual_chain(True)
            assert not lp.eligible([f], torch.zeros(0, 3)) and not lp.eligible([f], torch.zeros(4, 4))
            assert not lp.eligible([f], z.double()) and not lp.eligible([f], torch.zeros(4, 6)[:, ::2])
            with nfa.config.higher_order_gradients():
                assert not lp.eligible([f], z)
            g = Res(MLP([3, 8, 3]), reverse=False).eval()
            assert not lp.eligible([f, g], z) and lp.eligible([f, f], z)
            assert lp.eligible([f] * 8, z) and not lp.eligible([f] * 9, z)
            a = nfa.flows.AffineConstFlow(3)
            assert lp.eligible([f] + [a] * 31, z) and not lp.eligible([f] + [a] * 32, z) and not lp.eligible([a], z)
            assert not lp.eligible([f, nfa.flows.AffineConstFlow(4)], z)
            with torch.enable_grad():
                assert not lp.eligible([f], z)              # a parameter needs a gradient
                for p in f.parameters():
                    p.requires_grad_(False)
                assert lp.eligible([f], z) and not lp.eligible([f], z.clone().requires_grad_(True))
        finally:
            nfa.config.set_residual_nd(False)
            nfa.config.set_residual_chain(True)
        assert not lp.eligible([f], z)

    class Sub(Res):
        pass
    assert lp.residual_ok(f) and not lp.residual_ok(Sub(MLP([3, 8, 3])).eval())
    assert not lp.residual_ok(Res(MLP([3, 8, 3])).train())                      # training keeps the formulas
    assert not lp.residual_ok(Res(MLP([3, 8, 3]), exact_trace=True).eval())
    for channels in ([2, 8, 2], [65, 8, 65], [3, 3], [3, 129, 3], [3, 8, 8, 8, 8, 3], [3, 8, 4]):
        assert lp.linears(MLP(channels)) is None, channels
    assert len(lp.linears(MLP([64, 128, 128, 128, 64]))) == 4 and len(lp.linears(MLP([3, 1, 3]))) == 2
    an = nfa.flows.ActNorm(3)
    assert not lp.member(an) and lp.member(nfa.flows.AffineConstFlow(3)) and not lp.member(nfa.flows.AffineConstFlow(2))
    # the 2-D predicates give what they gave
    assert lp2.linears(MLP([3, 8, 3])) is None and not lp2.residual_ok(f) and lp2.residual_ok(Res(MLP([2, 8, 2])).eval())
    assert not lp2.eligible([f], z)
    assert (lp.MAX_RECORDS, lp.MAX_RES, lp.MAX_TERMS, lp.DMIN, lp.DMAX) == (32, 8, 48, 3, 64)


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_bound_and_validate_their_arguments(nfa):
    from normflows_amd.flows import lipmlp_nd_pack as lp
    lib = nfa._lib.lib()
    for sym in ("nf_lipmlp_nd_rows", "nf_lipmlp_nd_blob_floats", "nf_lipmlp_nd_chain", "nf_lipmlp_nd_apply"):
        assert sym in nfa._lib.exported_symbols_declared() and hasattr(lib, sym), sym
    assert "nf_lipmlp_nd_blob_floats" in nfa._lib.int64_functions_declared()
    assert lib.nf_lipmlp_nd_blob_floats.restype is ctypes.c_int64
    for name in ("lipmlp_nd_chain", "lipmlp_nd_apply", "lipmlp_nd_rows"):
        assert hasattr(nfa.ops, name)
    EINVAL, ENOTSUP, EFAULT, ERANGE = -22, -95, -14, -34
    rows = lib.nf_lipmlp_nd_rows
    # 4096 / hp, halved until rows x (4 (hp + 4) + 4 (dp + 4)) floats fit 160 KiB
    assert [rows(32, d) for d in (3, 36, 40, 41, 64)] == [128, 128, 128, 64, 64]
    assert [rows(64, d) for d in (3, 64)] == [64, 64] and [rows(128, d) for d in (3, 64)] == [32, 32]
    for hp in (32, 64, 128):
        for d in range(3, 65):
            r = rows(hp, d)
            assert r % 4 == 0 and r <= 4096 // hp and 4 * r * (4 * (hp + 4) + 4 * (emu.dpad(d) + 4)) <= 160 * 1024
    assert rows(48, 8) == ENOTSUP and rows(32, 2) == ENOTSUP and rows(32, 65) == ENOTSUP and nfa.ops.lipmlp_nd_rows(128, 64) == 32
    bf = lib.nf_lipmlp_nd_blob_floats
    assert bf(1, 1, 32, 3) == 16 + 8 + 2 * 32 * 32 + 2 * 4 * 32 + 3 * 32 + 4
    assert bf(5, 2, 64, 17) == lp.blob_floats(5, 2, 64, 17) == 5 * 16 + 5 * 40 + 2 * lp.rstride(64, 17)
    assert bf(1, 1, 48, 8) == ENOTSUP and bf(1, 1, 32, 2) == ENOTSUP and bf(1, 1, 32, 65) == ENOTSUP
    assert bf(33, 1, 32, 8) == ERANGE and bf(9, 9, 32, 8) == ERANGE
    assert bf(0, 0, 32, 8) == EINVAL and bf(2, 3, 32, 8) == EINVAL and bf(2, 0, 32, 8) == EINVAL
    vp = ctypes.c_void_p
    null, ok = vp(0), vp(4096)

    def chain(B=8, d=8, hp=32, K=2, nres=1, acc=0, nblob=None, terms=None, **p):
        a = dict(z=ok, vareps=ok, y=ok, logdet=ok, blob=ok)
        a.update(p)
        nblob = lp.blob_floats(K, nres, hp, d) if nblob is None else nblob
        nt = (ctypes.c_int * 8)(*([21] * 8 if terms is None else terms))
        cf = (ctypes.c_float * (8 * 48))()
        return lib.nf_lipmlp_nd_chain(a["z"], a["vareps"], a["y"], a["logdet"], a["blob"], nblob, B, d, hp, K, nres,
                                      p.get("nterms", nt), p.get("coef", cf), acc, None)

    def apply(B=8, d=8, hp=32, mode=1, nblob=None, atol=1e-5, rtol=1e-5, **p):
        a = dict(x=ok, yin=ok, out=ok, count=ok, blob=ok)
        a.update(p)
        nblob = lp.blob_floats(1, 1, hp, d) if nblob is None else nblob
        return lib.nf_lipmlp_nd_apply(a["x"], a["yin"], a["out"], a["count"], a["blob"], nblob, B, d, hp, mode, atol, rtol, None)

    for call in (chain, apply):
        assert call(hp=48, nblob=100) == ENOTSUP and call(hp=256, nblob=100) == ENOTSUP
        assert call(d=2, nblob=100) == ENOTSUP and call(d=65, nblob=100) == ENOTSUP
        assert call(B=-1) == EINVAL and call(nblob=17) == EINVAL and call(B=0) == 0
        assert call(blob=null) == EFAULT
    assert chain(K=33, nres=1, nblob=1) == ERANGE and chain(K=9, nres=9, nblob=1) == ERANGE
    assert chain(K=0, nres=0, nblob=0) == EINVAL and chain(K=2, nres=3, nblob=1) == EINVAL and chain(K=2, nres=0, nblob=1) == EINVAL
    assert chain(acc=2) == EINVAL and chain(acc=-2) == EINVAL
    assert chain(terms=[49] + [21] * 7) == ERANGE and chain(terms=[0] + [21] * 7) == EINVAL and chain(terms=[48] + [21] * 7, B=0) == 0
    assert chain(K=2, nres=2, terms=[21, 49] + [21] * 6) == ERANGE and chain(K=2, nres=1, terms=[21, 49] + [21] * 6, B=0) == 0
    assert chain(nterms=null) == EFAULT and chain(coef=null) == EFAULT
    assert chain(B=0, z=null, vareps=null, y=null, logdet=null, blob=null) == 0        # B == 0: no device pointer is looked at
    assert apply(B=0, x=null, yin=null, out=null, count=null, blob=null) == 0
    for k in ("z", "vareps", "y", "logdet"):
        assert chain(**{k: null}) == EFAULT, k
    for k in ("x", "yin", "out", "count"):
        assert apply(**{k: null}) == EFAULT, k
    assert apply(mode=0, yin=null, count=null, B=0) == 0
    assert apply(mode=2) == EINVAL and apply(atol=-1.0) == EINVAL and apply(atol=0.0, rtol=0.0) == EINVAL


def test_ops_refuse_bad_operands_before_any_launch(nfa, monkeypatch):
    from normflows_amd.flows import lipmlp_nd_pack as lp
    called = []
    monkeypatch.setattr(nfa._lib, "call", lambda *a: called.append(a))
    monkeypatch.setattr(nfa._lib, "_require_device", lambda tensors: None)
    monkeypatch.setattr(nfa._lib, "stream", lambda: None)
    z, v, blob = torch.zeros(4, 5), torch.zeros(1, 4, 5), torch.zeros(lp.blob_floats(1, 1, 32, 5))
    coef = [[1.0] * 21]
    chain = nfa.ops.lipmlp_nd_chain
    chain(z, v, blob, 1, 1, 32, [21], coef)
    assert len(called) == 1 and called[0][0] == "nf_lipmlp_nd_chain"
    del called[:]
    with pytest.raises(NotImplementedError):
        chain(torch.zeros(4, 2), torch.zeros(1, 4, 2), blob, 1, 1, 32, [21], coef)          # rows of 2
    with pytest.raises(ValueError):
        chain(z, v, blob[:-1], 1, 1, 32, [21], coef)                                         # a blob of the wrong size
    with pytest.raises(ValueError):
        chain(z, v, blob, 2, 1, 32, [21], coef)                                              # ... for this K
    with pytest.raises(ValueError):
        chain(z, v[0], blob, 1, 1, 32, [21], coef)                                           # vareps is not (nres, B, d)
    with pytest.raises(ValueError):
        chain(z, v, blob, 1, 1, 32, [21], [[1.0] * 20])                                      # fewer coefficients than terms
    with pytest.raises(ValueError):
        chain(z, v, blob, 1, 1, 32, [21, 21], coef * 2)
    with pytest.raises(ValueError):
        chain(z, v, blob, 1, 1, 32, [21], coef, logdet=torch.zeros(5), acc=1)                # logdet is not (B)
    with pytest.raises(TypeError):
        chain(z.double(), v, blob, 1, 1, 32, [21], coef)
    with pytest.raises(NotImplementedError):
        chain(z, v, blob, 1, 1, 48, [21], coef)
    cnt = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(ValueError):
        nfa.ops.lipmlp_nd_apply(z, torch.zeros(5, 5), blob, 32, 1, cnt)
    with pytest.raises(ValueError):
        nfa.ops.lipmlp_nd_apply(z, z, blob, 32, 1, torch.zeros(1, dtype=torch.int64))
    with pytest.raises(ValueError):
        nfa.ops.lipmlp_nd_apply(z, z, blob, 32, 1, None)
    with pytest.raises(ValueError):
        nfa.ops.lipmlp_nd_apply(z, z, blob, 32, 2, cnt)
    assert not called


# ---- run cutting and the order of the draws, the launch stubbed out ----------------------------------------------------------------
@pytest.fixture
def stubbed(nd_on, monkeypatch):
    """The route on CPU tensors with the launch replaced by a recorder that returns its input and a zero log-det."""
    from normflows_amd.flows import lipmlp_nd_pack as lp
    launches = []
    monkeypatch.setattr(lp, "on_device", lambda z: torch.is_tensor(z) and z.dtype == torch.float32 and z.dim() == 2
                        and 3 <= z.shape[1] <= 64 and z.shape[0] > 0 and z.is_contiguous())

    def launch(run, z, vareps, terms, coefs, ld, acc, inverse):
        launches.append(dict(run=list(run), nres=vareps.shape[0], terms=list(terms), coefs=coefs, vareps=vareps.clone(), inverse=inverse))
        return z, (torch.zeros(z.shape[0]) if ld is None else ld)
    monkeypatch.setattr(lp, "_launch", launch)
    return nd_on, lp, launches


def layers(nfa, n, d=3, **kw):
    torch.manual_seed(5)
    out = [nfa.flows.Residual(nfa.nets.LipschitzMLP([d, 8, d], lipschitz_const=0.9), **kw).eval() for _ in range(n)]
    for f in out:
        for p in f.parameters():
            p.requires_grad_(False)
    return out


def test_runs_are_cut_at_8_residual_records_and_at_32_records(stubbed):
    nfa, lp, launches = stubbed
    from normflows_amd import core
    z = torch.zeros(4, 3)
    flows = layers(nfa, 9)
    order = list(range(8, -1, -1))
    assert core._residual_nd_run_end(flows, order, 0, z, True) == 8 and core._residual_nd_run_end(flows, order, 8, z, True) == 9
    assert core._residual_nd_run_end(flows, order, 0, z, False) == 0          # not their density direction
    ld = torch.zeros(4)
    with torch.no_grad():
        core.run_chain(flows, z, True, ld, 1)
    assert [len(c["run"]) for c in launches] == [8, 1] and [c["nres"] for c in launches] == [8, 1]
    assert launches[0]["run"] == flows[:0:-1] and launches[1]["run"] == flows[:1]
    aff = [nfa.flows.AffineConstFlow(3) for _ in range(40)]
    mixed = layers(nfa, 1) + aff
    order = list(range(41))
    with torch.no_grad():
        assert core._residual_nd_run_end(mixed, order, 0, z, False) == 0
        mixed[0].reverse = False
        assert core._residual_nd_run_end(mixed, order, 0, z, False) == 32         # 32 records
        assert core._residual_nd_run_end(mixed, order, 32, z, False) == 32        # affine layers alone are no run
        four = layers(nfa, 1, d=4)
        assert core._residual_nd_run_end(flows[:1] + four, [1, 0], 0, torch.zeros(4, 4), True) == 1   # another d ends the run
    assert core._residual_nd_run_end(mixed, order, 0, z, False) == 0              # the affine parameters need a gradient
    # a stretch of affine layers with no Residual in it is classified once, not once per position
    seen = []
    real = lp.classify
    lp.classify = lambda f: (seen.append(f), real(f))[1]
    try:
        stretch = aff[:10] + [torch.nn.Identity()] + layers(nfa, 1)
        order, state = list(range(12)), {}
        with torch.no_grad():
            ends = [core._residual_nd_run_end(stretch, order, k, z, True, state) for k in range(12)]
    finally:
        lp.classify = real
    assert ends == list(range(11)) + [12] and state["skip"] == 10
    assert len(seen) == 11 + 1 + 1                       # ten affine layers and the Identity once, the Identity again at its own position, the Residual
    nfa.config.set_residual_nd(False)
    assert not lp.eligible(flows[:1], z)


def run_formulas(flows, z):
    ld = torch.zeros(z.shape[0])
    for f in flows:
        z, l = f._torch_pass(z, True)
        ld = ld + l
    return z, ld


def test_a_49_term_draw_cuts_the_run_and_both_generators_end_where_the_formulas_leave_them(stubbed, monkeypatch):
    nfa, lp, launches = stubbed
    from normflows_amd.flows import residual
    flows = layers(nfa, 4)
    z = torch.randn(6, 3, generator=torch.Generator().manual_seed(1))
    real = residual.geometric_sample
    calls = []

    def forced(p, n_samples):
        n = real(p, n_samples)
        calls.append(1)
        return np.full_like(n, 29) if len(calls) % 4 == 2 else n       # the second layer of every pass draws 29: 49 terms
    monkeypatch.setattr(residual, "geometric_sample", forced)
    passes = []
    orig = nfa.flows.Residual._torch_pass

    def spy(self, zz, density, truncation=None):
        passes.append((self, truncation))
        return orig(self, zz, density, truncation)
    with torch.no_grad():
        np.random.seed(3)
        torch.manual_seed(3)
        z_ref, ld_ref = run_formulas(flows, z)
        after_ref = (np.random.rand(), float(torch.rand(1)))
        monkeypatch.setattr(nfa.flows.Residual, "_torch_pass", spy)
        np.random.seed(3)
        torch.manual_seed(3)
        _, ld = lp.run_density(flows, z, None, None)
        after = (np.random.rand(), float(torch.rand(1)))
    assert after == after_ref
    assert [len(c["run"]) for c in launches] == [1, 2] and launches[0]["run"] == flows[:1] and launches[1]["run"] == flows[2:]
    assert len(passes) == 1 and passes[0][0] is flows[1] and passes[0][1][0] == 49 and passes[0][1][2].tolist() == [29]
    assert all(1 <= t <= 48 for c in launches for t in c["terms"]) and all(len(co) == t for c in launches for co, t in zip(c["coefs"], c["terms"]))
    # the same noise, in the same order, as the formulas draw: replay the torch stream by hand
    torch.manual_seed(3)
    want = [torch.randn_like(z) for _ in range(4)]
    assert torch.equal(launches[0]["vareps"][0], want[0])
    assert torch.equal(launches[1]["vareps"][0], want[2]) and torch.equal(launches[1]["vareps"][1], want[3])
    assert ld.shape == (6,)

    # without a long draw: one launch, every truncation first, then every vareps
    del launches[:]
    monkeypatch.setattr(residual, "geometric_sample", real)
    monkeypatch.setattr(nfa.flows.Residual, "_torch_pass", orig)
    with torch.no_grad():
        np.random.seed(4)
        torch.manual_seed(4)
        run_formulas(flows, z)
        after_ref = (np.random.rand(), float(torch.rand(1)))
        np.random.seed(4)
        torch.manual_seed(4)
        lp.run_density(flows, z, None, None)
        after = (np.random.rand(), float(torch.rand(1)))
        np.random.seed(4)
        terms = [f.iresblock._truncation()[0] for f in flows]
    assert after == after_ref and len(launches) == 1 and launches[0]["terms"] == terms


def test_explicit_noise_entry_draws_nothing(stubbed):
    nfa, lp, launches = stubbed
    f = layers(nfa, 1, d=5)[0]
    z, v = torch.zeros(4, 5), torch.ones(4, 5)
    np.random.seed(8)
    torch.manual_seed(8)
    want = (np.random.rand(), float(torch.rand(1)))
    np.random.seed(8)
    torch.manual_seed(8)
    with torch.no_grad():
        f._density_nd(z, v, 21, [1.0] * 21)
    assert (np.random.rand(), float(torch.rand(1))) == want
    assert len(launches) == 1 and launches[0]["terms"] == [21] and launches[0]["vareps"].shape == (1, 4, 5)
    nfa.config.set_residual_nd(False)
    with pytest.raises(NotImplementedError), torch.no_grad():
        f._density_nd(z, v, 21, [1.0] * 21)


# ---- the code objects ---------------------------------------------------------------------------------------------------------------
def test_kernels_use_no_scratch(nfa):
    """Accumulators, epilogue temporaries and the weight-block pointers stay in registers, the series coefficients in the launch
    arguments: zero scratch bytes for every kernel of lipmlp_nd.hip cross-compiled for gfx950."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    seen = 0
    for name, d in kr.resources(os.path.join(ROOT, "normalizing-flows_amd", "lib", "obj", "lipmlp_nd.o")).items():
        if "lipmlp_nd_" in name:
            seen += 1
            assert d["vgpr_spill_count"] == 0 and d["private_segment_fixed_size"] == 0 and d["vgpr_count"] <= 256, (name, d)
    assert seen == 12, seen     # chain and apply at three padded widths, 16-byte and 4-byte weight loads
