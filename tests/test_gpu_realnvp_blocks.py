"""GPU tests of the coupling block record of the RealNVP chain kernels: AffineCouplingBlock(nets.MLP) layers with the Permute
behind them as records of nf_realnvp_chain (inference) and of RealNVPChainFn (one forward, one backward launch under autograd) --
against the reference's autograd (tests/golden/grad_realnvp_block_*.npz), against the layer-by-layer route
(config.set_realnvp_blocks(False)), and the record's own contracts (the 32-record cut, the persistent loop, determinism, frozen
parameters, live parameters and permutations, capture, views, what stays outside)."""
import contextlib

import numpy as np
import pytest
import torch

import realnvp_block_cases as cases
import realnvp_block_emulator as emu
from conftest import assert_close, golden_state, ld_tol
from test_gpu_realnvp_train import DEV, N, T, _captured_step, assert_grads_of_scale, of_scale, step
from test_gpu_training import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nfa():
    import normflows_amd
    assert torch.cuda.is_available()
    return normflows_amd


@pytest.fixture
def calls(nfa, monkeypatch):
    """Counts of the chain ops' calls and of what the layer-by-layer route runs instead; "runs" / "iruns" = the list indices of every
    fused run under autograd / at inference (calls["flows"] must hold the model's flow list), "masks" = every backward's wmask."""
    n = {"fwd": 0, "bwd": 0, "chain": 0, "acf": 0, "ac": 0, "maf": 0, "lin": 0, "runs": [], "iruns": [], "masks": [], "flows": None}

    def counted(key, fn):
        def wrapper(*a, **k):
            n[key] += 1
            return fn(*a, **k)
        return wrapper

    def run_spy(key, fn):
        def wrapper(run, *a, **k):
            if n["flows"] is not None:
                n[key].append([[i for i, g in enumerate(n["flows"]) if g is f][0] for f in run])
            return fn(run, *a, **k)
        return wrapper
    real_bwd = nfa.ops.realnvp_chain_bwd

    def bwd_spy(*a, **k):
        n["bwd"] += 1
        n["masks"].append(a[8])
        return real_bwd(*a, **k)
    monkeypatch.setattr(nfa.ops, "realnvp_chain_train_fwd", counted("fwd", nfa.ops.realnvp_chain_train_fwd))
    monkeypatch.setattr(nfa.ops, "realnvp_chain_bwd", bwd_spy)
    monkeypatch.setattr(nfa.ops, "realnvp_chain", counted("chain", nfa.ops.realnvp_chain))
    monkeypatch.setattr(nfa.ops, "affine_coupling", counted("ac", nfa.ops.affine_coupling))
    monkeypatch.setattr(nfa.autograd.AffineCouplingFn, "apply", counted("acf", nfa.autograd.AffineCouplingFn.apply))
    monkeypatch.setattr(nfa.autograd.MaskedAffineFn, "apply", counted("maf", nfa.autograd.MaskedAffineFn.apply))
    monkeypatch.setattr(torch.nn.Linear, "forward", counted("lin", torch.nn.Linear.forward))
    monkeypatch.setattr(nfa.core, "_run_realnvp_train", run_spy("runs", nfa.core._run_realnvp_train))
    monkeypatch.setattr(nfa.core, "_run_realnvp", run_spy("iruns", nfa.core._run_realnvp))
    return n


def counts(calls, *keys):
    return tuple(calls[k] for k in keys)


@pytest.fixture
def layerwise(nfa):
    """Context manager factory: the record kind switched off (and, with train=True, the training route of the other kinds too)."""
    @contextlib.contextmanager
    def off(train=True):
        nfa.config.set_realnvp_blocks(False)
        if train:
            nfa.config.set_realnvp_train(False)
        try:
            yield
        finally:
            nfa.config.set_realnvp_blocks(True)
            nfa.config.set_realnvp_train(True)
    return off


def fixture_model(nfa, name):
    g = load_golden("grad_realnvp_block_" + name)
    m = cases.model(nfa, name)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in golden_state(g).items()}, strict=True)
    return m.to(DEV), g


def block_stack(nfa, pairs, d=2, widths=(8,), seed=3, scale=0.3, tail=0):
    """pairs x [AffineCouplingBlock(MLP [c1, *widths, 2 c2]), Permute(d, 'swap')] + `tail` more blocks, every parameter
    scale x N(0, 1)."""
    g = torch.Generator().manual_seed(seed)
    c1 = (d + 1) // 2
    mk = lambda: nfa.flows.AffineCouplingBlock(nfa.nets.MLP([c1] + list(widths) + [2 * (d - c1)]))  # noqa: E731
    flows = [f for _ in range(pairs) for f in (mk(), nfa.flows.Permute(d, mode="swap"))] + [mk() for _ in range(tail)]
    m = nfa.NormalizingFlow(nfa.distributions.DiagGaussian(d, trainable=False), flows)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(scale * torch.randn(p.shape, generator=g))
    return m.to(DEV)


# ---- 1. against the reference's autograd ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dname", ["fwd", "inv"])
@pytest.mark.parametrize("name", list(cases.CASES))
def test_fixture_gradients_vs_reference_autograd(nfa, calls, name, dname):
    """z and log-det at the parity bars, gx and every parameter gradient within max(1e-3 of scale, 4 x the reference's own
    float32-vs-float64 error) -- the bars of test_gpu_realnvp_train.test_fixture_gradients_vs_reference_autograd: one forward and one
    backward call for the whole model, no AffineCouplingFn, no Linear.forward."""
    m, g = fixture_model(nfa, name)
    calls["flows"] = list(m.flows)
    z, ld, gx, _ = step(m, T(g["x"]), dname == "inv", T(g["cz"]), T(g["cl"]))
    assert counts(calls, "fwd", "bwd", "acf", "maf", "lin") == (1, 1, 0, 0, 0), calls
    assert calls["runs"] == [list(range(len(m.flows)))]
    assert_close(N(z), g["z_" + dname], rtol=1e-4, atol=1e-4, what="z")
    assert_close(N(ld), g["ld_" + dname], what="ld", **ld_tol(np.float32))
    items = [("x", gx, "gx_" + dname)] + [(k, p.grad, "g_%s__%s" % (dname, k.replace(".", "__"))) for k, p in m.named_parameters()]
    for k, got, key in items:
        ref32, ref64 = g[key], g[key.replace("_" + dname, "_%s_f64" % dname, 1)]
        assert got is not None, k
        scale = float(np.abs(ref64).max())
        bar = max(1e-3 * scale, 4.0 * float(np.abs(ref32 - ref64).max()))
        err = float(np.abs(N(got) - ref32).max())
        print("%s %s %s: err %.3e bar %.3e (scale %.3e)" % (name, dname, k, err, bar, scale))
        assert err <= bar, (k, err, bar, scale)
    assert len(items) > 4


# ---- 2. forward_kld --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.CASES))
def test_forward_kld_step_vs_reference(nfa, calls, name):
    m, g = fixture_model(nfa, name)
    loss = m.forward_kld(T(g["x"]))
    loss.backward()
    assert counts(calls, "fwd", "bwd", "acf", "maf", "lin") == (1, 1, 0, 0, 0), calls
    print("%s: loss %.7f reference %.7f" % (name, float(loss.detach()), float(g["loss"])))
    assert abs(float(loss.detach()) - float(g["loss"])) < 2e-4 * abs(float(g["loss"]))
    n = 0
    for k, p in m.named_parameters():              # item 1's bar; the fixtures hold no float64 leg of this loss's gradients
        ref32 = g["g__" + k.replace(".", "__")]
        scale = float(np.abs(ref32).max())
        err = float(np.abs(N(p.grad) - ref32).max())
        print("%s %s: err %.3e of scale %.3e" % (name, k, err, scale))
        assert err <= 1e-3 * scale, (k, err, scale)
        n += 1
    assert n == len(list(m.flows.parameters())) > 0


# ---- 3. inference ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dname", ["fwd", "inv"])
@pytest.mark.parametrize("name", list(cases.CASES))
def test_inference_is_one_launch(nfa, calls, name, dname):
    """129 rows (the fixture's rows repeated): one nf_realnvp_chain call for the whole model, no nf_affine_coupling."""
    m, g = fixture_model(nfa, name)
    calls["flows"] = list(m.flows)
    idx = np.arange(129) % g["x"].shape[0]
    x = T(g["x"][idx])
    with torch.no_grad():
        z, ld = m.inverse_and_log_det(x) if dname == "inv" else m.forward_and_log_det(x)
    assert counts(calls, "chain", "ac", "fwd", "lin") == (1, 0, 0, 0), calls
    assert calls["iruns"] == [list(range(len(m.flows)))]
    assert_close(N(z), g["z_" + dname][idx], rtol=1e-4, atol=1e-4, what="z")
    assert_close(N(ld), g["ld_" + dname][idx], what="ld", **ld_tol(np.float32))


# ---- 4. route against route ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("name", list(cases.CASES))
def test_route_vs_layer_by_layer(nfa, calls, layerwise, name, inverse):
    m, g = fixture_model(nfa, name)
    x, cz, cl = T(g["x"]), T(g["cz"]), T(g["cl"])
    z, ld, gx, gp = step(m, x, inverse, cz, cl)
    assert counts(calls, "fwd", "bwd", "acf") == (1, 1, 0)
    with layerwise():
        z0, ld0, gx0, gp0 = step(m, x, inverse, cz, cl)
    assert counts(calls, "fwd", "bwd") == (1, 1) and calls["lin"] > 0 and calls["acf"] == sum(hasattr(f, "split_mode") for f in m.flows)
    assert_close(N(z), N(z0), rtol=1e-4, atol=1e-4, what="z")
    assert_close(N(ld), N(ld0), rtol=1e-4, atol=1e-4, what="ld")
    assert of_scale(gx, gx0) <= 2e-4
    assert_grads_of_scale(gp, gp0, 2e-4, name)
    # inference
    with torch.no_grad():
        zi, ldi = m.inverse_and_log_det(x) if inverse else m.forward_and_log_det(x)
        assert calls["chain"] == 1 and calls["ac"] == calls["acf"]
        with layerwise(train=False):
            zj, ldj = m.inverse_and_log_det(x) if inverse else m.forward_and_log_det(x)
    assert calls["ac"] > calls["acf"]
    assert_close(N(zi), N(zj), rtol=1e-4, atol=1e-4, what="z inference")
    assert_close(N(ldi), N(ldj), rtol=1e-4, atol=1e-4, what="ld inference")


# ---- 5. the README model at its real depth -------------------------------------------------------------------------------------------
def test_readme_model_at_32_layer_pairs(nfa, calls):
    """32 x [AffineCouplingBlock(MLP [1, 8, 8, 2]), Permute(2, 'swap')] = 64 layers = 32 records: one inference launch, one forward and
    one backward launch under autograd in either direction; with a 33rd block the cut falls after 32 RECORDS in processing order.
    (Parameters 0.12 x N(0, 1), as mixed_stack_cases.realnvp_records: 32 coupling layers stay finite.)"""
    m = block_stack(nfa, 32, widths=(8, 8), seed=21, scale=0.3 * 0.4)
    calls["flows"] = list(m.flows)
    assert len(m.flows) == 64
    x = torch.randn(200, 2, generator=torch.Generator().manual_seed(22)).to(DEV)
    for inverse in (False, True):
        with torch.no_grad():
            z, ld = m.inverse_and_log_det(x) if inverse else m.forward_and_log_det(x)
        assert calls["chain"] == 1 and calls["ac"] == 0 and calls["iruns"] == [list(range(64))]
        assert bool(torch.isfinite(z).all()) and bool(torch.isfinite(ld).all())
        zt, ldt, gx, gp = step(m, x, inverse)
        assert counts(calls, "fwd", "bwd", "acf", "lin") == (1, 1, 0, 0) and calls["runs"] == [list(range(64))]
        assert calls["masks"] == [sum(1 << (2 * r) for r in range(32))]
        assert_close(N(zt), N(z), rtol=1e-4, atol=1e-4, what="training forward vs inference")
        assert len(gp) == 32 * 6 and all(a is not None and bool(torch.isfinite(a).all()) for a in gp + [gx])
        assert all(float(a.abs().max()) > 0 for a in gp)
        calls.update(fwd=0, bwd=0, chain=0, runs=[], iruns=[], masks=[])
    m33 = nfa.NormalizingFlow(m.q0, list(m.flows) + list(block_stack(nfa, 0, widths=(8, 8), seed=23, scale=0.12, tail=1).flows))
    calls["flows"] = list(m33.flows)
    step(m33, x, False)
    assert calls["runs"] == [list(range(64)), [64]] and counts(calls, "fwd", "bwd") == (2, 2)
    assert calls["masks"] == [1, sum(1 << (2 * r) for r in range(32))]          # (the backward visits the runs in reverse)
    calls.update(fwd=0, bwd=0, runs=[], masks=[])
    step(m33, x, True)
    assert calls["runs"] == [list(range(2, 65)), [0, 1]] and counts(calls, "fwd", "bwd") == (2, 2)
    assert calls["acf"] == 0 and calls["lin"] == 0


# ---- 6. second round of the persistent loop --------------------------------------------------------------------------------------
def test_second_round_of_the_persistent_loop(nfa, calls, layerwise):
    m = block_stack(nfa, 2, widths=(8,), seed=31)
    rows = nfa.ops.realnvp_rows(8, 9)           # hmax 8; the MLP's Linear inputs: 1 + 8
    assert rows in (64, 128, 256)
    wg = nfa._lib.lib().nf_persistent_workgroups()
    B = wg * rows + rows + 3
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, 2, generator=g).to(DEV)
    # cotangents of one sign, as in test_gpu_realnvp_train: with random signs a sum over 65 795 rows can cancel to float32 noise
    cz, cl = (0.5 + torch.rand(B, 2, generator=g)).to(DEV), (0.5 + torch.rand(B, generator=g)).to(DEV)
    for inverse in (True, False):
        z, ld, gx, gp = step(m, x, inverse, cz, cl)
        for sl in (slice(0, rows + 3), slice(B - rows - 3, B)):
            z1, ld1, gx1, _ = step(m, x[sl].contiguous(), inverse, cz[sl].contiguous(), cl[sl].contiguous())
            assert torch.equal(z[sl], z1) and torch.equal(ld[sl], ld1) and torch.equal(gx[sl], gx1), (inverse, sl)
        n = calls["fwd"]
        with layerwise():
            _, _, gx0, gp0 = step(m, x, inverse, cz, cl)
        assert calls["fwd"] == n and calls["acf"] > 0
        assert of_scale(gx, gx0) <= 2e-4
        assert_grads_of_scale(gp, gp0, 2e-4, "second round")


# ---- 7. determinism, with a frozen param_map -------------------------------------------------------------------------------------
def test_gradients_are_bit_identical_from_run_to_run(nfa, calls):
    m, g = fixture_model(nfa, "readme_d2")
    x = torch.randn(3000, 2, generator=torch.Generator().manual_seed(5)).to(DEV)
    a = step(m, x)
    b = step(m, x)
    assert torch.equal(a[2], b[2]) and all(torch.equal(p, q) for p, q in zip(a[3], b[3])) and len(a[3]) == 24
    assert calls["masks"][-1] == 0b01010101
    frozen = list(m.flows[2].parameters())            # the second block's param_map: record 1
    for p in frozen:
        p.requires_grad_(False)
    c = step(m, x)
    d = step(m, x)
    assert calls["masks"][-1] == 0b01010001 and counts(calls, "fwd", "bwd", "acf", "lin") == (4, 4, 0, 0)
    assert torch.equal(c[2], a[2]) and torch.equal(d[2], a[2])
    ids = {id(p) for p in frozen}
    for p, u, v, w in zip(m.flows.parameters(), c[3], d[3], a[3]):
        if id(p) in ids:
            assert u is None and v is None and p.grad is None
        else:
            assert torch.equal(u, w) and torch.equal(v, w)


# ---- 8. live parameters and permutations -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["fused_adam", "data_update"])
def test_the_blob_follows_the_live_parameters(nfa, calls, layerwise, how):
    m, g = fixture_model(nfa, "d5_maps")
    x = T(g["x"])
    loss0 = m.forward_kld(x)
    loss0.backward()
    loss0 = loss0.detach()
    with torch.no_grad():
        lp0 = m.log_prob(x)
    if how == "fused_adam":
        torch.optim.Adam(m.parameters(), lr=5e-2, fused=True).step()
    else:
        for p in m.parameters():
            p.data.add_(0.05 * torch.sign(p.grad))
        nfa.invalidate_caches(m)
    n, c = calls["fwd"], calls["chain"]
    loss1 = m.forward_kld(x).detach()
    with torch.no_grad():
        lp1 = m.log_prob(x)
    assert calls["fwd"] == n + 1 and calls["chain"] == c + 1
    with layerwise():
        loss2 = m.forward_kld(x).detach()
        with torch.no_grad():
            lp2 = m.log_prob(x)
    assert calls["fwd"] == n + 1
    assert abs(float(loss1) - float(loss0)) > 1e-3 * abs(float(loss0)) and float((lp1 - lp0).abs().max()) > 1e-3
    assert abs(float(loss1) - float(loss2)) < 2e-4 * abs(float(loss2))
    assert_close(N(lp1), N(lp2), rtol=2e-4, atol=2e-4, what="log_prob after the update")


def test_a_replaced_permutation_changes_the_result_accordingly(nfa, calls, layerwise):
    m, g = fixture_model(nfa, "d5_maps")
    x, cz, cl = T(g["x"]), T(g["cz"]), T(g["cl"])
    before = step(m, x, False, cz, cl)
    with torch.no_grad():
        zi0, _ = m.forward_and_log_det(x)
    sd = m.state_dict()
    new = torch.roll(sd["flows.3.perm"], 1)
    sd["flows.3.perm"] = new
    sd["flows.3.inv_perm"] = torch.empty_like(new).scatter_(0, new, torch.arange(5, device=new.device))
    m.load_state_dict(sd)
    for inverse in (False, True):
        n = counts(calls, "fwd", "chain")
        got = step(m, x, inverse, cz, cl)
        with torch.no_grad():
            zi, ldi = m.inverse_and_log_det(x) if inverse else m.forward_and_log_det(x)
        assert counts(calls, "fwd", "chain") == (n[0] + 1, n[1] + 1)
        with layerwise():
            ref = step(m, x, inverse, cz, cl)
        assert_close(N(got[0]), N(ref[0]), rtol=1e-4, atol=1e-4, what="z")
        assert_close(N(zi), N(ref[0]), rtol=1e-4, atol=1e-4, what="z inference")
        assert_close(N(got[1]), N(ref[1]), rtol=1e-4, atol=1e-4, what="ld")
        assert of_scale(got[2], ref[2]) <= 2e-4
        assert_grads_of_scale(got[3], ref[3], 2e-4, "replaced perm")
        if not inverse:
            assert float((got[0] - before[0]).abs().max()) > 1e-2 and float((zi - zi0).abs().max()) > 1e-2


# ---- 9. capture ------------------------------------------------------------------------------------------------------------------
def test_training_step_captures_into_a_graph(nfa, calls):
    m, g = fixture_model(nfa, "readme_d2")
    gen = torch.Generator().manual_seed(13)
    B = nfa.config.realnvp_train_capture_min_batch
    static_x, x_new = torch.randn(B, 2, generator=gen).to(DEV), torch.randn(B, 2, generator=gen).to(DEV)
    n = calls["fwd"]
    got_loss, got = _captured_step(m, static_x, x_new)
    assert calls["fwd"] == n + 3 and calls["lin"] == 0 and calls["acf"] == 0           # two warm-up steps and the captured one
    m.zero_grad(set_to_none=True)
    ref_loss = m.forward_kld(x_new)
    ref_loss.backward()
    assert calls["fwd"] == n + 4
    assert abs(float(got_loss) - float(ref_loss)) <= 2e-4 * abs(float(ref_loss))
    assert_grads_of_scale(got, [p.grad for p in m.parameters()], 2e-4, "captured")
    assert len(got) == 24


# ---- 10. outside the route -------------------------------------------------------------------------------------------------------
def _check_vs_formulas(m, x, inverse, got, bar):
    z, ld, gx, gp = got
    z0, ld0, gx0, gp0 = emu.grads(list(m.flows), x, torch.ones_like(x), torch.ones(x.shape[0], dtype=x.dtype, device=x.device), inverse)
    assert of_scale(z, z0) <= bar and of_scale(ld, ld0) <= bar and of_scale(gx, gx0) <= bar
    for a, p in zip(gp, m.flows.parameters()):
        assert of_scale(a, gp0[id(p)]) <= bar


def _outside(nfa, case):
    MLP, Block, Permute = nfa.nets.MLP, nfa.flows.AffineCouplingBlock, nfa.flows.Permute
    d, dtype = 2, torch.float32
    if case == "checkerboard":
        d = 4
        flows = [Block(MLP([2, 8, 4]), split_mode="checkerboard"), Permute(4, mode="swap"), Block(MLP([2, 8, 4]), split_mode="checkerboard_inv")]
    elif case == "width65":
        flows = [Block(MLP([1, 65, 2])), Permute(2, mode="swap"), Block(MLP([1, 65, 2]))]
    elif case == "d17":
        d = 17
        flows = [Block(MLP([9, 8, 16])), Permute(17, mode="shuffle"), Block(MLP([8, 8, 18]), split_mode="channel_inv")]
    else:
        flows = [Block(MLP([1, 8, 2])), Permute(2, mode="swap"), Block(MLP([1, 8, 2]))]
        dtype = torch.float64 if case == "float64" else dtype
    m = nfa.NormalizingFlow(nfa.distributions.DiagGaussian(d, trainable=False), flows)
    g = torch.Generator().manual_seed(17)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(0.3 * torch.randn(p.shape, generator=g))
    return m.to(dtype).to(DEV), d


@pytest.mark.parametrize("case", ["checkerboard", "width65", "d17", "float64"])
def test_outside_the_route_shapes(nfa, calls, case):
    m, d = _outside(nfa, case)
    x = torch.randn(37, d, generator=torch.Generator().manual_seed(9)).to(next(m.parameters()).dtype).to(DEV)
    for inverse in (True, False):
        n = calls["acf"] + calls["lin"]
        got = step(m, x, inverse)
        assert counts(calls, "fwd", "bwd", "chain") == (0, 0, 0) and calls["acf"] + calls["lin"] > n
        _check_vs_formulas(m, x, inverse, got, 1e-9 if case == "float64" else 2e-4)
        with torch.no_grad():
            z, ld = m.inverse_and_log_det(x) if inverse else m.forward_and_log_det(x)
        assert calls["chain"] == 0 and of_scale(z, got[0]) <= (1e-9 if case == "float64" else 2e-4)


def test_higher_order_gradients_stay_outside(nfa, calls):
    m, _ = _outside(nfa, "plain")
    x = torch.randn(37, 2, generator=torch.Generator().manual_seed(12)).to(DEV)
    with nfa.config.higher_order_gradients():
        got = step(m, x)
        assert counts(calls, "fwd", "bwd") == (0, 0) and calls["acf"] == 2
        _check_vs_formulas(m, x, True, got, 2e-4)
    step(m, x)
    assert counts(calls, "fwd", "bwd") == (1, 1) and calls["acf"] == 2          # and the route is back outside the context


def test_a_permute_between_two_masked_affine_flows_ends_both_runs(nfa, calls):
    b = torch.tensor([1.0, 0.0, 1.0])
    mk = lambda i: nfa.flows.MaskedAffineFlow(b if i % 2 == 0 else 1 - b, nfa.nets.MLP([3, 8, 3]), nfa.nets.MLP([3, 8, 3]))  # noqa: E731
    flows = [mk(0), mk(1), nfa.flows.Permute(3, mode="swap"), mk(2), mk(3)]
    m = nfa.NormalizingFlow(nfa.distributions.DiagGaussian(3, trainable=False), flows)
    g = torch.Generator().manual_seed(19)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(0.3 * torch.randn(p.shape, generator=g))
    m = m.to(DEV)
    calls["flows"] = list(m.flows)
    x = torch.randn(37, 3, generator=torch.Generator().manual_seed(20)).to(DEV)
    for inverse in (False, True):
        calls.update(runs=[], iruns=[], fwd=0, bwd=0, chain=0)
        got = step(m, x, inverse)
        assert calls["runs"] == ([[3, 4], [0, 1]] if inverse else [[0, 1], [3, 4]]) and counts(calls, "fwd", "bwd", "maf") == (2, 2, 0)
        _check_vs_formulas(m, x, inverse, got, 2e-4)
        with torch.no_grad():
            z, _ = m.inverse_and_log_det(x) if inverse else m.forward_and_log_det(x)
        assert calls["iruns"] == calls["runs"] and calls["chain"] == 2 and of_scale(z, got[0]) <= 2e-4


# ---- 11. views -------------------------------------------------------------------------------------------------------------------
def test_offset_strided_input_view(nfa, calls):
    m, g = fixture_model(nfa, "d5_maps")
    wide = torch.randn(40, 9, generator=torch.Generator().manual_seed(8)).to(DEV)
    view = wide[3:36, 2:7]
    assert not view.is_contiguous() and view.storage_offset() > 0
    a = step(m, view)
    b = step(m, view.contiguous())
    assert calls["fwd"] == 2
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert all(torch.equal(p, q) for p, q in zip(a[3], b[3]))
    with torch.no_grad():
        zi, ldi = m.inverse_and_log_det(view)
        zj, ldj = m.inverse_and_log_det(view.contiguous())
    assert calls["chain"] == 2 and torch.equal(zi, zj) and torch.equal(ldi, ldj)
