"""GPU tests (-m gpu) of MIXED layer stacks: the segment boundaries of core._run_chain_impl and _prepack._plan.

Every other GPU test builds a model of one route (n x [CoupledRQS, LU] of one shape, n x [MaskedAffine, ActNorm], one layer).  A
segmentation mistake -- a layer skipped, run twice or out of order where two kernel families meet -- is wrong only in stacks nobody
built.  The stacks come from tests/mixed_stack_cases.py together with the hand-written call sequence each pass must consist of
("The chain router's rules").

| stack | boundary exercised                                                        | largest such case in the suite before     |
|-------|---------------------------------------------------------------------------|-------------------------------------------|
| I1    | fused chain of 66 pairs: two launches, log-det across them, pad / unpad    | 32 pairs (the benchmark), one launch      |
| I2    | exactly 64 and exactly 33 pairs: one launch                                | 32 pairs                                  |
| I3    | flush on a signature change; a lone pair between chains; chain | nf_nsf_wide | one signature per model                   |
| I4    | orphan LU / CoupledRQS / Permute; the same pairs from both ends            | none                                      |
| I5    | RealNVP runs cut by ineligible layers; a run of one record                 | one run of 4 layers                       |
| I6    | six kernel families in one pass                                            | none                                      |
| I7    | a RealNVP run directly between spline pairs: the flush in front of it      | none                                      |
| T1    | 32 / 33 / 40 records under autograd; bits 62, 63 of the gradient mask      | 8 records                                 |
| T2    | an all-constant run, fused runs of two, an ineligible layer under autograd | one run                                   |
| T3    | two "nsf" groups, an orphan LU, a frozen and a wide layer in the prepack   | one group of each kind                    |
| T4    | one pair module twice in the list                                          | none                                      |

Per stack and direction: (a) the recorded call sequence equals `expected`; (b) two runs give identical bits; (c) the expected segments
run one after another as separate core.run_chain calls on sub-lists, with one log-det buffer, give the bits of the whole model (each
sub-call must take the entry points it took inside the model); (d) against a float64 deep copy run by a plain Python loop over
flow.forward / flow.inverse with every one-launch switch off, the routed error is at most max(bar, 4 x the error of the same loop in
float32), in units of the bar: z 2e-5 (conftest.TOL) in the density direction and 1e-4 in the sampling direction and for the RealNVP
stacks (test_route_vs_layer_by_layer), log-det conftest.ld_tol (root_finding=True when sampling), gradients 2e-4 of the reference's
scale for RealNVP stacks (test_route_vs_layer_by_layer) and 3e-3 for spline pairs (test_gpu_training._check_grads); every element
is compared and the non-finite patterns must agree; (e) inverse(forward(x)) = x at 1e-3 and the log-dets cancel at 5e-3
(test_gpu_parity's bars for randomly initialised splines: bars of ONE layer), or 4 x what the float32 loop's own round trip misses them
by, as in (d): the float64 loop inverts every row to 1e-8, the float32 loop through 66 pairs (132 layers) leaves single rows 5e-2 / 1.3
away, and the routed pass is held to that yardstick, not to a single layer's.  Rows on which a circular layer wrapped a coordinate that
came in outside its period (I6) are not inverted by any precision: there the float64 loop's round trip is the target.

Every test prints what it measured before it asserts.  Worst per stack on an MI355X, in units of the bar, routed / float32 loop:

| stack | z             | log-det       | gx and gradients | round trip x    | round trip log-det |
|-------|---------------|---------------|------------------|-----------------|--------------------|
| I1    | 1.75 / 1.43   | 2.82 / 1.16   |                  | 23.6 / 22.8     | 275 / 252          |
| I2    | 1.34 / 1.80   | 2.52 / 0.97   |                  | 0.22 / 0.46     | 2.79 / 0.72        |
| I3    | 0.23 / 0.26   | 0.20 / 0.18   |                  | 0.011 / 0.013   | 0.043 / 0.167      |
| I4    | 0.09 / 0.07   | 0.11 / 0.08   |                  | 0.002 / 0.001   | 0.003 / 0.004      |
| I5    | 0.02 / 0.01   | 0.004 / 0.004 |                  | < 0.001         | < 0.001            |
| I6    | 0.12 / 0.07   | 0.03 / 0.02   |                  | 0.003 / 0.003   | 0.002 / 0.001      |
| T1    | 0.006 / 0.006 | 0.002 / 0.001 | 0.23 / 0.19      | 1.7e-6 absolute | 2.7e-7 absolute    |
| T2    | 0.01 / 0.01   | 0.004 / 0.004 | 0.015 / 0.013    | 1.1e-6 absolute | 3.0e-7 absolute    |
| T3    | loss 0.000    |               | 0.008 / 0.003    |                 |                    |
| T4    | loss 0.000    |               | 0.002 / 2.05 (the separate layers: 2.05 / 2.05) |  |                    |

The fused chain's log-det is 2.5-3.5 x further from float64 than the float32 loop's at every depth (33, 64, 66 pairs, both directions):
inside the factor 4, and no effect of the segment boundaries -- one chain launch of 33 pairs shows it as two launches of 64 + 2 do.
T3: prepack off against prepack on without the pair Functions: the loss bit for bit, gradients 3.0e-7 / 5.6e-7 of scale (steps 1, 2).
T4, step 1: the pair Functions and the separate layers differ by 6.1e-3 of scale in one LU gradient (1e-7 in the loss): rows on a ReLU
kink of a conditioner, O(1 / B) each at B = 1024 (test_pair_training_path_vs_separate_layers) -- the float32 loop is as far from float64.

Sensitivity (each change applied to core.py alone; the 712 GPU tests of the other modules pass under every one of them):
  1. `pairs[i:i + 63]` while stepping by 64 in _run_pairs_impl          -> I1[f32], I1[bf16x3] and I2[64] fail;
  2. no `flush(z)` in front of _run_realnvp                              -> I7 fails (and only I7: it was added for this);
  3. the training run capped at MAX_RECORDS, k advanced by one more      -> T1[33-all], T1[33-last], T1[40-all], T1[40-last] fail;
  4. no signature comparison in front of `pending.append`                -> I3 fails at the call sequence (checked with the library's
     launches skipped: a chain over pairs of two shapes reads beyond the smaller blob);
  and without the rule that keeps a module listed twice out of the prepack plan (_prepack._plan) T4's backward raises in PairTrainFn.
"""
import copy

import numpy as np
import pytest
import torch

import mixed_stack_cases as cases
import realnvp_train_emulator as emu
from conftest import TOL, ld_tol
from test_gpu_realnvp_train import of_scale, step
from test_gpu_tile_rounds import switched_off
from test_gpu_views import calls, nfa, rows, same  # noqa: F401  (calls, nfa: fixtures)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SWITCHES = ("fused_chain", "nsf_wide", "nsf_circular", "arnsf_density_ft", "made_fused", "made_train", "realnvp_train",
            "nsf_circular_train", "arnsf_train_ft", "train_full", "train_prepack", "train_pair")
ONE_LAUNCH = {cases.CHAIN, cases.CHAIN_X3, cases.WIDE, cases.CIRC, cases.RNVP, cases.MADE_SPLINE, cases.MADE_AFFINE}
Z_DENSITY, Z_SAMPLING = TOL[np.dtype("float32")], dict(rtol=1e-4, atol=1e-4)


def seq(log, keep=cases.COMPUTE):
    out = [cases.ALIAS.get(n, n) for n, _ in log]
    return [n for n in out if n in keep]


def layerwise_copy(model, dtype):
    """A deep copy of `model` in `dtype` whose coupling layers keep to the layer-wise path (the switch of every one-launch kernel of
    the layer off)."""
    m = copy.deepcopy(model).to(dtype)
    for mod in m.modules():
        if hasattr(mod, "use_fused"):
            mod.use_fused = False
    return m


def loop(flows, x, inverse):
    """The reference's loop: flow.forward / flow.inverse one after another; never enters core.run_chain."""
    ld = torch.zeros(x.shape[0], dtype=x.dtype, device=x.device)
    for f in (reversed(list(flows)) if inverse else flows):
        x, l = f.inverse(x) if inverse else f.forward(x)
        ld = ld + l.to(x.dtype)
    return x, ld


def units(got, ref, rtol, atol, what):
    """max |got - ref| / (atol + rtol |ref|) over EVERY element; the non-finite patterns must agree."""
    got, ref = got.detach().double(), ref.detach().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.equal(torch.isnan(got), torch.isnan(ref)), what + ": NaN patterns differ"
    assert torch.equal(torch.isinf(got), torch.isinf(ref)) and torch.equal(torch.sign(got[torch.isinf(got)]), torch.sign(ref[torch.isinf(ref)])), what
    fin = torch.isfinite(ref)
    if not bool(fin.any()):
        return 0.0
    return float(((got - ref).abs()[fin] / (atol + rtol * ref.abs()[fin])).max())


def within(tag, what, routed, yardstick):
    print("%s %s: routed %.3f, float32 loop %.3f (units of the bar)" % (tag, what, routed, yardstick))
    assert routed <= max(1.0, 4.0 * yardstick), (tag, what, routed, yardstick)


def run_model(model, x, inverse):
    return model.inverse_and_log_det(x) if inverse else model.forward_and_log_det(x)


def check_inference(nfa, calls, model, expected, tag, batches=(129, 257), circular=False):
    flows = model.flows
    D = int(model.q0.shape[0])
    m64, m32 = layerwise_copy(model, torch.float64), layerwise_copy(model, torch.float32)
    for B in batches:
        for dname, inverse in (("inv", True), ("fwd", False)):
            segs = expected[dname]
            t = "%s B=%d %s" % (tag, B, dname)
            x = rows(B, D, B + int(inverse)) if inverse else rows(B, D, B + int(inverse), scale=1.0)
            with torch.no_grad():
                # (a) segmentation
                del calls[:]
                z, ld = run_model(model, x, inverse)
                got = seq(calls)
                assert got == cases.names(segs), (t, got, cases.names(segs))
                # (b) determinism
                z2, ld2 = run_model(model, x, inverse)
                assert same(z, z2) and same(ld, ld2), t + ": two runs differ"
                # (c) composition
                zc, ldc = x, torch.zeros(B, dtype=x.dtype, device=x.device)
                for lo, hi, ns in segs:
                    del calls[:]
                    zc = nfa.core.run_chain(flows[lo:hi], zc, inverse, ldc, +1)
                    assert seq(calls) == ns, (t, lo, hi, seq(calls), ns)
                assert same(zc, z) and same(ldc, ld), t + ": the segments run one by one differ from the whole model"
                # (d) precision
                del calls[:]
                with switched_off(nfa, *SWITCHES):
                    z64, ld64 = loop(m64.flows, x.double(), inverse)
                    z32, ld32 = loop(m32.flows, x, inverse)
                assert not (set(seq(calls)) & ONE_LAUNCH), (t, seq(calls))
                assert z64.dtype == torch.float64 and ld64.dtype == torch.float64
                zt = Z_DENSITY if inverse else Z_SAMPLING
                lt = ld_tol(np.float32, root_finding=not inverse)
                within(t, "z", units(z, z64, what=t + " z", **zt), units(z32, z64, what=t + " z loop", **zt))
                within(t, "ld", units(ld, ld64, what=t + " ld", **lt), units(ld32, ld64, what=t + " ld loop", **lt))
                # (e) round trip.  The target is the float64 loop's round trip: x itself (to 1e-8) on every row the stack inverts --
                # all of them, except where a circular layer wrapped a coordinate that came in outside its period
                back, ldb = run_model(model, z, not inverse)
                with switched_off(nfa, *SWITCHES):
                    back64, ldb64 = loop(m64.flows, z64, not inverse)
                    back32, ldb32 = loop(m32.flows, z32, not inverse)
                inverted = (back64 - x.double()).abs().amax(1) <= 1e-8 * (1.0 + x.double().abs().amax(1))
                assert bool(inverted.all()) if not circular else int(inverted.sum()) >= B // 4, (t, int(inverted.sum()))
                assert float((ld64 + ldb64)[inverted].abs().max()) <= 1e-8
                print("%s round trip: max |x' - x| %.3e, max |ld + ld'| %.3e on the %d rows the stack inverts" % (
                    t, float((back - x)[inverted].abs().max()), float((ld + ldb)[inverted].abs().max()), int(inverted.sum())))
                within(t, "round trip x", units(back, back64, 1e-3, 1e-3, t + " round trip"), units(back32, back64, 1e-3, 1e-3, t + " round trip loop"))
                within(t, "round trip ld", units(ld + ldb, ld64 + ldb64, 0.0, 5e-3, t + " round trip ld"),
                       units(ld32 + ldb32, ld64 + ldb64, 0.0, 5e-3, t + " round trip ld loop"))


# ---- inference stacks -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def narrow66(nfa):
    return cases.narrow_pairs(nfa, 66)[0]


@pytest.mark.parametrize("gemm", ["f32", "bf16x3"])
def test_I1_chain_of_66_pairs_is_two_launches(nfa, calls, narrow66, gemm):
    entry = cases.CHAIN if gemm == "f32" else cases.CHAIN_X3
    nfa.config.set_fused_gemm(gemm)
    try:
        check_inference(nfa, calls, narrow66, cases.narrow_pairs_expected(66, entry), "I1 " + gemm)
    finally:
        nfa.config.set_fused_gemm("f32")


@pytest.mark.parametrize("pairs", [64, 33])
def test_I2_chains_of_64_and_33_pairs_are_one_launch(nfa, calls, narrow66, pairs):
    check_inference(nfa, calls, cases.prefix(nfa, narrow66, pairs), cases.narrow_pairs_expected(pairs), "I2 %d" % pairs)


def test_I3_flush_where_the_pair_signature_changes(nfa, calls):
    check_inference(nfa, calls, *cases.signature_changes(nfa), "I3")


def test_I4_orphans_and_the_same_pairs_from_both_ends(nfa, calls):
    check_inference(nfa, calls, *cases.orphans(nfa), "I4")


def test_I5_realnvp_runs_between_ineligible_layers(nfa, calls):
    check_inference(nfa, calls, *cases.realnvp_runs(nfa), "I5")


def test_I6_every_family_in_one_pass(nfa, calls):
    check_inference(nfa, calls, *cases.families(nfa), "I6", circular=True)


def test_I7_a_realnvp_run_between_spline_pairs_flushes_them_first(nfa, calls):
    check_inference(nfa, calls, *cases.pairs_around_records(nfa), "I7")


# ---- RealNVP training stacks ------------------------------------------------------------------------------------------------------
@pytest.fixture
def train_spy(nfa, monkeypatch):
    """{"runs": [[list indices of a fused run] ...], "fwd" / "bwd": launches, "masks": wmask of every backward launch, "maf" / "act":
    MaskedAffineFn / ActNormFn calls (the layer-by-layer route)}; spy["flows"] must hold the model's flow list."""
    n = {"runs": [], "fwd": 0, "bwd": 0, "masks": [], "maf": 0, "act": 0, "flows": None}
    real_run, real_fwd, real_bwd = nfa.core._run_realnvp_train, nfa.ops.realnvp_chain_train_fwd, nfa.ops.realnvp_chain_bwd

    def run_spy(run, *a, **k):
        fl = list(n["flows"])
        n["runs"].append([[i for i, g in enumerate(fl) if g is f][0] for f in run])
        return real_run(run, *a, **k)

    def fwd_spy(*a, **k):
        n["fwd"] += 1
        return real_fwd(*a, **k)

    def bwd_spy(*a, **k):
        n["bwd"] += 1
        n["masks"].append(a[8])
        return real_bwd(*a, **k)

    def counted(key, fn):
        def wrapper(*a, **k):
            n[key] += 1
            return fn(*a, **k)
        return wrapper
    monkeypatch.setattr(nfa.core, "_run_realnvp_train", run_spy)
    monkeypatch.setattr(nfa.ops, "realnvp_chain_train_fwd", fwd_spy)
    monkeypatch.setattr(nfa.ops, "realnvp_chain_bwd", bwd_spy)
    monkeypatch.setattr(nfa.autograd.MaskedAffineFn, "apply", counted("maf", nfa.autograd.MaskedAffineFn.apply))
    monkeypatch.setattr(nfa.autograd.ActNormFn, "apply", counted("act", nfa.autograd.ActNormFn.apply))
    return n


def reset(spy):
    spy.update(runs=[], fwd=0, bwd=0, masks=[], maf=0, act=0)


def signed64(m):
    return m - (1 << 64) if m >= 1 << 63 else m


def expected_masks(model, runs):
    """The gradient mask of every backward launch (the backward visits the runs in reverse): bits 2 r and 2 r + 1 of every record r
    of the run whose flow is trainable (every record of these stacks has an s side and a t side)."""
    out = []
    for run in reversed(runs):
        m = 0
        for r, i in enumerate(run):
            if any(p.requires_grad for p in model.flows[i].parameters()):
                m |= 3 << (2 * r)
        out.append(signed64(m))
    return out


def loop_step(flows, x, inverse, cz, cl):
    """step() of tests/test_gpu_realnvp_train.py through the reference's loop."""
    params = [p for p in flows.parameters()]
    for p in params:
        p.grad = None
    xx = x.detach().clone().requires_grad_(True)
    z, ld = loop(flows, xx, inverse)
    ((z * cz).sum() + (ld * cl).sum()).backward()
    return z.detach(), ld.detach(), xx.grad, [None if p.grad is None else p.grad.detach().clone() for p in params]


def check_training(nfa, spy, model, expected, tag, B=129):
    d = int(model.q0.shape[0])
    spy["flows"] = model.flows
    g = torch.Generator().manual_seed(B + d)
    x = torch.randn(B, d, generator=g).to(DEV)
    cz, cl = torch.randn(B, d, generator=g).to(DEV), torch.randn(B, generator=g).to(DEV)
    m64, m32 = layerwise_copy(model, torch.float64), layerwise_copy(model, torch.float32)
    for a, b, c in zip(model.parameters(), m64.parameters(), m32.parameters()):
        b.requires_grad_(a.requires_grad)
        c.requires_grad_(a.requires_grad)
    first = {}
    for dname, inverse in (("inv", True), ("fwd", False), ("inv", True)):      # (the third pass: the shared cache slot after a change of direction)
        t = "%s %s" % (tag, dname)
        runs = expected[dname]
        # (a) segmentation
        reset(spy)
        z, ld, gx, gp = step(model, x, inverse, cz, cl)
        assert spy["runs"] == runs, (t, spy["runs"], runs)
        assert (spy["fwd"], spy["bwd"]) == (len(runs), len(runs)) and (spy["maf"], spy["act"]) == expected["layerwise"], (t, dict(spy, flows=None))
        assert spy["masks"] == expected_masks(model, runs), (t, spy["masks"], expected_masks(model, runs))
        # (b) determinism, also across a change of direction
        if dname in first:
            for a, b in zip([z, ld, gx] + gp, first[dname]):
                assert (a is None and b is None) or same(a, b), t + ": a pass differs after the other direction ran"
            continue
        first[dname] = [z, ld, gx] + gp
        z2, ld2, gx2, gp2 = step(model, x, inverse, cz, cl)
        for a, b in zip([z, ld, gx] + gp, [z2, ld2, gx2] + gp2):
            assert (a is None and b is None) or same(a, b), t + ": two runs differ"
        # (c) composition: every expected run (and the layers between them) as a run_chain call of its own
        reset(spy)
        bounds = sorted({0, len(model.flows)} | {r[0] for r in runs} | {r[-1] + 1 for r in runs})
        pieces = list(zip(bounds[:-1], bounds[1:]))
        zc, ldc = x.detach().clone().requires_grad_(True), torch.zeros(B, device=DEV)
        for lo, hi in (reversed(pieces) if inverse else pieces):
            zc = nfa.core.run_chain(model.flows[lo:hi], zc, inverse, ldc, +1)
        assert spy["runs"] == runs, (t, "sub-lists", spy["runs"])
        assert same(zc.detach(), z) and same(ldc.detach(), ld), t + ": the runs one by one differ from the whole model"
        # (d) precision: float64 loop, the float32 loop as the yardstick, and the restated formulas
        reset(spy)
        with switched_off(nfa, *SWITCHES):
            r64 = loop_step(m64.flows, x.double(), inverse, cz.double(), cl.double())
            r32 = loop_step(m32.flows, x, inverse, cz, cl)
        assert spy["fwd"] == 0 and spy["bwd"] == 0
        me = copy.deepcopy(m64)             # (the restated formulas differentiate every parameter: a copy with none frozen)
        for p in me.parameters():
            p.requires_grad_(True)
        e64 = emu.grads(list(me.flows), x.double(), cz.double(), cl.double(), inverse)
        e64 = e64[:3] + ({id(p): e64[3][id(q)] for p, q in zip(m64.flows.parameters(), me.flows.parameters())},)
        assert of_scale(r64[0], e64[0]) < 1e-9 and of_scale(r64[1], e64[1]) < 1e-9 and of_scale(r64[2], e64[2]) < 1e-9
        within(t, "z", units(z, r64[0], 1e-4, 1e-4, t + " z"), units(r32[0], r64[0], 1e-4, 1e-4, t + " z loop"))
        within(t, "ld", units(ld, r64[1], what=t + " ld", **ld_tol(np.float32)), units(r32[1], r64[1], what=t + " ld loop", **ld_tol(np.float32)))
        worst = [of_scale(gx, r64[2]) / 2e-4, of_scale(r32[2], r64[2]) / 2e-4]
        assert torch.isfinite(gx).all()
        for k, (a, b, c, p64) in enumerate(zip(gp, r64[3], r32[3], m64.flows.parameters())):
            assert (a is None) == (b is None) == (not p64.requires_grad), (t, k)
            if a is None:
                continue
            assert of_scale(b, e64[3][id(p64)]) < 1e-9, (t, k)
            assert torch.isfinite(a).all(), (t, k)
            ra, rc = of_scale(a, b) / 2e-4, of_scale(c, b) / 2e-4
            assert ra <= max(1.0, 4.0 * rc), (t, "parameter %d" % k, ra, rc)
            worst = [max(worst[0], ra), max(worst[1], rc)]
        within(t, "gx and gradients (worst)", worst[0], worst[1])
        assert of_scale(gx, r64[2]) / 2e-4 <= max(1.0, 4.0 * of_scale(r32[2], r64[2]) / 2e-4)
    # (e) round trip
    with torch.no_grad():
        z, ld = model.inverse_and_log_det(x)
        back, ldb = model.forward_and_log_det(z)
    print("%s round trip: max |x' - x| %.3e, max |ld + ld'| %.3e" % (tag, float((back - x).abs().max()), float((ld + ldb).abs().max())))
    assert units(back, x, 1e-3, 1e-3, tag + " round trip") <= 1.0 and float((ld + ldb).abs().max()) <= 5e-3


@pytest.mark.parametrize("trainable", ["all", "last"])
@pytest.mark.parametrize("records", [32, 33, 40])
def test_T1_realnvp_runs_of_32_33_and_40_records(nfa, train_spy, records, trainable):
    model, expected = cases.realnvp_records(nfa, records)
    if trainable == "last":          # only the top bits of the last run's gradient mask
        for f in list(model.flows)[:-1]:
            for p in f.parameters():
                p.requires_grad_(False)
    assert [len(r) for r in expected["fwd"]] == {32: [32], 33: [32, 1], 40: [32, 8]}[records]
    assert expected["inv"][0][-1] == records - 1 and len(expected["inv"][0]) == 32
    if records == 32:
        top = expected_masks(model, expected["fwd"])[0]
        assert top == (-1 if trainable == "all" else -(1 << 63) + (1 << 62))
    check_training(nfa, train_spy, model, expected, "T1 %d %s" % (records, trainable))


def test_T2_constant_run_fused_runs_and_an_ineligible_layer(nfa, train_spy):
    check_training(nfa, train_spy, *cases.realnvp_train_mix(nfa), "T2")


# ---- spline pairs under the training prepack ---------------------------------------------------------------------------------------
def kld_step(model, x, flows_loop=False):
    """(loss, [gradient or None of every parameter]) of forward_kld; flows_loop: through the reference's loop."""
    for p in model.parameters():
        p.grad = None
    if flows_loop:
        z, ld = loop(model.flows, x, True)
        loss = -torch.mean(ld + model.q0.log_prob(z))
    else:
        loss = model.forward_kld(x)
    loss.backward()
    return loss.detach(), [None if p.grad is None else p.grad.detach().clone() for p in model.parameters()]


def check_grads(tag, got, ref64, ref32, names, bar):
    worst = [0.0, 0.0]
    for n, a, b, c in zip(names, got, ref64, ref32):
        assert (a is None) == (b is None), (tag, n)
        if a is None:
            continue
        assert torch.isfinite(a).all(), (tag, n)
        ra, rc = of_scale(a, b) / bar, of_scale(c, b) / bar
        assert ra <= max(1.0, 4.0 * rc), (tag, n, ra, rc)
        worst = [max(worst[0], ra), max(worst[1], rc)]
    print("%s gradients (worst): routed %.3f, float32 loop %.3f (units of the bar)" % (tag, worst[0], worst[1]))


def check_pair_training(nfa, calls, model, expected, tag):
    x = rows(1024, 64, 7, scale=1.0)
    names = [n for n, _ in model.named_parameters()]
    m64, m32 = layerwise_copy(model, torch.float64), layerwise_copy(model, torch.float32)
    for a, b, c in zip(model.parameters(), m64.parameters(), m32.parameters()):
        b.requires_grad_(a.requires_grad)
        c.requires_grad_(a.requires_grad)

    def references():
        with torch.no_grad():
            for a, b, c in zip(model.parameters(), m64.parameters(), m32.parameters()):
                b.copy_(a)
                c.copy_(a)
        with switched_off(nfa, *SWITCHES):
            return kld_step(m64, x.double(), flows_loop=True), kld_step(m32, x, flows_loop=True)

    for round_ in (1, 2):
        t = "%s step %d" % (tag, round_)
        # (a) segmentation: the forward pass of one step
        del calls[:]
        loss = model.forward_kld(x)
        got = seq(calls, cases.TRAIN)
        assert got == expected["pass"], (t, got, expected["pass"])
        for p in model.parameters():
            p.grad = None
        loss.backward()
        gp = [None if p.grad is None else p.grad.detach().clone() for p in model.parameters()]
        loss = loss.detach()
        # (d) against float64
        (l64, g64), (l32, g32) = references()
        rl, rc = abs(float(loss) - float(l64)) / abs(float(l64)) / 2e-4, abs(float(l32) - float(l64)) / abs(float(l64)) / 2e-4
        within(t, "loss", rl, rc)
        check_grads(t, gp, g64, g32, names, 3e-3)
        # (f) the switches change the launches, not the step
        variants = []
        for switch in ("train_prepack", "train_pair"):
            with switched_off(nfa, switch):
                del calls[:]
                l2, g2 = kld_step(model, x)
                seen = seq(calls, cases.TRAIN)
            assert cases.PAIR_FWD not in seen and (switch == "train_pair" or not (set(seen) & set(expected["packs"]))), (t, switch, seen)
            assert all((a is None) == (b is None) for a, b in zip(g2, gp)), (t, switch)
            worst = max((of_scale(a, b), n) for n, a, b in zip(names, g2, gp) if a is not None)
            print("%s %s off: loss %r (default %r); gradients vs default %.3e of scale (%s)" % (
                t, switch, float(l2), float(loss), worst[0], worst[1]))
            # every variant is a float32 evaluation of the same step: held to float64 like the default
            within(t + " " + switch + " off", "loss", abs(float(l2) - float(l64)) / abs(float(l64)) / 2e-4, rc)
            check_grads(t + " " + switch + " off", g2, g64, g32, names, 3e-3)
            variants.append((l2, g2))
        # prepack off against prepack on, both without the pair Functions: the SAME kernels on weight images packed by one launch per
        # layer or by one per group (what test_model_level_prepack_gives_identical_steps compares on one group per kind) -- the loss
        # bit for bit, the gradients to its 1e-5 of scale.  The pair Functions against the separate layers are other kernels (W_d
        # composed in float64: test_pair_training_path_vs_separate_layers): they meet in float64 above, not in bits.
        (l_off, g_off), (l_on, g_on) = variants
        assert torch.equal(l_off, l_on), (t, float(l_off), float(l_on))
        worst = max((of_scale(a, b), n) for n, a, b in zip(names, g_off, g_on) if a is not None)
        print("%s prepack off vs on (no pair Functions): gradients %.3e of scale (%s)" % (t, worst[0], worst[1]))
        assert worst[0] <= 1e-5, (t, worst)
        # (b) determinism of the forward
        assert torch.equal(model.forward_kld(x).detach(), loss)
        if round_ == 1:       # an in-place optimizer update: the second step must not read a stale pack image
            kld_step(model, x)
            torch.optim.SGD([p for p in model.parameters() if p.requires_grad], lr=2e-2).step()
    # after the step a layer called on its own packs for itself
    del calls[:]
    xx = x.clone().requires_grad_(True)
    y, _ = model.flows[0].inverse(xx)
    y, _ = model.flows[1].inverse(y)
    got = seq(calls, cases.TRAIN)
    assert got == [cases.PACK_ONE, cases.FULL_FWD, cases.FACTORS_ONE, cases.LU_FWD], (tag, got)


def test_T3_prepack_with_two_nsf_groups_an_orphan_a_frozen_and_a_wide_layer(nfa, calls):
    model, expected = cases.pair_training(nfa)
    assert all(p.grad is None for p in model.flows[7].parameters())
    check_pair_training(nfa, calls, model, expected, "T3")
    assert all(p.grad is None for p in model.flows[7].parameters())


def test_T4_one_pair_module_twice_in_the_list(nfa, calls):
    model, expected = cases.shared_pair(nfa)
    assert model.flows[0] is model.flows[4] and model.flows[1] is model.flows[5]
    check_pair_training(nfa, calls, model, expected, "T4")
