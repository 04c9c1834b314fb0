"""GPU tests (-m gpu) of every branch and every repeated sweep of the streaming kernels: the HBM-bound element-wise and reduction
kernels of csrc/affine.hip, affine_bwd.hip, image_glue.hip and the per-pixel product of inv1x1.hip.  Each picks among
hand-specialised paths by row length, plane size, channel count or dtype and walks a capped grid with a stride loop.  The cases,
their float64 references and float32 yardsticks live in tests/stream_kernel_cases.py (checked on the CPU by
tests/test_host_stream_kernel_cases.py); this module runs them through the `ops` wrappers and the autograd Functions.

Inventory, re-derived from the launchers ("second sweep": the first shape whose stride loop goes round twice; "before": what a GPU
test held to values before this module; every path below runs here in one sweep and in several, with a full and with a ragged last
sweep, unless stream_kernel_cases.UNREACHABLE says why it cannot):

| kernel | path | condition | second sweep from | before | here |
|---|---|---|---|---|---|
| masked_affine_kernel | 4 per lane, lanes per row a power of two | float32, inner % 4 == 0, inner <= 256, inner / 4 in {1, 2, .. 64} | B inner / 4 > 2048 x 256: (131 073, 16) | inner 16 in models | (1 | 256 | 257, 4), (70, 256), (131 137 | 262 144, 16) |
| | 4 per lane, idle lanes | inner / 4 not a power of two | the grid covers B L4 / P rows: (33, 20) | -- | (8 | 32 | 103 | 256 | 131 072, 20), (9, 132) |
| | short rows | inner <= 64 (float64, or inner % 4 != 0) | B > 4 x 64 / P: (257, 1) | inner 2, 7 | inner 1, 2, 5, 7, 33, 63; float64 4, 8, 64 |
| | generic, workgroup per row | otherwise | B > 4096 | (5, 105) | (4 099 | 8 192, 65 | 257), (7, 260), (3, 1 030), float64 (5, 128) |
| masked_affine_bwd_kernel | one element per thread | -- | B inner > 256 | (5, 105) | every forward shape |
| diag_gaussian_kernel | 4 per lane (both lane counts) | as masked_affine | as masked_affine | d 12, 64, 128 | d 4, 20, 132, 256 x B 1, 70, 257; (131 137 | 262 144, 16), (131 072, 20) |
| | wave per row, one / several lane passes | otherwise; d <= 64 / d > 64 | B > 8192 | d 2, 5 | d 1, 5, 63, 65, 260, 1 000; (8 197 | 16 384, 5 | 65); float64 8, 128 |
| affine_coupling[_bwd]_kernel | workgroup per image | -- | B > 4096 | (5, 7, 15) | (4 099 | 8 192, 3, HW 1 | 150), four scale maps x flip x bias |
| actnorm_kernel | element loop; per-row log-det loop | -- | N > 256 grid; B > 256 grid | inside models | (1 500, 1, 1), (1 000, 3, 1), (2 049, 4, 256), ... |
| actnorm_bwd_kernel | float32 quads / scalar; walk dq = 0, carry, dk = 0 | HW % 4 == 0 and float32 / not; row width divides 256, below 256, above | a workgroup's images x width > 256 | quads with dq = 0, one sweep | C = 2048 shapes: several images over several sweeps on all six walks |
| maf_affine_kernel | wave per row, one / several lane passes | D <= 64 / D > 64 | B > 8192 | (67, 13) | D 1, 3, 63, 64, 65, 130; B 67, 68, 8 197, 16 384 |
| maf_affine_bwd_kernel | one element per thread | -- | B D > 524 288: (8 070, 65) | (67, 13) | the same and (16 384, 64) |
| logit_kernel, diag_gaussian_rows_kernel | wave per row | row length <= 64 / > 64 | B > 8192 | one fixture each | 1 .. 3 072; (8 197 | 16 384, 3 | 5 | 65); labels -1 and num_rows |
| squeeze_kernel, bias_leaky_relu_kernel | one element per thread | direction | N > 256 grid | one fixture / -- | 12 .. 2 162 688 elements (past 2 048 x 1 024) |
| ld_fold_multi_kernel | tail only, unrolled, unrolled + tail, second launch | n < 8, n % 8 == 0, else, n > 120 | B > 524 288 | n <= 96 at one B | n 1 .. 250, sign flips at terms 31, 32, 63, 64, B up to 1 048 576 |
| inv1x1_conv_kernel | 4-channel loop, its tail, fewer than 4 channels; per-row log-det loop | C % 4, C < 4 | B HW ceil(C / 8) > 524 288; B > 524 288 | C 12, 24, 48 in Glow | C 1 .. 64 x HW 1, 15, 64; (4 100, 9, 64); (524 353 | 1 048 576, 1, 1) |
| inv1x1_wgrad_mfma_kernel<NB> | NB = 1 .. 4 | float32, HW % 16 == 0 | more than 16 chunks per workgroup: HW > 256 | C 12, 24, 48 | C 1, 3, 16, 17, 33, 49, 64; HW 16 .. 528 |
| inv1x1_wgrad_partial_kernel | float32, float64 | otherwise | images per workgroup: B > 256 | (5, 7, 15) | HW 1, 15, 100; B 5, 257, 512 |

Every case asserts
(a) every output and every gradient against the float64 reference on ALL elements, NaN / Inf patterns equal at the named non-finite
    entries.  The bar is the larger of the bar the suite already holds the kernel to (conftest.TOL for element-wise outputs, ld_tol
    for per-row sums, rtol 2e-5 / 1e-11 with atol 10 rtol -- 100 rtol for the per-channel and per-matrix sums gs, gt, gW -- for
    gradients: stream_kernel_cases._bar and KIND; inv1x1_conv's y and actnorm_bwd's gz are held to TOL and the 10 rtol bar) and 4 x the float32 yardstick's own error on that case; float64 kernels the float64 bars alone.  On
    these inputs the yardstick stays below 0.15 of the existing bars (the host test prints it), so the existing bars decide;
(b) two calls give identical bits;
(c) for the row-wise forward kernels, the rows of the last sweep (the last row when there is one sweep) equal, bit for bit, a fresh
    call on those rows alone;
(d) squeeze equals the permutation of reshape.py:116-128 (its reshape / permute, written out by index), ld_fold_multi a sequential
    float32 loop in the same order, bias_leaky_relu_ (y + bias) then leaky_relu in the same precision, bit for bit (it IS bit-exact:
    one add, one compare, one multiply per element, nothing to contract).
An accumulator given with logdet= / acc= sits inside a NaN-filled storage: a write outside the rows, or an add where a write was
asked for, shows.

Worst float32 case of each kernel on an MI355X, every output and gradient against the float64 reference: kernel error / bar, then
kernel error / the float32 yardstick's own error (float64 cases: below 0.0001 of their bars, inv1x1_wgrad 0.006, no yardstick).

| kernel              | error / bar | at                                  | error / yardstick | at                              |
|---------------------|-------------|-------------------------------------|-------------------|---------------------------------|
| masked_affine       | 0.008       | y (8 192, 257)                      | 6.1               | ld (3, 1 030)                   |
| masked_affine_bwd   | 0.007       | y (262 144, 16)                     | 2.4               | ld (3, 1 030)                   |
| diag_gaussian       | 0.003       | (131 072, 20)                       | 1.5               | (70, 20)                        |
| affine_coupling     | 0.012       | ld (8 192, 3, 150) exp              | 3.5               | ld (3, 5, 150) exp              |
| affine_coupling_bwd | 0.010       | ld (8 192, 3, 150) exp              | 6.7               | ld (3, 5, 150) exp              |
| actnorm             | 0.006       | y (1 000, 3, 1)                     | 7.0               | ld (256, 4, 1)                  |
| actnorm_bwd         | 0.032       | ld (40, 2 048, 36)                  | 34.8              | ld (256, 2 048, 2)              |
| maf_affine          | 0.013       | y (16 384, 65)                      | 1.2               | ld (67, 1)                      |
| maf_affine_bwd      | 0.010       | y (16 384, 64)                      | 1.3               | ld (67, 65)                     |
| logit               | 0.014       | y (16 384, 65) inverse              | 3.0               | ld (8, 3) forward               |
| diag_gaussian_rows  | 0.002       | (8 197, 5) labels                   | 1.2               | (37, 65) no labels              |
| inv1x1_conv         | 0.028       | y (3, 48, 15) affine                | 2.0               | y (3, 64, 1) affine             |
| inv1x1_wgrad        | 0.067       | gW (300, 33, 272)                   | 2.8               | gW (5, 3, 48)                   |
| squeeze, bias_leaky_relu_, ld_fold_multi | bit-equal to the formula in the kernel's precision on every case |

Where the kernel is several times the yardstick's error, a sum of a few hundred or thousand terms is a few float32 ulps from float64
in another summation order than torch's (eight sequential terms per thread and a block-wide tree against torch's pairwise sum; at
34.8, ActNorm's HW x sum of 2 048 scales, the yardstick happens to land within 1e-3 of the bar), far inside ld_tol.

Sensitivity: six one-line mutations that only skip work or change a value, each built into a library of its own, run once and not
kept.  New cases that fail; then what the suite as it was before this module did on the same library:
  1 masked_affine 4-per-lane path, later sweeps skipped: 27 -- masked_affine and _bwd at (103 | 256, 20) with every option,
    (131 072, 20), (9, 132), (131 137 | 262 144, 16).  Before: all 772 passed.
  2 diag_gaussian vector path, last butterfly step dropped: 18 -- every diag_gaussian case with more than one lane per row (d 16, 20,
    132, 256).  Before: 33 failed (the model parity, training-step and benchmark-contract tests, through the base distribution).
  3 actnorm_bwd quad path, `q >= Q` carry without ++k in the gradient sums: 5 -- actnorm_bwd (40, 2 048, 36), (90 | 256, 2 048, 12),
    (2, 2 048, 1 028 | 1 536).  Before: all 772 passed.
  4 ld_fold_multi, sign taken from word i >> 6: 14 -- every ld_fold case with n >= 119 (`flips` and `mixed`).  Before: 1 failed
    (test_glow_level_folds_its_log_dets_in_one_launch).
  5 MFMA wgrad, the last block's channel mask one short when the block holds one channel: 47 -- every float32 inv1x1_wgrad case on
    the MFMA path with C = 1, 17, 33, 49.  Before: all 772 passed.
  6 maf_affine_bwd, later sweeps of its stride loop skipped (the kernel has no lane stride): 4 -- maf_affine_bwd (8 070, 65) and
    (16 384, 64) in both dtypes.  Before: 2 failed (test_made_training_full_batch_vs_library_path and the counted-wait lint's
    made_train digest, both at 65 536 rows).
"""
import pytest
import torch

import stream_kernel_cases as sc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PAD = 5
NAN = float("nan")


@pytest.fixture(scope="module")
def nfa():
    import normflows_amd
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    assert normflows_amd.native_library_path().endswith("normalizing-flows_amd/lib/libnf_mi355x.so")
    normflows_amd._lib.lib()
    return normflows_amd


def same(a, b):
    """Bit equality that lets NaN equal NaN."""
    return (a.shape == b.shape and a.dtype == b.dtype and torch.equal(torch.isnan(a), torch.isnan(b))
            and torch.equal(torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0)))


def dev(x):
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in x.items()}


def accumulator(nfa, c, x):
    """(storage, view of the rows, acc code) for option `acc`; the view holds ld0 for add / sub and NaN for write."""
    a = c.p.get("acc")
    if a is None:
        return None, None, None
    L = nfa._lib
    B = next(v for k, v in x.items() if k in ("z", "x")).shape[0]
    buf = torch.full((B + 2 * PAD,), NAN, dtype=sc.DT[c.dtype], device=DEV)
    view = buf[PAD:PAD + B]
    if a != "write":
        view.copy_(x["ld0"])
    return buf, view, {"write": L.LD_WRITE, "add": L.LD_ADD, "sub": L.LD_SUB}[a]


def grads(c, x, leaves, names, fn):
    lv = [None if x[k] is None else x[k].detach().clone().requires_grad_(True) for k in leaves]
    y, ld = fn(*lv)
    loss = 0.0
    if c.p.get("gy", True):
        loss = loss + (y * x["cy"]).sum()
    if c.p.get("gld", True) and ld.requires_grad:
        loss = loss + (ld * x["cl"]).sum()
    loss.backward()
    out = dict(y=y.detach(), ld=ld.detach())
    for t, name in zip(lv, names):
        if t is not None:
            out[name] = t.grad if t.grad is not None else torch.zeros_like(t)
    return out


def run(nfa, c, x):
    """The case's outputs from the library, named as stream_kernel_cases' formulas name them."""
    ops, p, k = nfa.ops, c.p, c.kernel
    from normflows_amd import autograd as ag
    buf, view, code = accumulator(nfa, c, x)
    out = {}
    if k == "masked_affine":
        out["y"], out["ld"] = ops.masked_affine(x["z"], x["b"], x["s"], x["t"], p["direction"], logdet=view, acc=code)
    elif k == "masked_affine_bwd":
        if not p.get("gld", True):       # the kernel's gld == NULL branch: the wrapper itself (the Function materialises zeros)
            out["y"], out["ld"] = ops.masked_affine(x["z"], x["b"], x["s"], x["t"], p["direction"])
            out["gz"], out["gs"], out["gt"] = ops.masked_affine_bwd(x["z"], x["b"], x["s"], x["t"], x["cy"], None, p["direction"])
        else:
            out = grads(c, x, ("z", "s", "t"), ("gz", "gs", "gt"), lambda z, s, t: ag.MaskedAffineFn.apply(z, x["b"], s, t, p["direction"]))
    elif k == "diag_gaussian":
        out["lp"] = ops.diag_gaussian_log_prob(x["z"], x["loc"], x["ls"], p.get("shift", 0.0), out=view, acc=code)
    elif k == "rows":
        out["lp"] = ops.diag_gaussian_log_prob_rows(x["z"], x["loc"], x["ls"], x["idx"], p.get("shift", 0.0), out=view, acc=code)
    elif k == "affine_coupling":
        out["y"], out["ld"] = ops.affine_coupling(x["z"], x["param"], p["c1"], p["flip"], p["smap"], p["direction"], logdet=view, acc=code,
                                                  param_bias=x["pbias"])
    elif k == "affine_coupling_bwd":
        cfg = (p["c1"], p["flip"], p["smap"], p["direction"])
        if not p.get("gld", True):
            out["y"], out["ld"] = ops.affine_coupling(x["z"], x["param"], *cfg)
            out["gz"], out["gparam"] = ops.affine_coupling_bwd(x["z"], x["param"], x["cy"], None, *cfg)
        else:
            out = grads(c, x, ("z", "param"), ("gz", "gparam"), lambda z, prm: ag.AffineCouplingFn.apply(z, prm, *cfg))
    elif k == "actnorm":
        out["y"], lds = ops.actnorm(x["z"], x["s"], x["t"], p["direction"], logdet=view, acc=code, want_scalar=p["want_scalar"])
        if p["want_scalar"]:
            out["lds"] = lds
        else:
            assert lds is None
        if view is not None:
            out["ld"] = view
    elif k == "actnorm_bwd":
        if not p.get("gld", True):
            out["gz"], out["gs"], out["gt"] = ops.actnorm_bwd(x["z"], x["s"], x["t"], x["cy"], None, p["direction"])
        else:
            out = grads(c, x, ("z", "s", "t"), ("gz", "gs", "gt"), lambda z, s, t: ag.ActNormFn.apply(z, s, t, p["direction"]))
    elif k == "maf_affine":
        out["y"], out["ld"] = ops.maf_affine(x["x"], x["params"], p["direction"], logdet=view, acc=code)
    elif k == "maf_affine_bwd":
        out = grads(c, x, ("x", "params"), ("gx", "gparams"), lambda xx, prm: ag.MafAffineFn.apply(xx, prm, p["direction"]))
    elif k == "logit":
        out["y"], out["ld"] = ops.logit(x["z"], p["alpha"], p["direction"], logdet=view, acc=code)
    elif k == "squeeze":
        out["y"] = ops.squeeze(x["z"], p["direction"])
    elif k == "bias_leaky_relu":
        out["y"] = ops.bias_leaky_relu_(x["y"].clone(), x["bias"], p["slope"])
    elif k == "ld_fold":
        terms = [x["t%d" % (i % sc.LDF_DISTINCT)] for i in range(p["n"])]
        out["ld"] = ops.ld_fold_multi(x["ld0"].clone(), terms, sc.ld_fold_negate(p["n"], p["signs"]))
    elif k == "inv1x1_conv":
        if p["variant"] == "t":
            out["y"] = ops.inv1x1_conv_t(x["z"], x["W"])
        else:
            out["y"], out["lds"] = ops.inv1x1_conv(x["z"], x["W"], x["ldu"], logdet=view, acc=code, want_scalar=True, bias=x["bias"])
            if view is not None:
                out["ld"] = view
    elif k == "inv1x1_wgrad":
        out["gW"], out["gl"] = ops.inv1x1_wgrad(x["z"], x["gy"], x["gld"])
    else:
        raise KeyError(k)
    if buf is not None:
        assert bool(torch.isnan(buf[:PAD]).all()) and bool(torch.isnan(buf[-PAD:]).all()), "%s: a write outside the accumulator's rows" % c
    return {name: t.detach() for name, t in out.items()}


def last_sweep(c):
    """(first row of the last sweep, or the last row of a single sweep; the row-carrying inputs) for the row-isolation check."""
    loop, names = sc.ROW_WISE[c.kernel]
    pl = c.plans()[loop]
    B = c.p["B"]
    lo = (pl.sweeps - 1) * pl.per_sweep if pl.sweeps > 1 else B - 1
    assert 0 <= lo < B, (c, pl)
    if c.kernel == "rows" and not c.p["labels"]:
        names = names + ("loc", "ls")        # (without labels sample b reads parameter row b)
    return lo, names


@pytest.mark.parametrize("c", sc.CASES, ids=lambda c: c.id)
def test_stream_kernel(nfa, c):
    x, ref, yard = c.evaluate()
    xd = valid = dev(x)
    if c.p.get("bad_labels"):            # the two named rows: labels -1 and num_rows
        xd = dict(valid, idx=valid["idx"].clone())
        xd["idx"][sc.bad_label_rows(c.p["B"])[0]], xd["idx"][sc.bad_label_rows(c.p["B"])[1]] = -1, sc.ROWS_CLASSES
    got = run(nfa, c, xd)
    again = run(nfa, c, xd)
    kinds = sc.KIND[c.kernel]
    assert set(got) <= set(ref) and set(got) >= {n for n in ref if n not in ("ld", "lds", "y")}, (set(got), set(ref))
    for name, g in got.items():
        assert g.dtype == sc.DT[c.dtype], (c, name, g.dtype)
        assert same(g, again[name]), "%s %s: two calls differ" % (c, name)                                    # (b)
        g, r = g.cpu(), ref[name]
        assert g.shape == r.shape, (c, name, g.shape, r.shape)
        if kinds[name] == "exact":                                                                            # (d)
            want = (yard if yard is not None else ref)[name]
            assert torch.equal(g, want), "%s %s: %d elements differ from the formula's bits" % (c, name, int((g != want).sum()))
            continue
        assert torch.equal(torch.isnan(g), torch.isnan(r)) and torch.equal(torch.isinf(g), torch.isinf(r)), \
            "%s %s: NaN / Inf pattern differs from the reference's" % (c, name)
        err = sc.scaled_error(g, r, kinds[name], c.dtype)                                                     # (a)
        yerr = sc.scaled_error(yard[name], r, kinds[name], c.dtype) if yard is not None else 0.0
        bar = sc.allowed(yerr, c.dtype)
        print("STREAM %s %s %s err/bar %.4f err/yardstick %s" % (c.kernel, c.id, name, err / bar, "%.3f" % (err / yerr) if yerr > 0 else "-"))
        assert err <= bar, "%s %s: error %.3f x the existing bar, allowed %.3f (float32 yardstick %.3f)" % (c, name, err, bar, yerr)
    if c.p.get("bad_labels"):
        # every row but the two with an out-of-range label equals, bit for bit, the call with valid labels there
        valid = run(nfa, c, valid)["lp"]
        bad = list(sc.bad_label_rows(c.p["B"]))
        keep = torch.ones(c.p["B"], dtype=torch.bool, device=DEV)
        keep[bad] = False
        assert bool(torch.isnan(got["lp"][bad]).all()) and not bool(torch.isnan(valid).any())
        assert torch.equal(got["lp"][keep], valid[keep])
    if c.kernel in sc.ROW_WISE:                                                                               # (c)
        lo, names = last_sweep(c)
        xs = {k: (v[lo:].contiguous() if k in names and v is not None else v) for k, v in xd.items()}
        fresh = run(nfa, c, xs)
        for name, g in got.items():
            if g.dim() >= 1:
                assert same(g[lo:], fresh[name]), "%s %s: rows [%d, %d) differ from a fresh call on them" % (c, name, lo, c.p["B"])
