#!/usr/bin/env python3
"""Forward + backward of ONE circular NSF coupling layer in the density direction (D 64, hidden 256, K 8, 32 circular features,
B 65 536), timed in one process with device events, the variants alternating round by round:
  (a) config.nsf_circular_train off: eager torch modules for the conditioner (indexing, sin / cos, cat, one library GEMM per Linear)
      + nf_rqs_coupling_bwd_ft for the spline's backward (the path before this switch: the yardstick);
  (b) config.nsf_circular_train on : autograd.ResNetFtFn (nf_made_forward_train_ft, nf_made_backward, nf_made_feed_ft_bwd,
      nf_made_wgrad) + nf_rqs_coupling_bwd_ft_wave;
  (c) the linear-tails CoupledRationalQuadraticSpline(64, 2, 256) on its existing route (23 instead of 25 rows per feature, no feed:
      what (b) is recorded against, not gated).
The spline's backward alone, on the same tensors: nf_rqs_coupling_bwd_ft_wave (`wave`) against nf_rqs_coupling_bwd_ft (`elementwise`);
every element of gx on which the two differ by more than 1e-4 of scale is listed with its distance to the nearest knot of its own spline.
Peak memory of a step per variant; (a) and (b) are also compared on the same weights (faster and different is not faster).
    python tools/circ_coupled_train_bench.py [--out profiles/circ_coupled_train_bench.json] [--rounds 5] [--iters 10]
Needs an MI355X: it fails without one."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import normflows_amd as nfa  # noqa: E402

DEV = "cuda:0"
D, H, K, B = 64, 256, 8, 65536


def build():
    torch.manual_seed(0)
    circ = nfa.flows.CircularCoupledRationalQuadraticSpline(D, 2, H, ind_circ=list(range(0, D, 2)), num_bins=K, tail_bound=3.0,
                                                            init_identity=False).to(DEV)
    lin = nfa.flows.CoupledRationalQuadraticSpline(D, 2, H, num_bins=K, tail_bound=3.0, init_identity=False).to(DEV)
    with torch.no_grad():
        for m in (circ, lin):
            for p in m.parameters():
                p.add_(0.01 * torch.randn_like(p))
    return circ, lin


def knot_gap(x, raw, tb, inverse, min_bin=1e-3):
    """Distance of each x (n,) to the nearest INTERIOR knot of its own spline on the searched axis, as a fraction of the bound tb (n,),
    in float64.  raw (n, 2 K): the element's unnormalised widths | heights as the softmax sees them (already divided by wh_div); the
    forward spline searches the widths' knots, the inverse the heights' (utils/splines.py:127-157).  The log-det's x-derivative
    jumps at a knot, so two float32 kernels that round the knots differently may take either one-sided value for an x this close."""
    K = raw.shape[1] // 2
    r = raw.double()[:, K:] if inverse else raw.double()[:, :K]
    p = min_bin + (1.0 - min_bin * K) * torch.softmax(r, dim=1)
    tb = tb.double()
    knots = 2.0 * tb[:, None] * torch.cumsum(p, dim=1)[:, :K - 1] - tb[:, None]
    return (x.double()[:, None] - knots).abs().min(dim=1).values / tb


def far_elements(ga, gb, x, cond, uw, uh, iidx, tidx, bound_i, bound_t, wh_div, inverse, bar=1e-4):
    """The elements of two gx results (B, D) further apart than `bar` of scale: (rows, cols, knot gaps, is-identity flags)."""
    scale = max(1.0, float(gb.abs().max()))
    rows, cols = torch.nonzero((ga - gb).abs() > bar * scale, as_tuple=True)
    gaps = torch.zeros(rows.numel(), dtype=torch.float64, device=x.device)
    ident = torch.zeros(rows.numel(), dtype=torch.bool, device=x.device)
    for k in range(rows.numel()):
        b, c = int(rows[k]), int(cols[k])
        hit = torch.nonzero(iidx == c)
        if hit.numel():
            j = int(hit[0])
            ident[k] = True
            if uw is None:
                continue
            raw, tb = torch.cat([uw[j], uh[j]])[None], bound_i[j:j + 1]
        else:
            j = int(torch.nonzero(tidx == c)[0])
            raw, tb = cond.view(x.shape[0], -1, cond.numel() // (x.shape[0] * tidx.numel()))[b, j, :16][None] / wh_div, bound_t[j:j + 1]
        gaps[k] = knot_gap(x[b, c:c + 1], raw, tb, inverse)[0]
    return rows, cols, gaps, ident


KNOT_ROUNDING = 4e-6     # of the bound: a knot is a sum of <= 8 float32 terms of magnitude <= 2 tb behind a softmax through 1-ulp
                         # exponentials and reciprocals, in either kernel: about 16 roundings of 2.4e-7 tb


def timed(variants, rounds, iters):
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(rounds):                      # alternating: other work shares the machine
        for k, fn in variants.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(iters):
                fn()
            e.record()
            torch.cuda.synchronize()
            times[k].append(s.elapsed_time(e) / iters)
    return {k: {"median": sorted(v)[len(v) // 2], "min": min(v), "max": max(v)} for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "circ_coupled_train_bench.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--only", default=None, help="a | b | c: run that variant alone (kernel traces)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("circ_coupled_train_bench: no GPU")
    circ, lin = build()
    x = ((torch.rand(B, D, generator=torch.Generator().manual_seed(1)) * 2 - 1) * 2.9).to(DEV)
    cz, cl = torch.randn(B, D, device=DEV), torch.randn(B, device=DEV)

    def step(layer, on):
        nfa.config.set_nsf_circular_train(on)
        layer.zero_grad(set_to_none=True)
        xx = x.clone().requires_grad_(True)
        z, ld = layer.inverse(xx)
        ((z * cz).sum() + (ld * cl).sum()).backward()
        return z.detach(), ld.detach(), xx.grad, [p.grad for p in layer.parameters()]

    variants = {"a": lambda: step(circ, False), "b": lambda: step(circ, True), "c": lambda: step(lin, True)}
    if args.only:
        variants = {args.only: variants[args.only]}
    res = {"shape": {"D": D, "hidden": H, "K": K, "circular": D // 2, "B": B, "rounds": args.rounds, "iters": args.iters},
           "ms": timed(variants, args.rounds, args.iters)}
    peak = {}
    for k, fn in variants.items():
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        peak[k] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
    res["peak_step_MiB"] = peak
    rel = lambda p, q: float((p - q).abs().max()) / max(1.0, float(q.abs().max()))      # noqa: E731

    if "a" in variants and "b" in variants:
        ra, rb = variants["a"](), variants["b"]()
        res["b_vs_a"] = {"z": rel(rb[0], ra[0]), "ld": rel(rb[1], ra[1]), "gx": rel(rb[2], ra[2]),
                         "params": max(rel(p, q) for p, q in zip(rb[3], ra[3]))}
        res["b_over_a"] = res["ms"]["b"]["median"] / res["ms"]["a"]["median"]
        res["b_median_below_a_min"] = res["ms"]["b"]["median"] < res["ms"]["a"]["min"]
    if "b" in variants and "c" in variants:
        res["b_over_c"] = res["ms"]["b"]["median"] / res["ms"]["c"]["median"]
    nfa.config.set_nsf_circular_train(True)
    if not args.only:
        # the spline's backward alone, on the layer's own operands
        p = circ.prqct
        u = p.unconditional_transform
        kw = p._kernel_kwargs()
        with torch.no_grad():
            cond = p.transform_net(x.index_select(1, p.identity_features)).contiguous()
        ops_args = (x, cz, cl, cond, u.unnormalized_widths.detach(), u.unnormalized_heights.detach(), u.unnormalized_derivatives.detach(),
                    p.identity_features, p.transform_features, K, 0)
        kernels = {"elementwise": lambda: nfa.ops.rqs_coupling_bwd(*ops_args, **kw),
                   "wave": lambda: nfa.ops.rqs_coupling_bwd(*ops_args, ft_wave=True, **kw)}
        res["spline_bwd_ms"] = timed(kernels, args.rounds, args.iters)
        ge, gw = kernels["elementwise"](), kernels["wave"]()
        names = ("gx", "gcond", "guw", "guh", "gud")
        res["wave_vs_elementwise"] = {k: rel(a, b) for k, a, b in zip(names, gw, ge)}
        # attribution of the large differences: every element of gx beyond 1e-4 of scale, with its distance to a knot of its own spline
        ones = lambda n: torch.full((n,), float(kw["tail_bound"]), device=DEV) if "tail_bound" in kw else None      # noqa: E731
        bi = kw.get("bound_i", ones(p.identity_features.numel()))
        bt = kw.get("bound_t", ones(p.transform_features.numel()))
        rows, cols, gaps, ident = far_elements(gw[0], ge[0], x, cond, ops_args[4], ops_args[5], p.identity_features, p.transform_features,
                                               bi, bt, kw["wh_div"], False)
        res["gx_elements_beyond_1e-4"] = [
            {"row": int(r), "column": int(c), "x": float(x[r, c]), "wave": float(gw[0][r, c]), "elementwise": float(ge[0][r, c]),
             "knot_gap_of_bound": float(g), "identity_half": bool(i)} for r, c, g, i in zip(rows[:32], cols[:32], gaps[:32], ident[:32])]
        res["gx_elements_beyond_1e-4_count"] = int(rows.numel())
        res["gx_elements_total"] = int(x.numel())
        res["all_of_them_within_knot_rounding"] = bool((gaps <= KNOT_ROUNDING).all())
        keep = torch.ones(B, dtype=torch.bool, device=DEV)
        keep[rows] = False
        res["wave_vs_elementwise_other_rows"] = {"gx": rel(gw[0][keep], ge[0][keep]), "gcond": rel(gw[1][keep], ge[1][keep])}
        res["wave_over_elementwise"] = res["spline_bwd_ms"]["wave"]["median"] / res["spline_bwd_ms"]["elementwise"]["median"]
        res["wave_median_below_elementwise_min"] = res["spline_bwd_ms"]["wave"]["median"] < res["spline_bwd_ms"]["elementwise"]["min"]
    print(json.dumps(res))
    if not args.only:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
