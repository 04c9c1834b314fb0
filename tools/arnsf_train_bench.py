#!/usr/bin/env python3
"""Forward + backward of ONE circular, mask-permuted autoregressive spline layer in the density direction (D 64, hidden 256, K 8, 8
circular columns, B 65 536), timed three ways in one process with device events, the variants alternating round by round:
  (a) config.arnsf_train_ft off: eager MaskedLinear modules + torch.sin / torch.cos in front of SplineFn (the path before MadeFtFn);
  (b) config.arnsf_train_ft on : autograd.MadeFtFn (nf_made_forward_train_ft, nf_made_backward, nf_made_feed_ft_bwd, nf_made_wgrad);
  (c) the unpermuted linear-tails AutoregressiveRationalQuadraticSpline(64, 2, 256) through autograd.MadeFn (23 instead of 25 rows
      per feature, no feed, no gather: the yardstick (b) is recorded against, not gated).
Peak memory of a step per variant; (a) and (b) are also compared on the same weights (faster and different is not faster).
    python tools/arnsf_train_bench.py [--out profiles/circ_arnsf_train_bench.json] [--rounds 5] [--iters 10]
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
    circ = nfa.flows.CircularAutoregressiveRationalQuadraticSpline(D, 2, H, ind_circ=list(range(0, D, 8)), num_bins=K, tail_bound=3.0,
                                                                   permute_mask=True, init_identity=False).to(DEV)
    lin = nfa.flows.AutoregressiveRationalQuadraticSpline(D, 2, H, num_bins=K, tail_bound=3.0, init_identity=False).to(DEV)
    with torch.no_grad():
        for m in (circ, lin):
            for p in m.parameters():
                p.add_(0.01 * torch.randn_like(p))
    return circ, lin


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "circ_arnsf_train_bench.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--only", default=None, help="a | b | c: run that variant alone (kernel traces)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("arnsf_train_bench: no GPU")
    circ, lin = build()
    x = ((torch.rand(B, D, generator=torch.Generator().manual_seed(1)) * 2 - 1) * 2.9).to(DEV)
    cz, cl = torch.randn(B, D, device=DEV), torch.randn(B, device=DEV)

    def step(layer, ft):
        nfa.config.set_arnsf_train_ft(ft)
        layer.zero_grad(set_to_none=True)
        xx = x.clone().requires_grad_(True)
        z, ld = layer.inverse(xx)
        ((z * cz).sum() + (ld * cl).sum()).backward()
        return z.detach(), ld.detach(), xx.grad, [p.grad for p in layer.parameters()]

    variants = {"a": lambda: step(circ, False), "b": lambda: step(circ, True), "c": lambda: step(lin, True)}
    if args.only:
        variants = {args.only: variants[args.only]}
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(args.rounds):                      # alternating: other work shares the machine
        for k, fn in variants.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(args.iters):
                fn()
            e.record()
            torch.cuda.synchronize()
            times[k].append(s.elapsed_time(e) / args.iters)
    peak = {}
    for k, fn in variants.items():
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        peak[k] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
    res = {"shape": {"D": D, "hidden": H, "K": K, "circular": D // 8, "B": B, "rounds": args.rounds, "iters": args.iters},
           "ms": {k: {"median": sorted(v)[len(v) // 2], "min": min(v), "max": max(v)} for k, v in times.items()},
           "peak_step_MiB": peak}
    if "a" in variants and "b" in variants:
        ra, rb = variants["a"](), variants["b"]()
        nfa.config.set_arnsf_train_ft(True)
        rel = lambda p, q: float((p - q).abs().max()) / max(1.0, float(q.abs().max()))
        res["b_vs_a"] = {"z": rel(rb[0], ra[0]), "ld": rel(rb[1], ra[1]), "gx": rel(rb[2], ra[2]),
                         "params": max(rel(p, q) for p, q in zip(rb[3], ra[3]))}
        res["b_over_a"] = res["ms"]["b"]["median"] / res["ms"]["a"]["median"]
    if "b" in variants and "c" in variants:
        res["b_over_c"] = res["ms"]["b"]["median"] / res["ms"]["c"]["median"]
    nfa.config.set_arnsf_train_ft(True)
    print(json.dumps(res))
    if not args.only:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
