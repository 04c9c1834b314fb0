#!/usr/bin/env python3
"""A/B of the target / prior / mixture density kernels (config.target_density) on an MI355X.  Writes profiles/target_bench.json.

Densities: TwoMoons, CircularGaussianMixture(8), RingMixture(2), Sinusoidal_gap(0.4, 4), GaussianMixture at (M, d) = (10, 2) and
(10, 64).  Legs, at 1 024 and 65 536 rows: `log_prob` under no_grad; value plus input gradient (sum(log_prob) backward to z); for
the mixtures also forward plus backward to the parameters, and the peak memory of that step at (10, 64).  A whole reverse-KL step
(32 tanh Planar layers, DiagGaussian base, TwoModes(2, 0.1) target, fixed base noise, forward + backward) eager at those two sizes
and replayed from a captured graph over --sweep.  off = config.set_target_density(False): the torch formulas, the reference's
arithmetic op for op (the parent commit cannot run these classes at all); on = the kernels.  Switch off / on alternate over
--rounds rounds in ONE process; every step between its own pair of device events; median and minimum.

    timeout -k 10 900 python tools/target_bench.py

`default_on_criterion`: the eager `on` median below the eager `off` minimum in every case.  `graph_not_slower_from`: the first swept
size from which the replayed reverse-KL step `on` is not slower than `off` at every larger swept size."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from rank1_bench import captured, summary, timed_steps  # noqa: E402

DENSITIES = ("two_moons", "circ_gmm_8", "ring_2", "sinusoidal_gap", "gmm_10_2", "gmm_10_64")


def density(nfa, torch, np, name, dev):
    D = nfa.distributions
    if name.startswith("gmm"):
        M, d = (int(v) for v in name.split("_")[1:])
        rs = np.random.RandomState(0)
        return D.GaussianMixture(M, d, loc=2 * rs.randn(M, d), scale=0.5 + rs.rand(M, d)).float().to(dev), d
    p = {"two_moons": D.TwoMoons, "circ_gmm_8": lambda: D.CircularGaussianMixture(8), "ring_2": lambda: D.RingMixture(2),
         "sinusoidal_gap": lambda: D.Sinusoidal_gap(0.4, 4)}[name]()
    return (p.to(dev) if isinstance(p, torch.nn.Module) else p), 2


def ab(nfa, torch, legs, rounds, steps):
    """{off / on: {leg: summary}} of `legs` = {leg: fn}, the switch alternating over the rounds."""
    times = {key: {leg: [] for leg in legs} for key in ("off", "on")}
    for _ in range(rounds):
        for key, sw in (("off", False), ("on", True)):
            nfa.config.set_target_density(sw)
            for leg, fn in legs.items():
                times[key][leg].extend(timed_steps(torch, fn, steps))
    r = {key: {leg: summary(t) for leg, t in times[key].items()} for key in times}
    r["speedup_median"] = {leg: r["off"][leg]["median_ms"] / r["on"][leg]["median_ms"] for leg in legs}
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batches", type=int, nargs="*", default=[1024, 65536])
    ap.add_argument("--sweep", type=int, nargs="*", default=[1024, 2048, 4096, 8192, 16384, 32768, 65536])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "target_bench.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import normflows_amd as nfa
    dev = torch.device("cuda:0")
    default = nfa.config.target_density
    out = {"workload": "device-event times in ms; off = config.set_target_density(False): the torch formulas (the reference's arithmetic); "
                       "on = nf_density2d / nf_gmm_log_prob(_bwd)",
           "rounds": args.rounds, "steps": args.steps, "device": torch.cuda.get_device_name(0), "densities": {}}
    crit = {}
    for name in DENSITIES:
        p, d = density(nfa, torch, np, name, dev)
        params = list(p.parameters()) if isinstance(p, torch.nn.Module) else []
        res = {}
        for B in args.batches:
            z = (2.5 * torch.randn(B, d, generator=torch.Generator().manual_seed(2))).to(dev)
            zg = z.clone().requires_grad_(True)

            def value():
                with torch.no_grad():
                    return p.log_prob(z)

            def value_and_gz():
                for q in params:
                    q.requires_grad_(False)
                zg.grad = None
                p.log_prob(zg).sum().backward()

            def to_params():
                for q in params:
                    q.requires_grad_(True)
                    q.grad = None
                p.log_prob(z).sum().backward()

            legs = {"log_prob": value, "value_and_gz": value_and_gz}
            if params:
                legs["fwd_bwd_params"] = to_params
            r = ab(nfa, torch, legs, args.rounds, args.steps)
            if name == "gmm_10_64":
                r["peak_memory_MiB_fwd_bwd_params"] = {}
                for key, sw in (("off", False), ("on", True)):
                    nfa.config.set_target_density(sw)
                    to_params()
                    torch.cuda.synchronize()
                    base = torch.cuda.memory_allocated()
                    torch.cuda.reset_peak_memory_stats()
                    to_params()
                    torch.cuda.synchronize()
                    r["peak_memory_MiB_fwd_bwd_params"][key] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
            for leg in legs:
                crit["%s %d %s" % (name, B, leg)] = r["on"][leg]["median_ms"] < r["off"][leg]["min_ms"]
            res[str(B)] = r
            print("%s B = %d: %s" % (name, B, json.dumps(r["speedup_median"])), flush=True)
        out["densities"][name] = res

    # a whole reverse-KL step: 32 tanh Planar layers against TwoModes
    torch.manual_seed(0)
    model = nfa.NormalizingFlow(nfa.distributions.DiagGaussian(2), [nfa.flows.Planar((2,)) for _ in range(32)],
                                nfa.distributions.TwoModes(2, 0.1)).to(dev)
    step_res = {}
    for B in sorted(set(args.batches) | set(args.sweep)):
        eps = torch.randn(B, 2, generator=torch.Generator().manual_seed(3)).to(dev)

        def step():
            model.zero_grad(set_to_none=True)
            model.reverse_kld(eps=eps).backward()

        graphs, errors = {}, {}
        for key, sw in (("off", False), ("on", True)):
            nfa.config.set_target_density(sw)
            step()
            model.zero_grad(set_to_none=True)
            graphs[key], err = captured(torch, step, step)
            if err:
                errors[key] = err
        times = {key: {"step_graph": [], "step_eager": []} for key in ("off", "on")}
        for _ in range(args.rounds):
            for key, sw in (("off", False), ("on", True)):
                nfa.config.set_target_density(sw)
                if B in args.batches:
                    times[key]["step_eager"].extend(timed_steps(torch, step, args.steps))
                if graphs[key] is not None:
                    times[key]["step_graph"].extend(timed_steps(torch, graphs[key].replay, args.steps))
        r = {key: {leg: summary(t) for leg, t in times[key].items() if t} for key in times}
        r["speedup_median"] = {leg: r["off"][leg]["median_ms"] / r["on"][leg]["median_ms"] for leg in r["on"] if leg in r["off"]}
        if errors:
            r["graph_errors"] = errors
        if B in args.batches:
            crit["reverse_kld_planar32 %d step_eager" % B] = r["on"]["step_eager"]["median_ms"] < r["off"]["step_eager"]["min_ms"]
        step_res[str(B)] = r
        print("reverse_kld planar32 B = %d: %s" % (B, json.dumps(r["speedup_median"])), flush=True)
        del graphs
    sizes = sorted(int(B) for B in step_res)
    ok = [B for B in sizes if all(step_res[str(b)]["speedup_median"].get("step_graph", 0.0) >= 1.0 for b in sizes if b >= B)]
    out["reverse_kld_planar32"] = {"batches": step_res}
    out["graph_not_slower_from"] = ok[0] if ok else None
    out["smallest_swept_size"] = min(args.sweep)
    out["default_on_criterion"] = {"holds": all(crit.values()), "cases": crit}
    nfa.config.set_target_density(default)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print("default-on criterion holds:", out["default_on_criterion"]["holds"], "| graph_not_slower_from:", out["graph_not_slower_from"])
    print("wrote", args.out)


if __name__ == "__main__":
    main()
