#!/usr/bin/env python3
"""A/B of the stochastic-layer kernels (config.stochastic_kernels) on an MI355X.  Writes profiles/stochastic_bench.json.

Cases, eager at 1 024 and 65 536 rows: a HamiltonianMonteCarlo layer with 5 leapfrog steps against TwoModes(2, 0.1) and against
CircularGaussianMixture(8); a MetropolisHastings layer with 10 steps (DiagGaussianProposal) against TwoModes; a 10-layer HAIS chain
from a DiagGaussian prior to TwoModes (`sample`).  Legs: `forward` under no_grad (the layer draws its own random numbers: both routes
make the same draws), and for the HMC layers `fwd_bwd_params` = forward plus backward to log_step_size / log_mass.  The
explicit-noise transitions (`_transition`, no draws) replayed from a captured graph over --sweep.  off =
config.set_stochastic_kernels(False): the torch formulas, the reference's arithmetic op for op (the parent commit cannot run these
classes at all); on = nf_hmc2d / nf_mh2d.  Switch off / on alternate over --rounds rounds in ONE process; every step between its own
pair of device events; median and minimum.

    timeout -k 10 900 python tools/stochastic_bench.py

`default_on_criterion`: the eager `on` median below the eager `off` minimum in every case.  `graph_not_slower_from`: the first swept
size from which every replayed transition `on` is not slower than `off` at every larger swept size."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from rank1_bench import captured, summary, timed_steps  # noqa: E402

LSS, LM = (-2.6, -2.9), (0.1, -0.2)


def layers(nfa, torch, dev):
    D, F = nfa.distributions, nfa.flows

    def hmc(target):
        return F.HamiltonianMonteCarlo(target, 5, torch.tensor(LSS), torch.tensor(LM)).to(dev)
    return {"hmc5_two_modes": hmc(D.TwoModes(2.0, 0.1)), "hmc5_circ_gmm_8": hmc(D.CircularGaussianMixture(8)),
            "mh10_two_modes": F.MetropolisHastings(D.TwoModes(2.0, 0.1), D.DiagGaussianProposal((2,), 0.1), 10).to(dev)}


def ab(nfa, torch, legs, rounds, steps):
    """{off / on: {leg: summary}} of `legs` = {leg: fn}, the switch alternating over the rounds."""
    times = {key: {leg: [] for leg in legs} for key in ("off", "on")}
    for _ in range(rounds):
        for key, sw in (("off", False), ("on", True)):
            nfa.config.set_stochastic_kernels(sw)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stochastic_bench.json"))
    args = ap.parse_args()
    import torch
    sys.path.insert(0, ROOT)
    import normflows_amd as nfa
    dev = torch.device("cuda:0")
    default = nfa.config.stochastic_kernels
    out = {"workload": "device-event times in ms; off = config.set_stochastic_kernels(False): the torch formulas (the reference's "
                       "arithmetic); on = nf_hmc2d / nf_mh2d, one launch per layer call",
           "rounds": args.rounds, "steps": args.steps, "device": torch.cuda.get_device_name(0), "eager": {}, "graph": {},
           "not_measured": ["the reference itself (it does not exist on the GPU machine; off is its arithmetic in this package)",
                            "targets other than TwoModes and CircularGaussianMixture(8)", "max_abs_grad set",
                            "a NormalizingFlow that interleaves coupling layers with stochastic layers",
                            "the backward to z (only the backward to log_step_size / log_mass is timed)"]}
    crit = {}
    models = layers(nfa, torch, dev)
    prior = nfa.distributions.DiagGaussian(2, trainable=False).to(dev)
    hais = nfa.HAIS(torch.linspace(1.0, 0.0, 12), prior, nfa.distributions.TwoModes(2.0, 0.1), 5, torch.exp(torch.tensor(LSS)).to(dev),
                    torch.tensor(LM).to(dev))
    assert len(hais.layers) == 10
    for B in args.batches:
        z = (1.5 * torch.randn(B, 2, generator=torch.Generator().manual_seed(2))).to(dev)
        res = {}
        for name, layer in models.items():
            def forward(layer=layer):
                with torch.no_grad():
                    return layer(z)

            def fwd_bwd(layer=layer):
                layer.zero_grad(set_to_none=True)
                z_out, log_det = layer(z)
                (z_out.sum() + log_det.sum()).backward()

            legs = {"forward": forward}
            if name.startswith("hmc"):
                legs["fwd_bwd_params"] = fwd_bwd
            res[name] = ab(nfa, torch, legs, args.rounds, args.steps)

        def hais_sample():
            with torch.no_grad():
                return hais.sample(B)
        res["hais10_two_modes"] = ab(nfa, torch, {"forward": hais_sample}, args.rounds, args.steps)
        for name, r in res.items():
            for leg in r["speedup_median"]:
                crit["%s %d %s" % (name, B, leg)] = r["on"][leg]["median_ms"] < r["off"][leg]["min_ms"]
            print("%s B = %d: %s" % (name, B, json.dumps(r["speedup_median"])), flush=True)
        out["eager"][str(B)] = res

    # the explicit-noise transitions replayed from a graph
    for B in args.sweep:
        g = torch.Generator().manual_seed(3)
        z = (1.5 * torch.randn(B, 2, generator=g)).to(dev)
        eps, u = torch.randn(B, 2, generator=g).to(dev), torch.rand(B, generator=g).to(dev)
        eps10, u10 = torch.randn(10, B, 2, generator=g).to(dev), torch.rand(10, B, generator=g).to(dev)
        res = {}
        for name, layer in models.items():
            noise = (eps10, u10) if name.startswith("mh") else (eps, u)

            def step(layer=layer, noise=noise):
                with torch.no_grad():
                    return layer._transition(z, *noise)

            graphs, errors = {}, {}
            for key, sw in (("off", False), ("on", True)):
                nfa.config.set_stochastic_kernels(sw)
                graphs[key], err = captured(torch, step, step)
                if err:
                    errors[key] = err
            times = {"off": [], "on": []}
            for _ in range(args.rounds):
                for key in ("off", "on"):
                    if graphs[key] is not None:
                        times[key].extend(timed_steps(torch, graphs[key].replay, args.steps))
            r = {key: summary(t) for key, t in times.items() if t}
            if "off" in r and "on" in r:
                r["speedup_median"] = r["off"]["median_ms"] / r["on"]["median_ms"]
            if errors:
                r["graph_errors"] = errors
            res[name] = r
            del graphs
        print("graph B = %d: %s" % (B, json.dumps({k: v.get("speedup_median") for k, v in res.items()})), flush=True)
        out["graph"][str(B)] = res
    sizes = sorted(int(B) for B in out["graph"])
    ok = [B for B in sizes if all(r.get("speedup_median", 0.0) >= 1.0 for b in sizes if b >= B for r in out["graph"][str(b)].values())]
    out["graph_not_slower_from"] = ok[0] if ok else None
    out["smallest_swept_size"] = min(args.sweep) if args.sweep else None
    out["default_on_criterion"] = {"holds": all(crit.values()), "cases": crit}
    nfa.config.set_stochastic_kernels(default)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print("default-on criterion holds:", out["default_on_criterion"]["holds"], "| graph_not_slower_from:", out["graph_not_slower_from"])
    print("wrote", args.out)


if __name__ == "__main__":
    main()
