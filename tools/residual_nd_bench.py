#!/usr/bin/env python3
"""A/B of the d-dimensional residual-flow kernels (config.residual_nd) on an MI355X.  Writes profiles/residual_nd_bench.json.

Model: 16 x [Residual(LipschitzMLP([d, 128, 128, d])), ActNorm(d)] in evaluation mode, at the Lipschitz cap (weights and biases times
3, 50 power iterations), d = 8 and d = 64.  Legs under no_grad, eager: `log_prob` and `sample` (forward_and_log_det on noise) at
1 024 and 65 536 rows.  off = config.set_residual_nd(False): the torch formulas -- the parent commit's behaviour and the reference's
arithmetic, one autograd pass through the network per series term; on = the kernels of csrc/lipmlp_nd.hip.  Both legs draw their
truncations and noise themselves (np.random / torch seeded once per leg), so the number of series terms varies from call to call the
same way in both.  Switch off / on alternate over --rounds rounds in ONE process; every call between its own pair of device
events; medians and minima.

    timeout -k 10 1100 python tools/residual_nd_bench.py

Every leg's first call is its warm-up and is timed with the host's wall clock between two synchronisations; a leg whose first call
takes longer than --slow-seconds is not repeated: that one wall-clock time stands for it, marked `timed_once` with a `clock` note
(it includes one-time packing and library warm-up; every other figure is device-event time of warm calls)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def timed_steps(torch, fn, steps):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    torch.cuda.synchronize()
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def model(nfa, torch, dev, d):
    torch.manual_seed(0)
    flows = []
    for _ in range(16):
        flows.append(nfa.flows.Residual(nfa.nets.LipschitzMLP([d, 128, 128, d], init_zeros=False, lipschitz_const=0.9)))
        flows.append(nfa.flows.ActNorm(d))
    m = nfa.NormalizingFlow(nfa.distributions.DiagGaussian(d, trainable=False), flows).eval()
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, nfa.nets.InducedNormLinear):
                mod.weight.mul_(3.0)
                mod.bias.mul_(3.0)
            elif isinstance(mod, nfa.flows.ActNorm):
                mod.data_dep_init_done.fill_(1.0)
    nfa.utils.update_lipschitz(m, 50)
    return m.to(dev)


def summary(times):
    return {"median_ms": statistics.median(times), "min_ms": min(times), "calls": len(times)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--dims", type=int, nargs="*", default=[8, 64])
    ap.add_argument("--batches", type=int, nargs="*", default=[1024, 65536])
    ap.add_argument("--slow-seconds", type=float, default=60.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "residual_nd_bench.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import normflows_amd as nfa
    dev = torch.device("cuda:0")
    out = {"workload": "device-event times in ms per call under no_grad of 16 x [Residual([d,128,128,d]), ActNorm(d)] in eval mode at the "
                       "Lipschitz cap; off = config.set_residual_nd(False): the torch formulas (the parent commit's route); on = the "
                       "kernels of csrc/lipmlp_nd.hip",
           "clock": "device events around each warm call; a leg marked timed_once carries its own clock note",
           "rounds": args.rounds, "steps": args.steps, "device": torch.cuda.get_device_name(0), "cases": {}}
    for d in args.dims:
        m = model(nfa, torch, dev, d)
        for B in args.batches:
            x = (torch.randn(B, d, generator=torch.Generator().manual_seed(2)) * 1.5).to(dev)

            def log_prob():
                with torch.no_grad():
                    return m.log_prob(x)

            def sample():
                with torch.no_grad():
                    return m.forward_and_log_det(x)

            for leg, fn in (("log_prob", log_prob), ("sample", sample)):
                times, once = {"off": [], "on": []}, {}
                for key, sw in (("off", False), ("on", True)):      # the first call: the warm-up, and the test for a leg too slow to repeat
                    nfa.config.set_residual_nd(sw)
                    np.random.seed(1)
                    torch.manual_seed(1)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    wall = time.perf_counter() - t0
                    if wall > args.slow_seconds:
                        once[key] = wall * 1e3
                for _ in range(args.rounds):
                    for key, sw in (("off", False), ("on", True)):
                        if key in once:
                            continue
                        nfa.config.set_residual_nd(sw)
                        times[key].extend(timed_steps(torch, fn, args.steps))
                r = {}
                for key in ("off", "on"):
                    r[key] = ({"median_ms": once[key], "min_ms": once[key], "calls": 1, "timed_once": True,
                               "clock": "host wall clock around the leg's FIRST call, synchronised on both sides; it includes the one-time "
                                        "packing and library warm-up; no device events"} if key in once
                              else summary(times[key]))
                r["speedup_median"] = r["off"]["median_ms"] / r["on"]["median_ms"]
                out["cases"]["d%d B%d %s" % (d, B, leg)] = r
                print("d = %d B = %d %s: %s" % (d, B, leg, json.dumps(r)), flush=True)
                with open(args.out, "w") as f:          # (kept current: a run cut short still leaves what it measured)
                    json.dump(out, f, indent=1, sort_keys=True)
        del m
    nfa.config.set_residual_nd(False)
    out["on_faster_everywhere"] = all(c["on"]["median_ms"] < c["off"]["min_ms"] for c in out["cases"].values())
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
