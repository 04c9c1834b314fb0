#!/usr/bin/env python3
"""A/B of the residual-flow training kernels (config.residual_train) on an MI355X.  Writes profiles/residual_train_bench.json.

Model: the reference's example (residual.ipynb): 16 x [Residual(LipschitzMLP([2, 128, 128, 2])), ActNorm(2)] in training mode.
Variants: `default` (the Neumann estimator with the memory-saving wrapper and a random truncation: the host draws per layer, so it
is measured eager only) and `brute_force` (the exact determinant: eager, and replayed from a captured graph).  Step: forward_kld on
fixed rows + backward.  off = config.set_residual_train(False): every layer's torch formulas, the parent's behaviour and the
reference's arithmetic; on = one forward and one backward launch per Residual layer.  Switch off / on alternate over --rounds rounds
in ONE process; every step between its own pair of device events; median and minimum; and the peak memory of one step.

    timeout -k 10 900 python tools/residual_train_bench.py

`default_on_criterion`: the eager `on` median below the eager `off` minimum for both variants at every batch size (recorded for a
later change of the default; the switch stays off whatever this says)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def timed_steps(torch, fn, steps):
    """Per-step device times (ms) of `steps` calls of fn, each between its own pair of events."""
    for _ in range(2):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    torch.cuda.synchronize()
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def captured(torch, fn):
    """fn recorded into a graph after the usual side-stream warm-up; None (and the error) when the capture fails."""
    try:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                fn()
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fn()
        return g, None
    except Exception as e:          # noqa: BLE001  (capture is reported, not required)
        torch.cuda.synchronize()
        return None, "%s: %s" % (type(e).__name__, str(e)[:200])


def model(nfa, torch, dev, **kw):
    torch.manual_seed(0)
    flows = []
    for _ in range(16):
        flows.append(nfa.flows.Residual(nfa.nets.LipschitzMLP([2, 128, 128, 2], init_zeros=True, lipschitz_const=0.9), **kw))
        flows.append(nfa.flows.ActNorm(2))
    return nfa.NormalizingFlow(nfa.distributions.DiagGaussian(2, trainable=False), flows).to(dev).train()


def summary(times):
    return {"median_ms": statistics.median(times), "min_ms": min(times)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--batches", type=int, nargs="*", default=[1024, 65536])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "residual_train_bench.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import normflows_amd as nfa
    dev = torch.device("cuda:0")
    out = {"workload": "device-event times in ms per training step (forward_kld + backward) of 16 x [Residual([2,128,128,2]), ActNorm]; "
                       "off = config.set_residual_train(False): the torch formulas; on = csrc/lipmlp_train.hip",
           "rounds": args.rounds, "steps": args.steps, "device": torch.cuda.get_device_name(0), "variants": {}}
    crit = {}
    for variant, kw in (("default", {}), ("brute_force", {"brute_force": True})):
        np.random.seed(0)
        m = model(nfa, torch, dev, **kw)
        res = {}
        for B in args.batches:
            x = (torch.randn(B, 2, generator=torch.Generator().manual_seed(2)) * 1.5).to(dev)

            def step():
                m.zero_grad(set_to_none=True)
                m.forward_kld(x).backward()

            legs = {}
            for key, sw in (("off", False), ("on", True)):
                nfa.config.set_residual_train(sw)
                step()                      # (the first one also initialises the ActNorm layers)
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                step()
                torch.cuda.synchronize()
                legs[key] = {"step_eager": (step, []), "peak_step_bytes": torch.cuda.max_memory_allocated() - base, "errors": []}
                if variant == "brute_force":
                    g, err = captured(torch, step)
                    if g is not None:
                        legs[key]["step_graph"] = (g.replay, [])
                    else:
                        legs[key]["errors"].append(err)
            for _ in range(args.rounds):
                for key, sw in (("off", False), ("on", True)):
                    nfa.config.set_residual_train(sw)
                    for leg in ("step_eager", "step_graph"):
                        if leg in legs[key]:
                            legs[key][leg][1].extend(timed_steps(torch, legs[key][leg][0], args.steps))
            nfa.config.set_residual_train(False)
            r = {}
            for key in ("off", "on"):
                r[key] = {leg: summary(legs[key][leg][1]) for leg in ("step_eager", "step_graph") if leg in legs[key]}
                r[key]["peak_step_bytes"] = legs[key]["peak_step_bytes"]
                if legs[key]["errors"]:
                    r[key]["graph_errors"] = legs[key]["errors"]
            r["speedup_median"] = {leg: r["off"][leg]["median_ms"] / r["on"][leg]["median_ms"]
                                   for leg in ("step_eager", "step_graph") if leg in r["on"] and leg in r["off"]}
            res[str(B)] = r
            crit["%s %d step_eager" % (variant, B)] = r["on"]["step_eager"]["median_ms"] < r["off"]["step_eager"]["min_ms"]
            print("%s B = %d: %s" % (variant, B, json.dumps(r)), flush=True)
            del legs
        out["variants"][variant] = {"batches": res}
    out["default_on_criterion"] = {"holds": all(crit.values()), "cases": crit}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print("default-on criterion holds:", out["default_on_criterion"]["holds"])
    print("wrote", args.out)


if __name__ == "__main__":
    main()
