#!/usr/bin/env python3
"""A/B of the residual-flow kernels (config.residual_chain) on an MI355X.  Writes profiles/residual_bench.json.

Model (the reference's examples/residual.ipynb): 16 x [Residual(LipschitzMLP([2, 128, 128, 2])), ActNorm(2)] in evaluation mode, at
the Lipschitz cap (weights and biases times 3, 50 power iterations).  Legs under no_grad: `log_prob` at 1 024 and 65 536 rows and
`sample` at 1 024 rows, eager; `log_prob` also replayed from a captured graph over the sweep 1 024 .. 65 536 rows.  off =
config.set_residual_chain(False): the torch formulas, the reference's arithmetic op for op; on = the kernels.  The parent commit
cannot run this model at all and the reference does not run here: the switch-off route IS the baseline.  Switch off / on alternate
over --rounds rounds in ONE process; every call between its own pair of device events; medians and minima.

    timeout -k 10 900 python tools/residual_bench.py

`default_on_criterion`: the eager `on` median below the eager `off` minimum in every eager case.  `graph_not_slower_from`: the first
swept size from which the replayed `on` is not slower than the replayed `off` at every larger swept size (None: never, or the off
route could not be captured)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def timed_steps(torch, fn, steps):
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
    """fn recorded into a graph after a side-stream warm-up; (None, error) when the capture fails."""
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


def model(nfa, torch, dev):
    torch.manual_seed(0)
    flows = []
    for _ in range(16):
        flows.append(nfa.flows.Residual(nfa.nets.LipschitzMLP([2, 128, 128, 2], init_zeros=False, lipschitz_const=0.9)))
        flows.append(nfa.flows.ActNorm(2))
    m = nfa.NormalizingFlow(nfa.distributions.DiagGaussian(2, trainable=False), flows).eval()
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
    return {"median_ms": statistics.median(times), "min_ms": min(times)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--batches", type=int, nargs="*", default=[1024, 65536])
    ap.add_argument("--sample-batch", type=int, default=1024)
    ap.add_argument("--sweep", type=int, nargs="*", default=[1024, 2048, 4096, 8192, 16384, 32768, 65536])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "residual_bench.json"))
    args = ap.parse_args()
    import torch
    sys.path.insert(0, ROOT)
    import normflows_amd as nfa
    dev = torch.device("cuda:0")
    m = model(nfa, torch, dev)
    out = {"workload": "device-event times in ms per call under no_grad of the 16 x [Residual([2,128,128,2]), ActNorm] example model in "
                       "eval mode; off = config.set_residual_chain(False): the torch formulas; on = the kernels of csrc/lipmlp.hip",
           "rounds": args.rounds, "steps": args.steps, "device": torch.cuda.get_device_name(0), "log_prob": {}, "sample": {}}
    for B in sorted(set(args.batches) | set(args.sweep)):
        x = (torch.randn(B, 2, generator=torch.Generator().manual_seed(2)) * 1.5).to(dev)

        def log_prob():
            with torch.no_grad():
                return m.log_prob(x)

        legs = {}
        for key, sw in (("off", False), ("on", True)):
            nfa.config.set_residual_chain(sw)
            log_prob()
            g, err = captured(torch, log_prob)
            legs[key] = {"errors": [err] if err else []}
            if B in args.batches:
                legs[key]["eager"] = (log_prob, [])
            if g is not None:
                legs[key]["graph"] = (g.replay, [])
        for _ in range(args.rounds):
            for key, sw in (("off", False), ("on", True)):
                nfa.config.set_residual_chain(sw)
                for leg, val in legs[key].items():
                    if leg != "errors":
                        val[1].extend(timed_steps(torch, val[0], args.steps))
        r = {key: dict({leg: summary(val[1]) for leg, val in legs[key].items() if leg != "errors"},
                       **({"graph_errors": legs[key]["errors"]} if legs[key]["errors"] else {})) for key in ("off", "on")}
        r["speedup_median"] = {leg: r["off"][leg]["median_ms"] / r["on"][leg]["median_ms"]
                               for leg in ("eager", "graph") if leg in r["on"] and leg in r["off"]}
        out["log_prob"][str(B)] = r
        print("log_prob B = %d: %s" % (B, json.dumps(r)), flush=True)
        del legs
    B = args.sample_batch
    zs = torch.randn(B, 2, generator=torch.Generator().manual_seed(3)).to(dev)

    def sample():
        with torch.no_grad():
            return m.forward_and_log_det(zs)

    times = {"off": [], "on": []}
    for _ in range(args.rounds):
        for key, sw in (("off", False), ("on", True)):
            nfa.config.set_residual_chain(sw)
            times[key].extend(timed_steps(torch, sample, args.steps))
    out["sample"][str(B)] = {"off": {"eager": summary(times["off"])}, "on": {"eager": summary(times["on"])},
                             "speedup_median": {"eager": statistics.median(times["off"]) / statistics.median(times["on"])}}
    print("sample B = %d: %s" % (B, json.dumps(out["sample"][str(B)])), flush=True)
    crit = {}
    for B in args.batches:
        rb = out["log_prob"][str(B)]
        crit["log_prob %d eager" % B] = rb["on"]["eager"]["median_ms"] < rb["off"]["eager"]["min_ms"]
    rb = out["sample"][str(args.sample_batch)]
    crit["sample %d eager" % args.sample_batch] = rb["on"]["eager"]["median_ms"] < rb["off"]["eager"]["min_ms"]
    out["default_on_criterion"] = {"holds": all(crit.values()), "cases": crit}
    sizes = sorted(args.sweep)
    sp = {b: out["log_prob"][str(b)]["speedup_median"].get("graph") for b in sizes}
    ok = [b for b in sizes if all(sp[c] is not None and sp[c] >= 1.0 for c in sizes if c >= b)]
    out["graph_not_slower_from"] = ok[0] if ok else None
    out["smallest_swept_size"] = min(sizes)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print("default-on criterion holds:", out["default_on_criterion"]["holds"], "| graph_not_slower_from:", out["graph_not_slower_from"])
    print("wrote", args.out)


if __name__ == "__main__":
    main()
