#!/usr/bin/env python3
"""A/B of the rank-1 chain kernels (config.rank1_chain) for Planar / Radial stacks on an MI355X.  Writes profiles/rank1_bench.json.

Models (the reference's examples): 32 tanh Planar at d = 2 (planar.ipynb), 16 Radial at d = 2, 16 tanh Planar at d = 40 (the VAE
latent).  Legs: `forward_and_log_det` under no_grad, and a reverse_kld-style step, loss = mean(|z'|^2 / 2 - log_det) of
forward_and_log_det on fixed base samples + backward.  At 1 024 and 65 536 rows eager and replayed from a captured graph; the
sizes in between (--sweep) replayed only.  off = config.set_rank1_chain(False): every layer's torch formulas, the reference's
arithmetic and what a user gets without the kernels; on = the kernels.  Switch off / on alternate over --rounds rounds in ONE
process; every step between its own pair of device events; median and minimum.

    timeout -k 10 900 python tools/rank1_bench.py

`default_on_criterion`: the eager `on` median below the eager `off` minimum at both sizes for all three models and both legs.
`graph_not_slower_from`: the first swept size from which the replayed `on` is not slower than the replayed `off` at every larger
swept size, per model and leg, and the largest of the inference legs' (what config.rank1_graph_min_batch would have to be)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = {"planar_tanh_d2_k32": ("P", 32, 2), "radial_d2_k16": ("R", 16, 2), "planar_tanh_d40_k16": ("P", 16, 40)}


def timed_steps(torch, fn, steps):
    """Per-step device times (ms) of `steps` calls of fn, each between its own pair of events."""
    for _ in range(3):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    torch.cuda.synchronize()
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def captured(torch, fn, warm):
    """fn recorded into a graph after the usual side-stream warm-up; None (and the error) when the capture fails."""
    try:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                warm()
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fn()
        return g, None
    except Exception as e:          # noqa: BLE001  (capture is reported, not required)
        torch.cuda.synchronize()
        return None, "%s: %s" % (type(e).__name__, str(e)[:200])


def model(nfa, torch, name, dev):
    kind, K, d = MODELS[name]
    torch.manual_seed(0)
    flows = [nfa.flows.Radial((d,)) if kind == "R" else nfa.flows.Planar((d,)) for _ in range(K)]
    return nfa.NormalizingFlow(nfa.distributions.DiagGaussian(d, trainable=False), flows).to(dev)


def summary(times):
    return {"median_ms": statistics.median(times), "min_ms": min(times)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batches", type=int, nargs="*", default=[1024, 65536])
    ap.add_argument("--sweep", type=int, nargs="*", default=[1024, 2048, 4096, 8192, 16384, 32768, 65536])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rank1_bench.json"))
    args = ap.parse_args()
    import torch
    sys.path.insert(0, ROOT)
    import normflows_amd as nfa
    dev = torch.device("cuda:0")
    out = {"workload": "device-event times in ms per forward_and_log_det (no_grad) and per reverse_kld-style step (forward + backward); "
                       "off = config.set_rank1_chain(False): every layer's torch formulas; on = the rank-1 chain kernels",
           "rounds": args.rounds, "steps": args.steps, "device": torch.cuda.get_device_name(0), "models": {}}
    for name in MODELS:
        m = model(nfa, torch, name, dev)
        d = MODELS[name][2]
        res = {}
        for B in sorted(set(args.batches) | set(args.sweep)):
            z = torch.randn(B, d, generator=torch.Generator().manual_seed(2)).to(dev)
            eager = B in args.batches

            def infer():
                with torch.no_grad():
                    return m.forward_and_log_det(z)

            def train():
                m.zero_grad(set_to_none=True)
                x, ld = m.forward_and_log_det(z)
                (0.5 * (x * x).sum(1) - ld).mean().backward()

            legs = {}
            for key, sw in (("off", False), ("on", True)):
                nfa.config.set_rank1_chain(sw)
                infer()
                train()
                gi, ei = captured(torch, infer, infer)
                m.zero_grad(set_to_none=True)
                gt, et = captured(torch, train, train)
                legs[key] = {}
                if eager:
                    legs[key].update({"forward_eager": (infer, []), "step_eager": (train, [])})
                if gi is not None:
                    legs[key]["forward_graph"] = (gi.replay, [])
                if gt is not None:
                    legs[key]["step_graph"] = (gt.replay, [])
                legs[key]["errors"] = [e for e in (ei, et) if e]
            for _ in range(args.rounds):
                for key, sw in (("off", False), ("on", True)):
                    nfa.config.set_rank1_chain(sw)
                    for leg, val in legs[key].items():
                        if leg != "errors":
                            val[1].extend(timed_steps(torch, val[0], args.steps))
            nfa.config.set_rank1_chain(True)
            r = {key: dict({leg: summary(val[1]) for leg, val in legs[key].items() if leg != "errors"},
                           **({"graph_errors": legs[key]["errors"]} if legs[key]["errors"] else {})) for key in ("off", "on")}
            r["speedup_median"] = {leg: r["off"][leg]["median_ms"] / r["on"][leg]["median_ms"]
                                   for leg in r["on"] if leg in r["off"] and leg != "graph_errors"}
            res[str(B)] = r
            print("%s B = %d: %s" % (name, B, json.dumps(r["speedup_median"])), flush=True)
            del legs
        sizes = sorted(int(B) for B in res)
        nsf = {}
        for leg in ("forward_graph", "step_graph"):
            ok = [B for B in sizes if all(res[str(b)]["speedup_median"].get(leg, 0.0) >= 1.0 for b in sizes if b >= B)]
            nsf[leg] = ok[0] if ok else None
        out["models"][name] = {"batches": res, "graph_not_slower_from": nsf}
    crit = {}
    for name, r in out["models"].items():
        for B in args.batches:
            for leg in ("forward_eager", "step_eager"):
                rb = r["batches"][str(B)]
                crit["%s %d %s" % (name, B, leg)] = rb["on"][leg]["median_ms"] < rb["off"][leg]["min_ms"]
    out["default_on_criterion"] = {"holds": all(crit.values()), "cases": crit}
    inf = [r["graph_not_slower_from"]["forward_graph"] for r in out["models"].values()]
    out["graph_not_slower_from"] = None if any(v is None for v in inf) else max(inf)
    out["smallest_swept_size"] = min(args.sweep)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print("default-on criterion holds:", out["default_on_criterion"]["holds"], "| graph_not_slower_from:", out["graph_not_slower_from"])
    print("wrote", args.out)


if __name__ == "__main__":
    main()
