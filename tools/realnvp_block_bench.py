#!/usr/bin/env python3
"""A/B of the coupling block record of the RealNVP chain kernels (config.realnvp_blocks) on an MI355X, and the regression guard
for the stacks the chain kernels already ran.  Writes profiles/realnvp_block_bench.json in three steps:

  blocks   the reference README's model, 32 x [AffineCouplingBlock(MLP([1, 64, 64, 2])), Permute(2, 'swap')], d = 2, at 1024 and
           65 536 rows: `log_prob` (no_grad) and `forward_kld` + backward, eager and replayed from a captured graph; switch off / on
           alternate over --rounds rounds in ONE process; every step between its own pair of device events; median and minimum.
           "on" is the default configuration: a CAPTURED training step below config.realnvp_train_capture_min_batch rows takes the
           layer-by-layer route also with the switch on; "on_route" (capture_min_batch = 0) is the record itself there.  Batch
           sizes in between (--batches) locate the size from which the record is also the faster one when replayed from a graph:
           `inference_graph_not_slower_from`, `train_graph_not_slower_from`.
  guard    tools/realnvp_train_bench.py's model (4 x [MaskedAffineFlow(MLP([2, 64, 64, 2]) s, t) + ActNorm]: no block in it) in the
           default configuration, per round one median: run once from a checkout of the parent commit (--tree) and once from this
           tree, on the same box.  The bench file itself is the same for both; only the package it imports differs.
  assemble joins the parts and judges the guard: this tree's medians must lie within the parent's own min-max spread over its
           rounds -- that spread is the resolution of the measurement.

Every GPU step under its own time limit, chained so that a failure ends the sequence:

    timeout -k 10 900 python tools/realnvp_block_bench.py blocks --out /tmp/blocks.json \\
      && timeout -k 10 300 python tools/realnvp_block_bench.py guard --tree <parent checkout> --out /tmp/parent.json \\
      && timeout -k 10 300 python tools/realnvp_block_bench.py guard --out /tmp/this.json \\
      && python tools/realnvp_block_bench.py assemble --blocks /tmp/blocks.json --parent /tmp/parent.json --this /tmp/this.json

(`--parent` / `--this` take several files: alternate the two guard steps and hand all of them in.)"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def readme_model(nfa, torch, dev):
    torch.manual_seed(0)
    flows = []
    for _ in range(32):
        flows += [nfa.flows.AffineCouplingBlock(nfa.nets.MLP([1, 64, 64, 2], init_zeros=True)), nfa.flows.Permute(2, mode="swap")]
    m = nfa.NormalizingFlow(nfa.distributions.DiagGaussian(2), flows)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for p in m.flows.parameters():
            p.add_(0.05 * torch.randn(p.shape, generator=g))
    return m.to(dev)


def summary(times):
    return {"median_ms": statistics.median(times), "min_ms": min(times)}


def run_blocks(args):
    import torch
    sys.path.insert(0, ROOT)
    import normflows_amd as nfa
    dev = torch.device("cuda:0")
    m = readme_model(nfa, torch, dev)
    default_min = nfa.config.realnvp_train_capture_min_batch
    out = {"workload": "32 x [AffineCouplingBlock(MLP([1,64,64,2])), Permute(2,'swap')], d = 2; device-event times in ms per log_prob "
                       "(no_grad) and per forward_kld + backward; off = config.set_realnvp_blocks(False): every block its conditioner "
                       "modules + nf_affine_coupling, every Permute torch indexing; on = one coupling block record per pair",
           "rounds": args.rounds, "steps": args.steps, "device": torch.cuda.get_device_name(0),
           "train_capture_min_batch_in_config": default_min, "batches": {}}
    for B in args.batches:
        x = torch.randn(B, 2, generator=torch.Generator().manual_seed(2)).to(dev)

        def infer():
            with torch.no_grad():
                return m.log_prob(x)

        def train():
            m.zero_grad(set_to_none=True)
            m.forward_kld(x).backward()

        modes = {"off": (False, default_min), "on": (True, default_min)}
        if B < default_min:
            modes["on_route"] = (True, 0)
        legs = {}
        for key, (sw, cmin) in modes.items():
            nfa.config.set_realnvp_blocks(sw)
            nfa.config.set_realnvp_train(True, capture_min_batch=cmin)
            infer()
            train()
            gi, ei = captured(torch, infer, infer)
            m.zero_grad(set_to_none=True)
            gt, et = captured(torch, lambda: m.forward_kld(x).backward(), train)
            legs[key] = {"log_prob_eager": (infer, []), "train_eager": (train, [])}
            if gi is not None:
                legs[key]["log_prob_graph"] = (gi.replay, [])
            if gt is not None:
                legs[key]["train_graph"] = (gt.replay, [])
            legs[key]["errors"] = [e for e in (ei, et) if e]
        for _ in range(args.rounds):
            for key, (sw, cmin) in modes.items():
                nfa.config.set_realnvp_blocks(sw)
                nfa.config.set_realnvp_train(True, capture_min_batch=cmin)
                for leg, val in legs[key].items():
                    if leg != "errors":
                        val[1].extend(timed_steps(torch, val[0], args.steps))
        nfa.config.set_realnvp_blocks(True)
        nfa.config.set_realnvp_train(True, capture_min_batch=default_min)
        res = {key: dict({leg: summary(val[1]) for leg, val in legs[key].items() if leg != "errors"},
                         **({"graph_errors": legs[key]["errors"]} if legs[key]["errors"] else {})) for key in modes}
        res["speedup_median"] = {k2: {leg: res["off"][leg]["median_ms"] / res[k2][leg]["median_ms"]
                                      for leg in res[k2] if leg in res["off"] and leg != "graph_errors"} for k2 in modes if k2 != "off"}
        out["batches"][str(B)] = res
        print("B = %d: %s" % (B, json.dumps(res["speedup_median"])), flush=True)
    # the smallest measured size from which the record itself is no slower than the layer-by-layer route at every larger measured
    # size when replayed from a graph (training: what config.realnvp_train_capture_min_batch should be for this model)
    sizes = sorted(int(B) for B in out["batches"])
    route = {B: out["batches"][str(B)]["speedup_median"].get("on_route", out["batches"][str(B)]["speedup_median"]["on"]) for B in sizes}
    for name, leg in (("inference_graph_not_slower_from", "log_prob_graph"), ("train_graph_not_slower_from", "train_graph")):
        ok = [B for B in sizes if all(route[b].get(leg, 1.0) >= 1.0 for b in sizes if b >= B)]
        out[name] = ok[0] if ok else None
    out["on_not_faster_at"] = sorted("%s %s" % (B, leg) for B, r in out["batches"].items()
                                     for leg, v in r["speedup_median"]["on"].items() if v < 1.0)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print("wrote", args.out)


def run_guard(args):
    import torch
    tree = os.path.abspath(args.tree) if args.tree else ROOT
    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(tree, "tools"))
    import normflows_amd as nfa
    import realnvp_train_bench as tb             # its model(): the stack the chain kernels already ran
    assert os.path.abspath(nfa.__file__).startswith(tree + os.sep), nfa.__file__
    m = tb.model()
    out = {"tree": "parent" if args.tree else "this", "rounds": args.rounds, "steps": args.steps,
           "device": torch.cuda.get_device_name(0), "round_medians_ms": {}}
    for B in args.batches:
        x = torch.randn(B, 2, generator=torch.Generator().manual_seed(2)).to(tb.dev)
        with torch.no_grad():
            m.log_prob(x)                      # ActNorm's data-dependent initialisation

        def infer():
            with torch.no_grad():
                return m.log_prob(x)

        def train():
            m.zero_grad(set_to_none=True)
            m.forward_kld(x).backward()

        legs = {"log_prob_eager": infer, "train_eager": train}
        # a captured step below capture_min_batch takes the layer-by-layer route: its library GEMMs initialise outside the capture
        nfa.config.set_realnvp_train(False)
        train()
        nfa.config.set_realnvp_train(True)
        m.zero_grad(set_to_none=True)
        g, err = captured(torch, lambda: m.forward_kld(x).backward(), train)
        if g is not None:
            legs["train_graph"] = g.replay
        res = {leg: [] for leg in legs}
        for _ in range(args.rounds):
            for leg, fn in legs.items():
                res[leg].append(statistics.median(timed_steps(torch, fn, args.steps)))
        out["round_medians_ms"][str(B)] = res
        print("B = %d: %s" % (B, json.dumps(res)), flush=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print("wrote", args.out)


def run_assemble(args):
    out = json.load(open(args.blocks))
    pooled = {}
    for side, paths in (("parent", args.parent), ("this", args.this)):
        for p in paths:
            part = json.load(open(p))
            assert part["tree"] == side, (p, part["tree"])
            for B, legs in part["round_medians_ms"].items():
                for leg, meds in legs.items():
                    pooled.setdefault(B, {}).setdefault(leg, {}).setdefault(side, []).extend(meds)
    guard, outside = {}, []
    for B, legs in pooled.items():
        guard[B] = {}
        for leg, s in legs.items():
            lo, hi, med = min(s["parent"]), max(s["parent"]), statistics.median(s["this"])
            guard[B][leg] = {"parent_round_medians_ms": s["parent"], "this_round_medians_ms": s["this"], "parent_min_ms": lo,
                             "parent_max_ms": hi, "parent_median_ms": statistics.median(s["parent"]), "this_median_ms": med,
                             "this_within_parent_spread": lo <= med <= hi, "this_slower_than_parent_max": med > hi}
            if not lo <= med <= hi:
                outside.append("%s %s" % (B, leg))
    out["regression_guard"] = {"workload": "tools/realnvp_train_bench.py's model (4 x [MaskedAffineFlow + ActNorm], d = 2, no block), "
                                           "default configuration; one median per round, parent and this tree as alternating processes",
                               "batches": guard, "outside_parent_spread": sorted(outside)}
    path = os.path.join(ROOT, "profiles", "realnvp_block_bench.json")
    for p in [path] + ([args.out] if args.out else []):
        with open(p, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
    print("outside the parent's spread:", sorted(outside) or "nothing")
    print("wrote", path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("step", choices=["blocks", "guard", "assemble"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--batches", type=int, nargs="*", default=[1024, 65536])
    ap.add_argument("--tree", default=None, help="guard: a checkout of the parent commit, built")
    ap.add_argument("--out", default=None)
    ap.add_argument("--blocks")
    ap.add_argument("--parent", nargs="*", default=[])
    ap.add_argument("--this", nargs="*", default=[])
    args = ap.parse_args()
    {"blocks": run_blocks, "guard": run_guard, "assemble": run_assemble}[args.step](args)


if __name__ == "__main__":
    main()
