#!/usr/bin/env python3
"""A/B of the one-launch wide RealNVP coupling layer (config.affine_wide, nf_affine_wide) on an MI355X.  Writes
profiles/affine_wide_bench.json (or --out):

  masked  MaskedAffineFlow, d = 64, s and t MLP([64, 256, 256, 64]), alternating mask
  block   AffineCouplingBlock, d = 128, MLP([64, 512, 512, 128]), channel split, exp

each at 1024 and 65 536 rows: one layer.inverse(x) under no_grad (the density direction of a model; the forward direction is the same
conditioner pass), eager and replayed from a captured graph; switch off / on alternate over --rounds rounds in ONE process; every
call between its own pair of device events; median and minimum.  off = config.set_affine_wide(False): the conditioners as library
GEMMs + LeakyReLU launches, then nf_masked_affine / nf_affine_coupling.  `speedup_median` = off / on; `on_not_faster` lists the legs
where the switch did not win, `on_outside_off_spread_slower` those where the loss exceeds the off route's own min-max spread over
its rounds (the resolution of the measurement).

    timeout -k 10 600 python tools/affine_wide_bench.py"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from realnvp_block_bench import captured, timed_steps  # noqa: E402


def layers(nfa, torch, dev):
    torch.manual_seed(0)
    b = torch.tensor([1.0 if i % 2 == 0 else 0.0 for i in range(64)])
    masked = nfa.flows.MaskedAffineFlow(b, nfa.nets.MLP([64, 256, 256, 64], init_zeros=False), nfa.nets.MLP([64, 256, 256, 64], init_zeros=False))
    block = nfa.flows.AffineCouplingBlock(nfa.nets.MLP([64, 512, 512, 128], init_zeros=False))
    return {"masked": (masked.to(dev), 64), "block": (block.to(dev), 128)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--batches", type=int, nargs="*", default=[1024, 65536])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "affine_wide_bench.json"))
    args = ap.parse_args()
    import torch
    sys.path.insert(0, ROOT)
    import normflows_amd as nfa
    from normflows_amd.flows import affine_wide_pack
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    out = {"workload": "one layer.inverse(x) under no_grad, device-event times in ms; off = config.set_affine_wide(False): library GEMMs + "
                       "LeakyReLU launches + nf_masked_affine / nf_affine_coupling; on = nf_affine_wide (one launch)",
           "rounds": args.rounds, "steps": args.steps, "device": torch.cuda.get_device_name(0), "layers": {}}
    not_faster, outside = [], []
    for name, (layer, d) in layers(nfa, torch, dev).items():
        assert affine_wide_pack.supported(layer, d) is None
        res = {}
        for B in args.batches:
            x = torch.randn(B, d, generator=torch.Generator().manual_seed(2)).to(dev)
            fn = lambda: layer.inverse(x)      # noqa: E731
            legs = {}
            for key, sw in (("off", False), ("on", True)):
                nfa.config.set_affine_wide(sw)
                fn()
                g, err = captured(torch, fn, fn)
                legs[key] = {"eager": (fn, [], [])}
                if g is not None:
                    legs[key]["graph"] = (g.replay, [], [])
                else:
                    legs[key]["graph_error"] = err
            for _ in range(args.rounds):
                for key, sw in (("off", False), ("on", True)):
                    nfa.config.set_affine_wide(sw)
                    for leg, val in legs[key].items():
                        if leg != "graph_error":
                            t = timed_steps(torch, val[0], args.steps)
                            val[1].extend(t)
                            val[2].append(statistics.median(t))
            nfa.config.set_affine_wide(True)
            r = {key: {leg: ({"median_ms": statistics.median(v[1]), "min_ms": min(v[1]), "round_medians_ms": v[2]}
                             if leg != "graph_error" else v) for leg, v in legs[key].items()} for key in legs}
            r["speedup_median"] = {leg: r["off"][leg]["median_ms"] / r["on"][leg]["median_ms"]
                                   for leg in ("eager", "graph") if leg in r["on"] and leg in r["off"]}
            for leg, v in r["speedup_median"].items():
                if v < 1.0:
                    not_faster.append("%s %d %s" % (name, B, leg))
                    if r["on"][leg]["median_ms"] > max(r["off"][leg]["round_medians_ms"]):
                        outside.append("%s %d %s" % (name, B, leg))
            res[str(B)] = r
            print("%s B = %d: %s" % (name, B, json.dumps(r["speedup_median"])), flush=True)
        out["layers"][name] = res
        # the smallest measured size from which the one launch, replayed from a graph, is no slower at every larger measured size
        sizes = sorted(int(B) for B in res)
        ok = [B for B in sizes if all(res[str(b)]["speedup_median"].get("graph", 1.0) >= 1.0 for b in sizes if b >= B)]
        out.setdefault("graph_not_slower_from", {})[name] = ok[0] if ok else None
    out["graph_min_batch_in_config"] = nfa.config.affine_wide_graph_min_batch
    out["on_not_faster"] = sorted(not_faster)
    out["on_outside_off_spread_slower"] = sorted(outside)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
