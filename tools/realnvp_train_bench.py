#!/usr/bin/env python3
"""A/B of the RealNVP training route (config.realnvp_train: autograd.RealNVPChainFn, csrc/realnvp_train.hip) against the
layer-by-layer route on an MI355X: BASELINE configs[0]'s model, 4 x [MaskedAffineFlow + ActNorm], d = 2, s / t = MLP([2, 64, 64, 2]);
one step = forward_kld + backward, at B = 1024 and B = 65 536.  Switch off / on alternate over 5 rounds in ONE process; every
step is timed with device events; eager, and replayed from a captured graph where the capture succeeds.  Also the number of ops
calls per step on each route.  Batch sizes between the two (--sweep) locate the size from which the route is also the faster one
under graph replay: `capture_min_batch` = the smallest measured size from which on <= off at every larger measured size -- the value
of config.realnvp_train_capture_min_batch.  Writes profiles/realnvp_train_bench.json.

    python tools/realnvp_train_bench.py [--rounds 5] [--steps 30]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import normflows_amd as nfa  # noqa: E402

dev = torch.device("cuda:0")


def model():
    torch.manual_seed(0)
    b = torch.tensor([1.0, 0.0])
    fl = []
    for i in range(4):
        s = nfa.nets.MLP([2, 64, 64, 2], init_zeros=True)
        t = nfa.nets.MLP([2, 64, 64, 2], init_zeros=True)
        fl += [nfa.flows.MaskedAffineFlow(b if i % 2 == 0 else 1 - b, t, s), nfa.flows.ActNorm(2)]
    m = nfa.NormalizingFlow(nfa.distributions.DiagGaussian(2), fl)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for p in m.flows.parameters():
            p.add_(0.05 * torch.randn(p.shape, generator=g))
    return m.to(dev)


def timed_steps(fn, steps):
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


def count_ops(fn):
    """Calls into normflows_amd.ops during one fn()."""
    n = {}
    saved = {}
    for name, f in list(vars(nfa.ops).items()):
        if callable(f) and not name.startswith("_") and getattr(f, "__module__", None) == nfa.ops.__name__:
            saved[name] = f

            def wrap(f=f, name=name):
                def w(*a, **k):
                    n[name] = n.get(name, 0) + 1
                    return f(*a, **k)
                return w
            setattr(nfa.ops, name, wrap())
    try:
        fn()
    finally:
        for name, f in saved.items():
            setattr(nfa.ops, name, f)
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--sweep", type=int, nargs="*", default=[2048, 4096, 8192, 16384, 32768])
    args = ap.parse_args()
    m = model()
    default_min = nfa.config.realnvp_train_capture_min_batch
    nfa.config.set_realnvp_train(True, capture_min_batch=0)        # measure the route itself at every size, captured or not
    out = {"workload": "4 x [MaskedAffineFlow(MLP([2,64,64,2]) s, t) + ActNorm], d = 2: forward_kld + backward per step; device-event "
                       "times in ms; off = layer by layer, on = autograd.RealNVPChainFn", "rounds": args.rounds, "steps": args.steps,
           "device": torch.cuda.get_device_name(0), "batches": {}}
    for B in sorted(set([1024, 65536] + list(args.sweep))):
        x = torch.randn(B, 2, generator=torch.Generator().manual_seed(2)).to(dev)
        with torch.no_grad():
            m.log_prob(x)                      # ActNorm's data-dependent initialisation

        def step():
            m.zero_grad(set_to_none=True)
            m.forward_kld(x).backward()

        res = {}
        graphs = {}
        for mode in (False, True):
            nfa.config.set_realnvp_train(mode)
            key = "on" if mode else "off"
            step()
            calls = count_ops(step)
            res[key] = {"ops_calls_per_step": sum(calls.values()), "ops_calls": calls, "eager_ms": [], "graph_ms": []}
            try:
                s = torch.cuda.Stream()
                s.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(s):
                    for _ in range(2):
                        step()
                torch.cuda.current_stream().wait_stream(s)
                g = torch.cuda.CUDAGraph()
                m.zero_grad(set_to_none=True)
                with torch.cuda.graph(g):
                    m.forward_kld(x).backward()
                graphs[key] = g
            except Exception as e:          # noqa: BLE001  (capture is reported, not required)
                res[key]["graph_error"] = "%s: %s" % (type(e).__name__, str(e)[:200])
                torch.cuda.synchronize()
        for _ in range(args.rounds):
            for mode in (False, True):
                nfa.config.set_realnvp_train(mode)
                key = "on" if mode else "off"
                res[key]["eager_ms"] += timed_steps(step, args.steps)
                if key in graphs:
                    res[key]["graph_ms"] += timed_steps(graphs[key].replay, args.steps)
        nfa.config.set_realnvp_train(True)
        for key in ("off", "on"):
            for kind in ("eager_ms", "graph_ms"):
                t = res[key].pop(kind)
                if t:
                    res[key][kind.replace("_ms", "_median_ms")] = statistics.median(t)
                    res[key][kind.replace("_ms", "_min_ms")] = min(t)
        res["speedup_eager_median"] = res["off"]["eager_median_ms"] / res["on"]["eager_median_ms"]
        if "graph_median_ms" in res["off"] and "graph_median_ms" in res["on"]:
            res["speedup_graph_median"] = res["off"]["graph_median_ms"] / res["on"]["graph_median_ms"]
        out["batches"][str(B)] = res
        print("B = %d: %s" % (B, json.dumps({k: (v if not isinstance(v, dict) else {a: b for a, b in v.items() if a != "ops_calls"})
                                             for k, v in res.items()})))
    slower = [B for B, r in out["batches"].items() if r["speedup_eager_median"] < 1.0 or r.get("speedup_graph_median", 1.0) < 1.0]
    out["on_not_faster_at"] = slower
    sizes = sorted(int(B) for B in out["batches"])
    ok = [B for B in sizes if all(out["batches"][str(b)].get("speedup_graph_median", 1.0) >= 1.0 for b in sizes if b >= B)]
    out["capture_min_batch"] = ok[0] if ok else None
    out["capture_min_batch_in_config"] = default_min
    nfa.config.set_realnvp_train(True, capture_min_batch=default_min)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    path = os.path.join(ROOT, "profiles", "realnvp_train_bench.json")
    extra = os.environ.get("NF_BENCH_OUT")
    for p in [path] + ([extra] if extra else []):
        with open(p, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
    print("wrote", path)


if __name__ == "__main__":
    main()
