#!/usr/bin/env python3
"""A/B of the wide RealNVP coupling layers' training route (config.affine_wide_train: autograd.AffineWideFn, csrc/affine_wide_train.hip
around the MADE training kernels) against the layer-wise route on an MI355X, in the style of tools/affine_wide_bench.py:
  masked  MaskedAffineFlow d 64, s and t MLP([64, 256, 256, 64]), alternating mask
  block   AffineCouplingBlock d 128, MLP([64, 512, 512, 128])
One step = layer.inverse(x) + backward of sum(z cz) + sum(ld cl), input and parameters requiring gradients.  Switch off / on alternate
over 5 rounds in ONE process per shape; every step is timed with device events; eager, and replayed from a captured graph; B = 1 024
... 65 536, doubling.  Also the peak memory of a step under both settings and the launch counts of both routes (ops calls, Linear
calls).  `capture_not_slower_from` = the smallest swept batch from which the replayed "on" median is not above the "off" median by
more than the off leg's own spread over the rounds (max - min of its per-round medians), at every larger swept size too; the larger of
the two shapes' values is config.affine_wide_train_capture_min_batch.  Writes profiles/affine_wide_train_bench.json.

Without --shape the tool is a driver: it runs each shape in a child process of its own under `timeout`, stops at the first one that
fails, and merges the results.

    python tools/affine_wide_train_bench.py [--rounds 5] [--steps 20] [--timeout 420]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = ("masked", "block")
SIZES = [1024 << i for i in range(7)]


def build_layer(nfa, shape):
    import torch
    torch.manual_seed(0)
    if shape == "masked":
        b = torch.tensor([1.0 if i % 2 == 0 else 0.0 for i in range(64)])
        layer = nfa.flows.MaskedAffineFlow(b, nfa.nets.MLP([64, 256, 256, 64], init_zeros=False), nfa.nets.MLP([64, 256, 256, 64], init_zeros=False))
        d = 64
    else:
        layer = nfa.flows.AffineCouplingBlock(nfa.nets.MLP([64, 512, 512, 128], init_zeros=False))
        d = 128
    with torch.no_grad():           # (scale parameters of moderate size: exp stays finite at every row)
        for p in layer.parameters():
            p.mul_(0.5)
    return layer, d


def timed_steps(fn, steps):
    """Per-step device times (ms) of `steps` calls of fn, each between its own pair of events."""
    import torch
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


def count_calls(nfa, fn):
    """({ops function: calls}, Linear calls) during one fn()."""
    import torch
    n, lin, saved = {}, [0], {}
    for name, f in list(vars(nfa.ops).items()):
        if callable(f) and not name.startswith("_") and getattr(f, "__module__", None) == nfa.ops.__name__:
            saved[name] = f

            def wrap(f=f, name=name):
                def w(*a, **k):
                    n[name] = n.get(name, 0) + 1
                    return f(*a, **k)
                return w
            setattr(nfa.ops, name, wrap())
    real = torch.nn.Linear.forward

    def counted(self, x):
        lin[0] += 1
        return real(self, x)
    torch.nn.Linear.forward = counted
    try:
        fn()
    finally:
        torch.nn.Linear.forward = real
        for name, f in saved.items():
            setattr(nfa.ops, name, f)
    return n, lin[0]


def run_shape(shape, rounds, steps):
    import torch
    import normflows_amd as nfa
    dev = torch.device("cuda:0")
    layer, d = build_layer(nfa, shape)
    layer = layer.to(dev)
    gate = nfa.config.affine_wide_train_capture_min_batch
    nfa.config.set_affine_wide_train(True, capture_min_batch=0)         # measure the route itself at every size, captured or not
    out = {"layer": {"masked": "MaskedAffineFlow d 64, s / t MLP([64,256,256,64])", "block": "AffineCouplingBlock d 128, MLP([64,512,512,128])"}[shape],
           "batches": {}}
    for B in SIZES:
        g = torch.Generator().manual_seed(3)
        x = torch.randn(B, d, generator=g).to(dev).requires_grad_(True)
        cz, cl = torch.randn(B, d, generator=g).to(dev), torch.randn(B, generator=g).to(dev)

        def step():
            layer.zero_grad(set_to_none=True)
            x.grad = None
            z, ld = layer.inverse(x)
            ((z * cz).sum() + (ld * cl).sum()).backward()

        res, graphs = {}, {}
        for mode in (False, True):
            nfa.config.set_affine_wide_train(mode)
            key = "on" if mode else "off"
            step()
            calls, linear = count_calls(nfa, step)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            step()
            torch.cuda.synchronize()
            res[key] = {"ops_calls_per_step": sum(calls.values()), "ops_calls": calls, "linear_calls_per_step": linear,
                        "peak_step_memory_mib": (torch.cuda.max_memory_allocated() - base) / 2 ** 20, "eager_ms": [], "graph_ms": [],
                        "graph_round_medians": []}
            try:
                s = torch.cuda.Stream()
                s.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(s):
                    for _ in range(2):
                        step()
                torch.cuda.current_stream().wait_stream(s)
                gr = torch.cuda.CUDAGraph()
                layer.zero_grad(set_to_none=True)
                x.grad = None
                with torch.cuda.graph(gr):
                    z, ld = layer.inverse(x)
                    ((z * cz).sum() + (ld * cl).sum()).backward()
                graphs[key] = gr
            except Exception as e:          # noqa: BLE001  (capture is reported, not required)
                res[key]["graph_error"] = "%s: %s" % (type(e).__name__, str(e)[:200])
                torch.cuda.synchronize()
        for _ in range(rounds):
            for mode in (False, True):
                nfa.config.set_affine_wide_train(mode)
                key = "on" if mode else "off"
                res[key]["eager_ms"] += timed_steps(step, steps)
                if key in graphs:
                    t = timed_steps(graphs[key].replay, steps)
                    res[key]["graph_ms"] += t
                    res[key]["graph_round_medians"].append(statistics.median(t))
        for key in ("off", "on"):
            for kind in ("eager_ms", "graph_ms"):
                t = res[key].pop(kind)
                if t:
                    res[key][kind.replace("_ms", "_median_ms")] = statistics.median(t)
                    res[key][kind.replace("_ms", "_min_ms")] = min(t)
        res["speedup_eager_median"] = res["off"]["eager_median_ms"] / res["on"]["eager_median_ms"]
        if "graph_median_ms" in res["off"] and "graph_median_ms" in res["on"]:
            res["speedup_graph_median"] = res["off"]["graph_median_ms"] / res["on"]["graph_median_ms"]
            rm = res["off"]["graph_round_medians"]
            res["off_graph_spread_ms"] = max(rm) - min(rm)
            res["graph_on_not_slower"] = res["on"]["graph_median_ms"] <= res["off"]["graph_median_ms"] + res["off_graph_spread_ms"]
        out["batches"][str(B)] = res
        del graphs
        print("%s B = %d: %s" % (shape, B, json.dumps({k: (v if not isinstance(v, dict) else {a: b for a, b in v.items() if a != "ops_calls"})
                                                        for k, v in res.items()})), flush=True)
    nfa.config.set_affine_wide_train(False, capture_min_batch=gate)
    ok = [B for B in SIZES if all(out["batches"][str(b)].get("graph_on_not_slower", False) for b in SIZES if b >= B)]
    out["capture_not_slower_from"] = ok[0] if ok else None
    out["eager_on_slower_at"] = [B for B in SIZES if out["batches"][str(B)]["speedup_eager_median"] < 1.0]
    out["graph_on_slower_at"] = [B for B in SIZES if out["batches"][str(B)].get("speedup_graph_median", 1.0) < 1.0]
    out["device"] = torch.cuda.get_device_name(0)
    out["capture_min_batch_in_config"] = gate
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--timeout", type=int, default=420, help="seconds per shape (driver mode)")
    ap.add_argument("--shape", choices=SHAPES, help="run this shape in this process and print its JSON to --part")
    ap.add_argument("--part", help="where --shape writes its result")
    args = ap.parse_args()
    if args.shape:
        res = run_shape(args.shape, args.rounds, args.steps)
        with open(args.part, "w") as f:
            json.dump(res, f)
        return 0
    out = {"workload": "one wide RealNVP coupling layer: layer.inverse(x) + backward of sum(z cz) + sum(ld cl), x and parameters requiring "
                       "gradients; device-event times in ms; off = layer-wise (library GEMMs + LeakyReLU launches + MaskedAffineFn / "
                       "AffineCouplingFn), on = autograd.AffineWideFn", "rounds": args.rounds, "steps": args.steps, "shapes": {}}
    extra = os.environ.get("NF_BENCH_OUT")
    tmpdir = os.path.dirname(extra) if extra else os.path.join(ROOT, "profiles")
    os.makedirs(tmpdir, exist_ok=True)
    for shape in SHAPES:
        part = os.path.join(tmpdir, "affine_wide_train_bench.%s.part.json" % shape)
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--shape", shape, "--part", part,
               "--rounds", str(args.rounds), "--steps", str(args.steps)]
        rc = subprocess.call(cmd)
        if rc != 0:
            print("shape %s ended with status %d: nothing more is started on the GPU" % (shape, rc))
            return rc
        with open(part) as f:
            out["shapes"][shape] = json.load(f)
        os.remove(part)
    out["device"] = out["shapes"][SHAPES[0]].pop("device")
    out["shapes"][SHAPES[1]].pop("device")
    froms = [out["shapes"][s]["capture_not_slower_from"] for s in SHAPES]
    out["capture_not_slower_from"] = None if any(f is None for f in froms) else max(froms)
    out["capture_min_batch_in_config"] = out["shapes"][SHAPES[0]]["capture_min_batch_in_config"]
    path = os.path.join(ROOT, "profiles", "affine_wide_train_bench.json")
    for p in [path] + ([extra] if extra else []):
        with open(p, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
    print("wrote", path)
    return 0


if __name__ == "__main__":
    sys.exit(main())
