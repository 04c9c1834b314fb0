"""CircularCoupledRationalQuadraticSpline at inference: the one-launch kernel (nf_nsf_wide_ft, csrc/nsf_circ.hip) against the layer-wise
path of the same commit (library GEMMs + torch.sin / torch.cos + nf_rqs_coupling_ft) and against the linear-tails one-launch kernel
(nf_nsf_wide_k) on a CoupledRationalQuadraticSpline of the same shape, all in ONE process.
usage: python tools/circ_coupled_bench.py [--rows B] [--passes P] [--calls C] [--out FILE]

D 64, hidden 128 and 256, K = 8, two blocks, half the features circular (bound pi, the others 3), 65 536 rows, both directions.  Every
figure is the median over P = 5 passes of C = 50 back-to-back calls between two HIP events, per call, after a warm-up pass; written to
profiles/circ_coupled_bench.json."""
import argparse, importlib.util, json, os, statistics, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("normflows_amd", os.path.join(ROOT, "normalizing-flows_amd", "__init__.py"))
nfa = importlib.util.module_from_spec(spec); sys.modules["normflows_amd"] = nfa; spec.loader.exec_module(nfa)

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=65536)
ap.add_argument("--passes", type=int, default=5)
ap.add_argument("--calls", type=int, default=50)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "circ_coupled_bench.json"))
args = ap.parse_args()
dev = torch.device("cuda:0")
D, K, NB = 64, 8, 2


def median_ms(fn):
    """Median over the passes of the time per call (C calls between two HIP events)."""
    for _ in range(3):
        fn()
    times = []
    for _ in range(args.passes):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.calls):
            fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) / args.calls)
    return statistics.median(times), min(times), max(times)


def perturb(layer, seed):
    g = torch.Generator().manual_seed(seed)
    fin = layer.prqct.transform_net.final_layer
    with torch.no_grad():
        for p in (fin.weight, fin.bias):
            p.add_(0.3 * torch.randn(p.shape, generator=g, dtype=p.dtype))
    return layer.to(dev).eval()


results = []
for H in (128, 256):
    torch.manual_seed(H)
    ind_circ = list(range(0, D, 2))[:D // 4] + list(range(1, D, 2))[:D // 4]        # half of either half of the mask
    bound = torch.full((D,), 3.0)
    bound[ind_circ] = float(np.pi)
    circ = perturb(nfa.flows.CircularCoupledRationalQuadraticSpline(D, NB, H, ind_circ=ind_circ, num_bins=K, tail_bound=bound,
                                                                    init_identity=False), 1)
    lin = perturb(nfa.flows.CoupledRationalQuadraticSpline(D, NB, H, num_bins=K, tail_bound=3.0, init_identity=False), 2)
    x = ((torch.rand(args.rows, D) * 2 - 1) * bound * 0.98).to(dev)
    calls = {"ft": 0, "wide": 0, "fused": 0}
    ft, wide, fused = nfa.ops.nsf_wide_ft, nfa.ops.nsf_wide, nfa.ops.rqs_fused

    def count(name, fn):
        def inner(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return inner
    nfa.ops.nsf_wide_ft, nfa.ops.nsf_wide, nfa.ops.rqs_fused = count("ft", ft), count("wide", wide), count("fused", fused)
    for direction, name in ((0, "density"), (1, "sampling")):
        run = lambda layer: layer.prqct._route(x, None, direction, None, None)
        with torch.no_grad():
            y1, ld1 = run(circ)
            circ.prqct.use_fused = False
            y0, ld0 = run(circ)
            t_layerwise = median_ms(lambda: run(circ))
            circ.prqct.use_fused = True
            n0 = calls["ft"]
            t_one = median_ms(lambda: run(circ))
            assert calls["ft"] - n0 == 3 + args.passes * args.calls, "the one-launch route did not run"
            # the linear-tails layer on nf_nsf_wide_k (at D 64 / hidden 128 the route would pick the benchmark kernel: pinned off)
            lin.prqct._fused_ok = False
            w0 = calls["wide"]
            t_lin = median_ms(lambda: run(lin))
            assert calls["wide"] - w0 == 3 + args.passes * args.calls and calls["fused"] == 0, "nf_nsf_wide_k did not run"
        rec = dict(D=D, hidden=H, K=K, blocks=NB, rows=args.rows, circular=len(ind_circ), direction=name, passes=args.passes,
                   calls_per_pass=args.calls,
                   layerwise_ms=t_layerwise[0], layerwise_min_max=t_layerwise[1:],
                   one_launch_ms=t_one[0], one_launch_min_max=t_one[1:],
                   linear_tails_wide_ms=t_lin[0], linear_tails_wide_min_max=t_lin[1:],
                   speedup_vs_layerwise=t_layerwise[0] / t_one[0], ratio_to_linear_tails=t_one[0] / t_lin[0],
                   max_abs_diff_y=float((y1 - y0).abs().max()), max_abs_diff_ld=float((ld1 - ld0).abs().max()))
        print(json.dumps(rec), flush=True)
        results.append(rec)
    nfa.ops.nsf_wide_ft, nfa.ops.nsf_wide, nfa.ops.rqs_fused = ft, wide, fused

out = dict(device=torch.cuda.get_device_name(0), method="median over passes of (HIP-event time of C back-to-back calls) / C, one process",
           results=results)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
