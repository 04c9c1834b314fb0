"""AR-NSF sampling direction (second half): nf_arnsf_inverse against the D-pass loop.
usage: python tools/arnsf_bench.py [D H K B layers] [--circular N] [--permute] [--passes P] [--density]

--circular N / --permute: ONE layer of the per-feature kernel (nf_arnsf_inverse_ft) -- CircularAutoregressiveRationalQuadraticSpline with
the first N features circular (bound pi, the others 3) and / or a permuted mask -- timed with HIP events in the same process against
(i) the D-pass loop on the same layer (`Autoregressive.inverse(layer, z)`) and (iii) the linear-tails nf_arnsf_inverse at the same
D / H / K; medians over P >= 20 passes after warm-up, written to profiles/circ_arnsf_bench.json.

--density: the DENSITY direction of the same layer (`layer.inverse`, default --circular 8 on a permuted mask): the layer-wise path
(config.arnsf_density_ft = False: eager MaskedLinear modules + nf_rqs_coupling), the one-launch per-feature kernel
(nf_made_forward_spline_ft) and the linear-tails one-launch layer (nf_made_forward_spline) in one process; median of 5 blocks of 50
calls each (as profiles/context_bench.json was taken), written to profiles/circ_arnsf_density_bench.json."""
import argparse, importlib.util, json, os, statistics, sys, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("normflows_amd", os.path.join(ROOT, "normalizing-flows_amd", "__init__.py"))
nfa = importlib.util.module_from_spec(spec); sys.modules["normflows_amd"] = nfa; spec.loader.exec_module(nfa)
from normflows_amd.flows.autoregressive import Autoregressive

ap = argparse.ArgumentParser()
ap.add_argument("shape", nargs="*", type=int, help="D H K B layers")
ap.add_argument("--circular", type=int, default=0, metavar="N")
ap.add_argument("--permute", action="store_true")
ap.add_argument("--passes", type=int, default=20)
ap.add_argument("--density", action="store_true")
args = ap.parse_args()
D, H, K, B, L = args.shape if len(args.shape) == 5 else (64, 256, 8, 65536, 4)
dev = torch.device("cuda:0")
torch.manual_seed(0)


def run(fn, reps):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3, out


def median_ms(fn, passes, warmup=2):
    """Median over `passes` runs, each between two HIP events."""
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(passes):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), min(times)


def block_ms(fn, blocks=5, calls=50):
    """Per-call milliseconds of `blocks` blocks of `calls` back-to-back calls, each block between two HIP events."""
    for _ in range(5):
        fn()
    out = []
    for _ in range(blocks):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / calls)
    return statistics.median(out), out


if args.density:
    n = args.circular or 8
    bound = torch.full((D,), 3.0)
    bound[:n] = float(np.pi)
    circ = nfa.flows.CircularAutoregressiveRationalQuadraticSpline(D, 2, H, ind_circ=list(range(n)), num_bins=K, tail_bound=bound,
                                                                   permute_mask=True, init_identity=False).to(dev)
    lin = nfa.flows.AutoregressiveRationalQuadraticSpline(D, 2, H, num_bins=K, init_identity=False).to(dev)
    x = ((torch.rand(B, D) * 2 - 1) * bound * 0.98).to(dev)
    calls = {"ft": 0, "lin": 0}
    ft, ln = nfa.ops.made_forward_spline_ft, nfa.ops.made_forward_spline

    def counted_ft(*a, **k):
        calls["ft"] += 1
        return ft(*a, **k)

    def counted_lin(*a, **k):
        calls["lin"] += 1
        return ln(*a, **k)
    nfa.ops.made_forward_spline_ft, nfa.ops.made_forward_spline = counted_ft, counted_lin
    with torch.no_grad():
        z1, l1 = circ.inverse(x)
        lin.inverse(x)
        assert calls == {"ft": 1, "lin": 1}, "the one-launch paths were not taken"
        nfa.config.set_arnsf_density_ft(False)
        z0, l0 = circ.inverse(x)
        assert calls["ft"] == 1
        t_layer = block_ms(lambda: circ.inverse(x))
        nfa.config.set_arnsf_density_ft(True)
        t_ft = block_ms(lambda: circ.inverse(x))
        t_lin = block_ms(lambda: lin.inverse(x))
        t_ft2 = block_ms(lambda: circ.inverse(x))          # again after the others: drift of the device between the blocks
    rec = {"shape": {"D": D, "hidden": H, "K": K, "B": B, "circular": n, "permute": True}, "blocks": 5, "calls_per_block": 50,
           "timer": "HIP events around 50 back-to-back calls, per-call ms: median of 5 blocks (and the blocks)",
           "layerwise_ms": t_layer, "one_launch_ft_ms": t_ft, "one_launch_ft_again_ms": t_ft2, "linear_made_forward_spline_ms": t_lin,
           "ft_over_layerwise": t_ft[0] / t_layer[0], "ft_over_linear": t_ft[0] / t_lin[0],
           "max_abs_dz_vs_layerwise": float((z1 - z0).abs().max()), "max_abs_dld_vs_layerwise": float((l1 - l0).abs().max()),
           "device": torch.cuda.get_device_name(0)}
    print(json.dumps(rec))
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "circ_arnsf_density_bench.json"), "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    sys.exit(0)

if args.circular or args.permute:
    passes = max(args.passes, 20)
    n = args.circular
    bound = torch.full((D,), 3.0)
    bound[:n] = float(np.pi)
    if n:
        circ = nfa.flows.CircularAutoregressiveRationalQuadraticSpline(D, 2, H, ind_circ=list(range(n)), num_bins=K, tail_bound=bound,
                                                                       permute_mask=args.permute, init_identity=False).to(dev)
    else:
        circ = nfa.flows.AutoregressiveRationalQuadraticSpline(D, 2, H, num_bins=K, permute_mask=True, init_identity=False).to(dev)
    lin = nfa.flows.AutoregressiveRationalQuadraticSpline(D, 2, H, num_bins=K, init_identity=False).to(dev)
    z = ((torch.rand(B, D) * 2 - 1) * bound * 0.98).to(dev)
    calls = {"ft": 0}
    ft = nfa.ops.arnsf_inverse_ft

    def counted(*a, **k):
        calls["ft"] += 1
        return ft(*a, **k)
    nfa.ops.arnsf_inverse_ft = counted
    with torch.no_grad():
        xf, _ = circ.forward(z)
        assert calls["ft"] == 1 and lin.mprqat._packed(dev) is not None, "the one-launch paths were not taken"
        xd, _ = Autoregressive.inverse(circ.mprqat, z)
        t_ft = median_ms(lambda: circ.forward(z), passes)
        t_lin = median_ms(lambda: lin.forward(z), passes)
        t_loop = median_ms(lambda: Autoregressive.inverse(circ.mprqat, z), passes, warmup=1)
        t_ft2 = median_ms(lambda: circ.forward(z), passes)          # again after the others: drift of the device between the blocks
    rec = {"shape": {"D": D, "hidden": H, "K": K, "B": B, "circular": n, "permute": bool(args.permute)}, "passes": passes,
           "timer": "HIP events around one call, median (min) in ms",
           "d_pass_loop_ms": t_loop, "one_launch_ft_ms": t_ft, "one_launch_ft_again_ms": t_ft2, "linear_arnsf_inverse_ms": t_lin,
           "ft_over_loop": t_ft[0] / t_loop[0], "ft_over_linear": t_ft[0] / t_lin[0],
           "max_abs_dx_vs_loop": float((xf - xd).abs().max()), "device": torch.cuda.get_device_name(0)}
    print(json.dumps(rec))
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "circ_arnsf_bench.json"), "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    sys.exit(0)

layers = [nfa.flows.AutoregressiveRationalQuadraticSpline(D, 2, H, num_bins=K, init_identity=False).to(dev) for _ in range(L)]
z = torch.randn(B, D, device=dev)


def fused():
    x = z
    for l in layers:
        x, _ = l.forward(x)
    return x


def dpass():
    x = z
    for l in layers:
        x, _ = Autoregressive.inverse(l.mprqat, x)
    return x


with torch.no_grad():
    run(fused, 2)
    tf, xf = run(fused, 10)
    run(dpass, 1)
    td, xd = run(dpass, 2)
print("AR-NSF sample  D=%d H=%d K=%d B=%d layers=%d : one-pass %.2f ms (%.2f ms/layer, %.2f M rows/s)  D-pass %.1f ms  (x%.1f)  max|dx| %.2e"
      % (D, H, K, B, L, tf, tf / L, B / tf / 1e3, td, td / tf, float((xf - xd).abs().max())))
