#!/usr/bin/env python3
"""One conditional NSF coupling layer (CoupledRationalQuadraticSpline with num_context_channels) at 65 536 rows, 8 bins, 2 blocks,
both directions: the one-launch kernel (nf_nsf_wide_ctx), the same layer with config.set_nsf_context(False) (eager conditioner +
nf_rqs_coupling), and the context-free one-launch kernel (nf_nsf_wide_k) at the same D / hidden.  HIP events around REPS calls after
WARMUP calls, the median of TRIALS such means; roofline fraction on the algorithmic FLOP of the conditional layer,
2 (nI H + C H + NB (2 H^2 + C H) + (3 K - 1) nT H) per row, against the fp32 MFMA peak (157.3 TFLOP/s, MI355X_MICROARCH.md).

    python tools/context_bench.py [--out profiles/context_bench.json] [--rows 65536]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK = 157.3e12
SHAPES = ((64, 16, 128), (64, 16, 256), (64, 16, 512), (16, 4, 128), (64, 64, 256))   # D, C, hidden
K, NB, WARMUP, REPS, TRIALS = 8, 2, 10, 50, 5


def timed(fn):
    """Median over TRIALS of the mean of REPS calls (ms)."""
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(TRIALS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(REPS):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / REPS)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "context_bench.json"))
    ap.add_argument("--rows", type=int, default=65536)
    args = ap.parse_args()
    import normflows_amd as nfa
    from normflows_amd import ops
    B = args.rows
    res = {"rows": B, "bins": K, "blocks": NB, "unit": "ms per layer call", "peak_tflops": PEAK / 1e12, "shapes": {}}
    torch.manual_seed(0)
    for D, C, H in SHAPES:
        nI, nT = D // 2, D - D // 2
        flop = 2.0 * (nI * H + C * H + NB * (2 * H * H + C * H) + (3 * K - 1) * nT * H) * B
        layer = nfa.flows.CoupledRationalQuadraticSpline(D, NB, H, num_context_channels=C, num_bins=K, init_identity=False).eval().cuda()
        free = nfa.flows.CoupledRationalQuadraticSpline(D, NB, H, num_bins=K, init_identity=False).eval().cuda()
        with torch.no_grad():
            for m in (layer, free):
                for p in m.parameters():
                    p.add_(0.05 * torch.randn_like(p))
        x = torch.randn(B, D, device="cuda")
        c = torch.randn(B, C, device="cuda")
        p, pf = layer.prqct, free.prqct
        packed = p._ctx_pack(x, c)
        wide = pf._wide_pack(x, None)
        entry = {"D": D, "C": C, "hidden": H, "flop_per_row": flop / B}
        with torch.no_grad():
            for direction, tag in ((0, "density"), (1, "sampling")):
                r = {}
                if packed is not None:
                    r["one_launch_ms"] = timed(lambda: p._wide_ctx(x, c, packed, direction, None, None))
                    r["roofline"] = flop / (r["one_launch_ms"] * 1e-3) / PEAK
                else:
                    r["one_launch_ms"] = None
                    r["one_launch_note"] = "declined by the packer (hidden > 256: Hp 512 is not built)"
                nfa.config.set_nsf_context(False)
                try:
                    run = p._density if direction == 0 else p._sample
                    r["layerwise_ms"] = timed(lambda: run(x, c))
                finally:
                    nfa.config.set_nsf_context(True)
                r["context_free_wide_ms"] = timed(lambda: pf._wide(x, wide, direction, None, None)) if wide is not None else None
                if r["one_launch_ms"]:
                    r["speedup_vs_layerwise"] = r["layerwise_ms"] / r["one_launch_ms"]
                    if r["context_free_wide_ms"]:
                        r["ratio_vs_context_free"] = r["one_launch_ms"] / r["context_free_wide_ms"]
                entry[tag] = r
        res["shapes"]["d%d_c%d_h%d" % (D, C, H)] = entry
        print(json.dumps({"d%d_c%d_h%d" % (D, C, H): entry}), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
