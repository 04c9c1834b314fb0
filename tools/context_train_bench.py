#!/usr/bin/env python3
"""Training step of one conditional NSF coupling layer (CoupledRationalQuadraticSpline with num_context_channels) at 65 536 rows,
8 bins, 2 blocks (D 2 at the notebook's batch of 512 rows): forward (density direction) + backward, with the conditioner on the HIP training kernels (autograd.ResNetCtxFn)
and with config.set_nsf_context_train(False) (eager torch modules); plus the notebook-shaped model step, 4 x [CRQS(2, 2, 128,
context 4) + LULinearPermute(2)] under forward_kld, at 512 rows (LULinearPermute(2)'s backward declines batches of 1024 rows and
more: nf_linear_wgrad_pair).  HIP events around REPS steps after WARMUP steps, the median
of TRIALS such means (as tools/context_bench.py).

    python tools/context_train_bench.py [--out profiles/context_train_bench.json] [--rows 4096 16384 32768 65536]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = ((64, 16, 128), (64, 16, 256), (16, 4, 128), (64, 64, 256), (2, 4, 128))   # D, C, hidden
SMALL = 512             # the notebook's batch
K, NB, WARMUP, REPS, TRIALS = 8, 2, 5, 20, 5


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


def both(nfa, step, rows):
    from normflows_amd.flows import ctx_train_pack
    lim = ctx_train_pack.MAX_ROWS
    ctx_train_pack.MAX_ROWS = 1 << 30            # the kernels also above the route's batch limit
    try:
        r = {"hip_ms": timed(step)}
    finally:
        ctx_train_pack.MAX_ROWS = lim
    r["route"] = "hip" if rows <= lim else "eager"
    nfa.config.set_nsf_context_train(False)
    try:
        r["eager_ms"] = timed(step)
    finally:
        nfa.config.set_nsf_context_train(True)
    r["speedup"] = r["eager_ms"] / r["hip_ms"]
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "context_train_bench.json"))
    ap.add_argument("--rows", type=int, nargs="+", default=[4096, 16384, 32768, 65536])
    args = ap.parse_args()
    out = {"bins": K, "blocks": NB, "unit": "ms per training step (forward + backward)",
           "hip_ms": "the HIP training kernels (forced also above ctx_train_pack.MAX_ROWS)",
           "eager_ms": "config.set_nsf_context_train(False)", "route": "what the default configuration runs", "by_rows": {}}
    for B in args.rows:
        out["by_rows"][str(B)] = run(B)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


def run(B):
    import normflows_amd as nfa
    res = {"rows": B, "layers": {}}
    torch.manual_seed(0)
    for D, C, H in SHAPES:
        layer = nfa.flows.CoupledRationalQuadraticSpline(D, NB, H, num_context_channels=C, num_bins=K, init_identity=False).cuda()
        with torch.no_grad():
            for p in layer.parameters():
                p.add_(0.05 * torch.randn_like(p))
        rows = SMALL if D == 2 else B
        x = torch.randn(rows, D, device="cuda").requires_grad_(True)
        c = torch.randn(rows, C, device="cuda")

        def step():
            z, ld = layer.inverse(x, c)
            (z.square().sum() - ld.sum()).backward()
        entry = {"D": D, "C": C, "hidden": H, "rows": rows}
        entry.update(both(nfa, step, rows))
        res["layers"]["d%d_c%d_h%d" % (D, C, H)] = entry
        print(json.dumps({"rows": B, "d%d_c%d_h%d" % (D, C, H): entry}), flush=True)
    flows = []
    for _ in range(4):
        flows += [nfa.flows.CoupledRationalQuadraticSpline(2, 2, 128, num_context_channels=4, init_identity=False),
                  nfa.flows.LULinearPermute(2)]
    m = nfa.ConditionalNormalizingFlow(nfa.distributions.DiagGaussian(2), flows).cuda()
    x = torch.randn(SMALL, 2, device="cuda")
    c = torch.randn(SMALL, 4, device="cuda")

    def mstep():
        m.zero_grad(set_to_none=True)
        m.forward_kld(x, c).backward()
    res["notebook_model"] = dict(rows=SMALL, **both(nfa, mstep, SMALL))
    print(json.dumps({"notebook_model": res["notebook_model"]}), flush=True)
    return res


if __name__ == "__main__":
    main()
