"""Time of nf_final_bwd (+ reduce) at the benchmark shape on random saved tensors."""
import os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import normflows_amd as nfa
from normflows_amd import ops
from bench import build_c2_model
dev = torch.device("cuda:0")
B = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 65536
m = build_c2_model(num_layers=1).to(dev)
c = m.flows[0].prqct
u, net = c.unconditional_transform, c.transform_net
x = torch.randn(B, 64, device=dev)
assert c._fused_eligible(x, None)
gy, gld = torch.randn(B, 64, device=dev), torch.randn(B, device=dev)
cond24 = 0.5 * torch.randn(B, 32, 24, device=dev)
blob = c._train_blob_for(x)
_, wpad, _, wfull_t = c._train_buffers(x)
lin = [l for blk in net.blocks for l in blk.linear_layers]
d = lambda t: t.detach()
ops.rqs_fused_pack_all(blob, d(net.initial_layer.weight), d(net.initial_layer.bias), [d(l.weight) for l in lin], [d(l.bias) for l in lin],
                       d(net.final_layer.weight), d(net.final_layer.bias), d(u.unnormalized_widths), d(u.unnormalized_heights),
                       d(u.unnormalized_derivatives), wfull=wfull_t, wpad=wpad, identity_idx=c.identity_features)
f = lambda: ops.final_bwd(x, gy, gld, cond24, wpad, blob, d(u.unnormalized_widths), d(u.unnormalized_heights),
                          d(u.unnormalized_derivatives), c._fused_parity, len(net.blocks))
for _ in range(5): f()
torch.cuda.synchronize()
s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
s.record()
for _ in range(30): f()
e.record(); torch.cuda.synchronize()
print("%.1f us per call (nf_final_bwd + nf_final_bwd_reduce + allocations), B = %d" % (s.elapsed_time(e) / 30 * 1e3, B))
