"""The models of the RealNVP training fixtures (tests/golden/grad_realnvp_train_*.npz), built from whichever package is handed in:
the reference (tests/golden/make_golden_realnvp_train.py) or normflows_amd (the tests) -- same constructors, same state dict."""
import torch

CASES = {"d2_w64": 70, "d5_mixed": 33, "d16": 9}        # name -> rows


def build(nf, name):
    """(flows in forward order, d) of case `name`."""
    mlp, maf = nf.nets.MLP, nf.flows.MaskedAffineFlow
    if name == "d2_w64":       # more than one wave, ragged, the maximum width
        b = torch.tensor([1.0, 0.0])
        flows = []
        for i in range(2):
            flows += [maf(b if i % 2 == 0 else 1 - b, mlp([2, 64, 64, 2], init_zeros=True), mlp([2, 64, 64, 2], init_zeros=True)),
                      nf.flows.ActNorm(2)]
        return flows, 2
    if name == "d5_mixed":     # s only (leaky 0.1), an AffineConstFlow, t only (two hidden layers), no nets, an ActNorm
        b = torch.tensor([1.0, 0.0, 0.0, 1.0, 0.0])
        return [maf(b, None, mlp([5, 16, 5], leaky=0.1)), nf.flows.AffineConstFlow(5), maf(1 - b, mlp([5, 7, 3, 5]), None), maf(b),
                nf.flows.ActNorm(5)], 5
    if name == "d16":
        b = torch.tensor([1.0, 0.0] * 8)
        return [maf(b, mlp([16, 32, 16]), mlp([16, 32, 16])), nf.flows.ActNorm(16)], 16
    raise KeyError(name)


def model(nf, name):
    flows, d = build(nf, name)
    return nf.NormalizingFlow(nf.distributions.DiagGaussian(d, trainable=False), flows)
