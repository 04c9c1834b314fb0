"""The models of the coupling-block fixtures (tests/golden/grad_realnvp_block_*.npz): AffineCouplingBlock(nets.MLP) layers with the
Permute behind them, built from whichever package is handed in: the reference (tests/golden/make_golden_realnvp_blocks.py) or
normflows_amd (the tests) -- same constructors, same state dict (the shuffle permutations travel in it)."""
import torch

CASES = {"readme_d2": 70, "d5_maps": 33, "d16": 9, "d3_inv": 17}        # name -> rows


def build(nf, name):
    """(flows in forward order, d) of case `name`."""
    mlp, block, perm = nf.nets.MLP, nf.flows.AffineCouplingBlock, nf.flows.Permute
    if name == "readme_d2":    # the reference README's model at 4 layer pairs and width 8: more than one wave, ragged
        flows = []
        for _ in range(4):
            flows += [block(mlp([1, 8, 8, 2], init_zeros=True)), perm(2, mode="swap")]
        return flows, 2
    if name == "d5_maps":      # every scale map, scale=False, both splits, an odd swap, a shuffle, the old record kinds in between
        b = torch.tensor([1.0, 0.0, 0.0, 1.0, 0.0])
        return [block(mlp([3, 8, 4])),
                perm(5, mode="swap"),
                block(mlp([2, 7, 3, 6], leaky=0.1), True, "sigmoid", "channel_inv"),
                perm(5, mode="shuffle"),
                block(mlp([3, 8, 2]), scale=False),
                nf.flows.ActNorm(5),
                nf.flows.MaskedAffineFlow(b, mlp([5, 8, 5]), mlp([5, 8, 5])),
                block(mlp([3, 8, 4]), True, "sigmoid_inv")], 5
    if name == "d16":          # 16 MLP outputs: the register-array bound
        return [block(mlp([8, 32, 16])), perm(16, mode="shuffle"), block(mlp([8, 32, 16]), split_mode="channel_inv")], 16
    if name == "d3_inv":       # c1 = 1, c2 = 2
        return [block(mlp([1, 4, 4]), split_mode="channel_inv"), perm(3, mode="swap")], 3
    raise KeyError(name)


def records(name):
    """Number of chain records of case `name`: a block and the Permute behind it are one."""
    return {"readme_d2": 4, "d5_maps": 6, "d16": 2, "d3_inv": 1}[name]


def model(nf, name):
    flows, d = build(nf, name)
    return nf.NormalizingFlow(nf.distributions.DiagGaussian(d, trainable=False), flows)
