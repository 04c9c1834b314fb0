"""The layers of the wide RealNVP coupling fixtures (tests/golden/affine_wide_<name>.npz), shared by the generator
(tests/golden/make_golden_affine_wide.py, on the reference) and the tests (on normflows_amd): the smallest shapes at which
nf_affine_wide can still go wrong.

  a  MaskedAffineFlow d 17, s MLP([17,72,72,17]), t MLP([17,72,40,17]), alternating mask: odd row length (scalar path), 256 slots, the
     s block padded to 96, unequal widths
  b  MaskedAffineFlow d 64, s and t MLP([64,160,160,64]), mask 1 - alternating: 512 slots (NSB 2), 16-byte path
  c  MaskedAffineFlow d 128, s only MLP([128,264,264,128]), random binary mask: one net above 256 slots, 8 final row-blocks, t missing
  d  MaskedAffineFlow d 20, t only MLP([20,65,65,20]): s missing (log-det exactly 0), width just above the chain's limit
  e  AffineCouplingBlock d 33, channel, exp, MLP([17,130,130,32]): odd d, c1 != c2
  f  AffineCouplingBlock d 24, channel_inv, sigmoid, MLP([12,96,96,24]): flipped split, sigmoid
  g  as f with channel, sigmoid_inv
  h  AffineCouplingBlock d 19, scale=False, MLP([10,80,80,9]): shift-only rows
"""
import numpy as np
import torch

ROWS = 130
CASES = {
    "a": dict(kind="masked", d=17, s=[17, 72, 72, 17], t=[17, 72, 40, 17], mask="alt", seed=9101),
    "b": dict(kind="masked", d=64, s=[64, 160, 160, 64], t=[64, 160, 160, 64], mask="alt_inv", seed=9102),
    "c": dict(kind="masked", d=128, s=[128, 264, 264, 128], t=None, mask="random", seed=9103),
    "d": dict(kind="masked", d=20, s=None, t=[20, 65, 65, 20], mask="alt", seed=9104),
    "e": dict(kind="block", d=33, split="channel", scale=True, smap="exp", net=[17, 130, 130, 32], seed=9105),
    "f": dict(kind="block", d=24, split="channel_inv", scale=True, smap="sigmoid", net=[12, 96, 96, 24], seed=9106),
    "g": dict(kind="block", d=24, split="channel", scale=True, smap="sigmoid_inv", net=[12, 96, 96, 24], seed=9107),
    "h": dict(kind="block", d=19, split="channel", scale=False, smap="exp", net=[10, 80, 80, 9], seed=9108),
}


def mask(case):
    d = case["d"]
    alt = np.array([1.0 if i % 2 == 0 else 0.0 for i in range(d)], dtype=np.float32)
    if case["mask"] == "alt":
        return alt
    if case["mask"] == "alt_inv":
        return 1.0 - alt
    b = (np.random.RandomState(case["seed"]).rand(d) < 0.5).astype(np.float32)
    assert 0 < b.sum() < d
    return b


def build(lib, name):
    """The layer of case `name` from `lib` (normflows or normflows_amd: the same constructors), default-initialised under the
    case's seed (init_zeros off: the last layers are not zero)."""
    c = CASES[name]
    torch.manual_seed(c["seed"])
    if c["kind"] == "masked":
        s = None if c["s"] is None else lib.nets.MLP(c["s"], init_zeros=False)
        t = None if c["t"] is None else lib.nets.MLP(c["t"], init_zeros=False)
        return lib.flows.MaskedAffineFlow(torch.from_numpy(mask(c)), t, s)
    return lib.flows.AffineCouplingBlock(lib.nets.MLP(c["net"], init_zeros=False), scale=c["scale"], scale_map=c["smap"],
                                         split_mode=c["split"])


def scale_outputs(layer, case):
    """The Linear + the rows of it that produce the scale parameter (None: the layer has none)."""
    if case["kind"] == "masked":
        if case["s"] is None:
            return None
        return [m for m in layer.s.net if isinstance(m, torch.nn.Linear)][-1], slice(None)
    if not case["scale"]:
        return None
    return [m for m in layer.flows[1].param_map.net if isinstance(m, torch.nn.Linear)][-1], slice(1, None, 2)
