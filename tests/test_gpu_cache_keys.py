"""GPU test of the cache keys behind every cached route (normflows_amd._keys.cached / pcached): one layer per route at the smallest
shape that takes it, 96 rows (one full 64-row tile and a ragged one), both directions.  A second pass is a hit, invalidate_caches
and every kind of tensor a route's key covers (conditioner weight, batch-shared spline, tensor tail bound, LU parameter, the
conditioner's mode) lead to exactly what a freshly built layer with that state computes -- bit for bit: a key that misses one of
them serves a stale pack and fails here."""
import pytest
import torch

import ar_ft_train_cases
import circ_wide_cases

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B = 96


@pytest.fixture(autouse=True)
def _inference_mode():
    with torch.no_grad():
        yield


@pytest.fixture(scope="module")
def nfa():
    import normflows_amd
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    assert normflows_amd.native_library_path().endswith("normalizing-flows_amd/lib/libnf_mi355x.so")
    normflows_amd._lib.lib()
    return normflows_amd


def _perturbed(module, seed, sigma=0.05):
    g = torch.Generator().manual_seed(seed)
    for p in module.parameters():
        p.add_(sigma * torch.randn(p.shape, generator=g))
    return module


def _rows(*shape, seed=1):
    x = 1.5 * torch.randn(B, *shape, generator=torch.Generator().manual_seed(seed))
    x[: B // 8] *= 3.0                                   # some rows beyond the tail bounds
    return x.to(DEV)


class _Case:
    """make() -> the module on the CPU, deterministic; run(m, direction) -> tuple of tensors; slots(m, direction) -> the (owner,
    slot, sub) the route must have filled; changes(m) -> [(what, change in place, moves the numbers)]."""
    shape = None
    context = None

    def __init__(self, nfa):
        self.nfa = nfa
        self.x = _rows(*self.shape)
        self.c = None if self.context is None else torch.randn(B, self.context, generator=torch.Generator().manual_seed(2)).to(DEV)

    def build(self, state=None):
        m = self.make()
        if state is not None:
            m.load_state_dict(state, strict=True)
        return m.eval().to(DEV)

    def run(self, m, direction):
        args = (self.x,) if self.c is None else (self.x, self.c)
        return tuple((m.forward if direction else m.inverse)(*args))

    def prepare(self, m):
        pass


def _coupling_changes(p, mode=False, bounds=False):
    net, u = p.transform_net, p.unconditional_transform
    out = [("conditioner weight", lambda: net.final_layer.weight[::2].add_(0.05), True),
           ("batch-shared spline", lambda: u.unnormalized_heights[:, 0].add_(0.5), True)]     # (one bin: softmax ignores a common shift)
    if bounds:
        out += [("tail bound of the transform half", lambda: p.tail_bound.mul_(1.05), True),
                ("tail bound of the identity half", lambda: u.tail_bound.mul_(1.05), True)]
    if mode:       # dropout 0: the numbers stay, the key (and the pack) is another
        out += [("conditioner in train()", lambda: net.train(), False), ("conditioner back in eval()", lambda: net.eval(), False)]
    return out


class Circular(_Case):
    """tests/circ_wide_cases.py (a): D = 6, hidden 32, tensor tail bound -> nf_nsf_wide_ft, `_circ_cache`."""
    shape = (6,)

    def make(self):
        return circ_wide_cases.layer(self.nfa, "a")

    def slots(self, m, direction):
        return [(m.prqct, "_circ_cache", None)]

    def changes(self, m):
        return _coupling_changes(m.prqct, mode=True, bounds=True)


class Context(_Case):
    """tests/test_gpu_context.py's ctx_d6_c3_h40 -> nf_nsf_wide_ctx, `_ctx_cache`."""
    shape, context = (6,), 3

    def make(self):
        torch.manual_seed(0)
        return _perturbed(self.nfa.flows.CoupledRationalQuadraticSpline(6, 2, 40, num_context_channels=3, num_bins=8, init_identity=False), 3)

    def slots(self, m, direction):
        return [(m.prqct, "_ctx_cache", None)]

    def changes(self, m):
        return _coupling_changes(m.prqct, mode=True)


class PaddedBenchmarkKernel(_Case):
    """D = 6, hidden 40 on the benchmark kernel's 64 x 128 shape -> nf_rqs_fused, `_fused_cache`."""
    shape = (6,)

    def make(self):
        torch.manual_seed(0)
        return _perturbed(self.nfa.flows.CoupledRationalQuadraticSpline(6, 2, 40, num_bins=8, init_identity=False), 4)

    def slots(self, m, direction):
        return [(m.prqct, "_fused_cache", None)]

    def changes(self, m):
        return _coupling_changes(m.prqct)


class WidePair(_Case):
    """tests/test_gpu_parity.py's smallest wide pair, D = 33, hidden 300, with its LULinearPermute -> nf_nsf_wide with the dense LU
    matrix in the launch: `_wide_cache` per (LU layer, direction) and the LU layer's `_dense_cache`."""
    shape = (33,)

    def make(self):
        torch.manual_seed(33 + 300)
        flows = [self.nfa.flows.CoupledRationalQuadraticSpline(33, 2, 300, num_bins=8),
                 self.nfa.flows.LULinearPermute(33, identity_init=False)]
        return _perturbed(self.nfa.NormalizingFlow(self.nfa.distributions.DiagGaussian(33, trainable=False), flows), 5, 0.03)

    def run(self, m, direction):
        return tuple(m.sample_from_noise(self.x)) if direction else (m.log_prob(self.x),)

    def slots(self, m, direction):
        crqs, lu = m.flows
        return [(crqs.prqct, "_wide_cache", (id(lu), 1 if direction else 0)), (lu, "_dense_cache", None)]

    def changes(self, m):
        lin = m.flows[1].linear
        return _coupling_changes(m.flows[0].prqct) + [("LU parameter", lambda: lin.lower_entries.add_(0.05), True)]


class Maf(_Case):
    """One MAF layer: nf_made_forward_affine on MADE's `_fwd_pack_cache`, nf_maf_inverse on `_maf_pack_cache`."""
    shape = (6,)

    def make(self):
        torch.manual_seed(0)
        return _perturbed(self.nfa.flows.MaskedAffineAutoregressive(6, 16, num_blocks=2), 6)

    def slots(self, m, direction):
        return [(m.autoregressive_net, "_fwd_pack_cache", False)] if direction else [(m, "_maf_pack_cache", None)]

    def changes(self, m):
        return [("conditioner weight", lambda: m.autoregressive_net.final_layer.weight[::2].add_(0.05), True)]


class ArnsfScalarTails(_Case):
    """AR-NSF, scalar tails: nf_made_forward_spline on MADE's `_fwd_pack_cache`, nf_arnsf_inverse on `_arnsf_pack_cache`."""
    shape = (9,)

    def make(self):
        torch.manual_seed(0)
        return _perturbed(self.nfa.flows.AutoregressiveRationalQuadraticSpline(9, 2, 40, num_bins=8, tail_bound=3.0, init_identity=False), 7)

    def slots(self, m, direction):
        t = m.mprqat
        return [(t, "_arnsf_pack_cache", None)] if direction else [(t.autoregressive_net, "_fwd_pack_cache", True)]

    def changes(self, m):
        return [("conditioner weight", lambda: m.mprqat.autoregressive_net.final_layer.weight[::2].add_(0.05), True)]


class ArnsfListTails(_Case):
    """tests/ar_ft_train_cases.py's D = 21, hidden 40 circular layer (list tails, tensor bound, permuted mask): nf_made_forward_spline_ft on
    `_arnsf_fwd_ft_pack_cache`, nf_arnsf_inverse_ft on `_arnsf_ft_pack_cache`."""
    shape = (21,)
    name = "grad_circ_ar_perm_d21_h40"

    def make(self):
        return ar_ft_train_cases.make_layer(self.nfa, self.name, ar_ft_train_cases.load_case(self.name))

    def slots(self, m, direction):
        return [(m.mprqat, "_arnsf_ft_pack_cache" if direction else "_arnsf_fwd_ft_pack_cache", None)]

    def changes(self, m):
        t = m.mprqat
        return [("conditioner weight", lambda: t.autoregressive_net.final_layer.weight[::2].add_(0.05), True),
                ("tail bound", lambda: t.tail_bound.mul_(1.05), True)]


class Glow(_Case):
    """GlowBlock(4, 8) on 4 x 4 images: [Invertible1x1Conv, ActNorm] as one map in `_mix_cache`, on the 1x1 convolution's `_w_cache`."""
    shape = (4, 4, 4)

    def make(self):
        torch.manual_seed(0)
        return _perturbed(self.nfa.flows.GlowBlock(4, 8, init_zeros=False), 8)

    def prepare(self, m):
        m.inverse(self.x)          # ActNorm's data-dependent initialisation: once, then it is part of the state

    def slots(self, m, direction):
        return [(m, "_mix_cache", None), (m.flows[1], "_w_cache", None)]

    def changes(self, m):
        blk, conv, an = m.flows
        return [("conditioner weight", lambda: blk.flows[1].param_map.net[-1].weight.add_(0.05), True),
                ("ActNorm scale", lambda: an.s.add_(0.1), True), ("LU parameter of the 1x1 convolution", lambda: conv.L.add_(0.05), True)]


CASES = [Circular, Context, PaddedBenchmarkKernel, WidePair, Maf, ArnsfScalarTails, ArnsfListTails, Glow]


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(s, t) for s, t in zip(a, b))


def _filled(owner, slot, sub):
    ent = owner.__dict__.get(slot)
    if sub is not None or isinstance(ent, dict):
        ent = (ent or {}).get(sub)
    return isinstance(ent, tuple) and len(ent) == 2 and ent[1] is not None


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.__name__)
def test_cached_route_follows_every_tensor_of_its_key(nfa, case):
    case = case(nfa)
    m = case.build()
    case.prepare(m)
    y0 = {}
    for d in (0, 1):
        y0[d] = case.run(m, d)
        for owner, slot, sub in case.slots(m, d):        # the one-launch route was taken: its slot holds a pack
            assert _filled(owner, slot, sub), (slot, sub, "not filled: the layer did not take its cached route")
        assert all(torch.isfinite(t).all() for t in y0[d])
        assert _same(case.run(m, d), y0[d]), ("second pass (a hit)", d)
    nfa.invalidate_caches(m)
    assert not any(_filled(*s) for d in (0, 1) for s in case.slots(m, d))
    for d in (0, 1):
        assert _same(case.run(m, d), y0[d]), ("after invalidate_caches", d)
    prev = y0
    for what, change, moves in case.changes(m):
        change()
        fresh = case.build({k: v.cpu() for k, v in m.state_dict().items()})
        now = {}
        for d in (0, 1):
            now[d] = case.run(m, d)
            assert _same(now[d], case.run(fresh, d)), (what, d, "differs from a freshly built layer with this state")
            if moves:        # ... and the pack was rebuilt, not merely never consulted
                assert not _same(now[d], y0[d]) and not _same(now[d], prev[d]), (what, d, "the numbers did not move")
            else:
                assert _same(now[d], prev[d]), (what, d)
        prev = now


@pytest.mark.parametrize("D", [5, 70])
def test_dense_matrices_follow_the_parameters_on_the_device(nfa, D):
    """tests/test_host_cache_helper.py's check of LULinearPermute._dense_matrices on the real composers: nf_lu_compose (D = 5) and the
    float64 torch launches (D = 70)."""
    torch.manual_seed(D)
    lu = nfa.flows.LULinearPermute(D, identity_init=False).to(DEV)
    m0 = lu._dense_matrices()
    assert lu._dense_matrices() is m0
    nfa.invalidate_caches(lu)
    m1 = lu._dense_matrices()
    assert m1 is not m0 and _same(m0, m1)
    lu.linear.lower_entries.add_(0.1)
    m2 = lu._dense_matrices()
    assert not torch.equal(m2[0], m0[0])
    fresh = nfa.flows.LULinearPermute(D, identity_init=False)
    fresh.load_state_dict({k: v.cpu() for k, v in lu.state_dict().items()}, strict=True)
    assert _same(m2, fresh.to(DEV)._dense_matrices())
