"""GPU tests of the operand contract (run with -m gpu on an MI355X): what happens when one operand of a call has another dtype or
element count than the others ("Operand dtypes and shapes").

Every test runs under the audit spy of tests/operand_audit.py: each C-ABI call is checked against the header's typed pointers, the
call's own `dtype` argument and -- for the entry points a caller's tensor can get wrong -- its scalar sizes, and a call that breaks a
rule is NOT forwarded to the library.  So a missing guard in ops.py fails an assertion here; it never launches a kernel on
inconsistent operands.  Three kinds of outcome, no numeric tolerance anywhere: an exception, zero violations, or bit equality of the
same kernel on the same values.

Shapes: B in {0, 5}; d = 6 (scalar kernels) and d = 8 (the four-elements-per-lane kernels and their aligned copies); images 2x4x4."""
import copy

import pytest
import torch

import mixed_stack_cases as stacks
import operand_audit
from test_gpu_views import DEV, nfa, perturbed, same  # noqa: F401  (nfa: the module fixture)

pytestmark = pytest.mark.gpu

F32, F64, BF16, F16 = torch.float32, torch.float64, torch.bfloat16, torch.float16
B = 5


@pytest.fixture
def audit(nfa, monkeypatch):
    return operand_audit.install(nfa, monkeypatch)


@pytest.fixture
def blocked(nfa, monkeypatch):
    return operand_audit.install(nfa, monkeypatch, block_all=True)


def vec(n, d, seed, dtype=F32, lo=None):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, d, generator=g, dtype=F64) if lo is None else lo + (1 - 2 * lo) * torch.rand(n, d, generator=g, dtype=F64)
    return x.to(dtype).to(DEV)


def img(n, seed, dtype=F32, unit=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, 2, 4, 4, generator=g, dtype=F64) if unit else torch.randn(n, 2, 4, 4, generator=g, dtype=F64)
    return x.to(dtype).to(DEV)


# ---- the public layers, each on its smallest shape: name -> builder(nfa, d) -> (module, input factory(n, dtype), extra inputs(n)) ---
def _mlp(nfa, sizes):
    return nfa.nets.MLP(list(sizes), init_zeros=False)


def _vector_layers(nfa, d):
    fl, c1 = nfa.flows, (d + 1) // 2
    mask = torch.tensor([1.0, 0.0] * (d // 2))
    spl = dict(num_bins=8, init_identity=False)
    return {
        "affine_const": lambda: fl.AffineConstFlow(d),
        "actnorm": lambda: fl.ActNorm(d),
        "masked_affine": lambda: fl.MaskedAffineFlow(mask, _mlp(nfa, [d, 8, d]), _mlp(nfa, [d, 8, d])),
        "coupling_block": lambda: fl.AffineCouplingBlock(_mlp(nfa, [c1, 8, 2 * (d - c1)])),
        "coupling_block_inv_shift": lambda: fl.AffineCouplingBlock(_mlp(nfa, [d // 2, 8, d - d // 2]), scale=False, split_mode="channel_inv"),
        "lu": lambda: fl.LULinearPermute(d, identity_init=False),
        "inv_affine_lu": lambda: fl.InvertibleAffine(d, use_lu=True),
        "inv_affine_w": lambda: fl.InvertibleAffine(d, use_lu=False),
        "coupled_spline": lambda: fl.CoupledRationalQuadraticSpline(d, 1, 16, **spl),
        "ar_spline": lambda: fl.AutoregressiveRationalQuadraticSpline(d, 1, 16, **spl),
        "circ_coupled_spline": lambda: fl.CircularCoupledRationalQuadraticSpline(d, 1, 16, ind_circ=[1, 4], tail_bound=3.0, **spl),
        "circ_ar_spline": lambda: fl.CircularAutoregressiveRationalQuadraticSpline(d, 1, 16, ind_circ=[1, 4], tail_bound=3.0, **spl),
        "maf": lambda: fl.MaskedAffineAutoregressive(d, 16),
    }


def _image_layers(nfa):
    fl = nfa.flows
    return {
        "glow_block": lambda: fl.GlowBlock(2, 12, split_mode="channel", use_lu=True, init_zeros=False),
        "glow_block_w": lambda: fl.GlowBlock(2, 12, split_mode="channel", use_lu=False, init_zeros=False),
        "inv1x1_lu": lambda: fl.Invertible1x1Conv(2, True),
        "inv1x1_w": lambda: fl.Invertible1x1Conv(2, False),
        "actnorm_img": lambda: fl.ActNorm((2, 1, 1)),
    }


VECTOR = ["affine_const", "actnorm", "masked_affine", "coupling_block", "coupling_block_inv_shift", "lu", "inv_affine_lu", "inv_affine_w",
          "coupled_spline", "ar_spline", "circ_coupled_spline", "circ_ar_spline", "maf"]
IMAGE = ["glow_block", "glow_block_w", "inv1x1_lu", "inv1x1_w", "actnorm_img"]
LAYER_CASES = [(n, d) for n in VECTOR for d in (6, 8)] + [(n, 0) for n in IMAGE]       # (image layers: the one shape 2 x 4 x 4)


def build(nfa, name, d, seed=0):
    torch.manual_seed(seed + d)
    layer = (_image_layers(nfa) if name in IMAGE else _vector_layers(nfa, d))[name]()
    return perturbed(layer, seed + 1, 0.1)


def data(name, n, d, dtype, seed=3):
    return img(n, seed, dtype) if name in IMAGE else vec(n, d, seed, dtype)


def both_ways(layer, x, *extra):
    return layer.forward(x, *extra) + layer.inverse(x, *extra)


def one_backward(layer, x, *extra):
    """One backward through each direction: gradients for the input and every parameter."""
    for run in (layer.inverse, layer.forward):
        xg = x.detach().clone().requires_grad_(True)
        y, ld = run(xg, *extra)
        (y.sum() + (ld.sum() if torch.is_tensor(ld) else 0.0)).backward()
        assert xg.grad is not None and xg.grad.dtype == x.dtype
    layer.zero_grad(set_to_none=True)


# ---- 1. audit of correct calls ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("name,d", LAYER_CASES)
def test_layers_pass_consistent_operands(nfa, audit, name, d, dtype):
    layer = build(nfa, name, d).to(dtype).to(DEV)
    with torch.no_grad():
        both_ways(layer, data(name, B, d, dtype))          # (ActNorm / GlowBlock: the first call is the data-dependent initialisation)
        both_ways(layer, data(name, B, d, dtype, seed=4))
        for o in both_ways(layer, data(name, 0, d, dtype)):
            assert o.dim() == 0 or o.shape[0] == 0
    layer.train()
    one_backward(layer, data(name, B, d, dtype, seed=5))
    torch.cuda.synchronize()
    assert not audit.violations, audit.violations
    assert audit.forwarded, "no C-ABI call was made"


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_glue_bases_and_function_api_pass_consistent_operands(nfa, audit, dtype):
    fl, dist = nfa.flows, nfa.distributions
    with torch.no_grad():
        for n in (B, 0):
            z = img(n, 1, dtype)
            sq = fl.Squeeze()
            y, _ = sq.inverse(z)
            assert y.shape == (n, 8, 2, 2) and same(sq.forward(y)[0], z)
            lg = nfa.transforms.Logit(0.05)
            u = img(n, 2, dtype, unit=True)
            lg.forward(lg.inverse(u)[0])
            pm = fl.Permute(6, mode="shuffle").to(DEV)
            pm.inverse(pm.forward(vec(n, 6, 3, dtype))[0])
        for d in (6, 8):
            q = perturbed(dist.DiagGaussian(d), d).to(dtype).to(DEV)
            cc = perturbed(dist.ClassCondDiagGaussian(d, 3), d + 1).to(dtype).to(DEV)
            lab = torch.tensor([0, 2, 1, 1, 0], device=DEV)
            soft = torch.softmax(vec(B, 3, 7, dtype), 1)
            for n in (B, 0):
                q.log_prob(vec(n, d, 4, dtype))
                cc.log_prob(vec(n, d, 5, dtype), lab[:n])
                cc.log_prob(vec(n, d, 5, dtype), soft[:n])
            q.forward(B)
            cc.forward(B, lab)
            ug = dist.UniformGaussian(d, [1], torch.ones(d)).to(dtype).to(DEV)
            ug.log_prob(ug.sample(B))
            K = 8
            x = vec(B, d, 8, dtype)
            w, h, dd = (torch.randn(B, d, k, device=DEV, dtype=dtype) for k in (K, K, K - 1))
            nfa.utils.splines.unconstrained_rational_quadratic_spline(x, w, h, dd, tail_bound=3.0)
            dfull = torch.randn(B, d, K + 1, device=DEV, dtype=dtype)
            nfa.utils.splines.rational_quadratic_spline(vec(B, d, 9, dtype, lo=0.01), w, h, dfull)
            nfa.utils.splines.rational_quadratic_spline(vec(0, d, 9, dtype, lo=0.01), w[:0], h[:0], dfull[:0])
    for d in (6, 8):          # one backward each
        q = perturbed(dist.DiagGaussian(d), d).to(dtype).to(DEV)
        cc = perturbed(dist.ClassCondDiagGaussian(d, 3), d + 1).to(dtype).to(DEV)
        (q.log_prob(vec(B, d, 4, dtype)).sum() + cc.log_prob(vec(B, d, 5, dtype), torch.tensor([0, 2, 1, 1, 0], device=DEV)).sum()).backward()
        x = vec(B, d, 8, dtype).requires_grad_(True)
        w, h, dd = (torch.randn(B, d, k, device=DEV, dtype=dtype, requires_grad=True) for k in (8, 8, 7))
        y, lad = nfa.utils.splines.unconstrained_rational_quadratic_spline(x, w, h, dd, tail_bound=3.0)
        (y.sum() + lad.sum()).backward()
    cca = perturbed(fl.CCAffineConst(6, 3), 2).to(dtype).to(DEV)
    with torch.no_grad():     # integer labels beside float parameters: converted by the layer (y.to(self.s.dtype))
        onehot = torch.nn.functional.one_hot(torch.tensor([0, 2, 1, 1, 0]), 3).to(DEV)
        cca.inverse(cca.forward(vec(B, 6, 6, dtype), onehot)[0], onehot)
    torch.cuda.synchronize()
    assert not audit.violations, audit.violations
    seen = set(audit.forwarded)
    for entry in ("nf_squeeze", "nf_logit", "nf_diag_gaussian_log_prob", "nf_diag_gaussian_log_prob_rows", "nf_rqs_spline", "nf_masked_affine"):
        assert entry in seen, (entry, sorted(seen))


def _models(nfa):
    """(name, model, input factory): the stacks the chain router fuses -- mixed_stack_cases' D = 6 stack of narrow spline pairs around
    a RealNVP run (nf_rqs_fused_chain, nf_realnvp_chain), a wide pair, a context layer, a Glow level."""
    out = []
    m, _ = stacks.pairs_around_records(nfa)
    out.append(("nsf_pairs_realnvp", m, lambda n, dtype: vec(n, 6, 11, dtype), None))
    torch.manual_seed(5)
    wide = [nfa.flows.CoupledRationalQuadraticSpline(8, 1, 160, num_bins=8, init_identity=False), nfa.flows.LULinearPermute(8, identity_init=False)]
    out.append(("wide_pair", perturbed(nfa.NormalizingFlow(nfa.distributions.DiagGaussian(8, trainable=False), wide), 6).to(DEV).eval(),
                lambda n, dtype: vec(n, 8, 12, dtype), None))
    torch.manual_seed(7)
    ctx = [nfa.flows.CoupledRationalQuadraticSpline(6, 1, 16, num_context_channels=3, num_bins=8, init_identity=False)]
    out.append(("context", perturbed(nfa.ConditionalNormalizingFlow(nfa.distributions.DiagGaussian(6, trainable=False), ctx), 8).to(DEV).eval(),
                lambda n, dtype: vec(n, 6, 13, dtype), lambda n, dtype: vec(n, 3, 14, dtype)))
    torch.manual_seed(9)
    level = [[nfa.flows.GlowBlock(8, 12, split_mode="channel", scale=True, init_zeros=False) for _ in range(2)] + [nfa.flows.Squeeze()]]
    glow = perturbed(nfa.MultiscaleFlow([nfa.distributions.DiagGaussian((8, 2, 2))], level, [], class_cond=False), 10, 0.05).to(DEV).eval()
    with torch.no_grad():
        glow.log_prob(img(B, 20))        # ActNorm's data-dependent initialisation
    out.append(("glow_level", glow, lambda n, dtype: img(n, 15, dtype), None))
    return out


MODELS = ["nsf_pairs_realnvp", "wide_pair", "context", "glow_level"]
# the one-launch entry points a float32 log_prob of each stack goes through (the router's rules: DESIGN.md, tests/mixed_stack_cases.py)
ROUTES = {"nsf_pairs_realnvp": (stacks.CHAIN, stacks.RNVP), "wide_pair": (stacks.WIDE,), "context": ("nf_nsf_wide_ctx",),
          "glow_level": ("nf_affine_coupling_pb",)}       # (2 x 2 pixels: below nf_glow_level's layouts, block by block)


def model_case(nfa, name):
    return next(c for c in _models(nfa) if c[0] == name)


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", MODELS)
def test_models_pass_consistent_operands(nfa, audit, name, dtype):
    _, m, x_of, c_of = model_case(nfa, name)
    m = m.to(dtype)
    extra = lambda n: () if c_of is None else (c_of(n, dtype),)        # noqa: E731
    with torch.no_grad():
        for n in (B, 0):
            lp = m.log_prob(x_of(n, dtype), *extra(n))
            assert lp.shape == (n,) and lp.dtype == dtype
        if dtype == F32:
            assert set(ROUTES[name]) <= set(audit.forwarded), (ROUTES[name], sorted(set(audit.forwarded)))
        if c_of is None:
            xs, lq = m.sample(B)
            assert xs.dtype == dtype and lq.dtype == dtype
        else:
            m.sample(B, extra(B)[0])
    m.train()
    m.forward_kld(x_of(B, dtype), *extra(B)).backward()
    torch.cuda.synchronize()
    assert not audit.violations, audit.violations
    assert audit.forwarded


# ---- 2. the mismatch matrix -----------------------------------------------------------------------------------------------------------
def _refused(fn):
    """The call raises TypeError (this library's refusal) or the RuntimeError torch's own Linear / conv raise on mixed dtypes."""
    with pytest.raises((TypeError, RuntimeError)) as e:
        fn()
    if not isinstance(e.value, TypeError):
        assert "type" in str(e.value).lower(), "a RuntimeError that is not about dtypes: %s" % e.value
    return e.value


KINDS = ["f64_input", "f32_input_double_module", "bf16_module", "f16_module", "bf16_input"]


def _mismatch(kind, module, make_x):
    """(module, input) of one kind of mismatch."""
    if kind == "f64_input":
        return module, make_x(F64)
    if kind == "f32_input_double_module":
        return module.double(), make_x(F32)
    if kind == "bf16_module":
        return module.bfloat16(), make_x(F32)
    if kind == "f16_module":
        return module.half(), make_x(F32)
    return module, make_x(BF16)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,d", LAYER_CASES)
def test_layers_refuse_mismatched_dtypes(nfa, audit, name, d, kind):
    layer = build(nfa, name, d).to(DEV)
    if hasattr(layer, "data_dep_init_done") or name.startswith("glow_block"):
        with torch.no_grad():
            layer.forward(data(name, B, d, F32))            # initialised by consistent data first
    del audit.forwarded[:]
    layer, x = _mismatch(kind, layer, lambda dtype: data(name, B, d, dtype))
    with torch.no_grad():
        _refused(lambda: layer.inverse(x))
        _refused(lambda: layer.forward(x))
    _refused(lambda: layer.inverse(x.clone().requires_grad_(True)))
    torch.cuda.synchronize()
    assert not audit.violations, audit.violations


@pytest.mark.parametrize("kind", KINDS)
def test_glue_and_bases_refuse_mismatched_dtypes(nfa, audit, kind):
    fl, dist = nfa.flows, nfa.distributions
    lab = torch.tensor([0, 2, 1, 1, 0], device=DEV)
    with torch.no_grad():
        if kind == "bf16_input":                            # no floating parameter: only an input the kernels do not take is a mismatch
            _refused(lambda: fl.Squeeze().inverse(img(B, 1, BF16)))
            _refused(lambda: nfa.transforms.Logit(0.05).inverse(img(B, 2, BF16, unit=True)))
        for d in (6, 8):
            q, x = _mismatch(kind, dist.DiagGaussian(d).to(DEV), lambda dtype: vec(B, d, 4, dtype))
            _refused(lambda: q.log_prob(x))
            cc, x = _mismatch(kind, dist.ClassCondDiagGaussian(d, 3).to(DEV), lambda dtype: vec(B, d, 5, dtype))
            _refused(lambda: cc.log_prob(x, lab))
            K = 8
            w, h, dd = (torch.randn(B, d, k, device=DEV) for k in (K, K, K - 1))
            other = {"f64_input": F64, "f32_input_double_module": F64, "bf16_module": BF16, "f16_module": F16, "bf16_input": BF16}[kind]
            if kind in ("f64_input", "bf16_input"):
                _refused(lambda: nfa.utils.splines.unconstrained_rational_quadratic_spline(vec(B, d, 8, other), w, h, dd, tail_bound=3.0))
            else:
                _refused(lambda: nfa.utils.splines.unconstrained_rational_quadratic_spline(vec(B, d, 8), w, h.to(other), dd, tail_bound=3.0))
    torch.cuda.synchronize()
    assert not audit.violations, audit.violations


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", MODELS)
def test_models_refuse_mismatched_dtypes(nfa, audit, name, kind):
    _, m, x_of, c_of = model_case(nfa, name)
    m, x = _mismatch(kind, m, lambda dtype: x_of(B, dtype))
    cdt = next((p.dtype for p in m.parameters()), F32)
    extra = () if c_of is None else (c_of(B, cdt),)        # (the context follows the module: the input is the operand under test)
    with torch.no_grad():
        _refused(lambda: m.log_prob(x, *extra))
    _refused(lambda: m.forward_kld(x, *extra))
    with torch.no_grad():
        if kind in ("bf16_module", "f16_module"):
            _refused(lambda: m.sample(B, *extra))
        elif kind == "f32_input_double_module":             # sampling takes no input: a .double() model is consistent, and must stay so
            out = m.sample(B, *extra)
            assert out[0].dtype == F64 and out[1].dtype == F64
    torch.cuda.synchronize()
    assert not audit.violations, audit.violations


@pytest.mark.parametrize("amp", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("name", MODELS)
def test_models_under_autocast(nfa, audit, name, amp):
    """torch.autocast changes what torch's own modules return, never what a kernel of this library reads: a route that hands the
    parameters to one kernel is unaffected (float32 result); a layer-wise route whose conditioner output arrives in half precision casts
    it (the affine layers) or refuses (TypeError).  Either way no call with mixed operands is made."""
    _, m, x_of, c_of = model_case(nfa, name)
    extra = () if c_of is None else (c_of(B, F32),)
    with torch.no_grad(), torch.autocast("cuda", dtype=amp):
        try:
            lp = m.log_prob(x_of(B, F32), *extra)
        except (TypeError, RuntimeError) as e:
            assert isinstance(e, TypeError) or "type" in str(e).lower(), e
        else:
            assert lp.dtype == F32 and lp.shape == (B,)
    torch.cuda.synchronize()
    assert not audit.violations, audit.violations


# ---- 3. conditioner outputs -------------------------------------------------------------------------------------------------------------
class Net(torch.nn.Module):
    """A caller-supplied conditioner: a Linear whose output goes through `post`."""

    def __init__(self, d_in, d_out, post):
        super().__init__()
        self.lin = torch.nn.Linear(d_in, d_out)
        self.post = post

    def forward(self, x):
        return self.post(self.lin(x))


POSTS = {      # name -> (what the caller's module does to its output, the explicit form the layer must agree with bit for bit, autocast)
    "to_bf16": (lambda o, z: o.to(BF16), lambda o, z: o.to(BF16).float(), None),
    "to_f16": (lambda o, z: o.to(F16), lambda o, z: o.to(F16).float(), None),
    "autocast_bf16": (lambda o, z: o, lambda o, z: o.float(), BF16),
    "autocast_f16": (lambda o, z: o, lambda o, z: o.float(), F16),
    "B1": (lambda o, z: o[:, :1], lambda o, z: o[:, :1].expand(z), None),
    "inner": (lambda o, z: o[0], lambda o, z: o[0].expand(z), None),
    "1inner": (lambda o, z: o[:1], lambda o, z: o[:1].expand(z), None),
}


def _pair_of_layers(nfa, kind, d, posts):
    """(layer with the caller's module as it is, layer with the explicit cast / expansion, autocast dtype): the same weights.
    posts: an entry of POSTS."""
    post, explicit, amp = posts
    torch.manual_seed(d)
    c1 = (d + 1) // 2
    shape = (B, d) if kind == "masked" else (B, 2 * (d - c1))

    def make(p):
        if kind == "masked":
            mask = torch.tensor([1.0, 0.0] * (d // 2))
            return nfa.flows.MaskedAffineFlow(mask, Net(d, d, lambda o: p(o, shape)), Net(d, d, lambda o: p(o, shape)))
        return nfa.flows.AffineCouplingBlock(Net(c1, 2 * (d - c1), lambda o: p(o, shape)))
    a = make(post).to(DEV)
    b = make(explicit).to(DEV)
    b.load_state_dict(copy.deepcopy(a.state_dict()))
    return a, b, amp


def _run(layer, x, inverse, grad, amp):
    ctx = torch.autocast("cuda", dtype=amp) if amp is not None else torch.autocast("cuda", enabled=False)
    xg = x.clone().requires_grad_(grad)
    with torch.set_grad_enabled(grad), ctx:
        y, ld = layer.inverse(xg) if inverse else layer.forward(xg)
    if not grad:
        return [y, ld]
    (y * torch.arange(1, y.numel() + 1, device=DEV, dtype=y.dtype).view_as(y)).sum().add((ld * 0.5).sum()).backward()
    return [y.detach(), ld.detach(), xg.grad] + [p.grad for p in layer.parameters()]


@pytest.mark.parametrize("grad", [False, True], ids=["eager", "autograd"])
@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
@pytest.mark.parametrize("d", [6, 8])
@pytest.mark.parametrize("kind,post", [("masked", p) for p in sorted(POSTS)]
                         # (the expansion rule is MaskedAffineFlow's: a coupling block's parameter tensor has its own size check)
                         + [("block", p) for p in sorted(POSTS) if p not in ("B1", "inner", "1inner")])
def test_conditioner_outputs_are_cast_and_expanded(nfa, audit, kind, post, d, inverse, grad):
    a, b, amp = _pair_of_layers(nfa, kind, d, POSTS[post])
    x = vec(B, d, 21)
    got, want = _run(a, x, inverse, grad, amp), _run(b, x, inverse, grad, amp)
    torch.cuda.synchronize()
    assert not audit.violations, audit.violations
    assert len(got) == len(want) and audit.forwarded
    for i, (g, w) in enumerate(zip(got, want)):
        assert g is not None and w is not None and g.dtype == F32 and same(g, w), (i, kind, post)


@pytest.mark.parametrize("grad", [False, True], ids=["eager", "autograd"])
@pytest.mark.parametrize("kind", ["masked", "block"])
def test_wider_conditioner_output_is_refused(nfa, blocked, kind, grad):
    a, _, _ = _pair_of_layers(nfa, kind, 6, (lambda o, z: o.double(),) * 2 + (None,))
    x = vec(B, 6, 22).requires_grad_(grad)
    with torch.set_grad_enabled(grad):
        for run in (a.forward, a.inverse):
            with pytest.raises(TypeError):
                run(x)
    assert not blocked.seen, blocked.names()


@pytest.mark.parametrize("grad", [False, True], ids=["eager", "autograd"])
@pytest.mark.parametrize("bad", ["inner+1", "B-1"])
@pytest.mark.parametrize("kind", ["masked", "block"])
def test_missized_conditioner_output_is_refused_before_the_abi(nfa, blocked, kind, bad, grad):
    a, _, _ = _pair_of_layers(nfa, kind, 6, ((lambda o, z: torch.cat([o, o[:, :1]], 1)) if bad == "inner+1" else (lambda o, z: o[:-1]),) * 2 + (None,))
    x = vec(B, 6, 23).requires_grad_(grad)
    with torch.set_grad_enabled(grad):
        for run in (a.forward, a.inverse):
            with pytest.raises(ValueError):
                run(x)
    assert not blocked.seen, blocked.names()


# ---- 4. sizes at the bases and the function API -----------------------------------------------------------------------------------------
def test_missized_operands_are_refused_before_the_abi(nfa, blocked):
    dist = nfa.distributions
    K = 8
    w, h, dd = (torch.randn(B, 6, k, device=DEV) for k in (K, K, K + 1))
    cases = [
        lambda: dist.DiagGaussian(8).to(DEV).log_prob(vec(B, 6, 1)),
        lambda: dist.ClassCondDiagGaussian(8, 3).to(DEV).log_prob(vec(B, 6, 2), torch.tensor([0, 2, 1, 1, 0], device=DEV)),
        lambda: dist.ClassCondDiagGaussian(6, 3).to(DEV).log_prob(vec(B, 8, 2), torch.tensor([0, 2, 1, 1, 0], device=DEV)),
        lambda: nfa.utils.splines.rational_quadratic_spline(vec(B, 6, 3, lo=0.01), w[:4], h, dd),
        lambda: nfa.utils.splines.rational_quadratic_spline(vec(B, 6, 3, lo=0.01), w, h, dd[:, :5]),
        lambda: nfa.utils.splines.unconstrained_rational_quadratic_spline(vec(B, 6, 3), w, h, torch.randn(B, 6, K + 2, device=DEV)),
        lambda: nfa.ops.actnorm(vec(B, 6, 4), torch.zeros(7, device=DEV), torch.zeros(7, device=DEV), 0),
        lambda: nfa.ops.actnorm(img(B, 4), torch.zeros(3, device=DEV), torch.zeros(2, device=DEV), 0),
        lambda: nfa.ops.masked_affine(vec(B, 8, 5), torch.zeros(8, device=DEV), vec(B, 6, 5), None, 0),
        lambda: nfa.ops.lu_linear_permute(vec(B, 8, 6), torch.arange(8, device=DEV), torch.zeros(15, device=DEV), torch.zeros(28, device=DEV),
                                          torch.zeros(8, device=DEV), torch.zeros(8, device=DEV), 0),
    ]
    with torch.no_grad():
        for i, fn in enumerate(cases):
            with pytest.raises(ValueError):
                fn()
            assert not blocked.seen, (i, blocked.names())
