"""The blob of the residual-flow kernels (csrc/lipmlp.hip) for a run of [Residual | ActNorm | AffineConstFlow] layers, and the
routes onto them.

blob = K headers of 16 floats in EXECUTION order, then one weight block per Residual record; hp = the widest hidden layer of the
run padded to 32, 64 or 128 (include/nf_mi355x.h has the table):

    header   [0] kind: 0 Residual, 1 affine forward y = z e + t, 2 affine inverse y = (z - t) e
             [1] hidden products (0 .. 2)     [2 .. 5] softplus(beta) of the Swish in front of linear layer 0 .. 3
             [6, 7] e = exp(+-s)   [8, 9] t   [10] the affine log-det +-sum(s)   [11] index of the weight block
    block    W_0^T (2, hp) | b_0 (hp) | 2 x [W_m^T (hp, hp) | b_m (hp)] | W_last (2, hp) | b_last (2) | 2 zeros

Every W is the EFFECTIVE weight W / max(1, (u . W v) / coeff) (lipschitz.py:264-270), computed HERE with torch from the stored u, v,
on the run's linear layers stacked by shape -- one batched product per shape whatever the number of layers -- and, as on the torch
route, every layer's `scale` buffer receives its sigma.  The blob is cached against the versions of the parameters AND of the
buffers u, v (_keys.pcached): update_lipschitz rewrites those in place and changes the effective weight without touching a
parameter.

Training (csrc/lipmlp_train.hip, config.residual_train): ONE Residual layer per call; pack_train builds the same record from the
LIVE parameters with differentiable torch operations, so the kernel's blob gradient reaches weight, bias and beta -- through the
division by max(1, sigma / coeff) and through softplus -- by torch's autograd; train_eligible has the conditions, run_train the
order of the random draws."""
import torch
from torch.nn import functional as F

from .. import _keys
from .. import config as _config

MAX_RECORDS = 32        # records per launch (nf_lipmlp_chain); core.run_chain cuts longer runs
HMAX = 128              # widest hidden layer
HDR = 16
ATOL = RTOL = 1e-5      # the fixed-point stop rule (residual.py:133)
MAX_ITER = 1000
MAX_TERMS = 32          # series terms of one training forward (nf_lipmlp_train_fwd)

_lipmlp_cache = {}      # (id of the run's first layer, K) -> (version key, (blob, hp, nres))
last_iterations = None  # further fixed-point steps of the last run_sampling call (residual.py:135-141's i)


def linears(net):
    """[(Swish, InducedNormLinear), ...] of a LipschitzMLP the kernels take, else None: exact types, 2 -> h_1 (-> h_2 (-> h_3)) -> 2
    with every h <= 128 and every layer biased."""
    from ..nets import InducedNormLinear, LipschitzMLP, Swish
    if type(net) is not LipschitzMLP:
        return None
    mods = list(net.net)
    if len(mods) % 2 or not 4 <= len(mods) <= 8:
        return None
    pairs = list(zip(mods[0::2], mods[1::2]))
    if any(type(s) is not Swish or type(l) is not InducedNormLinear or l.bias is None for s, l in pairs):
        return None
    if pairs[0][1].in_features != 2 or pairs[-1][1].out_features != 2:
        return None
    if any(a[1].out_features != b[1].in_features or not 1 <= a[1].out_features <= HMAX for a, b in zip(pairs, pairs[1:])):
        return None
    return pairs


def _is_residual(f):
    from .residual import Residual
    return type(f) is Residual


def _affine_ok(f):
    from .affine import AffineConstFlow
    from .normalization import ActNorm
    if type(f) is ActNorm:
        if not f.initialised():
            return False
    elif type(f) is not AffineConstFlow:
        return False
    return f.s.numel() == 2 and f.t.numel() == 2


def residual_ok(f):
    """A Residual layer (exact type) whose log-det is the deterministic brute-force one on 2-D rows and whose net the kernels take."""
    return _is_residual(f) and (f.iresblock.brute_force or not f.iresblock.training) and linears(f.iresblock.nnet) is not None


def member(f):
    return residual_ok(f) or _affine_ok(f)


def tensors(run):
    """Everything the blob is computed from: parameters, s / t of the affine layers (buffers when not trainable), and u, v."""
    out = []
    for f in run:
        if _is_residual(f):
            for sw, lin in linears(f.iresblock.nnet):
                out += [sw.beta, lin.weight, lin.bias, lin.u, lin.v]
        else:
            out += [f.s, f.t]
    return out


def eligible(run, z, sampling=False):
    """True when the kernels take the layers `run` on z: the switch on, a CUDA float32 contiguous (B, 2) tensor, members only with at
    least one Residual, all Residuals' density direction the same, float32 tensors on z's device, no gradient needed (grad disabled,
    or neither z nor any parameter of the run requires one) and not inside config.higher_order_gradients().  sampling: the
    fixed-point route of ONE layer, which synchronises and so is not taken while a stream is being captured."""
    if not (_config.residual_chain and not _config.torch_elementwise and torch.is_tensor(z) and z.is_cuda
            and z.dtype == torch.float32 and z.dim() == 2 and z.shape[1] == 2 and z.is_contiguous()
            and 1 <= len(run) <= MAX_RECORDS):
        return False
    if not all(member(f) for f in run):
        return False
    res = [f for f in run if _is_residual(f)]
    if not res or any(bool(f.reverse) != bool(res[0].reverse) for f in res):
        return False
    if torch.is_grad_enabled() and (z.requires_grad or any(p.requires_grad for f in run for p in f.parameters())):
        return False
    if any(t.dtype != torch.float32 or t.device != z.device for t in tensors(run)):
        return False
    if sampling and (len(run) != 1 or torch.cuda.is_current_stream_capturing()):
        return False
    return True


def width(run):
    """hp of a run: its widest hidden layer padded to what the kernels are built for (nf_lipmlp_width: 32, 64 or 128)."""
    from .. import ops
    return ops.lipmlp_width(max(lin.out_features for f in run if _is_residual(f) for _, lin in linears(f.iresblock.nnet)[:-1]))


def rstride(hp):
    return 2 * hp * hp + 7 * hp + 4


def effective_weights(lins):
    """[W / max(1, sigma / coeff)] of the InducedNormLinear layers `lins`, sigma = u . W v from the stored buffers, computed on the
    layers stacked by (shape, coeff); every layer's `scale` receives its sigma (lipschitz.py:264-266)."""
    out = [None] * len(lins)
    groups = {}
    for i, l in enumerate(lins):
        groups.setdefault((tuple(l.weight.shape), float(l.coeff)), []).append(i)
    for (_, coeff), idx in groups.items():
        W = torch.stack([lins[i].weight.detach() for i in idx])
        u = torch.stack([lins[i].u for i in idx])
        v = torch.stack([lins[i].v for i in idx])
        sigma = (u * torch.bmm(W, v.unsqueeze(2)).squeeze(2)).sum(1)
        torch._foreach_copy_([lins[i].scale for i in idx], list(sigma.unbind(0)))
        Weff = W / torch.clamp(sigma / coeff, min=1.0).reshape(-1, 1, 1)
        for j, i in enumerate(idx):
            out[i] = Weff[j]
    return out


def pack(run, inverse, hp=None):
    """(blob, hp, nres) of the layers `run` in EXECUTION order; inverse: the affine layers run their inverse."""
    with torch.no_grad():
        hp = width(run) if hp is None else hp
        K = len(run)
        res = [f for f in run if _is_residual(f)]
        dev = res[0].iresblock.geom_p.device
        nets = [linears(f.iresblock.nnet) for f in res]
        flat = [lin for pairs in nets for _, lin in pairs]
        weff = effective_weights(flat)
        blob = torch.zeros(K * HDR + len(res) * rstride(hp), dtype=torch.float32, device=dev)
        hdr = blob[:K * HDR].view(K, HDR)
        ri = wi = 0
        for q, f in enumerate(run):
            if not _is_residual(f):
                s, t = f.s.detach().reshape(2), f.t.detach().reshape(2)
                hdr[q, 0] = 2.0 if inverse else 1.0
                hdr[q, 6:8] = torch.exp(-s) if inverse else torch.exp(s)
                hdr[q, 8:10] = t
                hdr[q, 10] = -s.sum() if inverse else s.sum()
                continue
            pairs = nets[ri]
            n = len(pairs)
            hdr[q, 1] = float(n - 2)
            hdr[q, 2:2 + n] = F.softplus(torch.cat([sw.beta.detach() for sw, _ in pairs]))
            hdr[q, 11] = float(ri)
            blk = blob[K * HDR + ri * rstride(hp):K * HDR + (ri + 1) * rstride(hp)]
            h1 = pairs[0][1].out_features
            blk[:2 * hp].view(2, hp)[:, :h1] = weff[wi].t()
            blk[2 * hp:2 * hp + h1] = pairs[0][1].bias.detach()
            for m in range(n - 2):
                lin = pairs[1 + m][1]
                o = 3 * hp + m * (hp * hp + hp)
                blk[o:o + hp * hp].view(hp, hp)[:lin.in_features, :lin.out_features] = weff[wi + 1 + m].t()
                blk[o + hp * hp:o + hp * hp + lin.out_features] = lin.bias.detach()
            o = 3 * hp + 2 * (hp * hp + hp)
            last = pairs[-1][1]
            blk[o:o + 2 * hp].view(2, hp)[:, :last.in_features] = weff[wi + n - 1]
            blk[o + 2 * hp:o + 2 * hp + 2] = last.bias.detach()
            ri += 1
            wi += n
    return blob, hp, len(res)


def _cached_pack(run, inverse):
    return _keys.pcached(globals(), "_lipmlp_cache", tensors(run), (bool(inverse),), lambda: pack(run, inverse),
                         sub=(id(run[0]), len(run)))


def run_density(run, z, ld, acc, inverse=False):
    """The layers `run` (EXECUTION order; eligible(run, z) holds) as one launch, every Residual in its density direction x + g(x) and
    every affine layer in the direction `inverse` says.  ld None: returns (z', log_det); else folds the log-det into `ld` by `acc`
    and returns z'."""
    from .. import ops
    blob, hp, nres = _cached_pack(run, inverse)
    y, log_det = ops.lipmlp_chain(z, blob, len(run), nres, hp, logdet=ld, acc=acc)
    return (y, log_det) if ld is None else y


def run_sampling(layer, z):
    """The fixed-point direction of ONE Residual layer: x <- z - g(x) from x = z, one launch and one read-back per step, with the
    reference's stop rule over all rows (residual.py:133-142); then one launch for the Jacobian at the point found.  Returns
    (x, -log|det(I + J(x))|)."""
    global last_iterations
    from .. import ops
    blob, hp, _ = _cached_pack([layer], False)
    counts = torch.zeros(MAX_ITER + 2, dtype=torch.int32, device=z.device)
    x = ops.lipmlp_apply(z, z, blob, hp, 1, counts[0:1])
    i = 0
    while z.shape[0] and int(counts[i]) != 0:
        x = ops.lipmlp_apply(x, z, blob, hp, 1, counts[i + 1:i + 2])
        i += 1
        if i > MAX_ITER:
            break
    last_iterations = i
    _, log_det = ops.lipmlp_chain(x, blob, 1, 1, hp)
    return x, -log_det


def pack_train(layer, hp=None):
    """The blob of ONE Residual record (the layout at the head of this file, K = 1) as a differentiable function of the layer's live
    parameters: effective weights W / max(1, (u . W v) / coeff) with the gradient through sigma and the maximum left to torch,
    softplus(beta), biases, zero padding.  Every layer's `scale` buffer receives its sigma, as on the torch route."""
    pairs = linears(layer.iresblock.nnet)
    hp = width([layer]) if hp is None else hp
    n = len(pairs)
    dev = pairs[0][1].weight.device
    weff = []
    for _, lin in pairs:
        sigma = torch.dot(lin.u, torch.mv(lin.weight, lin.v))
        with torch.no_grad():
            lin.scale.copy_(sigma)
        weff.append(lin.weight / torch.max(torch.ones(1, device=dev), sigma / lin.coeff))       # (lipschitz.py:270, as written)

    def zeros(k):
        return torch.zeros(k, dtype=torch.float32, device=dev)

    parts = [zeros(1), torch.full((1,), float(n - 2), dtype=torch.float32, device=dev),
             F.softplus(torch.cat([sw.beta for sw, _ in pairs])), zeros(HDR - 2 - n)]
    h1 = pairs[0][1].out_features
    parts += [F.pad(weff[0].t(), (0, hp - h1)).reshape(-1), F.pad(pairs[0][1].bias, (0, hp - h1))]
    for m in range(2):
        if m < n - 2:
            lin = pairs[1 + m][1]
            parts += [F.pad(weff[1 + m].t(), (0, hp - lin.out_features, 0, hp - lin.in_features)).reshape(-1),
                      F.pad(lin.bias, (0, hp - lin.out_features))]
        else:
            parts.append(zeros(hp * hp + hp))
    last = pairs[-1][1]
    parts += [F.pad(weff[-1], (0, hp - last.in_features)).reshape(-1), last.bias, zeros(2)]
    return torch.cat(parts)


def _on_device(z):
    """The kernels' input: a CUDA float32 contiguous (B, 2) tensor with B > 0."""
    return bool(torch.is_tensor(z) and z.is_cuda and z.dtype == torch.float32 and z.dim() == 2 and z.shape[1] == 2
                and z.shape[0] > 0 and z.is_contiguous())


def _stochastic(ires):
    """True when the layer's log-det on 2-D rows is one of the series estimators (training mode without brute_force)."""
    return bool(ires.training and not ires.brute_force)


def train_eligible(layer, z, density=True):
    """True when the training kernels take `layer` on z: both switches on, exact type Residual with a net linears() accepts, the
    density direction, a CUDA float32 contiguous (B, 2) tensor with B > 0, float32 tensors on z's device, not inside
    config.higher_order_gradients(), and EITHER a gradient is needed (grad enabled, and z or a parameter of the layer requires one)
    OR the layer is in training mode on a stochastic estimator (which the inference kernels do not compute).  While a stream is
    being captured only deterministic truncations are taken (brute force, evaluation mode, or n_power_series set): the host draw
    of a random truncation cannot be recorded."""
    if not (_config.residual_train and _config.residual_chain and not _config.torch_elementwise and density
            and _is_residual(layer) and _on_device(z)):
        return False
    ires = layer.iresblock
    if linears(ires.nnet) is None:
        return False
    needs_grad = torch.is_grad_enabled() and (z.requires_grad or any(p.requires_grad for p in layer.parameters()))
    if not (needs_grad or _stochastic(ires)):
        return False
    if any(t.dtype != torch.float32 or t.device != z.device for t in tensors([layer])):
        return False
    if _stochastic(ires) and ires.n_power_series is None and torch.cuda.is_current_stream_capturing():
        return False
    if _stochastic(ires) and ires.n_power_series is not None and not 1 <= ires.n_power_series <= MAX_TERMS:
        return False
    return True


def run_train(layer, z):
    """((y, log_det), None) of `layer` (train_eligible(layer, z) holds) in its density direction on the training kernels, or
    (None, truncation) when the drawn truncation has more than MAX_TERMS terms (or none): the caller runs the torch formulas
    with that draw.  The random draws come in the reference's order in front of the launch (residual.py:163-190): the NumPy
    truncation draw, then ONE torch.randn_like(z)."""
    from ..autograd import LipMlpTrainFn
    ires = layer.iresblock
    kind, coef, vareps, first_row, drawn = 0, (), None, False, None
    if _stochastic(ires):
        trunc = ires._truncation()
        n_terms, coeff, drawn = trunc
        if not 1 <= n_terms <= MAX_TERMS:
            return None, trunc
        coef = [float(coeff(k)) for k in range(1, n_terms + 1)]
        if ires.exact_trace:
            kind, coef[0] = 3, 1.0      # (the reference takes the first term's trace unweighted)
        else:
            vareps = torch.randn_like(z)
            kind = 2 if ires.neumann_grad else 1
            first_row = bool(ires.grad_in_forward)
    hp = width([layer])
    y, ld = LipMlpTrainFn.apply(z, pack_train(layer, hp), hp, kind, tuple(coef), vareps, first_row)
    if _stochastic(ires) and ires.n_power_series is None:
        with torch.no_grad():
            est = ld.detach()
            ires.last_n_samples.copy_(torch.tensor(drawn).to(ires.last_n_samples))
            ires.last_firmom.copy_(torch.mean(est).to(ires.last_firmom))
            ires.last_secmom.copy_(torch.mean(est ** 2).to(ires.last_secmom))
    return (y, ld), None
