"""The blob of the d-dimensional residual-flow kernels (csrc/lipmlp_nd.hip) for a run of [Residual | ActNorm | AffineConstFlow]
layers on (B, d) rows, 3 <= d <= 64, at inference, and the routes onto them (config.residual_nd, default off; config.residual_chain
must be on as well).  The 2-D route's predicates (flows/lipmlp_pack.py: linears, residual_ok, eligible) keep their results; the
conditions of this route are the ones below.

blob, dp = d rounded up to a multiple of 4, hp = the widest hidden layer of the run padded to 32, 64 or 128 (include/nf_mi355x.h has
the table):

    K headers of 16 floats in EXECUTION order
             [0] kind: 0 Residual, 1 affine forward y = z e + t, 2 affine inverse y = (z - t) e
             [1] hidden products (0 .. 2)     [2 .. 5] softplus(beta) of the Swish in front of linear layer 0 .. 3
             [10] the affine log-det +-sum(s)   [11] index of the weight block = index into vareps / terms / coefs
    K affine slots of 2 dp floats: e = exp(+-s) (dp) | t (dp); zeros for a Residual record
    one block per Residual record: W_0^T (dp, hp) | b_0 (hp) | 2 x [W_m^T (hp, hp) | b_m (hp)] | W_last^T (hp, dp) | b_last (dp)

Every W is the EFFECTIVE weight W / max(1, (u . W v) / coeff), built with lipmlp_pack.effective_weights (every layer's `scale` buffer
receives its sigma, as on the torch route), and the blob is cached through _keys.pcached against the tensors of the 2-D pack.

Random draws (residual.py:188-228): the reference draws np.random.geometric / poisson, then ONE torch.randn_like(x), per layer at
that layer's turn; the two generators are independent streams and the affine layers draw nothing.  A run therefore draws every
layer's truncation in layer order (iResBlock._truncation(), unchanged), then every layer's vareps in layer order, then launches.  A
layer whose draw has more than MAX_TERMS terms cuts the run in front of it: it takes Residual._torch_pass with the draw it already
has and draws its own randn_like at its turn; the later layers' draws are made after that.  Both generators end where the formulas
leave them."""
import torch
from torch.nn import functional as F

from .. import _keys
from .. import config as _config
from . import lipmlp_pack

MAX_RECORDS = 32        # records per launch (nf_lipmlp_nd_chain); core.run_chain cuts longer runs
MAX_RES = 8             # Residual records per launch
MAX_TERMS = 48          # series terms per record
DMIN, DMAX = 3, 64
HDR = 16
HMAX = lipmlp_pack.HMAX
ATOL = RTOL = lipmlp_pack.ATOL
MAX_ITER = lipmlp_pack.MAX_ITER

_lipmlp_nd_cache = {}   # (id of the run's first layer, K) -> (version key, (blob, hp, nres, d))
last_iterations = None  # further fixed-point steps of the last run_sampling call (residual.py:135-141's i)


def linears(net):
    """[(Swish, InducedNormLinear), ...] of a LipschitzMLP these kernels take, else None: exact types, d -> h_1 (-> h_2 (-> h_3))
    -> d with 3 <= d <= 64, every h <= 128 and every layer biased."""
    from ..nets import InducedNormLinear, LipschitzMLP, Swish
    if type(net) is not LipschitzMLP:
        return None
    mods = list(net.net)
    if len(mods) % 2 or not 4 <= len(mods) <= 8:
        return None
    pairs = list(zip(mods[0::2], mods[1::2]))
    if any(type(s) is not Swish or type(l) is not InducedNormLinear or l.bias is None for s, l in pairs):
        return None
    d = pairs[0][1].in_features
    if not DMIN <= d <= DMAX or pairs[-1][1].out_features != d:
        return None
    if any(a[1].out_features != b[1].in_features or not 1 <= a[1].out_features <= HMAX for a, b in zip(pairs, pairs[1:])):
        return None
    return pairs


_is_residual = lipmlp_pack._is_residual


def dim(f):
    """d of a Residual layer whose net linears() accepts."""
    return f.iresblock.nnet.net[1].in_features


def residual_ok(f):
    """A Residual layer (exact type) in evaluation mode whose log-det is Hutchinson's power series (exact_trace off) and whose net
    the kernels take."""
    return bool(_is_residual(f) and not f.iresblock.training and not f.iresblock.exact_trace
                and f.iresblock.n_dist in ("geometric", "poisson") and linears(f.iresblock.nnet) is not None)


def _affine_ok(f, d=None):
    from .affine import AffineConstFlow
    from .normalization import ActNorm
    if type(f) is ActNorm:
        if not f.initialised():
            return False
    elif type(f) is not AffineConstFlow:
        return False
    n = f.s.numel()
    return DMIN <= n <= DMAX and f.t.numel() == n and (d is None or n == d)


def classify(f):
    """d for a Residual layer these kernels take (residual_ok), -d for an affine layer of d elements they take, 0 for anything
    else: one walk of the layer, for the callers that look at every layer of a run."""
    if _is_residual(f):
        return dim(f) if residual_ok(f) else 0
    if _affine_ok(f):
        return -f.s.numel()
    return 0


def member(f, d=None):
    c = abs(classify(f))
    return bool(c) and (d is None or c == d)


def tensors(run):
    """Everything the blob is computed from: parameters, s / t of the affine layers, and u, v (the tensors of the 2-D pack)."""
    out = []
    for f in run:
        if _is_residual(f):
            for sw, lin in linears(f.iresblock.nnet):
                out += [sw.beta, lin.weight, lin.bias, lin.u, lin.v]
        else:
            out += [f.s, f.t]
    return out


def on_device(z):
    """The kernels' input: a CUDA float32 contiguous (B, d) tensor with 3 <= d <= 64 and B > 0."""
    return bool(torch.is_tensor(z) and z.is_cuda and z.dtype == torch.float32 and z.dim() == 2 and DMIN <= z.shape[1] <= DMAX
                and z.shape[0] > 0 and z.is_contiguous())


def eligible(run, z, sampling=False, kinds=None):
    """True when the kernels take the layers `run` on z: both switches on, a CUDA float32 contiguous (B, d) tensor with 3 <= d <= 64
    and B > 0, members of that d only with 1 .. 8 Residuals among at most 32 layers, all Residuals' density direction the same,
    float32 tensors on z's device, no gradient needed (grad disabled, or neither z nor any parameter of the run requires one) and
    not inside config.higher_order_gradients(), and not while a stream is being captured: iResBlock._truncation() reads geom_p /
    lamb back from the device (one `.item()` per Residual layer, as on the torch formulas), so the route synchronises once per
    Residual layer in front of its launch and cannot be recorded.  sampling: the fixed-point route of ONE layer.  kinds: classify() of every layer, where the caller has them already."""
    if not (_config.residual_nd and _config.residual_chain and not _config.torch_elementwise and on_device(z)
            and 1 <= len(run) <= MAX_RECORDS):
        return False
    d = z.shape[1]
    if kinds is None:
        kinds = [classify(f) for f in run]
    if any(abs(c) != d for c in kinds):
        return False
    res = [f for f, c in zip(run, kinds) if c > 0]
    if not 1 <= len(res) <= MAX_RES or any(bool(f.reverse) != bool(res[0].reverse) for f in res):
        return False
    if torch.is_grad_enabled() and (z.requires_grad or any(p.requires_grad for f in run for p in f.parameters())):
        return False
    if any(t.dtype != torch.float32 or t.device != z.device for t in tensors(run)):
        return False
    if z.is_cuda and torch.cuda.is_current_stream_capturing():
        return False
    if sampling and len(run) != 1:
        return False
    return True


def width(run):
    """hp of a run: its widest hidden layer padded to what the kernels are built for (nf_lipmlp_width: 32, 64 or 128)."""
    from .. import ops
    return ops.lipmlp_width(max(lin.out_features for f in run if _is_residual(f) for _, lin in linears(f.iresblock.nnet)[:-1]))


def dpad(d):
    return (d + 3) // 4 * 4


def rstride(hp, d):
    return 2 * hp * hp + 2 * dpad(d) * hp + 3 * hp + dpad(d)


def blob_floats(K, nres, hp, d):
    return K * HDR + K * 2 * dpad(d) + nres * rstride(hp, d)


def pack(run, inverse, hp=None):
    """(blob, hp, nres, d) of the layers `run` in EXECUTION order; inverse: the affine layers run their inverse."""
    with torch.no_grad():
        hp = width(run) if hp is None else hp
        K = len(run)
        res = [f for f in run if _is_residual(f)]
        d = dim(res[0])
        dp = dpad(d)
        dev = res[0].iresblock.geom_p.device
        nets = [linears(f.iresblock.nnet) for f in res]
        weff = lipmlp_pack.effective_weights([lin for pairs in nets for _, lin in pairs])
        blob = torch.zeros(blob_floats(K, len(res), hp, d), dtype=torch.float32, device=dev)
        hdr = blob[:K * HDR].view(K, HDR)
        aff = blob[K * HDR:K * HDR + K * 2 * dp].view(K, 2, dp)
        base = K * HDR + K * 2 * dp
        ri = wi = 0
        for q, f in enumerate(run):
            if not _is_residual(f):
                s, t = f.s.detach().reshape(d), f.t.detach().reshape(d)
                hdr[q, 0] = 2.0 if inverse else 1.0
                aff[q, 0, :d] = torch.exp(-s) if inverse else torch.exp(s)
                aff[q, 1, :d] = t
                hdr[q, 10] = -s.sum() if inverse else s.sum()
                continue
            pairs = nets[ri]
            n = len(pairs)
            hdr[q, 1] = float(n - 2)
            hdr[q, 2:2 + n] = F.softplus(torch.cat([sw.beta.detach() for sw, _ in pairs]))
            hdr[q, 11] = float(ri)
            blk = blob[base + ri * rstride(hp, d):base + (ri + 1) * rstride(hp, d)]
            h1 = pairs[0][1].out_features
            blk[:dp * hp].view(dp, hp)[:d, :h1] = weff[wi].t()
            blk[dp * hp:dp * hp + h1] = pairs[0][1].bias.detach()
            for m in range(n - 2):
                lin = pairs[1 + m][1]
                o = dp * hp + hp + m * (hp * hp + hp)
                blk[o:o + hp * hp].view(hp, hp)[:lin.in_features, :lin.out_features] = weff[wi + 1 + m].t()
                blk[o + hp * hp:o + hp * hp + lin.out_features] = lin.bias.detach()
            o = dp * hp + hp + 2 * (hp * hp + hp)
            last = pairs[-1][1]
            blk[o:o + hp * dp].view(hp, dp)[:last.in_features, :d] = weff[wi + n - 1].t()
            blk[o + hp * dp:o + hp * dp + d] = last.bias.detach()
            ri += 1
            wi += n
    return blob, hp, len(res), d


def _cached_pack(run, inverse):
    return _keys.pcached(globals(), "_lipmlp_nd_cache", tensors(run), (bool(inverse),), lambda: pack(run, inverse),
                         sub=(id(run[0]), len(run)))


def coefficients(truncation):
    """(terms, [coef(1) .. coef(terms)]) of an iResBlock._truncation() result."""
    n_terms, coeff, _ = truncation
    n_terms = int(n_terms)
    return n_terms, [float(coeff(k)) for k in range(1, n_terms + 1)]


def _launch(run, z, vareps, terms, coefs, ld, acc, inverse):
    from .. import ops
    blob, hp, nres, _ = _cached_pack(run, inverse)
    return ops.lipmlp_nd_chain(z, vareps, blob, len(run), nres, hp, terms, coefs, logdet=ld, acc=acc)


def run_density_noise(run, z, vareps, terms, coefs, ld=None, acc=None, inverse=False):
    """The explicit-noise entry of a run (EXECUTION order; eligible(run, z) holds): vareps (nres, B, d), terms and coefs per Residual
    layer in execution order.  Nothing is drawn.  ld None: returns (z', log_det); else folds the log-det into `ld` by `acc` and
    returns z'."""
    y, log_det = _launch(run, z, vareps, terms, coefs, ld, acc, inverse)
    return (y, log_det) if ld is None else y


def run_density(run, z, ld, acc, inverse=False):
    """The layers `run` (EXECUTION order; eligible(run, z) holds), every Residual in its density direction x + g(x) and every affine
    layer in the direction `inverse` says: one launch, or -- where a layer's drawn truncation has more than MAX_TERMS terms -- one
    launch per stretch between such layers, which take the torch formulas with their draw.  The draws come in the order the module
    docstring gives.  ld None: returns (z', log_det); else folds the log-det into `ld` by `acc` and returns z'."""
    from .. import _lib as L
    from .base import run_flow
    own = ld is None
    if own:
        ld, acc = torch.zeros(z.shape[0], dtype=z.dtype, device=z.device), L.LD_ADD
    k = 0
    while k < len(run):
        truncs, end, long_draw = [], len(run), None
        for q in range(k, len(run)):
            if _is_residual(run[q]):
                t = run[q].iresblock._truncation()
                if not 1 <= t[0] <= MAX_TERMS:
                    end, long_draw = q, t
                    break
                truncs.append(t)
        seg = run[k:end]
        if truncs:
            pairs = [coefficients(t) for t in truncs]
            vareps = torch.empty((len(truncs),) + tuple(z.shape), dtype=z.dtype, device=z.device)
            for v in vareps:                    # one draw per layer in layer order, as randn_like(z) makes it, straight into its slice
                v.normal_()
            z = _launch(seg, z, vareps, [p[0] for p in pairs], [p[1] for p in pairs], ld, acc, inverse)[0]
        else:
            for f in seg:                       # affine layers in front of a layer that keeps the formulas
                z = run_flow(f, z, inverse, ld, acc)
        k = end
        if long_draw is not None:
            z, log_det = run[k]._torch_pass(z, True, long_draw)
            if acc > 0:
                ld += log_det
            else:
                ld -= log_det
            k += 1
    return (z, ld) if own else z


def run_sampling(layer, z, noise=None):
    """The fixed-point direction of ONE Residual layer: x <- z - g(x) from x = z, one launch and one 4-byte read-back per step, with
    the reference's stop rule over all rows (residual.py:133-142); then the layer's truncation and noise are drawn and one K = 1
    density launch gives the series at the point found (more than MAX_TERMS terms: the formulas' estimator, with that draw).
    noise: (vareps (B, d), terms, coefs) handed in instead of drawn (tests and fixtures).  Returns (x, -log_det estimate)."""
    global last_iterations
    from .. import ops
    blob, hp, _, _ = _cached_pack([layer], False)
    counts = torch.zeros(MAX_ITER + 2, dtype=torch.int32, device=z.device)
    x = ops.lipmlp_nd_apply(z, z, blob, hp, 1, counts[0:1])
    i = 0
    while int(counts[i]) != 0:
        x = ops.lipmlp_nd_apply(x, z, blob, hp, 1, counts[i + 1:i + 2])
        i += 1
        if i > MAX_ITER:
            break
    last_iterations = i
    if noise is None:
        trunc = layer.iresblock._truncation()
        if not 1 <= trunc[0] <= MAX_TERMS:
            return x, layer.iresblock._logdetgrad(x, trunc)[1].view(-1).neg()
        terms, coefs = coefficients(trunc)
        vareps = torch.randn_like(x)
    else:
        vareps, terms, coefs = noise
    _, log_det = _launch([layer], x, vareps.reshape((1,) + tuple(x.shape)), [terms], [coefs], None, None, False)
    return x, -log_det
