"""Records of the rank-1 chain kernels (csrc/rank1_chain.hip) for a run of Planar / Radial layers, and the route onto them.

P is one float32 tensor of shape (K, 2 d + 4), one record per layer, d = prod(shape):

    [kind, s0, s1, s2, vecA[d], vecB[d]]

    field   Planar                      Radial
    kind    0 (tanh) or 1 (leaky)       2
    s0      b                           a = |alpha|
    s1      w . u_hat                   beta' = log(1 + exp(beta)) - |alpha|
    s2      slope 0.2                   d - 1
    vecA    w                           z_0
    vecB    u_hat                       unused, zero

Neither constraint is in a kernel: u_hat = u + (log(1 + exp(w . u)) - 1 - w . u) w / |w|^2 and beta' are computed HERE, with the
reference's torch expressions (planar.py:54-56, radial.py:38), on the run's parameters stacked with one torch.cat per kind of
parameter -- a handful of launches on (K, d) and (K) tensors whatever K is.  Under no_grad P is cached against the parameters'
versions (_keys.pcached); under autograd it is built from the live parameters in every forward, the kernels' gradient arrives as
gP (K, 2 d + 4), and torch's autograd carries it through these expressions and the cat to the leaves -- the reference's overflow
behaviour of log(1 + exp(.)) included.  The constant columns and the interleaving index live in a value-independent structure
(`_rank1_struct`), so a pass that has run once allocates nothing from host memory (stream capture)."""
import math

import torch

from .. import _keys
from .. import config as _config

KIND_RADIAL = 2
MAX_RECORDS = 64        # records per launch (nf_rank1_chain: P in LDS); core.run_chain cuts longer runs
DMAX = 128


def width(f):
    """d of a Planar / Radial layer: the elements of one row."""
    return (f.z_0 if hasattr(f, "z_0") else f.w).numel()


def kinds(run):
    from .planar import ACTS
    return tuple(KIND_RADIAL if hasattr(f, "z_0") else ACTS.index(f.act) for f in run)


def parameters(run):
    return [p for f in run for p in f.parameters()]


def _structure(kd, d, device):
    """Constant columns and the interleaving index of a run with kinds `kd`: {"pl": (Kp, 2) [kind, slope] columns, "ra": (Kr, 2)
    [kind, d - 1], "zeros": (Kr, d), "perm": index that puts [Planar rows; Radial rows] into layer order, or None}."""
    from .planar import SLOPE
    ip = [i for i, k in enumerate(kd) if k != KIND_RADIAL]
    ir = [i for i, k in enumerate(kd) if k == KIND_RADIAL]
    st = {"pl": None, "ra": None, "zeros": None, "perm": None}
    if ip:
        st["pl"] = torch.tensor([[float(kd[i]), SLOPE] for i in ip], dtype=torch.float32).to(device)
    if ir:
        st["ra"] = torch.tensor([[float(KIND_RADIAL), float(d - 1)] for _ in ir], dtype=torch.float32).to(device)
        st["zeros"] = torch.zeros(len(ir), d, dtype=torch.float32, device=device)
    if ip and ir:
        pos = {layer: row for row, layer in enumerate(ip + ir)}
        st["perm"] = torch.tensor([pos[i] for i in range(len(kd))], dtype=torch.int64).to(device)
    return st


_rank1_struct = {}      # (kinds, d, device) -> structure: no parameter value in it
_rank1_cache = {}       # (id of the run's first layer, K) -> (parameter-version key, P): the no_grad packs, both directions


def planar_rows(U, W, b, const):
    """(Kp, 2 d + 4) records of Planar layers from stacked u, w (Kp, d) and b (Kp); const = their [kind, slope] columns."""
    inner = (W * U).sum(1, keepdim=True)
    Uh = U + (torch.log(1 + torch.exp(inner)) - 1 - inner) * W / (W ** 2).sum(1, keepdim=True)
    s1 = (W * Uh).sum(1, keepdim=True)
    return torch.cat([const[:, :1], b.reshape(-1, 1), s1, const[:, 1:], W, Uh], 1)


def radial_rows(Z0, alpha, beta, const, zeros):
    """(Kr, 2 d + 4) records of Radial layers from stacked z_0 (Kr, d), alpha and beta (Kr)."""
    a = torch.abs(alpha).reshape(-1, 1)
    bp = torch.log(1 + torch.exp(beta)).reshape(-1, 1) - a
    return torch.cat([const[:, :1], a, bp, const[:, 1:], Z0, zeros], 1)


def pack(run, d, device):
    """P (K, 2 d + 4) of the layers `run` (forward order), differentiable in their parameters."""
    kd = kinds(run)
    key = (kd, d, str(device))
    st = _keys.cached(globals(), "_rank1_struct", key, lambda: _structure(kd, d, device), sub=key)
    pl = [f for f, k in zip(run, kd) if k != KIND_RADIAL]
    ra = [f for f, k in zip(run, kd) if k == KIND_RADIAL]
    rows = []
    if pl:
        rows.append(planar_rows(torch.cat([f.u.reshape(1, d) for f in pl]), torch.cat([f.w.reshape(1, d) for f in pl]),
                                torch.cat([f.b.reshape(1) for f in pl]), st["pl"]))
    if ra:
        rows.append(radial_rows(torch.cat([f.z_0.reshape(1, d) for f in ra]), torch.cat([f.alpha.reshape(1) for f in ra]),
                                torch.cat([f.beta.reshape(1) for f in ra]), st["ra"], st["zeros"]))
    P = rows[0] if len(rows) == 1 else torch.cat(rows).index_select(0, st["perm"])
    return P.contiguous()


def eligible(run, z, inverse):
    """True when the kernels take the layers `run` (exact Planar / Radial types, the caller's business) on input z: a CUDA float32
    tensor, contiguous, of prod(shape) <= 128 elements per row, float32 parameters on its device, the switch on and not inside
    config.higher_order_gradients() (the Function is once-differentiable); in the inverse direction every layer leaky."""
    if not (_config.rank1_chain and not _config.torch_elementwise and torch.is_tensor(z) and z.is_cuda
            and z.dtype == torch.float32 and z.dim() >= 2 and z.is_contiguous() and 1 <= len(run) <= MAX_RECORDS):
        return False
    d = math.prod(z.shape[1:])
    if not 1 <= d <= DMAX or any(width(f) != d or (hasattr(f, "u") and f.u.numel() != d) for f in run):
        return False
    if any(p.dtype != torch.float32 or p.device != z.device for p in parameters(run)):
        return False
    return not inverse or all(k == 1 for k in kinds(run))


def run(run_, z, inverse, ld, acc):
    """The layers `run_` (forward order; eligible(run_, z, inverse) holds) as one launch, or one forward and one backward launch
    under autograd.  ld None: returns (z', log_det); else folds the log-det into `ld` by `acc` and returns z'."""
    from .. import ops
    from .affine import _fold_ld
    B, d, K = z.shape[0], math.prod(z.shape[1:]), len(run_)
    direction = 1 if inverse else 0
    params = parameters(run_)
    z2 = z.reshape(B, d)
    if torch.is_grad_enabled() and (z.requires_grad or any(p.requires_grad for p in params)):
        from ..autograd import Rank1ChainFn
        y, log_det = Rank1ChainFn.apply(z2, pack(run_, d, z.device), kinds(run_), direction)
        y = y.reshape(z.shape)
        if ld is None:
            return y, log_det
        _fold_ld(ld, acc, log_det)
        return y

    def build():
        with torch.no_grad():
            return pack(run_, d, z.device)

    P = _keys.pcached(globals(), "_rank1_cache", params, (str(z.device), d), build, sub=(id(run_[0]), K))
    y, log_det = ops.rank1_chain(z2, P, kinds(run_), direction, logdet=ld, acc=acc)
    y = y.reshape(z.shape)
    return (y, log_det) if ld is None else y
