"""The operand audit of the C ABI: a spy in front of every call that CHECKS the tensors behind the pointers against the header and
the call's own scalar arguments, and does not forward a call that breaks a rule.

    audit = install(nfa, monkeypatch)               # every call is checked, a consistent one is forwarded
    audit = install(nfa, monkeypatch, block_all=True)   # nothing is forwarded: for cases that must raise before the ABI

While installed, `_lib.ptr` / `_lib.ptr_any` (and the names ops.py imported) return a c_void_p that remembers its tensor; the spy
replaces `_lib.call` and `_lib.call_rc`, looks every pointer argument up by the parameter NAME and declared pointee type of
include/nf_mi355x.h, and applies three rules:

  1. every floating-point tensor has the dtype the call's `dtype` argument names (float32 where the entry point has none);
  2. a parameter declared `const int64_t *`, `const int *` / `int32_t *`, `const double *`, `const float *` gets a tensor of exactly
     that element type;
  3. for the entry points of COUNTS the element counts hold against the scalar arguments of the same call.

A violating call is recorded in `audit.violations` and AuditViolation (an AssertionError: no `pytest.raises(TypeError)` swallows
it) is raised INSTEAD of the launch; the real entry point is reached with plain c_void_p arguments only when every rule holds.  So a
missing guard in ops.py shows as a failed assertion, never as a kernel reading past a buffer.  Pure Python on tensor attributes:
usable on CPU tensors with a stubbed forward (tests/test_host_operand_contract.py)."""
import ctypes
import re

import torch


class AuditViolation(AssertionError):
    pass


class TensorPtr(ctypes.c_void_p):
    """A c_void_p that remembers the tensor it points into."""
    tensor = None


_POINTEE = {"int64_t": torch.int64, "int": torch.int32, "int32_t": torch.int32, "uint32_t": torch.int32, "double": torch.float64,
            "float": torch.float32}

# (entry point, parameter) whose tensor differs from the call's dtype ON PURPOSE, with the dtype it must have instead
INTENDED = {("nf_actnorm_bwd", "scratch"): torch.float64}      # fp64 partial sums whatever the element type


def signatures(nfa):
    """{entry point: [(parameter name, declared pointee type or None for a scalar)]} from the header text."""
    out = {}
    for _, fn, params in re.findall(r"([A-Za-z_][\w \*]*?)\b(nf_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", nfa._lib._header_text()):
        sig = []
        for q in params.split(","):
            if q.strip() == "void":
                continue
            words = [w for w in q.replace("*", " * ").split() if w != "const"]
            sig.append((re.findall(r"\w+", q)[-1], words[0] if "*" in words else None))
        out[fn] = sig
    return out


# ---- rule 3: element counts by header parameter name (a: the call's scalars by name, t: its tensors by name) -----------------------
def _nd(K, tails):
    return K - 1 if tails == 1 else (K if tails == 2 else K + 1)


def _P(a):
    return (a["C"] - a["c1"]) * (1 if a["scale_map"] == 3 else 2)


def _spline_rows(a, t):
    bad = []
    N, K = a["N"], a["K"]
    for name, ld, ok in (("w", "ldw", (K,)), ("h", "ldh", (K,)), ("d", "ldd", (K - 1, K, K + 1))):
        x = t.get(name)
        if x is None:
            continue
        if x.dim() != 2 or x.shape[0] != N or x.shape[1] not in ok or (N > 0 and a[ld] != x.stride(0)) or (x.stride(1) != 1 and N > 0):
            bad.append("%s: rows %s stride %s for N = %d, K = %d, ld = %d" % (name, tuple(x.shape), x.stride(), N, K, a[ld]))
    for name in ("x", "y", "logabsdet"):
        if t.get(name) is not None and t[name].numel() != N:
            bad.append("%s: %d elements for N = %d" % (name, t[name].numel(), N))
    return bad


def _numel(rules):
    def check(a, t):
        want = rules(a)          # name -> exact element count, or (least element count,)
        return ["%s: %d elements, the call's scalars ask for %s" % (k, t[k].numel(), n)
                for k, n in want.items() if t.get(k) is not None and (t[k].numel() < n[0] if isinstance(n, tuple) else t[k].numel() != n)]
    return check


def _coupling(a):
    nd = _nd(a["K"], a["tails"])
    return {"x": a["B"] * a["D"], "y": a["B"] * a["D"], "logdet": a["B"], "cond": a["B"] * a["nT"] * (2 * a["K"] + nd),
            "uw": a["nI"] * a["K"], "uh": a["nI"] * a["K"], "ud": a["nI"] * nd, "identity_idx": a["nI"], "transform_idx": a["nT"],
            "grad_y": a["B"] * a["D"], "grad_logdet": a["B"], "grad_x": a["B"] * a["D"], "grad_cond": a["B"] * a["nT"] * (2 * a["K"] + nd),
            "grad_uw": a["nI"] * a["K"], "grad_uh": a["nI"] * a["K"], "grad_ud": a["nI"] * nd,
            # (the layer hands its whole per-feature tables to each half's call: read up to nT / nI entries)
            "tails_t": (a["nT"],), "bound_t": (a["nT"],), "tails_i": (a["nI"],), "bound_i": (a["nI"],)}


def _masked(a):
    n = a["B"] * a["inner"]
    return {"z": n, "y": n, "s": n, "t": n, "gy": n, "gz": n, "gs": n, "gt": n, "b": a["inner"], "logdet": a["B"], "gld": a["B"]}


def _coupling_affine(a):
    n, p = a["B"] * a["C"] * a["HW"], a["B"] * _P(a) * a["HW"]
    return {"z": n, "y": n, "gy": n, "gz": n, "param": p, "gparam": p, "param_bias": _P(a), "logdet": a["B"], "gld": a["B"]}


def _actnorm(a):
    n = a["B"] * a["C"] * a["HW"]
    return {"z": n, "y": n, "gy": n, "gz": n, "s": a["C"], "t": a["C"], "gs": a["C"], "gt": a["C"], "logdet": a["B"], "gld": a["B"],
            "logdet_scalar": 1}


def _inv1x1(a):
    n = a["B"] * a["C"] * a["HW"]
    return {"z": n, "y": n, "W": a["C"] * a["C"], "bias": a["C"], "logdet_unit": 1, "logdet_scalar": 1, "logdet": a["B"]}


def _tri(D):
    return D * (D - 1) // 2


COUNTS = {
    "nf_masked_affine": _numel(_masked),
    "nf_masked_affine_bwd": _numel(_masked),
    "nf_affine_coupling": _numel(_coupling_affine),
    "nf_affine_coupling_pb": _numel(_coupling_affine),
    "nf_affine_coupling_bwd": _numel(_coupling_affine),
    "nf_actnorm": _numel(_actnorm),
    "nf_actnorm_bwd": _numel(_actnorm),
    "nf_actnorm_init": _numel(lambda a: {"mean": a["C"], "std_unbiased": a["C"], "s": a["C"], "t": a["C"]}),
    "nf_diag_gaussian_log_prob": _numel(lambda a: {"z": a["B"] * a["d"], "loc": a["d"], "log_scale": a["d"], "out": a["B"]}),
    "nf_diag_gaussian_log_prob_rows": _numel(lambda a: {"z": a["B"] * a["d"], "loc_rows": a["num_rows"] * a["d"],
                                                        "log_scale_rows": a["num_rows"] * a["d"], "row_idx": a["B"], "out": a["B"]}),
    "nf_inv1x1_conv_affine": _numel(_inv1x1),
    "nf_inv1x1_conv_t": _numel(_inv1x1),
    "nf_lu_linear_permute": _numel(lambda a: {"x": a["B"] * a["D"], "y": a["B"] * a["D"], "logdet": a["B"], "perm": a["D"],
                                              "unconstrained_upper_diag": a["D"], "bias": a["D"], "lower_entries": _tri(a["D"]),
                                              "upper_entries": _tri(a["D"])}),
    "nf_rqs_spline": _spline_rows,
    "nf_rqs_coupling": _numel(_coupling),
    "nf_rqs_coupling_ft": _numel(_coupling),
    "nf_rqs_coupling_bwd": _numel(_coupling),
    "nf_rqs_coupling_bwd_ft": _numel(_coupling),
    "nf_rqs_coupling_bwd_ft_wave": _numel(_coupling),
}


def judge(sig, name, args):
    """The violations (strings) of one call: `sig` its header signature, `args` what Python passed."""
    if len(sig) != len(args):
        return ["%s: %d arguments for %d parameters" % (name, len(args), len(sig))]
    scalars, tensors, bad = {}, {}, []
    for (pname, pointee), a in zip(sig, args):
        if pointee is None:
            scalars[pname] = a.value if hasattr(a, "value") else a
        elif isinstance(a, TensorPtr) and a.tensor is not None:
            tensors[pname] = a.tensor
    want = torch.float64 if scalars.get("dtype", 0) == 1 else torch.float32
    for (pname, pointee), a in zip(sig, args):
        t = tensors.get(pname)
        if t is None:
            continue
        if pointee in _POINTEE:                                             # rule 2
            if t.dtype != _POINTEE[pointee]:
                bad.append("%s(%s): declared %s *, got a %s tensor" % (name, pname, pointee, t.dtype))
        elif t.dtype.is_floating_point and t.dtype != INTENDED.get((name, pname), want):     # rule 1
            bad.append("%s(%s): a %s tensor in a call that reads %s" % (name, pname, t.dtype, INTENDED.get((name, pname), want)))
    if name in COUNTS:                                                      # rule 3
        bad += ["%s(%s)" % (name, b) for b in COUNTS[name](scalars, tensors)]
    return bad


class Audit:
    def __init__(self):
        self.forwarded = []       # entry points that reached the library
        self.blocked = []         # entry points stopped in block-everything mode
        self.violations = []      # rule breaches (never forwarded)
        self.seen = []            # every call, with its tensors by parameter name

    def names(self):
        return [n for n, _ in self.seen]


def install(nfa, monkeypatch, block_all=False, forward=None):
    """Patch the pointer helpers and the call functions of nfa._lib / nfa.ops (undone by monkeypatch).  forward(name, *args) -> rc:
    what stands in for the library (default: the real entry point); block_all: nothing is forwarded, every call raises."""
    L, ops = nfa._lib, nfa.ops
    sigs = signatures(nfa)
    audit = Audit()
    real_ptr, real_any, real_rc, check = L.ptr, L.ptr_any, L.call_rc, L.check

    def track(real):
        def f(t):
            p = real(t)                      # (keeps the helper's own refusals: contiguity)
            out = TensorPtr(p.value)
            out.tensor = t
            return out
        return f

    def spy_rc(name, *args):
        sig = sigs[name]
        audit.seen.append((name, {p: a.tensor for (p, _), a in zip(sig, args) if isinstance(a, TensorPtr) and a.tensor is not None}))
        bad = judge(sig, name, args)
        if bad:
            audit.violations += bad
            raise AuditViolation("not forwarded: " + "; ".join(bad))
        if block_all:
            audit.blocked.append(name)
            raise AuditViolation("%s reached the C ABI in a case that must raise before it" % name)
        audit.forwarded.append(name)
        plain = [ctypes.c_void_p(a.value) if isinstance(a, TensorPtr) else a for a in args]
        return (forward or real_rc)(name, *plain)

    def spy_call(name, *args):
        check(spy_rc(name, *args), name)

    for mod in (L, ops):
        monkeypatch.setattr(mod, "ptr", track(real_ptr))
        monkeypatch.setattr(mod, "ptr_any", track(real_any))
    monkeypatch.setattr(L, "call", spy_call)
    monkeypatch.setattr(L, "call_rc", spy_rc)
    return audit
