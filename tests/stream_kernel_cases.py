"""Case table of the streaming kernels (csrc/affine.hip, affine_bwd.hip, image_glue.hip and the per-pixel product of inv1x1.hip),
importable without a GPU: tests/test_host_stream_kernel_cases.py checks the table, tests/test_gpu_stream_kernels.py runs it.

A Case is (kernel, dtype, options).  From it follow
  plans()      {loop: Plan(path, sweeps, ragged, per_sweep)}: which hand-specialised path the launcher picks and how many times the
               kernel's stride loop goes round -- the launcher's conditions and grid_for restated in pure Python below;
  inputs()     seeded CPU tensors in the case's dtype (generated in float64 and rounded once, so that the float64 reference and the
               float32 yardstick read the same numbers as the kernel);
  formula(x)   the plain closed formula in torch on the CPU, in the precision of the tensors it is given: on float64 copies it is
               the REFERENCE, on float32 copies the YARDSTICK (what a straightforward float32 evaluation of the same formula loses).
Gradients come from torch autograd of the same formula for the cotangents (cy, cl) among the inputs.

Inputs are benign: scales 0.3 randn, Logit.inverse inputs uniform in [0.02, 0.98], Logit.forward inputs 3 randn; non-finite values
only where a case names them (option `nonfinite`, option `bad_labels`).

Every shape runs in float32 and float64 and in both directions, with one exception kept for size: a shape of more than 2^20 elements
(masked_affine, actnorm; 2^19 for actnorm_bwd, whose large shapes come in numbers) runs ONE direction per dtype, alternating from
shape to shape, and the backward of the large masked_affine shapes runs at inner = 16 only (it is one element-wise path)."""
import math
import zlib
from collections import namedtuple

import numpy as np
import torch

from conftest import TOL, ld_tol

# ---- launch constants, each with the line it was read from --------------------------------------------------------------------------
WG = 256                 # threads per workgroup of every kernel here: dim3(256) in every launcher (e.g. affine.hip:367)
WAVE = 64                # lanes per wave: `threadIdx.x & 63`, `>> 6` (affine.hip:28-30)
CAP = 2048               # common.hpp:382  grid_for(..., max_blocks = 256 * 8)
CAP_IMG = 4096           # affine.hip:364, :385, affine_bwd.hip:510  grid_for(B, 1, 256 * 16)
PER_BLOCK = 1024         # affine.hip:364, :410, :481, affine_bwd.hip:490, image_glue.hip:185  grid_for(N, 256 * 4)
VEC_MAX = 256            # affine.hip:20, :236, :365, :461  `inner <= 256 && (inner & 3) == 0`
SHORT_MAX = 64           # affine.hip:62, :364  `inner <= 64`
ACTNORM_BWD_WGS = 2048   # affine_bwd.hip:523  nsplit = ceil(2048 / C), at most B
WGRAD_PARTS = 256        # affine_bwd.hip:568  parts = min(B, 256)
LDF_MAX = 120            # image_glue.hip:130
OT = 8                   # inv1x1.hip:147

DT = {"f32": torch.float32, "f64": torch.float64}
Plan = namedtuple("Plan", "path sweeps ragged per_sweep")


def grid_for(work, per_block, max_blocks=CAP):
    """common.hpp:382-387."""
    return max(1, min(-(-work // per_block), max_blocks))


def _sweep(path, n, per):
    return Plan(path, -(-n // per), n % per != 0, per)


def _pow2(n):
    p = 1
    while p < n:
        p <<= 1
    return p


def _rows_vec4(B, d):
    """affine.hip:25-34, :241-258, :365, :461: a lane owns 4 columns, P = lanes per row rounded up to a power of two, 64 / P rows
    per wave, grid_for(B d / 4, 256) workgroups of 4 waves."""
    L4 = d // 4
    P = _pow2(L4)
    return _sweep("vec4/pow2" if P == L4 else "vec4/idle-lanes", B, grid_for(B * d // 4, WG) * 4 * (WAVE // P))


def _rows_wave(B, d, name="wave"):
    """One wave per row, grid_for(B, 4) workgroups (affine.hip:276, :331, :460, :497; image_glue.hip:22, :51, :96, :115); lanes stride
    over the row: rows longer than 64 take a second pass of the lane loop."""
    return _sweep("%s/%s" % (name, "one-pass" if d <= WAVE else "lane-stride"), B, grid_for(B, 4) * 4)


def _elements(path, n, per_block=PER_BLOCK):
    """`for (i = global thread; i < N; i += threads)` on grid_for(N, per_block) workgroups."""
    return _sweep(path, n, grid_for(n, per_block) * WG)


def plans(c):
    """{loop: Plan} of a case: the launcher's branch conditions, restated."""
    k, p, f32 = c.kernel, c.p, c.dtype == "f32"
    if k == "masked_affine":
        B, n = p["B"], p["inner"]
        if f32 and n <= VEC_MAX and n % 4 == 0:                    # affine.hip:20, :365
            return {"rows": _rows_vec4(B, n)}
        if n <= SHORT_MAX:                                          # affine.hip:62-70, grid :364 (first arm)
            P = _pow2(n)
            return {"rows": _sweep("short/pow2" if P == n else "short/idle-lanes", B, grid_for(B * n, PER_BLOCK) * 4 * (WAVE // P))}
        return {"rows": _sweep("generic/one-pass" if n <= WG else "generic/thread-stride", B, grid_for(B, 1, CAP_IMG))}   # :90, :364
    if k == "masked_affine_bwd":
        return {"elements": _elements("elements", p["B"] * p["inner"])}             # affine_bwd.hip:20, :490
    if k == "diag_gaussian":
        B, d = p["B"], p["d"]
        if f32 and d <= VEC_MAX and d % 4 == 0:                    # affine.hip:236, :461
            return {"rows": _rows_vec4(B, d)}
        return {"rows": _rows_wave(B, d)}                           # affine.hip:276, :460
    if k in ("affine_coupling", "affine_coupling_bwd"):
        n2 = (p["C"] - p["c1"]) * p["HW"]
        return {"images": _sweep("image/one-pass" if n2 <= WG else "image/thread-stride", p["B"], grid_for(p["B"], 1, CAP_IMG))}
    if k == "actnorm":
        per = grid_for(p["B"] * p["C"] * p["HW"], PER_BLOCK) * WG   # affine.hip:174, :181, :410: both loops share the grid
        return {"elements": _sweep("elements", p["B"] * p["C"] * p["HW"], per), "ld-rows": _sweep("ld-rows", p["B"], per)}
    if k == "actnorm_bwd":
        B, C, HW = p["B"], p["C"], p["HW"]
        nsplit = max(1, min(-(-ACTNORM_BWD_WGS // C), B))           # affine_bwd.hip:522-526
        nimg = -(-B // nsplit)                                      # workgroup j = 0 (the longest walk), affine_bwd.hip:107
        quad = f32 and HW % 4 == 0                                  # affine_bwd.hip:108-109
        w = HW // 4 if quad else HW                                 # the (k, q) / (k, p) walk's row width, :113-115 / :145-146
        walk = "dq=0" if WG % w == 0 else ("carry" if w < WG else "dk=0")
        pl = _sweep("%s/%s" % ("quad" if quad else "scalar", walk), nimg * w, WG)
        # the carry `q >= Q -> ++k` is only USED by a later sweep of a workgroup that holds a second image
        return {"walk": pl._replace(path=pl.path + ("/images>=2" if nimg >= 2 else "/one-image"))}
    if k == "maf_affine":
        return {"rows": _rows_wave(p["B"], p["D"])}
    if k == "maf_affine_bwd":
        return {"elements": _elements("elements", p["B"] * p["D"], WG)}             # affine_bwd.hip:358, :610
    if k == "logit":
        return {"rows": _rows_wave(p["B"], p["inner"])}
    if k == "rows":
        return {"rows": _rows_wave(p["B"], p["d"])}
    if k == "squeeze":
        return {"elements": _elements("direction %d" % p["direction"], p["B"] * p["C"] * p["H"] * p["W"])}
    if k == "bias_leaky_relu":
        return {"elements": _elements("elements", p["B"] * p["C"] * p["HW"])}
    if k == "ld_fold":
        n = p["n"]                                                  # image_glue.hip:141-151, :165
        path = "second-launch" if n > LDF_MAX else ("tail-only" if n < 8 else ("unrolled" if n % 8 == 0 else "unrolled+tail"))
        return {"rows": _elements(path, p["B"], WG)}
    if k == "inv1x1_conv":
        B, C, HW = p["B"], p["C"], p["HW"]
        nwork = B * HW * (-(-C // OT))                              # inv1x1.hip:162-165, :226-227
        per = grid_for(nwork, WG) * WG
        path = "channels<4" if C < 4 else ("4-loop" if C % 4 == 0 else "4-loop+tail")      # inv1x1.hip:175-190
        return {"pixels": _sweep(path, nwork, per), "ld-rows": _sweep("ld-rows", B, per)}
    if k == "inv1x1_wgrad":
        B, C, HW = p["B"], p["C"], p["HW"]
        parts = min(B, WGRAD_PARTS)                                 # affine_bwd.hip:568-570
        if f32 and HW % 16 == 0:                                    # affine_bwd.hip:573 (the wrapper's tensors are 16-byte aligned)
            nchunks = B * (HW // 16)
            wg = max(1, min(-(-nchunks // 16), parts))              # :576-578
            return {"chunks": _sweep("mfma/NB=%d" % (-(-C // 16)), nchunks, 16 * wg)}     # :273: four chunks per wave and sweep
        ipw = -(-B // parts)                                        # images per workgroup: the `bb` loop, :216-217
        return {"images": Plan("partial/%s" % c.dtype, ipw, B % ipw != 0, ipw)}
    raise KeyError(k)


# ---- bars -----------------------------------------------------------------------------------------------------------------------------
def _bar(kind, dtype):
    """The bar the suite already holds the kernel to.  elem / sum: conftest.TOL / ld_tol.  grad: test_gpu_hygiene.py
    test_affine_family_backward_kernels_vs_torch_autograd (rtol 2e-5 / 1e-11, atol 10 rtol).  chan: the per-channel and per-matrix
    sums of the same test (ActNormFn, Inv1x1Fn: atol 100 rtol), which is the inv1x1_wgrad bar quoted in test_gpu_views.py."""
    npd = np.dtype("float32" if dtype == "f32" else "float64")
    if kind == "elem":
        return dict(TOL[npd])
    if kind == "sum":
        return ld_tol(npd)
    rtol = 2e-5 if dtype == "f32" else 1e-11
    return dict(rtol=rtol, atol=(10 if kind == "grad" else 100) * rtol)


KIND = {          # output name -> bar kind; "exact": bit equality with the formula in the kernel's own precision
    "masked_affine": dict(y="elem", ld="sum"),
    "masked_affine_bwd": dict(y="elem", ld="sum", gz="grad", gs="grad", gt="grad"),
    "diag_gaussian": dict(lp="sum"),
    "affine_coupling": dict(y="elem", ld="sum"),
    "affine_coupling_bwd": dict(y="elem", ld="sum", gz="grad", gparam="grad"),
    "actnorm": dict(y="elem", ld="sum", lds="sum"),
    "actnorm_bwd": dict(y="elem", ld="sum", gz="grad", gs="chan", gt="chan"),      # (gz is one product per element)
    "maf_affine": dict(y="elem", ld="sum"),
    "maf_affine_bwd": dict(y="elem", ld="sum", gx="grad", gparams="grad"),
    "logit": dict(y="elem", ld="sum"),
    "rows": dict(lp="sum"),
    "squeeze": dict(y="exact"),
    "bias_leaky_relu": dict(y="exact"),
    "ld_fold": dict(ld="exact"),
    "inv1x1_conv": dict(y="elem", ld="sum", lds="sum"),      # (y: a dot product of at most 64 terms, held to TOL)
    "inv1x1_wgrad": dict(gW="chan", gl="chan"),
}
MARGIN = 4.0      # the suite's margin for two equally valid float32 summation orders (routed-versus-loop comparisons)


def scaled_error(got, ref, kind, dtype):
    """max over the finite entries of ref of |got - ref| / (atol + rtol |ref|): the error in units of the suite's existing bar."""
    bar = _bar(kind, dtype)
    ref = ref.double()
    ok = torch.isfinite(ref)
    if not bool(ok.any()):
        return 0.0
    e = (got.double() - ref).abs() / (bar["atol"] + bar["rtol"] * ref.abs())
    e = torch.where(ok, e, torch.zeros_like(e))
    return float(torch.nan_to_num(e, nan=float("inf")).max())


def allowed(yard_err, dtype):
    """The bar of one output in units of the existing bar: the larger of that bar (1) and MARGIN x the float32 yardstick's own error
    on this case; float64 kernels are held to the existing float64 bars alone."""
    return 1.0 if dtype == "f64" else max(1.0, MARGIN * yard_err)


# ---- the case ----------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, kernel, dtype="f32", **p):
        self.kernel, self.dtype, self.p = kernel, dtype, p

    @property
    def id(self):
        return "%s-%s-%s" % (self.kernel, self.dtype, "-".join("%s%s" % (k, v) for k, v in self.p.items()))

    def __repr__(self):
        return self.id

    def plans(self):
        return plans(self)

    def inputs(self):
        g = torch.Generator().manual_seed(zlib.crc32(self.id.encode()))
        x = INPUTS[self.kernel](self, g)
        return {k: (v.to(DT[self.dtype]) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in x.items()}

    def formula(self, x):
        """Outputs (and gradients) of the plain formula in the precision of x's tensors."""
        return FORMULA[self.kernel](self, x)

    def evaluate(self):
        """(inputs, float64 reference, float32 yardstick or None for a float64 case)."""
        x = self.inputs()
        ref = self.formula(cast(x, torch.float64))
        yard = self.formula(cast(x, torch.float32)) if self.dtype == "f32" else None
        return x, ref, yard


def cast(x, dtype):
    return {k: (v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in x.items()}


def rn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float64)


def _acc_inputs(c, g, x, n):
    """The accumulator's previous contents for acc = add / sub (option `acc`; None: the wrapper allocates and the kernel writes)."""
    if c.p.get("acc") in ("add", "sub"):
        x["ld0"] = rn(g, n)
    return x


def _acc(c, x, ld):
    a = c.p.get("acc")
    return x["ld0"] + ld if a == "add" else (x["ld0"] - ld if a == "sub" else ld)


def _vjp(c, x, leaves, fn, names):
    """fn({inputs with leaves}) -> (y, ld); gradients of sum(y cy) + sum(ld cl) (option gy / gld = False: that cotangent is absent)."""
    lv = {k: x[k].detach().clone().requires_grad_(True) for k in leaves if x.get(k) is not None}
    y, ld = fn(dict(x, **lv))
    loss = 0.0
    if c.p.get("gy", True):
        loss = loss + (y * x["cy"]).sum()
    if c.p.get("gld", True) and ld.requires_grad:
        loss = loss + (ld * x["cl"]).sum()
    loss.backward()
    out = dict(y=y.detach(), ld=ld.detach())
    for k, name in zip(leaves, names):
        if k in lv:
            out[name] = lv[k].grad if lv[k].grad is not None else torch.zeros_like(lv[k])
    return out


def _cot(g, x, yshape, B):
    x["cy"], x["cl"] = rn(g, *yshape), rn(g, B)
    return x


# ---- MaskedAffineFlow (coupling.py:209-229) ---------------------------------------------------------------------------------------
def _ma_inputs(c, g):
    B, n = c.p["B"], c.p["inner"]
    x = dict(z=rn(g, B, n), b=(torch.arange(n) % 2).double(), s=0.3 * rn(g, B, n), t=rn(g, B, n))
    if c.p.get("only") == "s":
        x["t"] = None
    if c.p.get("only") == "t":
        x["s"] = None
    if c.p.get("nonfinite"):        # the named non-finite entries: columns 0 and 2 have b = 0
        x["s"][B // 2, 0], x["t"][B - 1, 2], x["s"][0, 2] = float("-inf"), float("inf"), float("nan")
    return _cot(g, _acc_inputs(c, g, x, B), (B, n), B) if c.kernel.endswith("bwd") else _acc_inputs(c, g, x, B)


def _ma_fwd(c, x):
    z, b = x["z"], x["b"]
    s = torch.zeros_like(z) if x["s"] is None else x["s"]
    t = torch.zeros_like(z) if x["t"] is None else x["t"]
    nan = torch.full_like(z, float("nan"))
    s, t = torch.where(torch.isfinite(s), s, nan), torch.where(torch.isfinite(t), t, nan)     # this library's rule (affine.hip:47-48)
    if c.p["direction"] == 0:
        return b * z + (1 - b) * (z * torch.exp(s) + t), ((1 - b) * s).sum(1)
    return b * z + (1 - b) * (z - t) * torch.exp(-s), -((1 - b) * s).sum(1)


def _ma_formula(c, x):
    y, ld = _ma_fwd(c, x)
    return dict(y=y, ld=_acc(c, x, ld))


def _ma_bwd_formula(c, x):
    return _vjp(c, x, ("z", "s", "t"), lambda v: _ma_fwd(c, v), ("gz", "gs", "gt"))


# ---- DiagGaussian.log_prob (distributions/base.py:94-103) and its per-sample-rows variant (base.py:326-345) ----------------------------
def _dg_inputs(c, g):
    B, d = c.p["B"], c.p["d"]
    return _acc_inputs(c, g, dict(z=rn(g, B, d), loc=rn(g, d), ls=0.3 * rn(g, d)), B)


def _gauss(z, loc, ls, d):
    return -0.5 * d * math.log(2 * math.pi) - (ls + 0.5 * ((z - loc) / torch.exp(ls)) ** 2).sum(1)


def _dg_formula(c, x):
    return dict(lp=_acc(c, x, _gauss(x["z"], x["loc"], x["ls"] + c.p.get("shift", 0.0), c.p["d"])))


ROWS_CLASSES = 7


def _rows_inputs(c, g):
    B, d = c.p["B"], c.p["d"]
    R = ROWS_CLASSES if c.p["labels"] else B
    x = dict(z=rn(g, B, d), loc=rn(g, R, d), ls=0.3 * rn(g, R, d), idx=None)
    if c.p["labels"]:
        x["idx"] = torch.randint(0, R, (B,), generator=g)
    return _acc_inputs(c, g, x, B)


def bad_label_rows(B):
    """(row with label -1, row with label num_rows) of option `bad_labels`."""
    return B // 3, B - 1


def _rows_formula(c, x):
    idx = torch.arange(c.p["B"]) if x["idx"] is None else x["idx"]
    lp = _gauss(x["z"], x["loc"][idx], x["ls"][idx] + c.p.get("shift", 0.0), c.p["d"])
    if c.p.get("bad_labels"):
        lp[list(bad_label_rows(c.p["B"]))] = float("nan")
    return dict(lp=_acc(c, x, lp))


# ---- AffineCouplingBlock with the channel split / merge (coupling.py:117-171, reshape.py:30-85) ------------------------------------
def _ac_inputs(c, g):
    B, C, c1, HW, smap = c.p["B"], c.p["C"], c.p["c1"], c.p["HW"], c.p["smap"]
    P = (C - c1) * (1 if smap is None else 2)
    x = dict(z=rn(g, B, C, HW), param=0.3 * rn(g, B, P, HW), pbias=0.3 * rn(g, P) if c.p.get("pb") else None)
    return _cot(g, _acc_inputs(c, g, x, B), (B, C, HW), B) if c.kernel.endswith("bwd") else _acc_inputs(c, g, x, B)


def _ac_fwd(c, x):
    z, prm = x["z"], x["param"]
    C, c1, flip, smap, d = c.p["C"], c.p["c1"], c.p["flip"], c.p["smap"], c.p["direction"]
    if x.get("pbias") is not None:
        prm = prm + x["pbias"].view(1, -1, 1)
    z1, z2 = (z[:, C - c1:], z[:, :C - c1]) if flip else (z[:, :c1], z[:, c1:])
    if smap is None:
        y2, ld = (z2 + prm if d == 0 else z2 - prm), torch.zeros(z.shape[0], dtype=z.dtype)
    else:
        sh, sc = prm[:, 0::2], prm[:, 1::2]
        if smap == "exp":
            y2, ld = (z2 * torch.exp(sc) + sh, sc.sum((1, 2))) if d == 0 else ((z2 - sh) * torch.exp(-sc), -sc.sum((1, 2)))
        else:
            sg = torch.sigmoid(sc + 2)
            mult = (smap == "sigmoid_inv") == (d == 0)
            if d == 0:
                y2 = (z2 * sg if mult else z2 / sg) + sh
            else:
                y2 = (z2 - sh) * sg if mult else (z2 - sh) / sg
            ld = torch.log(sg).sum((1, 2)) * (1.0 if mult else -1.0)
    return torch.cat([y2, z1] if flip else [z1, y2], 1), ld


def _ac_formula(c, x):
    y, ld = _ac_fwd(c, x)
    return dict(y=y, ld=_acc(c, x, ld))


def _ac_bwd_formula(c, x):
    return _vjp(c, x, ("z", "param"), lambda v: _ac_fwd(c, v), ("gz", "gparam"))


# ---- AffineConstFlow / ActNorm with per-channel s, t (coupling.py:38-54) -----------------------------------------------------------
def _an_inputs(c, g):
    B, C, HW = c.p["B"], c.p["C"], c.p["HW"]
    x = dict(z=rn(g, B, C, HW), s=0.3 * rn(g, C), t=rn(g, C))
    return _cot(g, x, (B, C, HW), B) if c.kernel.endswith("bwd") else _acc_inputs(c, g, x, B)


def _an_fwd(c, x):
    s, t = x["s"].view(1, -1, 1), x["t"].view(1, -1, 1)
    ones = torch.ones(c.p["B"], dtype=x["z"].dtype)
    if c.p["direction"] == 0:
        return x["z"] * torch.exp(s) + t, c.p["HW"] * x["s"].sum() * ones
    return (x["z"] - t) * torch.exp(-s), -c.p["HW"] * x["s"].sum() * ones


def _an_formula(c, x):
    y, ld = _an_fwd(c, x)
    return dict(y=y, lds=ld[0], ld=_acc(c, x, ld))


def _an_bwd_formula(c, x):
    return _vjp(c, x, ("z", "s", "t"), lambda v: _an_fwd(c, v), ("gz", "gs", "gt"))


# ---- MaskedAffineAutoregressive's element-wise transform (affine/autoregressive.py:98-128) -------------------------------------------
def _maf_inputs(c, g):
    B, D = c.p["B"], c.p["D"]
    x = dict(x=rn(g, B, D), params=torch.stack([0.3 * rn(g, B, D), rn(g, B, D)], 2))
    return _cot(g, x, (B, D), B) if c.kernel.endswith("bwd") else _acc_inputs(c, g, x, B)


def _maf_fwd(c, x):
    scale, sh = torch.sigmoid(x["params"][..., 0] + 2) + 1e-3, x["params"][..., 1]
    if c.p["direction"] == 0:
        return scale * x["x"] + sh, torch.log(scale).sum(1)
    return (x["x"] - sh) / scale, -torch.log(scale).sum(1)


def _maf_formula(c, x):
    y, ld = _maf_fwd(c, x)
    return dict(y=y, ld=_acc(c, x, ld))


def _maf_bwd_formula(c, x):
    return _vjp(c, x, ("x", "params"), lambda v: _maf_fwd(c, v), ("gx", "gparams"))


# ---- Logit (transforms.py:8-47) ---------------------------------------------------------------------------------------------------
def _logit_inputs(c, g):
    B, n = c.p["B"], c.p["inner"]
    z = 3.0 * rn(g, B, n) if c.p["direction"] == 0 else 0.02 + 0.96 * torch.rand(B, n, generator=g, dtype=torch.float64)
    return _acc_inputs(c, g, dict(z=z), B)


def _logit_formula(c, x):
    z, alpha, n = x["z"], c.p["alpha"], c.p["inner"]
    beta = 1 - 2 * alpha
    if c.p["direction"] == 0:
        F = torch.nn.functional
        ld = -math.log(beta) * n + F.logsigmoid(z).sum(1) + F.logsigmoid(-z).sum(1)
        return dict(y=(torch.sigmoid(z) - alpha) / beta, ld=_acc(c, x, ld))
    u = alpha + beta * z
    lu, l1 = torch.log(u), torch.log(1 - u)
    return dict(y=lu - l1, ld=_acc(c, x, math.log(beta) * n - lu.sum(1) - l1.sum(1)))


# ---- Squeeze (reshape.py:116-128), the bias + LeakyReLU pass of ConvNet2d (nets/cnn.py:40-50), the log-det fold -------------------
def _sq_inputs(c, g):
    return dict(z=rn(g, c.p["B"], c.p["C"], c.p["H"], c.p["W"]))


def _sq_formula(c, x):
    """The permutation of reshape.py:116-128 written out by index: forward out[c, 2h + i, 2w + j] = in[4c + 2i + j, h, w]."""
    z = x["z"]
    B, C, H, W = z.shape
    fwd = c.p["direction"] == 0
    y = torch.empty((B, C // 4, 2 * H, 2 * W) if fwd else (B, 4 * C, H // 2, W // 2), dtype=z.dtype)
    for i in (0, 1):
        for j in (0, 1):
            if fwd:
                y[:, :, i::2, j::2] = z[:, 2 * i + j::4]
            else:
                y[:, 2 * i + j::4] = z[:, :, i::2, j::2]
    return dict(y=y)


def _blr_inputs(c, g):
    return dict(y=rn(g, c.p["B"], c.p["C"], c.p["HW"]), bias=rn(g, c.p["C"]))


def _blr_formula(c, x):
    v = x["y"] + x["bias"].view(1, -1, 1)
    return dict(y=torch.where(v > 0, v, v * torch.tensor(c.p["slope"], dtype=v.dtype)))


LDF_DISTINCT = 5      # distinct term vectors of a fold; term i reads vector i % 5 (the kernel only sees pointers)
LDF_FLIPS = (31, 32, 63, 64)


def ld_fold_negate(n, signs):
    """`flips`: the sign changes at terms 31, 32, 63 and 64 (bits 31 of word 0, 0 of word 1, 31 of word 1, 0 of word 2) on an
    otherwise constant pattern; `mixed`: i % 3 == 1."""
    if signs == "flips":
        neg, cur = [], 0
        for i in range(n):
            if i in LDF_FLIPS:
                cur ^= 1
            neg.append(cur)
        return neg
    return [int(i % 3 == 1) for i in range(n)]


def _ldf_inputs(c, g):
    B = c.p["B"]
    x = dict(ld0=rn(g, B))
    for i in range(min(c.p["n"], LDF_DISTINCT)):
        x["t%d" % i] = rn(g, B)
    return x


def _ldf_formula(c, x):
    a = x["ld0"].clone()
    for i, neg in enumerate(ld_fold_negate(c.p["n"], c.p["signs"])):
        t = x["t%d" % (i % LDF_DISTINCT)]
        a = a - t if neg else a + t
    return dict(ld=a)


# ---- Invertible1x1Conv's per-pixel product and its weight gradient (mixing.py:106-133) ---------------------------------------------
def _conv_inputs(c, g):
    B, C, HW = c.p["B"], c.p["C"], c.p["HW"]
    x = dict(z=rn(g, B, C, HW), W=rn(g, C, C) / math.sqrt(C), bias=rn(g, C) if c.p["variant"] == "affine" else None,
             ldu=torch.tensor(0.37, dtype=torch.float64))
    return _acc_inputs(c, g, x, B)


def _conv_formula(c, x):
    W = x["W"].t() if c.p["variant"] == "t" else x["W"]
    y = torch.einsum("oc,bcp->bop", W, x["z"])
    if x["bias"] is not None:
        y = y + x["bias"].view(1, -1, 1)
    if c.p["variant"] == "t":
        return dict(y=y)
    lds = x["ldu"] * c.p["HW"]
    return dict(y=y, lds=lds, ld=_acc(c, x, lds * torch.ones(c.p["B"], dtype=y.dtype)))


def _wg_inputs(c, g):
    B, C, HW = c.p["B"], c.p["C"], c.p["HW"]
    return dict(z=rn(g, B, C, HW), gy=rn(g, B, C, HW), gld=rn(g, B) if c.p.get("gld", True) else None)


def _wg_formula(c, x):
    gl = torch.zeros((), dtype=x["z"].dtype) if x["gld"] is None else c.p["HW"] * x["gld"].sum()
    # gW = sum over images of the per-image products: written so, the float32 yardstick's longest sums (81 600 terms per entry at
    # (300, 49, 272)) go through torch.sum's pairwise order on every CPU instead of whatever order its matrix product library picks
    return dict(gW=torch.einsum("bip,bjp->bij", x["gy"], x["z"]).sum(0), gl=gl)


INPUTS = dict(masked_affine=_ma_inputs, masked_affine_bwd=_ma_inputs, diag_gaussian=_dg_inputs, rows=_rows_inputs,
              affine_coupling=_ac_inputs, affine_coupling_bwd=_ac_inputs, actnorm=_an_inputs, actnorm_bwd=_an_inputs,
              maf_affine=_maf_inputs, maf_affine_bwd=_maf_inputs, logit=_logit_inputs, squeeze=_sq_inputs,
              bias_leaky_relu=_blr_inputs, ld_fold=_ldf_inputs, inv1x1_conv=_conv_inputs, inv1x1_wgrad=_wg_inputs)
FORMULA = dict(masked_affine=_ma_formula, masked_affine_bwd=_ma_bwd_formula, diag_gaussian=_dg_formula, rows=_rows_formula,
               affine_coupling=_ac_formula, affine_coupling_bwd=_ac_bwd_formula, actnorm=_an_formula, actnorm_bwd=_an_bwd_formula,
               maf_affine=_maf_formula, maf_affine_bwd=_maf_bwd_formula, logit=_logit_formula, squeeze=_sq_formula,
               bias_leaky_relu=_blr_formula, ld_fold=_ldf_formula, inv1x1_conv=_conv_formula, inv1x1_wgrad=_wg_formula)
# the row-wise forward kernels of the row-isolation check: {kernel: (loop, the inputs that carry one row per sample)}
ROW_WISE = dict(masked_affine=("rows", ("z", "s", "t", "ld0")), diag_gaussian=("rows", ("z", "ld0")), rows=("rows", ("z", "idx", "ld0")),
                logit=("rows", ("z", "ld0")), maf_affine=("rows", ("x", "params", "ld0")),
                affine_coupling=("images", ("z", "param", "ld0")))


# ---- the table -----------------------------------------------------------------------------------------------------------------------
def _table():
    T = []
    seen = set()

    def add(kernel, dtype="f32", **p):
        c = Case(kernel, dtype, **p)
        if c.id not in seen:          # (a shape named twice below is one case)
            seen.add(c.id)
            T.append(c)

    # masked_affine, forward and backward.  Sizes: the issue's, then the ones that fill the remaining (path, sweeps, ragged) cells
    ma32 = [(1, 4), (257, 4), (103, 20), (9, 132), (70, 256), (131137, 16),                    # 4 per lane
            (256, 4), (262144, 16), (32, 20), (8, 20), (256, 20),                             # ... full sweeps, one sweep with idle lanes
            (300, 1), (100, 33), (64, 63), (3, 5), (4, 33), (32, 7), (256, 2), (1, 1),         # short rows
            (131072, 20),                                                                     # (idle lanes: two full sweeps need the cap)
            (4099, 65), (7, 260), (3, 1030), (8192, 65), (8192, 257), (4099, 257)]             # generic
    ma64 = [(50, 8), (50, 64), (5, 128), (4, 4), (32, 8), (3, 5), (4, 33), (64, 63), (4099, 65), (8192, 65), (3, 260), (4099, 257),
            (8192, 257)]
    for dt, shapes in (("f32", ma32), ("f64", ma64)):
        for i, (B, n) in enumerate(shapes):
            big = B * n > 1 << 20
            for d in ((i % 2,) if big else (0, 1)):
                add("masked_affine", dt, B=B, inner=n, direction=d)
                if not big or n == 16:
                    add("masked_affine_bwd", dt, B=B, inner=n, direction=d)
    for B, n in ((103, 20), (100, 33), (7, 260)):             # one case per path with s only and one with t only
        for only in ("s", "t"):
            add("masked_affine", B=B, inner=n, direction=1, only=only)
            add("masked_affine_bwd", B=B, inner=n, direction=0, only=only)
    add("masked_affine", B=103, inner=20, direction=0, nonfinite=True)
    add("masked_affine", B=103, inner=20, direction=1, nonfinite=True)
    for acc in ("write", "add", "sub"):
        add("masked_affine", B=103, inner=20, direction=0, acc=acc)
    add("masked_affine_bwd", B=9, inner=132, direction=0, gld=False)
    for B, n in ((1, 256), (256, 4), (64, 3), (1300, 1)):     # the backward's element loop: one full sweep, full later sweep
        add("masked_affine_bwd", B=B, inner=n, direction=1)

    # diag_gaussian_log_prob
    for d in (4, 20, 132, 256):
        for B in (1, 70, 257):
            add("diag_gaussian", B=B, d=d)
    for B, d in ((131137, 16), (262144, 16), (256, 4), (32, 20), (256, 20), (131072, 20),
                 (70, 1), (70, 5), (70, 63), (70, 65), (70, 260), (70, 1000), (8197, 5), (16384, 5), (8, 5), (8, 65), (8197, 65), (16384, 65)):
        add("diag_gaussian", B=B, d=d)
    for B, d in ((70, 8), (70, 128), (8, 8), (8197, 8), (16384, 8), (8, 128), (8197, 128), (16384, 128)):
        add("diag_gaussian", "f64", B=B, d=d)
    for dt in ("f32", "f64"):
        add("diag_gaussian", dt, B=70, d=20, shift=0.25)
        add("diag_gaussian", dt, B=70, d=65, shift=-0.4)
    for acc in ("write", "add", "sub"):
        add("diag_gaussian", B=103, d=20, acc=acc)
        add("diag_gaussian", B=70, d=65, acc=acc)

    # affine_coupling[_pb] and its backward
    for dt in ("f32", "f64"):
        for smap in ("exp", "sigmoid", "sigmoid_inv", None):
            for flip in (False, True):
                for d in (0, 1):
                    for pb in (False, True):
                        add("affine_coupling", dt, B=3, C=5, c1=2, HW=150, smap=smap, flip=flip, direction=d, pb=pb)
                    add("affine_coupling_bwd", dt, B=3, C=5, c1=2, HW=150, smap=smap, flip=flip, direction=d)
        for i, (B, C, c1, HW) in enumerate([(4099, 3, 2, 1), (4099, 3, 1, 1), (1, 2, 1, 1), (8192, 3, 1, 1), (4099, 3, 1, 150), (8192, 3, 1, 150)]):
            for j, smap in enumerate(("exp", "sigmoid", "sigmoid_inv", None)):
                if HW == 150 and (smap in ("sigmoid", None) or dt == "f64"):
                    continue
                opt = dict(smap=smap, flip=bool((i + j) % 2), direction=(i + j // 2) % 2)
                add("affine_coupling", dt, B=B, C=C, c1=c1, HW=HW, pb=bool(j % 2), **opt)
                add("affine_coupling_bwd", dt, B=B, C=C, c1=c1, HW=HW, **opt)
    for acc in ("write", "add", "sub"):
        add("affine_coupling", B=4099, C=3, c1=2, HW=1, smap="exp", flip=False, direction=0, pb=False, acc=acc)
    add("affine_coupling_bwd", B=3, C=5, c1=2, HW=150, smap="exp", flip=False, direction=0, gld=False)

    # actnorm
    for dt in ("f32", "f64"):
        for i, (B, C, HW) in enumerate([(1500, 1, 1), (1000, 3, 1), (2049, 4, 256), (1, 1, 256), (4, 1, 256), (3, 2, 5), (1024, 1, 1),
                                         (512, 1, 1), (5, 3, 100), (256, 1, 1), (256, 4, 1)]):
            for d in ((i % 2,) if B * C * HW > 1 << 20 else (0, 1)):
                add("actnorm", dt, B=B, C=C, HW=HW, direction=d, want_scalar=bool((i + d) % 2), acc="write")
    for acc in ("add", "sub"):
        add("actnorm", B=1500, C=1, HW=1, direction=0, want_scalar=True, acc=acc)
    add("actnorm", B=1000, C=3, HW=1, direction=1, want_scalar=True, acc=None)      # (no per-sample log-det at all)

    # actnorm_bwd: the issue's shapes hold ONE image per workgroup or finish in one sweep, so the (k, q) carry is computed and never
    # used there; C = 2048 makes nsplit = 1 (every image in one workgroup) at a few MB
    an = [(100, 48, 12), (5, 3, 20), (700, 3, 36), (2, 2, 1296), (9, 5, 6), (3, 2, 300),
          (40, 2048, 36), (90, 2048, 12), (2, 2048, 1028), (70, 2048, 16), (128, 2048, 16), (2, 2, 1024), (3, 2, 16), (2, 2048, 1024),
          (64, 2048, 16), (64, 2048, 12), (256, 2048, 12), (2, 2048, 512), (2, 2048, 36), (2, 2048, 16), (3, 2, 2048), (1, 2048, 2048),
          (50, 2048, 6), (2, 2048, 300), (2, 2048, 6), (128, 2048, 6), (128, 2048, 1), (3, 5, 1), (256, 2048, 1), (300, 2048, 1),
          (2, 2048, 128), (2, 2048, 256), (1, 1, 256), (1, 1, 512), (2, 2048, 257), (1, 2, 257), (1, 2, 514), (2, 2048, 2), (1, 2, 768),
          (2, 2048, 384), (2, 2048, 1536), (256, 2048, 2), (512, 2048, 1)]
    for i, (B, C, HW) in enumerate(an):
        big = B * C * HW > 1 << 19
        for d in ((i % 2,) if big else (0, 1)):
            add("actnorm_bwd", B=B, C=C, HW=HW, direction=d, gld=bool((i // 2 + d) % 2) or i < 6)
            if i < 6:
                add("actnorm_bwd", B=B, C=C, HW=HW, direction=d, gld=False)
    for i, (B, C, HW) in enumerate([(100, 48, 12), (5, 3, 20), (3, 2, 300), (50, 2048, 12), (2, 2048, 300), (2, 2048, 6), (128, 2048, 6),
                                     (128, 2048, 1), (3, 5, 1), (300, 2048, 1), (2, 2048, 128), (1, 1, 256), (1, 1, 512), (2, 2048, 257),
                                     (1, 2, 257), (1, 2, 514), (2, 2048, 2), (64, 2048, 12), (1, 2, 768), (2, 2048, 384), (256, 2048, 1)]):
        add("actnorm_bwd", "f64", B=B, C=C, HW=HW, direction=i % 2, gld=bool(i % 3))

    # maf_affine and its backward
    for dt in ("f32", "f64"):
        for D in (1, 63, 64, 65, 130):
            for d in (0, 1):
                add("maf_affine", dt, B=67, D=D, direction=d)
                add("maf_affine_bwd", dt, B=67, D=D, direction=d)
        for B, D in ((8197, 3), (16384, 3), (68, 3), (68, 65), (8197, 65), (16384, 65)):
            add("maf_affine", dt, B=B, D=D, direction=B % 2)
        for B, D in ((8070, 65), (16384, 64), (4, 64), (16, 16)):
            add("maf_affine_bwd", dt, B=B, D=D, direction=B % 2)
        add("maf_affine_bwd", dt, B=67, D=65, direction=0, gy=False)
        add("maf_affine_bwd", dt, B=67, D=65, direction=1, gld=False)
    for acc in ("write", "add", "sub"):
        add("maf_affine", B=67, D=65, direction=0, acc=acc)

    # logit
    for dt in ("f32", "f64"):
        for d in (0, 1):
            for n in (1, 63, 65, 3072):
                for alpha in (0.0, 0.05):
                    add("logit", dt, B=5, inner=n, alpha=alpha, direction=d)
            for B, n in ((8197, 3), (16384, 3), (8, 3), (8, 65), (8197, 65), (16384, 65)):
                add("logit", dt, B=B, inner=n, alpha=0.05, direction=d)
    for acc in ("write", "add", "sub"):
        add("logit", B=5, inner=65, alpha=0.05, direction=1, acc=acc)

    # diag_gaussian_log_prob_rows
    for dt in ("f32", "f64"):
        for labels in (True, False):
            for d in (1, 5, 65, 200):
                add("rows", dt, B=37, d=d, labels=labels)
            for B, d in ((8197, 5), (16384, 5), (8, 5), (8, 65), (8197, 65), (16384, 65)):
                if labels or B < 100:
                    add("rows", dt, B=B, d=d, labels=labels)
        add("rows", dt, B=37, d=65, labels=True, bad_labels=True)
        add("rows", dt, B=8197, d=5, labels=True, bad_labels=True, shift=0.25)
    for acc in ("write", "add", "sub"):
        add("rows", B=37, d=65, labels=True, acc=acc)

    # squeeze
    for dt in ("f32", "f64"):
        for B, C, H, W in ((2, 4, 3, 5), (1, 8, 2, 2), (3, 4, 1, 1), (33, 4, 128, 128), (1, 4, 8, 8), (1, 4, 16, 16), (5, 4, 6, 10)):
            add("squeeze", dt, B=B, C=C, H=H, W=W, direction=0)
            add("squeeze", dt, B=B, C=C // 4, H=2 * H, W=2 * W, direction=1)

    # bias_leaky_relu_
    for dt in ("f32", "f64"):
        for B, C, HW in ((3, 1, 1), (5, 5, 7), (33, 4, 16384), (1, 4, 64), (4, 4, 64), (5, 5, 70)):
            for slope in (0.0, 0.1):
                add("bias_leaky_relu", dt, B=B, C=C, HW=HW, slope=slope)

    # ld_fold_multi (float32 only)
    for n in (1, 7, 8, 9, 119, 120, 121, 250):
        for B in (1, 257):
            add("ld_fold", B=B, n=n, signs="flips" if n > 31 else "mixed")
    for n in (120, 121, 250):       # subtracted terms in every launch: bits set in the second and third launch's rebased sign words
        add("ld_fold", B=257, n=n, signs="mixed")
    for n in (7, 8, 9, 121):
        for B in (256, 524353, 1048576):
            add("ld_fold", B=B, n=n, signs="flips" if n > 31 else "mixed")

    # inv1x1_conv / _conv_t / _conv_affine
    variants = ("plain", "t", "affine")
    for dt in ("f32", "f64"):
        for i, C in enumerate((1, 3, 4, 7, 8, 9, 17, 48, 64)):
            for j, HW in enumerate((1, 15, 64)):
                add("inv1x1_conv", dt, B=3, C=C, HW=HW, variant=variants[(i + j) % 3], acc="write")
        for B, C, HW in ((4100, 9, 64), (524353, 1, 1), (1048576, 1, 1), (256, 1, 1), (256, 4, 1), (64, 9, 2), (4100, 4, 128), (4096, 4, 256),
                         (16384, 9, 32)):
            add("inv1x1_conv", dt, B=B, C=C, HW=HW, variant="affine" if C == 9 else "plain", acc="write")
        for v in variants:
            add("inv1x1_conv", dt, B=3, C=9, HW=15, variant=v, acc="write")
    for acc in ("add", "sub", None):
        add("inv1x1_conv", B=3, C=9, HW=15, variant="affine", acc=acc)

    # inv1x1_wgrad
    for C in (1, 3, 16, 17, 33, 49, 64):
        for HW in (16, 48):
            for B in (1, 5, 257, 600):
                add("inv1x1_wgrad", B=B, C=C, HW=HW, gld=bool((C + B) % 2))
    for C in (3, 17, 33, 49):          # later sweeps of the MFMA kernel: more than 16 chunks per workgroup needs HW > 256
        for B, HW in ((1, 512), (1, 528), (1, 256), (300, 256), (300, 272)):
            add("inv1x1_wgrad", B=B, C=C, HW=HW)
    for dt in ("f32", "f64"):
        for C in (3, 17, 64):
            for HW in (15, 1, 100) if dt == "f32" else (15, 1, 16, 100):
                for B in (5, 257, 512):
                    add("inv1x1_wgrad", dt, B=B, C=C, HW=HW, gld=bool(B % 2))
    return T


CASES = _table()

# Every path a launcher can take: {kernel: {loop: [paths]}}.  A (path, more than one sweep, ragged last sweep) cell that no shape can
# reach is listed in UNREACHABLE with the reason.
PATHS = {
    "masked_affine": {"rows": ["vec4/pow2", "vec4/idle-lanes", "short/pow2", "short/idle-lanes", "generic/one-pass", "generic/thread-stride"]},
    "masked_affine_bwd": {"elements": ["elements"]},
    "diag_gaussian": {"rows": ["vec4/pow2", "vec4/idle-lanes", "wave/one-pass", "wave/lane-stride"]},
    "affine_coupling": {"images": ["image/one-pass", "image/thread-stride"]},
    "affine_coupling_bwd": {"images": ["image/one-pass", "image/thread-stride"]},
    "actnorm": {"elements": ["elements"], "ld-rows": ["ld-rows"]},
    "actnorm_bwd": {"walk": ["%s/%s/%s" % (a, b, n) for a in ("quad", "scalar") for b in ("dq=0", "carry", "dk=0")
                             for n in ("one-image", "images>=2")]},
    "maf_affine": {"rows": ["wave/one-pass", "wave/lane-stride"]},
    "maf_affine_bwd": {"elements": ["elements"]},
    "logit": {"rows": ["wave/one-pass", "wave/lane-stride"]},
    "rows": {"rows": ["wave/one-pass", "wave/lane-stride"]},
    "squeeze": {"elements": ["direction 0", "direction 1"]},
    "bias_leaky_relu": {"elements": ["elements"]},
    "ld_fold": {"rows": ["tail-only", "unrolled", "unrolled+tail", "second-launch"]},
    "inv1x1_conv": {"pixels": ["channels<4", "4-loop", "4-loop+tail"], "ld-rows": ["ld-rows"]},
    "inv1x1_wgrad": {"chunks": ["mfma/NB=1", "mfma/NB=2", "mfma/NB=3", "mfma/NB=4"], "images": ["partial/f32", "partial/f64"]},
}

_ONE_PER_ROW = "grid_for(B, 1, 4096) gives every row its own workgroup up to the cap: a single sweep is never ragged"
_WIDE = "a row wider than 256 elements: one image alone takes two sweeps"
_NARROW = "a row of at most 256 elements: a workgroup with one image finishes in one sweep"
_EXACT = "one full sweep is 256 elements = nimg x width: the width divides 256 and the walk is the dq=0 one"
UNREACHABLE = {}
for _k, _loop in (("masked_affine", "rows"), ("affine_coupling", "images"), ("affine_coupling_bwd", "images")):
    for _p in PATHS[_k][_loop]:
        if not _p.startswith(("vec4", "short")):
            UNREACHABLE[_k, _loop, _p, False, True] = _ONE_PER_ROW
for _w in ("quad", "scalar"):
    for _n in ("one-image", "images>=2"):
        for _r in (False, True):
            UNREACHABLE["actnorm_bwd", "walk", "%s/dk=0/%s" % (_w, _n), False, _r] = _WIDE
        UNREACHABLE["actnorm_bwd", "walk", "%s/carry/%s" % (_w, _n), False, False] = _EXACT
    for _walk in ("dq=0", "carry"):
        for _r in (False, True):
            UNREACHABLE["actnorm_bwd", "walk", "%s/%s/one-image" % (_w, _walk), True, _r] = _NARROW
for _dt in ("f32", "f64"):
    UNREACHABLE["inv1x1_wgrad", "images", "partial/" + _dt, False, True] = "one image per workgroup (ipw = 1) leaves no ragged last part"


def cells(kernel):
    """{(loop, path, more than one sweep, ragged last sweep): [cases]} held by the table for one kernel."""
    out = {}
    for c in CASES:
        if c.kernel == kernel:
            for loop, pl in c.plans().items():
                out.setdefault((loop, pl.path, pl.sweeps > 1, pl.ragged), []).append(c)
    return out
