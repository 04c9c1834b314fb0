"""ctypes binding of libnf_mi355x.so (the C ABI declared in include/nf_mi355x.h).

The library is built in-tree by `build()` (hipcc --offload-arch=gfx950) and loaded from
normalizing-flows_amd/lib/.  There is NO fallback: if the shared object is missing or a tensor does not
live on a HIP device, the calling layer raises.  torch is used here only to obtain device pointers and the
current HIP stream.
"""
import ctypes as C
import glob
import math
import os
import subprocess
import sys

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIBDIR = os.path.join(_HERE, "lib")
LIBPATH = os.path.join(LIBDIR, "libnf_mi355x.so")
INCLUDE = os.path.join(os.path.dirname(_HERE), "include")

NF_F32, NF_F64 = 0, 1
LD_WRITE, LD_ADD, LD_SUB = 0, 1, -1
TAILS = {None: 0, "linear": 1, "circular": 2}
SCALE = {"exp": 0, "sigmoid": 1, "sigmoid_inv": 2, None: 3}
RQS_DENSITY, RQS_SAMPLE_IDENTITY, RQS_SAMPLE_TRANSFORM = 0, 1, 2
ENOTSUP = -95          # NF_ENOTSUP: the entry point does not take this shape / dtype (check() raises NotImplementedError for it)

_lib = None


class NativeLibraryError(RuntimeError):
    pass


def sources():
    return sorted(glob.glob(os.path.join(CSRC, "*.hip")))


def _hip_includes(src):
    """Other .hip sources a .hip source #includes (rqs_fused_nw4.hip is a second build of rqs_fused.hip)."""
    import re
    return [os.path.join(CSRC, m) for m in re.findall(r'^#include "([^"]+\.hip)"', open(src).read(), flags=re.M)]


def build(force=False, verbose=False):
    """Compile every HIP source into lib/libnf_mi355x.so for gfx950 (cross-compiles without a GPU)."""
    srcs = sources()
    deps = srcs + glob.glob(os.path.join(CSRC, "*.hpp")) + glob.glob(os.path.join(INCLUDE, "*.h"))
    if not force and os.path.exists(LIBPATH) and all(os.path.getmtime(d) <= os.path.getmtime(LIBPATH) for d in deps):
        return LIBPATH
    os.makedirs(LIBDIR, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objs = []
    procs = []
    objdir = os.path.join(LIBDIR, "obj")
    os.makedirs(objdir, exist_ok=True)
    for s in srcs:
        o = os.path.join(objdir, os.path.basename(s)[:-4] + ".o")
        objs.append(o)
        if not force and os.path.exists(o) and all(
                os.path.getmtime(d) <= os.path.getmtime(o)
                for d in [s] + _hip_includes(s) + glob.glob(os.path.join(CSRC, "*.hpp")) + glob.glob(os.path.join(INCLUDE, "*.h"))):
            continue
        cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-pass-failed"] + os.environ.get("NF_HIPCC_FLAGS", "").split() + ["-c", s, "-o", o]
        if verbose:
            print(" ".join(cmd))
        procs.append((cmd, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
    for cmd, p in procs:
        out, _ = p.communicate()
        if p.returncode != 0:
            raise NativeLibraryError("hipcc failed: %s\n%s" % (" ".join(cmd), out.decode(errors="replace")))
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIBPATH] + objs
    subprocess.check_call(cmd)
    return LIBPATH


SAFE_WAITS_LIB = os.path.join(LIBDIR, "variants", "safe_waits.so")


def build_safe_waits(force=False):
    """The differential build of the counted-wait lint (tests/test_gpu_hygiene.py): every source that uses NF_WAIT_VMCNT recompiled
    with -DNF_SAFE_WAITS (each hand-counted `s_waitcnt vmcnt(N)` becomes a full drain), the other objects reused; selected at run
    time with NF_MI355X_LIB.  Built by __graft_entry__.build() so that it travels to the GPU box with the tree."""
    build()
    srcs = [s for s in sources() if "NF_WAIT_VMCNT" in open(s).read() or any("NF_WAIT_VMCNT" in open(i).read() for i in _hip_includes(s))]
    deps = srcs + glob.glob(os.path.join(CSRC, "*.hpp")) + glob.glob(os.path.join(INCLUDE, "*.h")) + [LIBPATH]
    if not force and os.path.exists(SAFE_WAITS_LIB) and all(os.path.getmtime(d) <= os.path.getmtime(SAFE_WAITS_LIB) for d in deps):
        return SAFE_WAITS_LIB
    vdir = os.path.dirname(SAFE_WAITS_LIB)
    os.makedirs(vdir, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    procs, objs = [], []
    for s in sources():
        base = os.path.basename(s)[:-4]
        if s in srcs:
            o = os.path.join(vdir, "safe_waits_%s.o" % base)
            cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-pass-failed", "-DNF_SAFE_WAITS", "-c", s, "-o", o]
            procs.append((cmd, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
        else:
            o = os.path.join(LIBDIR, "obj", base + ".o")
        objs.append(o)
    for cmd, p in procs:
        out, _ = p.communicate()
        if p.returncode != 0:
            raise NativeLibraryError("hipcc failed: %s\n%s" % (" ".join(cmd), out.decode(errors="replace")))
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", SAFE_WAITS_LIB] + objs)
    return SAFE_WAITS_LIB


def _header_text():
    import re
    txt = open(os.path.join(INCLUDE, "nf_mi355x.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def exported_symbols_declared():
    """Names of every function declared in include/nf_mi355x.h (used by the symbol-export test)."""
    import re
    return sorted(set(re.findall(r"\b(nf_[a-z0-9_]+)\s*\(", _header_text())))


def int64_functions_declared():
    """Names of the functions include/nf_mi355x.h declares as returning int64_t (scratch / pack sizes): ctypes assumes a 32-bit int
    unless told otherwise, and a size above 2^31 elements then arrives truncated.  (Round 6, last session: nf_maf_solve_t_scratch_floats
    had its return type set only on the ablation-build path -- the density-direction backward of config 5's layer failed above
    ~720 000 rows per call with a scratch buffer a fraction of the size the kernel addressed.)"""
    import re
    return sorted(set(re.findall(r"^\s*int64_t\s+(nf_[a-z0-9_]+)\s*\(", _header_text(), flags=re.M)))


_SCALARS = {"int": C.c_int, "int64_t": C.c_int64, "double": C.c_double, "float": C.c_float, "nf_stream_t": C.c_void_p}


def _ctype(decl, fn):
    """The ctypes type of one C declarator (a return type, or a parameter with or without its name) of function `fn`: any pointer is
    c_void_p (which accepts None, ints, ctypes arrays and string buffers), scalars by _SCALARS; anything else is an error, never skipped."""
    words = [w for w in decl.replace("*", " * ").split() if w != "const"]
    if "*" in words:
        return C.c_char_p if words[0] == "char" else C.c_void_p
    if len(words) > 2 or not words or words[0] not in _SCALARS:
        raise NativeLibraryError("include/nf_mi355x.h: %s has a type this binding does not know: %r" % (fn, decl))
    return _SCALARS[words[0]]


def prototypes_declared():
    """{name: (restype, [argtypes])} of every function include/nf_mi355x.h declares, parsed like the two lists above."""
    import re
    out = {}
    for ret, fn, params in re.findall(r"([A-Za-z_][\w \*]*?)\b(nf_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", _header_text()):
        params = [p.strip() for p in params.split(",")]
        out[fn] = (_ctype(ret, fn), [] if params == ["void"] else [_ctype(p, fn) for p in params])
    return out


def _declare_prototypes(handle):
    """restype and argtypes of every entry point from the header: a bare Python number is then converted to the width the C side reads
    (not passed as a 32-bit int), and a wrong count or kind of argument raises instead of reaching the kernel launch."""
    for fn, (restype, argtypes) in prototypes_declared().items():
        if hasattr(handle, fn):
            f = getattr(handle, fn)
            f.restype, f.argtypes = restype, argtypes


def lib():
    global _lib
    if _lib is None:
        path = os.environ.get("NF_MI355X_LIB")   # another build of the SAME sources: the safe-waits library of the counted-wait differential test
        if not path:
            path = LIBPATH
            if not os.path.exists(LIBPATH):
                raise NativeLibraryError(
                    "libnf_mi355x.so is missing (%s). Build it with `python -c 'import __graft_entry__ as g; g.build()'`."
                    " There is no CPU or eager fallback." % LIBPATH)
        handle = C.CDLL(path)
        _declare_prototypes(handle)       # (every function of the header, not a hand-kept list)
        _lib = handle
    return _lib


def call(name, *args):
    """Call the entry point `name` (returns an errno-style code) and raise on failure under that same name."""
    check(call_rc(name, *args), name)


def call_rc(name, *args):
    """The raw return code of the entry point `name`, for the callers that read NF_ENOTSUP as "this shape is declined" (every C-ABI
    call goes through here: one place to observe them)."""
    return getattr(lib(), name)(*args)


def query(name, *args):
    """The value of a size / scratch / layout query `name` (*_pack_size, *_scratch_floats, *_partials, ...) as a Python int."""
    return int(getattr(lib(), name)(*args))


def size(name, *args):
    """query() for the size functions whose negative values are error codes: those raise under the function's name."""
    n = query(name, *args)
    if n < 0:
        check(n, name)
    return n


def check(rc, what):
    if rc == 0:
        return
    msg = lib().nf_strerror(rc).decode()
    if rc == -22:
        raise ValueError("%s: %s" % (what, msg))
    if rc in (-95, -34):
        raise NotImplementedError("%s: %s" % (what, msg))
    raise RuntimeError("%s: %s (code %d)" % (what, msg, rc))


def dtype_code(t):
    if t.dtype == torch.float32:
        return NF_F32
    if t.dtype == torch.float64:
        return NF_F64
    raise TypeError("nf_mi355x kernels support float32/float64 tensors, got %s" % t.dtype)


KERNEL_DTYPES = (torch.float32, torch.float64)


def check_operands(entry, tensors, dtype=None):
    """The dtype contract of one C-ABI call ("Operand dtypes and shapes"): every floating-point tensor among `tensors`
    has ONE dtype, float32 or float64, and that is `dtype` when one is given (an entry point without a `dtype` parameter reads
    float32).  Integer / bool tensors (index tables, pointer tables, ReLU bits) and None are not looked at.  The C side sees
    `const void *`: a kernel instantiated for one element type would read another's bytes, past the end of the narrower buffer.
    Attribute reads only: no synchronisation, no allocation, any device (safe under stream capture).  Returns the common dtype (None
    when no floating tensor is among the operands)."""
    ref, ref_i = dtype, None
    for i, t in enumerate(tensors):
        if t is None or not t.dtype.is_floating_point:
            continue
        if ref is None:
            ref, ref_i = t.dtype, i
        if t.dtype != ref or ref not in KERNEL_DTYPES:
            if ref not in KERNEL_DTYPES:
                raise TypeError("%s: operand %d is %s; the kernels take float32 / float64 tensors only" % (entry, i, t.dtype))
            raise TypeError("%s: operand %d is %s but %s: one call takes tensors of one floating-point dtype (nothing is converted "
                            "silently; cast the input or the module)"
                            % (entry, i, t.dtype, "this entry point reads %s" % ref if ref_i is None else "operand %d is %s" % (ref_i, ref)))
    return ref


def check_count(entry, name, t, want, why):
    """ValueError unless the tensor `t` (None passes) holds exactly `want` elements (`why`: the formula, for the message): the kernels
    index an operand by the call's scalar arguments, whatever its size."""
    if t is not None and t.numel() != want:
        raise ValueError("%s: %s has %d elements (shape %s), the call reads %d (%s)" % (entry, name, t.numel(), tuple(t.shape), want, why))


def tri_count(D):
    """Entries of a strict triangle of a D x D matrix (LULinearPermute's lower_entries / upper_entries)."""
    return D * (D - 1) // 2


def coupling_param_channels(C, c1, scale_map):
    """P of nf_affine_coupling[_pb|_bwd]: channels of `param` for z (B, C, HW) with c1 identity channels -- (shift, scale) interleaved per
    transformed channel, or the shift alone without a scale map."""
    return (C - c1) * (1 if scale_map is None else 2)


def rqs_derivative_count(K, tails_code):
    """Derivative logits per element that nf_rqs_coupling reads behind the 2 K widths and heights: K - 1 (linear tails), K (circular),
    K + 1 (no tails, or per-feature tails)."""
    return {TAILS["linear"]: K - 1, TAILS["circular"]: K}.get(tails_code, K + 1)


def rqs_derivative_ok(K, n):
    """nf_rqs_spline takes (K-1 | K | K+1) derivative logits per element (linear | circular | no tails)."""
    return n in (K - 1, K, K + 1)


def rows_ok(n_loc, n_log_scale, d, B, indexed):
    """nf_diag_gaussian_log_prob_rows: both parameter blocks are the same whole number of rows of d elements -- one per sample unless the
    rows are picked by an index (class labels)."""
    if n_loc != n_log_scale or (n_loc % d if d else n_loc):
        return False
    return indexed or d == 0 or n_loc // d == B


def leading_shape_ok(x_shape, p_shape):
    """A per-element parameter block (..., K) of nf_rqs_spline has one row per input element (the leading shape itself may be the
    inputs' flattened: the kernel sees N rows)."""
    return len(p_shape) >= 1 and math.prod(p_shape[:-1]) == math.prod(x_shape)


def require_device(*tensors, dtype=None, entry=None, also=()):
    """Every tensor operand of a wrapper: on the current HIP device, and (check_operands) of one kernel dtype -- `dtype` when the entry
    point is float32-only.  `also`: operands the wrapper converts itself (a mask, a label matrix) -- device check only.  `entry`: the
    name for the message (default: the calling function's)."""
    _require_device(tensors)
    if also:
        _require_device(also)
    if entry is None:
        entry = sys._getframe(1).f_code.co_name
    return check_operands(entry, tensors, dtype)


def _require_device(tensors):
    cur = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError(
                "normflows_amd layers run only on an MI355X (HIP) device; got a %s tensor. There is no CPU path."
                % t.device)
        if cur is None:
            cur = torch.cuda.current_device()
        if t.device.index != cur:   # kernels are enqueued on the CURRENT device's stream (one process per GPU)
            raise RuntimeError("tensor on %s but the current device is cuda:%d: call torch.cuda.set_device first"
                               % (t.device, cur))


def ptr(t):
    if t is None:
        return C.c_void_p(0)
    if not t.is_contiguous():
        raise ValueError("tensor handed to the C ABI must be contiguous")
    return C.c_void_p(t.data_ptr())


def ptr_any(t):
    """Device pointer of a tensor whose rows may be strided (last dim unit stride)."""
    return C.c_void_p(0 if t is None else t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


i64 = C.c_int64
i32 = C.c_int
f64 = C.c_double
