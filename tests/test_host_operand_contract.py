"""Host tests of the operand contract ("Operand dtypes and shapes"): the dtype check every wrapper runs, the size
predicates, a source sweep of ops.py for wrappers without a check, and the cast / expand rule of the layers that evaluate a
caller-supplied module -- on CPU tensors, with the device check, the stream and the library stubbed (tests/operand_audit.py)."""
import ast
import ctypes
import os

import pytest
import torch

import operand_audit


@pytest.fixture(scope="module")
def nfa():
    import __graft_entry__
    import normflows_amd
    if not os.path.exists(normflows_amd.native_library_path()):
        __graft_entry__.build()
    return normflows_amd


F32, F64, BF16, F16 = torch.float32, torch.float64, torch.bfloat16, torch.float16


def T(*shape, dtype=F32):
    return torch.zeros(*shape, dtype=dtype)


# ---- 1. check_operands ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("other", [F64, BF16, F16], ids=str)
def test_check_operands_refuses_mixed_floating_dtypes(nfa, other):
    with pytest.raises(TypeError) as e:
        nfa._lib.check_operands("nf_some_entry", [T(3), None, T(3, dtype=other)])
    msg = str(e.value)
    assert "nf_some_entry" in msg and str(F32) in msg and str(other) in msg and "operand 2" in msg
    with pytest.raises(TypeError):
        nfa._lib.check_operands("nf_some_entry", [T(3, dtype=other), T(3)])


def test_check_operands_passes_uniform_kernel_dtypes_and_ignores_the_rest(nfa):
    L = nfa._lib
    assert L.check_operands("e", [T(2, dtype=F64), T(5, dtype=F64)]) == F64
    assert L.check_operands("e", [T(2), T(5)]) == F32
    assert L.check_operands("e", [T(2), None, T(2, dtype=torch.int64), T(2, dtype=torch.int32), T(2, dtype=torch.bool)]) == F32
    assert L.check_operands("e", [None, T(2, dtype=torch.int64)]) is None
    assert L.check_operands("e", []) is None


@pytest.mark.parametrize("dtype", [BF16, F16], ids=str)
def test_check_operands_refuses_uniform_narrow_dtypes(nfa, dtype):
    with pytest.raises(TypeError) as e:
        nfa._lib.check_operands("entry_x", [T(2, dtype=dtype), T(2, dtype=dtype)])
    assert "entry_x" in str(e.value) and str(dtype) in str(e.value)


def test_check_operands_demands_the_given_dtype(nfa):
    L = nfa._lib
    assert L.check_operands("e", [T(2)], dtype=F32) == F32
    with pytest.raises(TypeError) as e:
        L.check_operands("float32_only_entry", [T(2, dtype=torch.int32), T(2, dtype=F64)], dtype=F32)
    assert "float32_only_entry" in str(e.value) and str(F64) in str(e.value) and str(F32) in str(e.value)


def test_require_device_runs_the_dtype_check_and_names_the_wrapper(nfa, monkeypatch):
    L = nfa._lib
    with pytest.raises(RuntimeError):                   # the device check still comes first
        L.require_device(T(2), T(2, dtype=F64))
    monkeypatch.setattr(L, "_require_device", lambda tensors: None)

    def some_wrapper():
        L.require_device(T(2), T(2, dtype=F64))
    with pytest.raises(TypeError) as e:
        some_wrapper()
    assert "some_wrapper" in str(e.value)
    assert L.require_device(T(2), also=(T(2, dtype=F64),)) == F32          # converted by the wrapper: device check only


# ---- 2. size predicates ------------------------------------------------------------------------------------------------------
def test_size_predicates(nfa):
    L = nfa._lib
    assert [L.tri_count(D) for D in (0, 1, 2, 6, 8, 64)] == [0, 0, 1, 15, 28, 2016]
    assert L.coupling_param_channels(8, 4, "exp") == 8 and L.coupling_param_channels(5, 3, "sigmoid") == 4
    assert L.coupling_param_channels(5, 3, None) == 2 and L.coupling_param_channels(6, 0, "exp") == 12
    K = 8
    assert [L.rqs_derivative_count(K, c) for c in (0, 1, 2, 3)] == [9, 7, 8, 9]
    assert [L.rqs_derivative_ok(K, n) for n in (6, 7, 8, 9, 10)] == [False, True, True, True, False]
    assert L.leading_shape_ok((5, 6), (5, 6, 8)) and L.leading_shape_ok((0, 6), (0, 6, 8)) and L.leading_shape_ok((), (8,))
    assert L.leading_shape_ok((5, 6), (30, 8)) and L.leading_shape_ok((130, 1), (130, 8))       # (flattened inputs: N rows)
    assert not L.leading_shape_ok((5, 6), (5, 7, 8)) and not L.leading_shape_ok((5, 6), (29, 8)) and not L.leading_shape_ok((5,), ())
    assert L.rows_ok(3 * 6, 3 * 6, 6, 5, True) and L.rows_ok(5 * 6, 5 * 6, 6, 5, False) and L.rows_ok(0, 0, 6, 0, False)
    assert not L.rows_ok(3 * 6, 3 * 6, 6, 5, False) and not L.rows_ok(3 * 6 + 1, 3 * 6 + 1, 6, 5, True)
    assert not L.rows_ok(3 * 6, 2 * 6, 6, 5, True) and L.rows_ok(3 * 6, 3 * 6, 6, 0, True)
    L.check_count("e", "s", None, 7, "")
    L.check_count("e", "s", T(0, 6), 0, "B * inner")             # B = 0
    with pytest.raises(ValueError) as e:
        L.check_count("nf_entry", "s", T(5, 7), 30, "B * inner")
    assert "nf_entry" in str(e.value) and "35" in str(e.value) and "30" in str(e.value)


# ---- 3. source sweep ---------------------------------------------------------------------------------------------------------
# wrappers that hand pointers to the C ABI without a check of their own, on purpose
UNCHECKED = {
    "_train_fwd": "shared body of the three training forwards: each caller runs require_device on x / h2 / blob first",
    "mfma_clock_mhz": "takes no tensor: it allocates both operands itself",
}
_ABI = ("call", "call_rc", "query", "size")
_PTR = ("ptr", "ptr_any", "_cptr", "_ptr_array")


def _calls(node, names, attr_of=None):
    for n in ast.walk(node):
        if isinstance(n, ast.Call):
            f = n.func
            if attr_of is None and isinstance(f, ast.Name) and f.id in names:
                yield n
            if attr_of is not None and isinstance(f, ast.Attribute) and f.attr in names and isinstance(f.value, ast.Name) \
                    and f.value.id == attr_of:
                yield n


def test_every_wrapper_that_passes_pointers_checks_its_operands(nfa):
    src = open(nfa.ops.__file__).read()
    tree = ast.parse(src)
    unchecked, no_f32, feeder = [], [], []
    n_wrappers = 0
    for fn in [n for n in tree.body if isinstance(n, ast.FunctionDef)]:
        abi = [c for c in _calls(fn, _ABI, "L") if any(True for a in c.args for _ in _calls(a, _PTR))]
        if not abi:
            continue
        n_wrappers += 1
        checks = list(_calls(fn, ("require_device", "check_operands"), "L"))
        if not checks:
            unchecked.append(fn.name)
            continue
        codes = list(_calls(fn, ("dtype_code",), "L"))
        if not codes:           # no `dtype` argument goes to the C side: a float32-only entry point
            if not all(any(k.arg == "dtype" and ast.unparse(k.value) == "torch.float32" for k in c.keywords) for c in checks):
                no_f32.append(fn.name)
        for c in codes:         # the tensor that names the call's dtype is itself among the checked operands
            who = ast.unparse(c.args[0])
            if not any(ast.unparse(a) == who for chk in checks for a in chk.args):
                feeder.append((fn.name, who))
    assert n_wrappers > 80, n_wrappers
    assert sorted(unchecked) == sorted(UNCHECKED), "wrappers that pass pointers without L.require_device / L.check_operands: %s" % unchecked
    assert not no_f32, "float32-only wrappers whose check does not demand float32: %s" % no_f32
    assert not feeder, "the tensor given to L.dtype_code is not among the checked operands: %s" % feeder
    # and nothing goes round the one function every call passes through
    assert "L.lib()." not in src


# ---- 4. the audit itself, and the layers' cast / expand rule, on CPU ------------------------------------------------------------
@pytest.fixture
def cpu_abi(nfa, monkeypatch):
    """The library stubbed out behind the audit: device check and stream replaced, every consistent call "succeeds"."""
    L = nfa._lib
    monkeypatch.setattr(L, "_require_device", lambda tensors: None)
    monkeypatch.setattr(L, "stream", lambda: ctypes.c_void_p(0))
    return operand_audit.install(nfa, monkeypatch, forward=lambda name, *args: 0)


def test_audit_blocks_an_inconsistent_call(nfa, cpu_abi):
    L = nfa._lib
    z, b, y, ld = T(5, 6), T(6), T(5, 6), T(5)
    L.call("nf_masked_affine", L.ptr(z), L.ptr(b), L.ptr(T(5, 6)), L.ptr(None), L.ptr(y), L.ptr(ld), 5, 6, 0, 0, L.NF_F32, L.stream())
    assert cpu_abi.forwarded == ["nf_masked_affine"] and not cpu_abi.violations
    for bad in (T(5, 1), T(5, 6, dtype=F64), T(5, 6, dtype=BF16)):
        with pytest.raises(operand_audit.AuditViolation):
            L.call("nf_masked_affine", L.ptr(z), L.ptr(b), L.ptr(bad), L.ptr(None), L.ptr(y), L.ptr(ld), 5, 6, 0, 0, L.NF_F32, L.stream())
    with pytest.raises(operand_audit.AuditViolation):       # a typed pointer: perm is `const int64_t *`
        L.call("nf_lu_linear_permute", L.ptr(z), L.ptr(y), L.ptr(ld), L.ptr(T(6, dtype=torch.int32)), L.ptr(T(15)), L.ptr(T(15)), L.ptr(T(6)),
               L.ptr(T(6)), 5, 6, 1e-3, 0, 0, L.NF_F32, L.stream())
    assert cpu_abi.forwarded == ["nf_masked_affine"] and len(cpu_abi.violations) == 4


def test_wrappers_refuse_before_the_abi(nfa, monkeypatch):
    L, ops = nfa._lib, nfa.ops
    monkeypatch.setattr(L, "_require_device", lambda tensors: None)
    monkeypatch.setattr(L, "stream", lambda: ctypes.c_void_p(0))
    audit = operand_audit.install(nfa, monkeypatch, block_all=True)
    z = T(5, 6)
    cases = [
        (TypeError, lambda: ops.masked_affine(z, T(6), T(5, 6, dtype=F64), None, 0)),
        (TypeError, lambda: ops.masked_affine(z, T(6), T(5, 6, dtype=BF16), None, 0)),
        (ValueError, lambda: ops.masked_affine(z, T(6), T(5, 1), None, 0)),
        (ValueError, lambda: ops.masked_affine(z, T(6), None, T(4, 6), 0)),
        (ValueError, lambda: ops.masked_affine_bwd(z, T(6), T(5, 7), None, T(5, 6), T(5), 0)),
        (TypeError, lambda: ops.diag_gaussian_log_prob(T(5, 6, dtype=F64), T(1, 6), T(1, 6))),
        (ValueError, lambda: ops.diag_gaussian_log_prob(T(5, 6), T(1, 8), T(1, 8))),
        (ValueError, lambda: ops.diag_gaussian_log_prob_rows(T(5, 6), T(3, 7), T(3, 7), torch.zeros(5, dtype=torch.long))),
        (ValueError, lambda: ops.diag_gaussian_log_prob_rows(T(5, 6), T(4, 6), T(4, 6))),
        (TypeError, lambda: ops.actnorm(T(5, 6, dtype=F64), T(6), T(6), 0)),
        (ValueError, lambda: ops.actnorm(T(5, 6), T(7), T(7), 0)),
        (ValueError, lambda: ops.actnorm_bwd(T(5, 6), T(7), T(6), T(5, 6), T(5), 0)),
        (ValueError, lambda: ops.actnorm_init(T(6), T(6), T(7), T(6), 0)),
        (ValueError, lambda: ops.affine_coupling(T(5, 4, 2, 2), T(5, 3, 2, 2), 2, False, "exp", 0)),
        (ValueError, lambda: ops.affine_coupling(T(5, 4, 2, 2), T(5, 4, 2, 2), 2, False, None, 0)),
        (ValueError, lambda: ops.affine_coupling(T(5, 4, 2, 2), T(5, 4, 2, 2), 2, False, "exp", 0, param_bias=T(5))),
        (TypeError, lambda: ops.affine_coupling(T(5, 4, 2, 2), T(5, 4, 2, 2, dtype=F16), 2, False, "exp", 0)),
        (ValueError, lambda: ops.affine_coupling_bwd(T(5, 4, 2, 2), T(5, 4, 2, 1), T(5, 4, 2, 2), T(5), 2, False, "exp", 0)),
        (ValueError, lambda: ops.inv1x1_conv(T(5, 4, 2, 2), T(5, 5), T(()))),
        (ValueError, lambda: ops.inv1x1_conv(T(5, 4, 2, 2), T(4, 4), T(()), bias=T(5))),
        (TypeError, lambda: ops.inv1x1_conv(T(5, 4, 2, 2, dtype=F64), T(4, 4), T(()))),
        (ValueError, lambda: ops.inv1x1_conv_t(T(5, 4, 2, 2), T(3, 4))),
        (TypeError, lambda: ops.lu_linear_permute(T(5, 6, dtype=F64), torch.arange(6), T(15), T(15), T(6), T(6), 0)),
        (TypeError, lambda: ops.lu_linear_permute(z, torch.arange(6, dtype=torch.int32), T(15), T(15), T(6), T(6), 0)),
        (ValueError, lambda: ops.lu_linear_permute(z, torch.arange(6), T(14), T(15), T(6), T(6), 0)),
        (ValueError, lambda: ops.lu_linear_permute(z, torch.arange(6), T(15), T(15), T(6), T(8), 0)),
        (ValueError, lambda: ops.rqs_spline(z, T(5, 5, 8), T(5, 6, 8), T(5, 6, 7))),
        (ValueError, lambda: ops.rqs_spline(z, T(5, 6, 8), T(5, 6, 8), T(5, 6, 10))),
        (TypeError, lambda: ops.rqs_spline(z, T(5, 6, 8), T(5, 6, 8, dtype=F64), T(5, 6, 7))),
        (ValueError, lambda: ops.rqs_coupling(z, T(5, 3 * 22), T(3, 8), T(3, 8), T(3, 7), torch.arange(3), torch.arange(3, 6), 8, 0)),
        (ValueError, lambda: ops.rqs_coupling(z, T(5, 3 * 23), T(3, 8), T(2, 8), T(3, 7), torch.arange(3), torch.arange(3, 6), 8, 0)),
        (TypeError, lambda: ops.rqs_coupling(z, T(5, 3 * 23, dtype=F64), T(3, 8), T(3, 8), T(3, 7), torch.arange(3), torch.arange(3, 6), 8, 0)),
        (TypeError, lambda: ops.rows_matvec_affine(T(5, 6, dtype=F64), T(6, 6, dtype=F64), T(6, dtype=F64))),   # float32-only entry
        (TypeError, lambda: ops.lu_compose(torch.arange(6), *[T(n, dtype=F64) for n in (15, 15, 6, 6)])),
        (TypeError, lambda: ops.realnvp_chain(z, T(100, dtype=F64), 6, 16, 0)),
    ]
    for i, (exc, fn) in enumerate(cases):
        with pytest.raises(exc):
            fn()
        assert not audit.seen, "case %d reached the C ABI: %s" % (i, audit.names())


class _Net(torch.nn.Module):
    """A caller-supplied conditioner: a Linear whose output is post-processed by `post` (a cast, a slice)."""

    def __init__(self, d_in, d_out, post=lambda o: o):
        super().__init__()
        self.lin = torch.nn.Linear(d_in, d_out)
        self.post = post

    def forward(self, x):
        return self.post(self.lin(x.reshape(x.shape[0], -1)))


def _full_f32(audit, name, params, shape):
    got = [ts for n, ts in audit.seen if n == name]
    assert got, audit.names()
    for ts in got:
        for p in params:
            assert ts[p].dtype == F32 and ts[p].numel() == int(torch.Size(shape).numel()) and ts[p].is_contiguous(), (name, p, ts[p].dtype, ts[p].shape)


@pytest.mark.parametrize("grad", [False, True], ids=["eager", "autograd"])
@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
@pytest.mark.parametrize("post", [lambda o: o.to(BF16), lambda o: o.to(F16), lambda o: o[:, :1], lambda o: o[0], lambda o: o[:1]],
                         ids=["bf16", "f16", "B1", "inner", "1inner"])
def test_masked_affine_flow_casts_and_expands_conditioner_outputs(nfa, cpu_abi, post, inverse, grad):
    torch.manual_seed(0)
    b = torch.tensor([1.0, 0.0] * 3)
    flow = nfa.flows.MaskedAffineFlow(b, _Net(6, 6, post), _Net(6, 6, post))
    z = torch.randn(5, 6, requires_grad=grad)
    with torch.set_grad_enabled(grad):
        y, ld = flow.inverse(z) if inverse else flow.forward(z)
    assert y.dtype == F32 and ld.dtype == F32 and not cpu_abi.violations
    _full_f32(cpu_abi, "nf_masked_affine", ("z", "s", "t", "y"), (5, 6))
    if grad:
        (y.sum() + ld.sum()).backward()
        _full_f32(cpu_abi, "nf_masked_affine_bwd", ("z", "s", "t", "gy", "gz", "gs", "gt"), (5, 6))
        assert flow.s.lin.weight.grad is not None and flow.s.lin.weight.grad.dtype == F32


@pytest.mark.parametrize("post,exc", [(lambda o: o.double(), TypeError), (lambda o: torch.cat([o, o[:, :1]], 1), ValueError),
                                      (lambda o: o[:-1], ValueError), (lambda o: o[:, :2], ValueError)],
                         ids=["f64", "inner+1", "B-1", "two"])
@pytest.mark.parametrize("grad", [False, True], ids=["eager", "autograd"])
def test_masked_affine_flow_refuses_wider_or_unbroadcastable_outputs(nfa, cpu_abi, post, exc, grad):
    flow = nfa.flows.MaskedAffineFlow(torch.tensor([1.0, 0.0] * 3), _Net(6, 6), _Net(6, 6, post))
    with torch.set_grad_enabled(grad), pytest.raises(exc):
        flow.forward(torch.randn(5, 6, requires_grad=grad))
    assert not cpu_abi.seen


@pytest.mark.parametrize("grad", [False, True], ids=["eager", "autograd"])
@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
@pytest.mark.parametrize("cast", [BF16, F16], ids=str)
def test_affine_coupling_block_casts_narrow_parameters(nfa, cpu_abi, cast, inverse, grad):
    torch.manual_seed(0)
    block = nfa.flows.AffineCouplingBlock(_Net(4, 8, lambda o: o.to(cast)))
    z = torch.randn(5, 8, requires_grad=grad)
    with torch.set_grad_enabled(grad):
        y, ld = block.inverse(z) if inverse else block.forward(z)
    assert y.dtype == F32 and not cpu_abi.violations
    got = [ts for n, ts in cpu_abi.seen if n == "nf_affine_coupling_pb"]
    assert got and all(ts["param"].dtype == F32 and ts["param"].numel() == 5 * 8 for ts in got)
    if grad:
        (y.sum() + ld.sum()).backward()
        got = [ts for n, ts in cpu_abi.seen if n == "nf_affine_coupling_bwd"]
        assert got and all(ts["param"].dtype == F32 and ts["gparam"].dtype == F32 for ts in got)
        assert block.flows[1].param_map.lin.weight.grad is not None


@pytest.mark.parametrize("post,exc", [(lambda o: o.double(), TypeError), (lambda o: o[:, :7], ValueError), (lambda o: o[:-1], ValueError)],
                         ids=["f64", "P-1", "B-1"])
def test_affine_coupling_block_refuses_wider_or_missized_parameters(nfa, cpu_abi, post, exc):
    block = nfa.flows.AffineCouplingBlock(_Net(4, 8, post))
    with torch.no_grad(), pytest.raises(exc):
        block.forward(torch.randn(5, 8))
    assert not cpu_abi.seen
