"""GPU tests on offset, strided and misaligned tensor VIEWS (run with -m gpu on an MI355X).

Every other GPU test hands the kernels tensors that start at a fresh allocation.  Here each operand in turn is a view placed inside
a larger storage whose every other element is NaN -- a flat offset of 1, 2 or 3 elements (4 / 8 / 12 bytes off a 16-byte boundary
in float32, 8 bytes in float64: what dp.FlatParameters and `data[i:i + B]` with D % 4 != 0 produce), a row or column slice, every
second row, a transpose, a stride-0 expand, a channel slice or a padded batch stride of an image tensor -- and three things are asked
of the call:

  1. its result equals the result on clones of the operands: bit for bit (NaN-aware) wherever both calls end in the same kernel,
     which after the alignment rule of INTEGRATION.md ("Pointer alignment") is every case that ops._a16 realigns by a copy; where
     the misaligned pointer selects another kernel instead (the "switches path" row of that table), BOTH results are held against
     a float64 evaluation of the same operation at the tolerance the existing test of that operation uses;
  2. the storage around (and under) the view is unchanged, compared as bits: a call does not write to its input's storage;
  3. no NaN appears that the clones' result does not have: a read beyond the view that is used would poison the output.

The `calls` fixture records every C-ABI call with the alignment of its pointer arguments, so that a test can state which entry point
saw a misaligned pointer (and so which side of an alignment-gated branch ran: the gates are integer tests on those pointers)."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from conftest import TOL, assert_close, ld_tol

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
KINDS_2D = ("elem1", "elem2", "elem3", "row1", "cols", "rows2", "tr")


@pytest.fixture(scope="module")
def nfa():
    import normflows_amd
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    assert normflows_amd.native_library_path().endswith("normalizing-flows_amd/lib/libnf_mi355x.so")
    normflows_amd._lib.lib()
    return normflows_amd


@pytest.fixture
def calls(nfa, monkeypatch):
    """[(entry point, {pointer parameter: its address % 16})] of every C-ABI call made while the test runs."""
    from test_host import _abi_signatures
    sigs = _abi_signatures(nfa)
    log = []
    real = nfa._lib.call

    def spy(name, *args):
        al = {}
        for (pname, is_ptr), a in zip(sigs[name], args):
            if is_ptr and isinstance(a, ctypes.c_void_p) and a.value:
                al[pname] = a.value % 16
        log.append((name, al))
        return real(name, *args)
    monkeypatch.setattr(nfa._lib, "call", spy)
    return log


def saw(log, name, misaligned=(), aligned=()):
    """Was `name` called with every pointer of `misaligned` off a 16-byte boundary and every pointer of `aligned` on one?"""
    return any(n == name and all(al.get(p_, 0) != 0 for p_ in misaligned) and all(al.get(p_, 0) == 0 for p_ in aligned)
               for n, al in log)


# ---- views ------------------------------------------------------------------------------------------------------------------
def embed(t, kind):
    """(view, base): `view` has t's values and shape and lies inside the NaN-filled contiguous tensor `base`."""
    def nan(*shape):
        return torch.full(shape, NAN, dtype=t.dtype, device=t.device)
    n = t.numel()
    if kind in ("elem1", "elem2", "elem3"):
        k = int(kind[-1])
        base = nan(n + k + 5)
        view = base[k:k + n].view(t.shape)
    elif kind == "row1":                       # rows [1, B + 1) of a taller tensor: misaligned when the row length is not 16 bytes
        base = nan(t.shape[0] + 2, *t.shape[1:])
        view = base[1:t.shape[0] + 1]
    elif kind == "cols":                       # a column slice: row stride > D
        base = nan(t.shape[0], t.shape[1] + 7)
        view = base[:, 3:3 + t.shape[1]]
    elif kind == "rows2":                      # every second row
        base = nan(2 * t.shape[0], *t.shape[1:])
        view = base[::2]
    elif kind == "tr":                         # the transpose of a (D, B) tensor that itself starts 2 elements into its storage
        base = nan(n + 7)
        view = base[2:2 + n].view(t.shape[1], t.shape[0]).t()
    elif kind == "expand":                     # one row, stride 0 (the caller passes a tensor of equal rows)
        base = nan(t[0].numel() + 7)
        base[3:3 + t[0].numel()] = t[0].reshape(-1)
        return base[3:3 + t[0].numel()].view(t[0].shape).expand(t.shape), base
    elif kind == "chan":                       # channels [1, 1 + C) of a (B, C + 2, H, W) image tensor
        base = nan(t.shape[0], t.shape[1] + 2, *t.shape[2:])
        view = base[:, 1:1 + t.shape[1]]
    elif kind == "bstride":                    # contiguous images, batch stride C H W + 5
        per = t[0].numel()
        base = nan(t.shape[0], per + 5)
        view = base[:, :per].unflatten(1, tuple(t.shape[1:]))
    else:
        raise KeyError(kind)
    view.copy_(t)
    assert view.shape == t.shape and view.untyped_storage().data_ptr() == base.untyped_storage().data_ptr()
    return view, base


def bits(t):
    return t.contiguous().view(-1).view(torch.int32 if t.element_size() == 4 else torch.int64)


def same(a, b):
    """Bit equality that lets NaN equal NaN (and tells inf from the largest float)."""
    return (a.shape == b.shape and a.dtype == b.dtype and torch.equal(torch.isnan(a), torch.isnan(b))
            and torch.equal(torch.isinf(a), torch.isinf(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b)))


def assert_same(got, want, what):
    assert len(got) == len(want), what
    for i, (a, b) in enumerate(zip(got, want)):
        if a is None or b is None:
            assert a is None and b is None, (what, i)
            continue
        assert a.shape == b.shape and a.dtype == b.dtype, (what, i, a.shape, b.shape)
        new_nan = int((torch.isnan(a) & ~torch.isnan(b)).sum())
        assert new_nan == 0, "%s output %d: %d NaN the result on clones does not have" % (what, i, new_nan)
        assert same(a, b), "%s output %d: max |diff| %.3e" % (what, i, float((torch.nan_to_num(a.double()) - torch.nan_to_num(b.double())).abs().max()))


def on_views(fn, args, kinds, compare=assert_same, tag=""):
    """fn(**args) -> a tuple of tensors.  For every (argument name, kind) of `kinds`: the call with that argument embedded (embed)
    against the call on clones; the embedding storage must come back bit for bit.  `compare(got, want, what)` decides equality."""
    clones = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in args.items()}
    want = tuple(fn(**clones))
    n = 0
    for name, ks in kinds.items():
        for kind in ks:
            view, base = embed(args[name], kind)
            before = base.clone()
            want_k = want if kind != "expand" else tuple(fn(**dict(clones, **{name: view.clone()})))
            got = tuple(fn(**dict(clones, **{name: view})))
            torch.cuda.synchronize()
            what = "%s %s=%s" % (tag, name, kind)
            assert torch.equal(bits(base), bits(before)), what + ": the call wrote to its input's storage"
            compare(got, want_k, what)
            n += 1
    return n


def rows(B, D, seed, dtype=torch.float32, scale=1.5):
    g = torch.Generator().manual_seed(seed)
    x = scale * torch.randn(B, D, generator=g, dtype=torch.float64)
    x[: max(B // 8, 1)] *= 3.0                 # some rows beyond the tail bound
    return x.to(dtype).to(DEV)


def perturbed(module, seed, sigma=0.05):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p_ in module.parameters():
            p_.add_(sigma * torch.randn(p_.shape, generator=g).to(p_.dtype))
    return module


def nsf_model(nfa, D, hidden, blocks, pairs, seed, K=8, dtype=torch.float32):
    torch.manual_seed(seed)
    flows = []
    for i in range(pairs):
        flows += [nfa.flows.CoupledRationalQuadraticSpline(D, blocks, hidden, num_bins=K, init_identity=False, reverse_mask=bool(i & 1)),
                  nfa.flows.LULinearPermute(D, identity_init=False)]
    m = nfa.NormalizingFlow(nfa.distributions.DiagGaussian(D, trainable=False), flows)
    return perturbed(m, seed + 1).to(dtype).to(DEV).eval()


# ---- 1. layers on views -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [65, 129])
def test_fused_chain_on_views(nfa, calls, B):
    """2 x [CoupledRQS(64, 2 blocks, hidden 128, 8 bins), LULinearPermute(64)]: the persistent fused chain in both directions.  Its rows
    move as 16-byte vectors and the entry point refuses a misaligned x, so every view reaches it as an aligned copy: same bits."""
    m = nsf_model(nfa, 64, 128, 2, 2, seed=B)
    x, eps = rows(B, 64, B), rows(B, 64, B + 1, scale=1.0)
    with torch.no_grad():
        on_views(lambda x: (m.log_prob(x),), dict(x=x), dict(x=KINDS_2D), tag="log_prob")
        on_views(lambda eps: m.sample_from_noise(eps), dict(eps=eps), dict(eps=KINDS_2D), tag="sample")
    assert saw(calls, "nf_rqs_fused_chain") and not saw(calls, "nf_rqs_fused_chain", misaligned=["x"])


def _coupling_f64(nfa, x, cond, uw, uh, ud, ii, ti, mode, kw):
    y, ld = nfa.ops.rqs_coupling(x.double(), cond.double(), uw.double(), uh.double(), ud.double(), ii, ti, 8, mode,
                                 y=(x.double().clone() if mode != nfa._lib.RQS_DENSITY else None), **kw)
    return y, ld


@pytest.mark.parametrize("B", [1024, 33])
def test_rqs_coupling_kernel_choice_on_views(nfa, calls, B):
    """nf_rqs_coupling with the conditioner output in HBM (the unfused path of the D = 64 layer), density and sample-transform.
    B = 1024 is the smallest batch the pipelined (LDS-DMA) kernel takes, and it takes it only when x, y and cond are 16-byte
    aligned (rqs_spline.hip, the gate in front of rqs_coupling_pipe_kernel): a misaligned x, cond or caller-supplied y sends the
    call to the wave kernel, which moves the rows element by element.  The two kernels agree to a few ulp, not bit for bit
    (test_rqs_coupling_pipelined_kernel_vs_wave_kernel), so at B = 1024 BOTH results are held against the float64 kernel at
    conftest.TOL / ld_tol; at B = 33 both calls run the wave kernel: same bits.  Outputs given by the caller (y=, logdet=) that lie
    inside a NaN-filled storage are written inside their view only."""
    L = nfa._lib
    NT, D = 32, 64
    g = torch.Generator().manual_seed(B)
    x = (1.2 * torch.randn(B, D, generator=g)).to(DEV)
    cond = torch.randn(B, NT * 23, generator=g).to(DEV)
    uw, uh, ud = (torch.randn(NT, n, generator=g).to(DEV) for n in (8, 8, 7))
    ii, ti = torch.arange(0, D, 2, device=DEV), torch.arange(1, D, 2, device=DEV)
    kw = dict(tail_bound=3.0, wh_div=float(np.sqrt(128.0)))
    t32 = TOL[np.dtype("float32")]
    for mode in (L.RQS_DENSITY, L.RQS_SAMPLE_TRANSFORM):
        y64, ld64 = _coupling_f64(nfa, x, cond, uw, uh, ud, ii, ti, mode, kw)
        tld = ld_tol(np.float32, root_finding=(mode != L.RQS_DENSITY))

        def fn(x, cond):
            return nfa.ops.rqs_coupling(x, cond, uw, uh, ud, ii, ti, 8, mode, y=(x.clone(memory_format=torch.contiguous_format) if mode != L.RQS_DENSITY else None), **kw)

        def near_f64(got, want, what):
            for (y, ld) in (got, want):
                assert not torch.isnan(y).any() and not torch.isnan(ld).any(), what
                assert float((y.double() - y64).abs().max()) <= t32["atol"] + t32["rtol"] * float(y64.abs().max()), what
                assert bool(((ld.double() - ld64).abs() <= tld["atol"] + tld["rtol"] * ld64.abs()).all()), what
        del calls[:]
        on_views(fn, dict(x=x, cond=cond), dict(x=("elem1", "elem3", "cols", "tr"), cond=("elem1", "elem2", "rows2")),
                 compare=(near_f64 if B >= 1024 else assert_same), tag="mode %d" % mode)
        assert saw(calls, "nf_rqs_coupling", misaligned=["x"]) and saw(calls, "nf_rqs_coupling", misaligned=["cond"])
        assert saw(calls, "nf_rqs_coupling", aligned=["x", "y", "cond"])
        # caller-supplied outputs inside a NaN-filled storage
        want_y, want_ld = fn(x, cond)
        yv, ybase = embed(x, "elem1")                 # (sampling: the call owns the transform columns only, the rest stays x)
        lv, lbase = embed(torch.zeros(B, device=DEV), "elem1")
        ysnap, lsnap = ybase.clone(), lbase.clone()
        y, ld = nfa.ops.rqs_coupling(x, cond, uw, uh, ud, ii, ti, 8, mode, y=yv, logdet=lv, acc=L.LD_WRITE, **kw)
        assert y.data_ptr() == yv.data_ptr() and ld.data_ptr() == lv.data_ptr()
        (near_f64 if B >= 1024 else assert_same)((y, ld), (want_y, want_ld), "y=, logdet= views")
        for base, snap, n in ((ybase, ysnap, x.numel()), (lbase, lsnap, B)):
            keep = torch.ones(base.numel(), dtype=torch.bool, device=DEV)
            keep[1:1 + n] = False
            assert torch.equal(bits(base)[keep], bits(snap)[keep]), "an output view was overrun"


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("D", [5, 6, 7])
def test_narrow_layers_on_views(nfa, calls, D, dtype):
    """[CoupledRQS(D, 1 block, hidden 32), LULinearPermute(D)] at D = 5, 6, 7, where rows [1:] of a batch are misaligned: the fused
    kernel on rows padded to 64 columns (float32) and the layer-wise path (use_fused = False; the only path in float64), whose
    kernels (nf_rqs_coupling's generic kernel, nf_rows_matvec_affine / nf_lu_linear_permute below D = 64) move rows element by
    element and take the misaligned pointer as it is."""
    m = nsf_model(nfa, D, 32, 1, 1, seed=D, dtype=dtype)
    x, eps = rows(65, D, D, dtype), rows(65, D, D + 1, dtype, scale=1.0)
    kinds = ("row1", "elem1", "cols", "rows2", "tr")
    with torch.no_grad():
        for fused in (True, False):
            for f in m.flows:
                if hasattr(f, "prqct"):
                    f.prqct.use_fused = fused
            on_views(lambda x: (m.log_prob(x),), dict(x=x), dict(x=kinds), tag="log_prob fused=%s" % fused)
            on_views(lambda eps: m.sample_from_noise(eps), dict(eps=eps), dict(eps=kinds), tag="sample fused=%s" % fused)
    assert any(any(v for v in al.values()) for _, al in calls), "no kernel saw a misaligned pointer"


@pytest.mark.parametrize("D,H", [(96, 192), (33, 300)])
def test_nsf_wide_on_views(nfa, calls, D, H):
    """The one-launch wide coupling layer (nf_nsf_wide_k), B = 65 (one tile and one row): D = 96 loads and stores its x / y tile as
    16-byte vectors (the entry point refuses a misaligned x: aligned copy), D = 33 element by element -- there the misaligned
    pointer itself reaches the kernel."""
    torch.manual_seed(D)
    layer = perturbed(nfa.flows.CoupledRationalQuadraticSpline(D, 2, H, num_bins=8, init_identity=False), D).to(DEV).eval()
    x = rows(65, D, D + H)
    with torch.no_grad():
        on_views(lambda x: layer.inverse(x), dict(x=x), dict(x=KINDS_2D), tag="density")
        on_views(lambda x: layer.forward(x), dict(x=x), dict(x=KINDS_2D), tag="sampling")
    assert saw(calls, "nf_nsf_wide_k")
    assert saw(calls, "nf_nsf_wide_k", misaligned=["x"]) == (D % 4 != 0)


def test_context_layer_on_views(nfa, calls):
    """The conditional coupling layer (nf_nsf_wide_ctx, D = 17, C = 33, hidden 200): x as for the wide layer; the context is read
    element by element through its row stride -- a column slice, a stride-0 expand and a misaligned flat offset in place."""
    torch.manual_seed(3)
    layer = perturbed(nfa.flows.CoupledRationalQuadraticSpline(17, 2, 200, num_context_channels=33, num_bins=8, init_identity=False),
                      4).to(DEV).eval()
    x, c = rows(65, 17, 5), rows(65, 33, 6, scale=1.0)
    with torch.no_grad():
        for run, tag in ((layer.inverse, "density"), (layer.forward, "sampling")):
            on_views(lambda x, c: run(x, c), dict(x=x, c=c), dict(x=("elem1", "row1", "cols"), c=("cols", "expand", "elem1")), tag=tag)
    assert saw(calls, "nf_nsf_wide_ctx", misaligned=["context"]) and saw(calls, "nf_nsf_wide_ctx", misaligned=["x"])


@pytest.mark.parametrize("name", ["d", "f"])
def test_circular_wide_layer_on_views(nfa, calls, name):
    """nf_nsf_wide_ft on the fixture layers (d) (D = 16: vector tile) and (f) (D = 22: element-wise tile) of circ_wide_cases."""
    import circ_wide_cases as cw
    layer = cw.layer(nfa, name).to(DEV)
    D = cw.LAYERS[name][0]
    x = rows(65, D, 7, scale=1.0)
    with torch.no_grad():
        on_views(lambda x: layer.inverse(x), dict(x=x), dict(x=KINDS_2D), tag="density")
        on_views(lambda x: layer.forward(x), dict(x=x), dict(x=KINDS_2D), tag="sampling")
    assert saw(calls, "nf_nsf_wide_ft")
    assert saw(calls, "nf_nsf_wide_ft", misaligned=["x"]) == (D % 4 != 0)


@pytest.mark.parametrize("D,H", [(6, 16), (33, 300), (17, 40), (20, 40)])
def test_made_family_on_views(nfa, calls, D, H):
    """MaskedAffineAutoregressive (one MADE pass: nf_made_forward_affine; D-pass inverse in one launch: nf_maf_inverse_h) and the
    autoregressive spline layer (nf_made_forward_spline; the per-feature sampler) at B = 65.  D = 20 moves its rows as vectors."""
    torch.manual_seed(D + H)
    maf = perturbed(nfa.flows.MaskedAffineAutoregressive(D, H), D).to(DEV).eval()
    ar = perturbed(nfa.flows.AutoregressiveRationalQuadraticSpline(D, 2, H, num_bins=8, init_identity=False), H).to(DEV).eval()
    x = rows(65, D, D * H, scale=1.0)
    kinds = ("elem1", "elem3", "row1", "cols", "tr")
    with torch.no_grad():
        for layer, tag in ((maf, "maf"), (ar, "arnsf")):
            on_views(lambda x: layer.forward(x), dict(x=x), dict(x=kinds), tag=tag + " forward")
            on_views(lambda x: layer.inverse(x), dict(x=x), dict(x=kinds), tag=tag + " inverse")
    assert saw(calls, "nf_made_forward_affine") and saw(calls, "nf_made_forward_spline")
    assert saw(calls, "nf_made_forward_affine", misaligned=["x"]) == (D % 4 != 0)
    # MADE.forward alone: the raw (B, mult D) parameters of nf_made_forward
    made = perturbed(nfa.nets.MADE(features=D, hidden_features=H, num_blocks=2, output_multiplier=3), D + 1).to(DEV).eval()
    assert made.packed_forward(DEV) is not None
    with torch.no_grad():
        on_views(lambda x: (made(x),), dict(x=x), dict(x=kinds), tag="made_forward")
    assert saw(calls, "nf_made_forward") and saw(calls, "nf_made_forward", misaligned=["x"]) == (D % 4 != 0)


@pytest.mark.parametrize("name", ["grad_circ_ar_perm_d21_h40", "grad_ar_perm_lin_d12_h24"])
def test_per_feature_autoregressive_spline_on_views(nfa, calls, name):
    """The circular / mask-permuted autoregressive spline layers of tests/ar_ft_train_cases.py (D = 21 with five circular
    coordinates; D = 12 with a permuted mask) at B = 65: the density direction in one launch (nf_made_forward_spline_ft), the
    per-feature sampler (nf_arnsf_inverse_ft) and the density direction under autograd (autograd.MadeFtFn: nf_made_forward_train_ft,
    nf_made_backward_t64, nf_made_feed_ft_bwd, nf_made_wgrad).  These kernels gather x element by element through the feature
    table, so a misaligned x reaches them where it is (D = 12 included: no vector path on x); grad_y and grad_logdet as views."""
    import ar_ft_train_cases as cases
    layer = cases.make_layer(nfa, name, cases.load_case(name)).to(DEV)
    D, B = int(name.split("_d")[1].split("_")[0]), 65
    x = rows(B, D, D, scale=1.0)
    kinds = ("elem1", "elem3", "row1", "cols", "tr")
    layer.eval()
    with torch.no_grad():
        on_views(lambda x: layer.inverse(x), dict(x=x), dict(x=kinds), tag="density")
        on_views(lambda x: layer.forward(x), dict(x=x), dict(x=kinds), tag="sampler")
    assert saw(calls, "nf_made_forward_spline_ft", misaligned=["x"]) and saw(calls, "nf_arnsf_inverse_ft", misaligned=["z"])
    layer.train()
    params = list(layer.parameters())
    pn = [n for n, _ in layer.named_parameters()]
    gy, gld = rows(B, D, D + 1, scale=1.0), rows(B, 1, D + 2, scale=1.0).view(B)

    def fn(x, gy, gld):
        xl = x.detach().requires_grad_(True)
        z, ld = layer.inverse(xl)
        return (z.detach(), ld.detach()) + _grads((z, ld), [xl] + params, (gy, gld))
    del calls[:]
    on_views(fn, dict(x=x, gy=gy, gld=gld), dict(x=("elem1", "row1", "cols"), gy=("elem1", "cols", "tr"), gld=("expand", "elem1")),
             compare=grads_compare(3, 2e-3, 2e-4, pn), tag="training")
    for entry in ("nf_made_forward_train_ft", "nf_made_backward_t64", "nf_made_feed_ft_bwd", "nf_made_wgrad"):
        assert saw(calls, entry), entry
    assert saw(calls, "nf_made_forward_train_ft", misaligned=["x"])


@pytest.mark.parametrize("HW", [4, 8])
@pytest.mark.parametrize("C", [4, 5])
def test_glow_block_on_image_views(nfa, calls, C, HW):
    """GlowBlock (hidden 12) on B = 3 images: a channel slice of a wider tensor and a padded batch stride -- the two layouts
    nf_conv3x3_gather / nf_glow_convnet read in place -- and the flat offsets."""
    torch.manual_seed(C * HW)
    layer = perturbed(nfa.flows.GlowBlock(C, 12, split_mode="channel", use_lu=True, init_zeros=False), C + HW, 0.1).to(DEV).eval()
    g = torch.Generator().manual_seed(HW)
    z = torch.randn(3, C, HW, HW, generator=g).to(DEV)
    with torch.no_grad():
        layer.inverse(z)                            # the data-dependent ActNorm initialisation, once
        kinds = ("chan", "bstride", "elem1", "elem2", "elem3")
        on_views(lambda z: layer.inverse(z), dict(z=z), dict(z=kinds), tag="inverse")
        on_views(lambda z: layer.forward(z), dict(z=z), dict(z=kinds), tag="forward")


def test_conv_kernels_read_image_views_in_place(nfa, calls):
    """nf_glow_convnet and nf_conv3x3_gather take a channel slice of a wider tensor and a padded batch stride in place (through the
    image stride), and a flat offset as it is: they read the images element by element."""
    g = torch.Generator().manual_seed(4)
    Cin, Cout, B, H, W = 2, 4, 3, 4, 4
    w1, b1 = 0.2 * torch.randn(256, Cin, 3, 3, generator=g), 0.1 * torch.randn(256, generator=g)
    w2, b2 = 0.05 * torch.randn(256, 256, 1, 1, generator=g), 0.1 * torch.randn(256, generator=g)
    w3, b3 = 0.05 * torch.randn(Cout, 256, 3, 3, generator=g), 0.1 * torch.randn(Cout, generator=g)
    x = torch.randn(B, Cin, H, W, generator=g).to(DEV)
    layout = nfa.ops.glow_convnet_layout(B, H, W)
    assert layout is not None
    blob = nfa.ops.glow_convnet_pack(*[t.to(DEV) for t in (w1, b1, w2, b2, w3, b3)], layout=layout)
    assert blob is not None
    kinds = ("chan", "bstride", "elem1", "elem2", "elem3")
    with torch.no_grad():
        on_views(lambda x: (nfa.ops.glow_convnet(x, blob, Cout, 0.0, layout=layout),), dict(x=x), dict(x=kinds), tag="glow_convnet")
        on_views(lambda x: (nfa.ops.conv3x3_gather(x),), dict(x=x), dict(x=kinds), tag="conv3x3_gather")
    assert saw(calls, "nf_glow_convnet", misaligned=["x"]) and saw(calls, "nf_conv3x3_gather", misaligned=["in"])


def test_image_layers_on_views(nfa, calls):
    """ActNorm, Invertible1x1Conv (C = 3, 12) and an AffineCouplingBlock with a checkerboard split on image views."""
    g = torch.Generator().manual_seed(0)
    kinds = ("chan", "bstride", "elem1", "elem3")
    with torch.no_grad():
        for C in (3, 12):
            z = torch.randn(3, C, 4, 4, generator=g).to(DEV)
            torch.manual_seed(C)
            conv = perturbed(nfa.flows.Invertible1x1Conv(C, True), C, 0.1).to(DEV).eval()
            act = nfa.flows.ActNorm((C, 1, 1)).to(DEV).eval()
            act.forward(z)                          # data-dependent initialisation
            for layer, tag in ((conv, "inv1x1 C%d" % C), (act, "actnorm C%d" % C)):
                on_views(lambda z: layer.forward(z), dict(z=z), dict(z=kinds), tag=tag + " forward")
                on_views(lambda z: layer.inverse(z), dict(z=z), dict(z=kinds), tag=tag + " inverse")
        torch.manual_seed(1)
        net = nfa.nets.ConvNet2d((4, 8, 8, 8), (3, 1, 3), 0.0, init_zeros=False)
        block = perturbed(nfa.flows.AffineCouplingBlock(net, True, "sigmoid", "checkerboard"), 2, 0.1).to(DEV).eval()
        z = torch.randn(3, 4, 8, 8, generator=g).to(DEV)
        on_views(lambda z: block.forward(z), dict(z=z), dict(z=kinds), tag="checkerboard forward")
        on_views(lambda z: block.inverse(z), dict(z=z), dict(z=kinds), tag="checkerboard inverse")


def test_standalone_ops_on_views(nfa, calls):
    """rqs_spline with w / h / d as row-strided slices of one (N, 3K - 1) block (the documented use) that itself starts off
    alignment; lu_fwd with a caller-supplied log-det accumulator inside a NaN-filled storage; diag_gaussian_log_prob with a
    misaligned z and misaligned parameters (d = 64 takes the four-elements-per-lane kernel, which the entry point guards)."""
    g = torch.Generator().manual_seed(2)
    K, Nn = 8, 130
    x = (1.5 * torch.randn(Nn, generator=g)).to(DEV)
    block = torch.randn(Nn, 3 * K - 1, generator=g).to(DEV)

    def spline(x, block):
        w, h, d = block[:, :K], block[:, K:2 * K], block[:, 2 * K:]
        return nfa.ops.rqs_spline(x, w, h, d, tails="linear", tail_bound=3.0)
    with torch.no_grad():
        on_views(spline, dict(x=x.view(Nn, 1), block=block), dict(block=("elem1", "row1", "cols", "rows2")), tag="rqs_spline")
        assert saw(calls, "nf_rqs_spline", misaligned=["w"])
        # lu_fwd(logdet=): D = 64, B a multiple of 64
        lu = perturbed(nfa.flows.LULinearPermute(64, identity_init=False), 3).to(DEV)
        lin = lu.linear
        f = nfa.ops.lu_factors(lu.permutation._permutation, lin.lower_entries.detach(), lin.upper_entries.detach(),
                               lin.unconstrained_upper_diag.detach())
        xr = rows(128, 64, 9)
        lv, lbase = embed(torch.randn(128, generator=g).to(DEV), "elem1")
        lsnap, l0 = lbase.clone(), lv.clone()
        u, y, ld = nfa.ops.lu_fwd(xr, f[6], f[5], lin.bias.detach(), ld_const=f[4], logdet=lv)
        u2, y2, ld2 = nfa.ops.lu_fwd(xr, f[6], f[5], lin.bias.detach(), ld_const=f[4], logdet=l0)
        assert ld.data_ptr() == lv.data_ptr() and same(ld, ld2) and same(y, y2) and same(u, u2)
        keep = torch.ones(lbase.numel(), dtype=torch.bool, device=DEV)
        keep[1:129] = False
        assert torch.equal(bits(lbase)[keep], bits(lsnap)[keep])
        on_views(lambda x: nfa.ops.lu_fwd(x, f[6], f[5], lin.bias.detach(), ld_const=f[4]), dict(x=xr),
                 dict(x=("elem1", "cols", "rows2", "tr")), tag="lu_fwd")
        assert not saw(calls, "nf_lu_fwd", misaligned=["x"])
        # diag_gaussian_log_prob
        for d in (64, 5):
            z, loc, ls = rows(65, d, d), torch.randn(d, generator=g).to(DEV), (0.3 * torch.randn(d, generator=g)).to(DEV)
            on_views(lambda z, loc, ls: (nfa.ops.diag_gaussian_log_prob(z, loc, ls),), dict(z=z, loc=loc.view(1, d), ls=ls.view(1, d)),
                     dict(z=("elem1", "row1", "cols"), loc=("elem1", "elem2"), ls=("elem3",)), tag="diag_gaussian d=%d" % d)
        assert saw(calls, "nf_diag_gaussian_log_prob", misaligned=["z"])        # (d = 5: element by element, in place)


# ---- 2. backward on views -----------------------------------------------------------------------------------------------------
def _grads(outs, leaves, grad_outputs):
    return torch.autograd.grad(outs, leaves, grad_outputs=grad_outputs, allow_unused=True)


# Parameters whose gradient is a sum in an order that is not fixed by the values alone: the batch-shared spline parameters
# (nf_rqs_coupling_bwd accumulates them with atomics) and LULinearPermute's diagonal (nf_lu_param_grads[_composed] sum the log-det
# cotangent with 16-byte loads when it is 16-byte aligned and element by element otherwise: the gld B4 branch of rows_matvec.hip /
# lu_bwd.hip, which a misaligned grad_logdet view drives here)
ATOMIC = ("unconditional_transform", "unconstrained_upper_diag")


def grads_compare(n_exact, rtol, atol, names=None):
    """The first n_exact outputs (the layer's outputs and its input gradient: no reduction over the batch but fixed-order ones) bit
    for bit; the parameter gradients bit for bit too, unless the kernel accumulates them with atomics (nf_rqs_coupling_bwd's
    batch-shared spline parameters: the order of the additions changes from run to run) -- those within the bar
    test_gpu_training.check_layer_grads holds a layer's parameter gradients to (rtol, atol x scale).  names: the parameters' names,
    so that only those gradients (ATOMIC) may fall back to the bar."""
    def compare(got, want, what):
        assert_same(got[:n_exact], want[:n_exact], what)
        for i, (a, b) in enumerate(zip(got[n_exact:], want[n_exact:])):
            if a is None or b is None:
                assert a is None and b is None, (what, i)
            elif not same(a, b):
                assert names is None or any(k in names[i] for k in ATOMIC), (what, names[i], float((a - b).abs().max()))
                scale = max(1.0, float(b.abs().max()))
                assert not torch.isnan(a).any() and bool(((a - b).abs() <= atol * scale + rtol * b.abs()).all()), \
                    (what, i, float((a - b).abs().max()))
    return compare


@pytest.mark.parametrize("B", [128, 192, 1024 + 64])
def test_training_functions_backward_on_views(nfa, calls, B):
    """The D = 64 training Functions (autograd.LULinearPermuteFn, CouplingTrainFn layer by layer; PairTrainFn through
    NormalizingFlow.log_prob) with the input, grad_y and grad_logdet as views: gradients of the input and of every parameter against
    the same call on clones.  Every row operand of these kernels is refused when misaligned, so ops._a16 copies it: same bits.
    The one exception is the log-det cotangent under PairTrainFn: its sum (for LULinearPermute's diagonal) is taken with 16-byte
    loads when the vector is aligned and element by element otherwise (train_bwd.hip, vsum) -- another order of additions, so the
    diagonal's gradient is held to the bar test_pair_training_path_vs_separate_layers sets for parameter gradients (5e-4 of scale)
    and everything else stays bit-identical.
    The Functions take batches of 1024 rows and more (B = 1088 here); at B = 128 and 192 the same layers run kernel by kernel, where
    nf_rqs_coupling_bwd adds the batch-shared spline parameters' gradients with atomics: two runs on the SAME aligned tensors differ
    there by 5e-7 .. 8e-6 at values of order 10 (measured; every other output is reproducible), so those gradients -- and only
    gradients that are not bit-equal -- fall back to the bar of test_gpu_training.check_layer_grads (grads_compare)."""
    from bench import build_c2_model
    torch.manual_seed(B)
    m = build_c2_model(num_layers=2, sigma=0.05, blocks=2).to(DEV)
    params = list(m.parameters())
    names = [n for n, _ in m.named_parameters()]
    x = rows(B, 64, B, scale=1.0)
    gy, gld = rows(B, 64, B + 1, scale=1.0), rows(B, 1, B + 2, scale=1.0).view(B)

    def layerwise(x, gy, gld):
        xl = x.detach().requires_grad_(True)         # (a view stays a view: same storage, same offset)
        z, ld = xl, torch.zeros(B, device=DEV)
        for f in reversed(m.flows):
            z, l_ = f.inverse(z)
            ld = ld + l_
        return (z.detach(), ld.detach()) + _grads((z, ld), [xl] + params, (gy, gld))

    def model(x, gl):
        xl = x.detach().requires_grad_(True)
        lp = m.log_prob(xl)
        return (lp.detach(),) + _grads((lp,), [xl] + params, (gl,))

    def pair_compare(got, want, what):
        loose = [i for i, n in enumerate(names) if n.endswith("unconstrained_upper_diag")]
        keep = [i for i in range(len(got)) if i - 2 not in loose]
        grads_compare(2, 2e-3, 2e-4, [names[i - 2] for i in keep[2:]])([got[i] for i in keep], [want[i] for i in keep], what)
        for i in loose:
            a, b = got[i + 2], want[i + 2]
            assert float((a - b).abs().max()) <= 5e-4 * max(float(b.abs().max()), 1e-6), (what, names[i])

    on_views(layerwise, dict(x=x, gy=gy, gld=gld),
             dict(x=("elem1", "cols"), gy=("elem1", "cols", "tr"), gld=("expand", "elem1")), compare=grads_compare(3, 2e-3, 2e-4, names),
             tag="layerwise")
    on_views(model, dict(x=x, gl=gld), dict(x=("elem1", "rows2"), gl=("expand",)), compare=grads_compare(2, 2e-3, 2e-4, names), tag="pair")
    on_views(model, dict(x=x, gl=gld), dict(gl=("elem1",)), compare=pair_compare, tag="pair")
    for name in ("nf_coupling_train_bwd", "nf_pair_train_bwd", "nf_pair_train_bwd_head", "nf_lu_bwd", "nf_lu_fwd", "nf_final_bwd"):
        assert not any(n == name and any(al.get(p_, 0) for p_ in ("x", "x_in", "xlu", "grad_y", "gy", "g")) for n, al in calls), name
    if B >= 1024:
        assert saw(calls, "nf_rqs_fused_train_pair_fwd") and saw(calls, "nf_lu_fwd"), "the training Functions did not run"
        assert any(n.startswith("nf_pair_train_bwd") and al.get("grad_logdet", 0) for n, al in calls), "the element-wise vsum did not run"


def test_narrow_and_autoregressive_training_backward_on_views(nfa, calls):
    """Training gradients at B = 65 on the element-wise kernels (narrow coupling layer + LU in float32 and float64, MAF, AR-NSF, the
    conditional coupling layer): input, grad_y (elem1, cols, tr) and grad_logdet (expand, elem1) as views."""
    torch.manual_seed(0)
    B = 65
    cases = []
    for dt in (torch.float32, torch.float64):
        cases.append(("crqs7", nfa.flows.CoupledRationalQuadraticSpline(7, 1, 20, num_bins=4, init_identity=False), 7, dt, None))
        cases.append(("lu7", nfa.flows.LULinearPermute(7, identity_init=False), 7, dt, None))
    cases.append(("maf", nfa.flows.MaskedAffineAutoregressive(5, 18), 5, torch.float32, None))
    cases.append(("arnsf", nfa.flows.AutoregressiveRationalQuadraticSpline(6, 2, 16, num_bins=8, init_identity=False), 6, torch.float32, None))
    cases.append(("ctx", nfa.flows.CoupledRationalQuadraticSpline(6, 2, 40, num_context_channels=3, num_bins=8, init_identity=False), 6,
                  torch.float32, 3))
    for tag, layer, D, dt, C in cases:
        layer = perturbed(layer, D).to(dt).to(DEV)
        params = list(layer.parameters())
        x, gy, gld = rows(B, D, D, dt, scale=1.0), rows(B, D, D + 1, dt, scale=1.0), rows(B, 1, D + 2, dt, scale=1.0).view(B)
        ctx = None if C is None else rows(B, C, 11, dt, scale=1.0)
        for direction in ("inverse", "forward"):
            def fn(x, gy, gld, ctx=ctx):
                xl = x.detach().requires_grad_(True)
                z, ld = getattr(layer, direction)(xl) if ctx is None else getattr(layer, direction)(xl, ctx)
                if ld.dim() == 0:
                    ld = ld.expand(B)
                return (z.detach(), ld.detach()) + _grads((z, ld), [xl] + params, (gy, gld))
            pn = [n for n, _ in layer.named_parameters()]
            bar = grads_compare(3, 2e-3, 2e-4, pn) if dt == torch.float32 else grads_compare(3, 1e-8, 1e-9, pn)
            on_views(fn, dict(x=x, gy=gy, gld=gld), dict(x=("elem1", "row1"), gy=("elem1", "cols", "tr"), gld=("expand", "elem1")),
                     compare=bar, tag="%s %s %s" % (tag, dt, direction))


def test_training_ops_on_views(nfa, calls):
    """The stand-alone training kernels with each row operand as a view: rows_block, resblock_bwd, lu_bwd, linear_wgrad (every
    operand refused when misaligned: aligned copies, same bits), and the alignment-gated branches that take the misaligned pointer
    as it is -- rows_block's weights (rows_linear.hip vec_ok: 16-byte or element-wise staging, the same values in the same LDS
    slots), rqs_coupling_bwd[_p24] (rqs_bwd.hip: pipelined or wave kernel), inv1x1_wgrad (affine_bwd.hip: MFMA or element-wise
    kernel), lu_param_grads[_composed] (rows_matvec.hip / lu_bwd.hip B4: 16-byte or element-wise sum of the log-det cotangent) --
    where both results are held against float64 torch at the tolerance of the operation's own test."""
    ops, L = nfa.ops, nfa._lib
    g = torch.Generator().manual_seed(5)
    rn = lambda *s: torch.randn(*s, generator=g).to(DEV)        # noqa: E731
    # rows_block against float64 torch at the bars of test_rows_block_kernel_vs_torch (rtol 3e-5, atol 3e-5 sqrt(H); y through OUR t)
    B, H = 192, 128
    x, M1, M2, c1, c2 = rn(B, H), 0.1 * rn(H, H), 0.1 * rn(H, H), rn(H), rn(H)

    def rb(x, M1, c1):
        return ops.rows_block(x, M1, c1.view(-1), M2, c2)

    def rb_near(got, want, what):
        tol = dict(rtol=3e-5, atol=3e-5 * np.sqrt(H))
        t64 = x.double().clamp_min(0) @ M1.double().t() + c1.double()
        for t_o, y_o in (got, want):
            assert_close(t_o.cpu().numpy(), t64.float().cpu().numpy(), what=what + " t", **tol)
            y_ref = x.double() + t_o.double().clamp_min(0) @ M2.double().t() + c2.double()
            assert_close(y_o.cpu().numpy(), y_ref.float().cpu().numpy(), what=what + " y", **tol)
    on_views(rb, dict(x=x, M1=M1, c1=c1.view(1, H)), dict(x=("elem1", "cols", "rows2"), c1=("elem1",)), tag="rows_block")
    on_views(rb, dict(x=x, M1=M1, c1=c1.view(1, H)), dict(M1=("elem1", "elem2")), compare=rb_near, tag="rows_block weights")
    assert saw(calls, "nf_rows_block", misaligned=["M1"]) and not saw(calls, "nf_rows_block", misaligned=["in"])
    # resblock_bwd, lu_bwd, linear_wgrad: same bits
    gh, t_, h_in = rn(B, H), rn(B, H), rn(B, H)
    on_views(lambda gh, t_, h_in: ops.resblock_bwd(gh, t_, h_in, M1, M2), dict(gh=gh, t_=t_, h_in=h_in),
             dict(gh=("elem1", "cols"), t_=("elem2",), h_in=("tr",)), tag="resblock_bwd")
    gy, u, xx, Lm, Up = rn(B, 64), rn(B, 64), rn(B, 64), 0.2 * rn(64, 64), 0.2 * rn(64, 64)
    on_views(lambda gy, u, xx: ops.lu_bwd(gy, u, xx, Lm, Up), dict(gy=gy, u=u, xx=xx),
             dict(gy=("elem1", "tr"), u=("elem3",), xx=("cols",)), tag="lu_bwd")
    for (Bw, M, N) in ((128, 256, 128), (65, 20, 24), (65, 7, 5)):        # ring shape | vector kernel | element-wise kernel
        dy, xw = rn(Bw, M), rn(Bw, N)
        on_views(lambda dy, xw: ops.linear_wgrad(dy, xw), dict(dy=dy, xw=xw), dict(dy=("elem1", "cols", "tr"), xw=("elem1", "rows2")),
                 tag="linear_wgrad %d %d %d" % (Bw, M, N))
    assert saw(calls, "nf_linear_wgrad_skip", misaligned=["dY"])              # (N = 5: the element-wise kernel, in place)
    # rqs_coupling_bwd[_p24]: pipelined or wave kernel.  Reference and bars are those of test_spline_backward_pipelined_kernel_full_batch,
    # literally: the same rows with one more row appended (an odd batch takes the wave kernel on aligned tensors); row gradients
    # |err| / (1 + |ref|) < 1e-4, the shared parameters' (minus the extra row's own call) 1e-3 max|ref| + 1e-2
    NT, D, Bs = 32, 64, 130
    xs, cond = 1.2 * rn(Bs, D), rn(Bs, NT * 23)
    uw, uh, ud = rn(NT, 8), rn(NT, 8), rn(NT, 7)
    gys, gls = rn(Bs, D), rn(Bs)
    ii, ti = torch.arange(0, D, 2, device=DEV), torch.arange(1, D, 2, device=DEV)
    kw = dict(tail_bound=3.0, wh_div=float(np.sqrt(128.0)))
    xe, ge, le, ce = (torch.cat([t, e_]) for t, e_ in ((xs, 1.2 * rn(1, D)), (gys, rn(1, D)), (gls, rn(1)), (cond, rn(1, NT * 23))))

    def odd_batch_ref(run, cond_of):
        c = run(xe, ge, le, cond_of(ce))
        e = run(xe[Bs:].contiguous(), ge[Bs:].contiguous(), le[Bs:].contiguous(), cond_of(ce[Bs:].contiguous()))
        return [c[0][:Bs].double(), c[1][:Bs].double()] + [c[i].double() - e[i].double() for i in (2, 3, 4)]
    ref = odd_batch_ref(lambda a, b, c_, d: ops.rqs_coupling_bwd(a, b, c_, d, uw, uh, ud, ii, ti, 8, L.RQS_DENSITY, **kw), lambda c_: c_)

    def bwd_near(got, want, what, ref_=None):
        for res in (got, want):
            for i, (a, r) in enumerate(zip(res, ref_ or ref)):
                assert not torch.isnan(a).any(), what
                if i < 2:
                    err = (a.double() - r).abs() / (1.0 + r.abs())
                    assert float(err.max()) < 1e-4, (what, i, float(err.max()))
                else:
                    assert float((a.double() - r).abs().max()) < 1e-3 * float(r.abs().max()) + 1e-2, (what, i)
    del calls[:]
    on_views(lambda xs, gys, cond: ops.rqs_coupling_bwd(xs, gys, gls, cond, uw, uh, ud, ii, ti, 8, L.RQS_DENSITY, **kw),
             dict(xs=xs, gys=gys, cond=cond), dict(xs=("elem1",), gys=("elem2", "cols"), cond=("elem3",)), compare=bwd_near,
             tag="rqs_coupling_bwd")
    assert saw(calls, "nf_rqs_coupling_bwd", misaligned=["x"]) and saw(calls, "nf_rqs_coupling_bwd", misaligned=["grad_y"])
    assert saw(calls, "nf_rqs_coupling_bwd", misaligned=["cond"]) and saw(calls, "nf_rqs_coupling_bwd", aligned=["x", "grad_y", "cond"])
    # ... and on the 24-float parameter rows: a misaligned cond24 is refused by the entry point (ops copies it), x / grad_y choose the kernel
    def pad24(c_):
        out = torch.zeros(c_.shape[0], NT, 24, device=DEV)
        out[:, :, :23] = c_.view(-1, NT, 23)
        return out
    cond24 = pad24(cond)
    r24 = odd_batch_ref(lambda a, b, c_, d: ops.rqs_coupling_bwd_p24(a, b, c_, d, uw, uh, ud, ii, ti, **kw), pad24)
    r24[1][:, :, 23] = 0.0

    def p24_near(got, want, what):
        got, want = [list(r_) for r_ in (got, want)]
        for r_ in (got, want):
            r_[1] = r_[1].clone()
            r_[1][:, :, 23] = 0.0                   # (the pad column of the gradient rows is not specified)
        bwd_near(got, want, what, r24)
    on_views(lambda xs, gys, c24: ops.rqs_coupling_bwd_p24(xs, gys, gls, c24.view(Bs, NT, 24), uw, uh, ud, ii, ti, **kw),
             dict(xs=xs, gys=gys, c24=cond24.view(Bs, NT * 24)), dict(xs=("elem1", "cols"), gys=("elem3",), c24=("elem1", "rows2")),
             compare=p24_near, tag="rqs_coupling_bwd_p24")
    assert saw(calls, "nf_rqs_coupling_bwd_p24", misaligned=["x"]) and saw(calls, "nf_rqs_coupling_bwd_p24", misaligned=["grad_y"])
    assert saw(calls, "nf_rqs_coupling_bwd_p24", aligned=["x", "grad_y"]) and not saw(calls, "nf_rqs_coupling_bwd_p24", misaligned=["cond24"])
    # inv1x1_wgrad: MFMA kernel (HW % 16 == 0, aligned) or the element-wise one; both against float64 torch at the bar
    # test_affine_family_backward_kernels_vs_torch_autograd holds Inv1x1Fn's gradients to in float32 (rtol 2e-5, atol 100 x 2e-5)
    z, gz, gl = rn(4, 8, 4, 4), rn(4, 8, 4, 4), rn(4)

    def wg_near(got, want, what):
        r = torch.einsum("bop,bcp->oc", gz.double().flatten(2), z.double().flatten(2))
        for gW, _ in (got, want):
            assert_close(gW.cpu().numpy(), r.float().cpu().numpy(), what=what, rtol=2e-5, atol=100 * 2e-5)
    on_views(lambda z, gz: ops.inv1x1_wgrad(z, gz, gl), dict(z=z, gz=gz), dict(z=("elem1", "chan"), gz=("elem2", "bstride")),
             compare=wg_near, tag="inv1x1_wgrad")
    assert saw(calls, "nf_inv1x1_wgrad", misaligned=["z"]) and saw(calls, "nf_inv1x1_wgrad", misaligned=["gy"])
    # lu_param_grads: the sum of the log-det cotangent (B4), against the float64 formula at the bar of
    # test_lu_linear_permute_training_wide_vs_float64 (2e-5 x max(1, max |ref|))
    Dd = 64
    n_tri = Dd * (Dd - 1) // 2
    gL, gU, udiag, gldv = rn(Dd, Dd), rn(Dd, Dd), rn(Dd), rn(1000)

    def pg_near(got, want, what):
        d = torch.nn.functional.softplus(udiag.double()) + 1e-3
        r = (gU.double().diagonal() + gldv.double().sum() / d) * torch.sigmoid(udiag.double())
        for res in (got, want):
            assert same(res[0], want[0]) and same(res[1], want[1]), what
            assert float((res[2].double() - r).abs().max()) <= 2e-5 * max(1.0, float(r.abs().max())), what
    on_views(lambda gldv: ops.lu_param_grads(gL, gU, gldv.view(-1), udiag, n_tri), dict(gldv=gldv.view(1000, 1)),
             dict(gldv=("elem1", "elem2", "elem3")), compare=pg_near, tag="lu_param_grads")
    assert saw(calls, "nf_lu_param_grads", misaligned=["gld"]) and saw(calls, "nf_lu_param_grads", aligned=["gld"])
    # autograd.linear (LinearFn from 1024 rows: library products for y and gx, nf_linear_wgrad for the weight gradient) on views of x
    # and of the cotangent; the library may pick another product kernel for a misaligned operand, so both results are held against
    # float64 torch at the bars of test_linear_autograd_matches_torch
    torch.manual_seed(6)
    lin = nfa.nets.Linear(48, 96).to(DEV)
    xl_, wl_ = rn(1024, 48), rn(1024, 96)

    def lin_fn(xl_, wl_):
        xq = xl_.detach().requires_grad_(True)
        y = lin(xq)
        return (y.detach(),) + _grads((y,), [xq, lin.weight, lin.bias], (wl_,))

    def lin_near(got, want, what):
        W64, b64 = lin.weight.detach().double(), lin.bias.detach().double()
        r = (xl_.double() @ W64.t() + b64, wl_.double() @ W64, wl_.double().t() @ xl_.double(), wl_.double().sum(0))
        for res in (got, want):
            for a, r_, (rt, at) in zip(res, r, ((1e-5, 1e-5), (1e-5, 1e-5), (1e-4, 1e-3), (1e-4, 1e-3))):
                assert torch.allclose(a.double(), r_, rtol=rt, atol=at), (what, float((a.double() - r_).abs().max()))
    on_views(lin_fn, dict(xl_=xl_, wl_=wl_), dict(xl_=("elem1", "cols"), wl_=("elem1", "tr")), compare=lin_near, tag="linear")
    assert saw(calls, "nf_linear_wgrad_skip") or saw(calls, "nf_linear_wgrad") or saw(calls, "nf_linear_wgrad_act")


# ---- 3. FlatParameters whose slices are not multiples of four floats --------------------------------------------------------------
class _Chain(torch.nn.Module):
    """log q(x7, x5, x6, img) of four independent small flows: every kind of parameter tensor the training kernels write."""

    def __init__(self, nfa):
        super().__init__()
        F = nfa.flows
        # (registration order = order in the flat buffer: this one puts weight matrices at all three misaligned offsets)
        self.c = F.AutoregressiveRationalQuadraticSpline(6, 2, 16, num_bins=8, init_identity=False)
        self.a = torch.nn.ModuleList([F.CoupledRationalQuadraticSpline(7, 1, 20, num_bins=4, init_identity=False),
                                      F.LULinearPermute(7, identity_init=False)])
        self.b = F.MaskedAffineAutoregressive(5, 18)
        self.d = F.GlowBlock(5, 12, split_mode="channel", use_lu=True, init_zeros=False)

    def forward(self, xa, xb, xc, img):
        ld = torch.zeros(xa.shape[0], device=xa.device)
        z = xa
        for f in reversed(self.a):
            z, l_ = f.inverse(z)
            ld = ld + l_
        zb, lb = self.b.inverse(xb)
        zc, lc = self.c.inverse(xc)
        zd, ldd = self.d.inverse(img)
        nll = 0.5 * ((z ** 2).sum(1) + (zb ** 2).sum(1) + (zc ** 2).sum(1) + (zd ** 2).flatten(1).sum(1)) - (ld + lb + lc + ldd)
        return nll.mean()


def test_flat_parameters_with_misaligned_slices(nfa, calls):
    """dp.FlatParameters lays the parameters out back to back without padding: with sizes such as D = 5, K = 4, hidden 18 weights,
    biases and gradient destinations start 4, 8 and 12 bytes off a 16-byte boundary.  Three Adam steps on fixed data -- the second
    one accumulating the gradients of two different micro-batches -- with FlatParameters and with the plain parameters, held to
    the bars of test_flat_parameters_training_step_on_the_benchmark_kernels: equal losses, bit-equal gradients, parameters to 1e-7
    absolute after Adam with lr 1e-3.  The one exception are the batch-shared spline parameters of the coupling layer
    (`unconditional_transform.*`): nf_rqs_coupling_bwd adds their gradients with atomics, so two runs on the SAME tensors differ
    in the last bits (grads_compare says where that was measured); those three gradients are held to check_layer_grads' bar, and
    after each step these three parameters are copied from the plain run, so that the atomics' noise cannot reach the next
    step's loss and every other comparison stays exact."""
    torch.manual_seed(7)
    m = perturbed(_Chain(nfa), 8).to(DEV)
    g = torch.Generator().manual_seed(9)
    data = [(torch.randn(50, 7, generator=g).to(DEV), torch.randn(50, 5, generator=g).to(DEV), torch.randn(50, 6, generator=g).to(DEV),
             torch.randn(50, 5, 4, 4, generator=g).to(DEV)) for _ in range(2)]
    with torch.no_grad():
        m(*data[0])                                 # the GlowBlock's data-dependent ActNorm initialisation, before the copy
    ref = copy.deepcopy(m)
    flat = nfa.dp.FlatParameters(m)
    offs = {}
    for (n, p_) in m.named_parameters():
        offs.setdefault(p_.data_ptr() % 16, []).append((n, tuple(p_.shape)))
    print("byte offsets of the parameter slices:", {k: len(v) for k, v in sorted(offs.items())})
    for off in (4, 8, 12):
        assert any(len(shape) >= 2 and shape[0] > 1 for _, shape in offs.get(off, [])), \
            "no weight matrix %d bytes off alignment: %s" % (off, offs.get(off))
    opt = torch.optim.Adam(flat.parameters(), lr=1e-3)
    opt_ref = torch.optim.Adam(ref.parameters(), lr=1e-3)
    for step in range(3):
        batches = data if step == 1 else data[:1]
        flat.zero_grad()
        ref.zero_grad(set_to_none=True)
        losses = []
        for b in batches:
            la, lb = m(*b), ref(*b)
            la.backward()
            lb.backward()
            losses.append((float(la.detach()), float(lb.detach())))
        flat.sync()
        print("step", step, "losses", losses)
        assert all(a == b for a, b in losses), (step, losses)
        off = 0
        for (n, p_), q in zip(m.named_parameters(), ref.parameters()):
            gflat = flat.grad[off:off + p_.numel()].view(p_.shape)
            off += p_.numel()
            assert q.grad is not None or float(gflat.abs().max()) == 0.0, n
            if q.grad is not None and not torch.equal(gflat, q.grad):
                assert "unconditional_transform" in n, (step, n, float((gflat - q.grad).abs().max()))
                scale = max(1.0, float(q.grad.abs().max()))
                assert bool(((gflat - q.grad).abs() <= 2e-4 * scale + 2e-3 * q.grad.abs()).all()), \
                    (step, n, float((gflat - q.grad).abs().max()), float(q.grad.abs().max()))
        opt.step()
        opt_ref.step()
        for (n, p_), q in zip(m.named_parameters(), ref.parameters()):
            assert torch.allclose(p_, q, rtol=0, atol=1e-7), (step, n, float((p_ - q).abs().max()))
            if "unconditional_transform" in n:
                with torch.no_grad():
                    p_.copy_(q)
    flat.release()
