"""GPU tests of the fused chain kernel's trimmed vector code (csrc/rqs_fused.hip, csrc/fused_common.hpp): the ReLUs as one v_med3 on the
raw accumulators (relu_raw), the identity half's batch-shared splines two elements per packed bin evaluation (rqs_table_fast2) and the
rotating accumulator sets of the compact final layer.  Chains of three coupling layers (alone, and as [coupling, LULinearPermute]
pairs) at the kernel's own shape (D 64, 128 hidden units, 2 blocks) and at one zero-padded shape (D 7, 48 hidden units), 33 and 257
rows, both mask parities, both directions, 4 / 8 / 16 bins, against the layer-wise unfused path and the float64 oracle with the
tolerances of tests/test_gpu_parity.py::test_fused_kernel_on_narrower_layers_vs_unfused_and_oracle (single layer 2e-4, chain 1e-3), and
256-row against 128-row workgroups bit for bit."""
import numpy as np
import pytest
import torch

from conftest import assert_close

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SHAPES = [(64, 128), (7, 48)]
TOL_LAYER = dict(rtol=2e-4, atol=2e-4)
TOL_CHAIN = dict(rtol=1e-3, atol=1e-3)


@pytest.fixture(autouse=True)
def _inference_mode():
    with torch.no_grad():
        yield


@pytest.fixture(scope="module")
def nfa():
    import __graft_entry__
    import normflows_amd
    import os
    if not os.path.exists(normflows_amd.native_library_path()):
        __graft_entry__.build()
    return normflows_amd


def N(t):
    return t.detach().cpu().numpy()


def _flows(nfa, D, hidden, bins, lu, reverse0, seed):
    """The layers of tests/test_gpu_parity.py::test_fused_kernel_on_narrower_layers_vs_unfused_and_oracle, whose tolerances this file
    uses: init_identity=False, every parameter (the identity half's batch-shared spline and the LU factors included) moved by
    0.05 * randn."""
    torch.manual_seed(seed)
    flows = []
    for i in range(3):
        flows.append(nfa.flows.CoupledRationalQuadraticSpline(D, 2, hidden, num_bins=bins, init_identity=False,
                                                              reverse_mask=bool(i & 1) != reverse0))
        if lu:
            flows.append(nfa.flows.LULinearPermute(D, identity_init=False))
    for f in flows:
        for p_ in f.parameters():
            p_.add_(0.05 * torch.randn_like(p_))
    return flows


def _state(flows):
    st = {}
    for i, f in enumerate(flows):
        st.update({"flows.%d.%s" % (i, k): v.detach().cpu().numpy() for k, v in f.state_dict().items()})
    return {k: v.astype(np.float64) if v.dtype == np.float32 else v for k, v in st.items()}


def _oracle64(oracle, flows, x, inverse, bins):
    ora = oracle.OracleNSF(_state(flows), num_layers=len(flows), K=bins, tail_bound=3.0)
    z, logq = x.astype(np.float64), np.zeros(len(x), np.float64)
    for i in (range(len(flows) - 1, -1, -1) if inverse else range(len(flows))):
        z = (ora.coupling if ora._is_coupling(i) else ora.lu)(i, z, 0 if inverse else 1, logq, +1)
    return z, logq


def _layerwise(flows, xd, inverse):
    """Every layer on its own launch(es), the fused route off."""
    z, ld = xd, torch.zeros(xd.shape[0], device=DEV)
    for f in (reversed(flows) if inverse else flows):
        if hasattr(f, "prqct"):
            f.prqct.use_fused = False
        try:
            z, l = (f.inverse if inverse else f.forward)(z)
        finally:
            if hasattr(f, "prqct"):
                f.prqct.use_fused = True
        ld = ld + l
    return z, ld


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _fused(nfa, flows, xd, inverse):
    """The chain as one persistent launch on 128-row and on 256-row workgroups: the same bits (NaN payloads included)."""
    from normflows_amd.core import run_chain
    out = []
    try:
        for small in (True, False):
            nfa.config.set_fused_small_batch(small)
            ld = torch.zeros(xd.shape[0], device=DEV)
            out.append((run_chain(flows, xd, inverse, ld, +1), ld))
    finally:
        nfa.config.set_fused_small_batch(True)
    (z1, l1), (z0, l0) = out
    assert _same_bits(z1, z0) and _same_bits(l1, l0), "128-row and 256-row workgroups differ"
    return z1, l1


def _first(flows, inverse):
    """The coupling layer a chain runs first in this direction."""
    return [f for f in (reversed(flows) if inverse else flows) if hasattr(f, "prqct")][0]


def _table(layer, bins, nblk=2):
    """The identity half's knot table as the kernel reads it from the packed blob (fused_common.hpp FusedLayout: header 64 floats,
    tables behind the initial, hidden and final biases): (32, 3 (K + 1)) = cumulative widths | heights | derivatives per feature."""
    blob = layer.prqct._fused_blob(None)
    off = 64 + 128 + 256 * nblk + 96 * bins
    return N(blob[off:off + 32 * 3 * (bins + 1)]).reshape(32, 3 * (bins + 1)).copy()


def _specials(knots):
    """Inputs for one feature: every inner knot exactly, +-tail_bound, the floats just outside, one point inside every bin."""
    K = len(knots) - 1
    assert knots[0] == np.float32(-3.0) and knots[K] == np.float32(3.0) and np.all(np.diff(knots) > 0)
    mid = ((knots[:-1].astype(np.float64) + knots[1:]) / 2).astype(np.float32)
    assert np.all(mid > knots[:-1]) and np.all(mid < knots[1:])
    edge = np.float32([3.0, -3.0, np.nextafter(np.float32(3.0), np.float32(4.0)), np.nextafter(np.float32(-3.0), np.float32(-4.0))])
    return np.concatenate([knots[1:K], edge, mid]).astype(np.float32)


def _compare(nfa, oracle, flows, x, inverse, bins, finite_rows, what):
    """Fused chain (both workgroup sizes) and fused first layer against the layer-wise path and the float64 oracle on `finite_rows`."""
    xd = x.to(DEV)
    assert all(f.prqct._fused_eligible(xd, None) for f in flows if hasattr(f, "prqct"))
    zf, lf = _fused(nfa, flows, xd, inverse)
    zu, lu_ = _layerwise(flows, xd, inverse)
    first = _first(flows, inverse)
    if first is (flows[-1] if inverse else flows[0]):        # the chain starts with the coupling itself: that layer alone, too
        z1, l1 = (first.inverse if inverse else first.forward)(xd)
        z1u, l1u = _layerwise([first], xd, inverse)
        assert_close(N(z1)[finite_rows], N(z1u)[finite_rows], what=what + ": first layer z", **TOL_LAYER)
        assert_close(N(l1)[finite_rows], N(l1u)[finite_rows], what=what + ": first layer ld", **TOL_LAYER)
    r = finite_rows
    zo, lo = _oracle64(oracle, flows, x.numpy()[r], inverse, bins)      # (rows are independent: the oracle sees the finite ones)
    assert np.isfinite(N(zf)[r]).all() and np.isfinite(N(lf)[r]).all(), what
    assert_close(N(zf)[r], N(zu)[r], what=what + ": chain vs layer-wise z", **TOL_CHAIN)
    assert_close(N(lf)[r], N(lu_)[r], what=what + ": chain vs layer-wise ld", **TOL_CHAIN)
    assert_close(N(zf)[r].astype(np.float64), zo, what=what + ": chain vs float64 oracle z", **TOL_CHAIN)
    assert_close(N(lf)[r].astype(np.float64), lo, what=what + ": chain vs float64 oracle ld", **TOL_CHAIN)
    return zf, lf, zu, lu_


@pytest.mark.parametrize("lu", [False, True])
@pytest.mark.parametrize("bins", [4, 8, 16])
@pytest.mark.parametrize("D,hidden", SHAPES)
def test_identity_half_on_knots_edges_and_non_finite_inputs(nfa, oracle, D, hidden, bins, lu):
    """The identity half of the layer the chain runs first gets, feature by feature, inputs exactly ON every inner knot of its packed
    table (the knots the kernel's own bin search compares against: widths in the density direction, heights in the sample
    direction), on +-tail_bound, on the floats just outside, and one point inside every bin; spread over the rows so that every one of
    them occurs (checked).  With a fused LU the density direction runs the LU first, so its knots are only met approximately there.
    Chains without an LU also carry three rows with +inf, -inf and NaN in one identity column: the linear tails pass such a value
    through (the layer alone: the identity half of these rows equals the layer-wise path's, non-finite entry included), the rest of
    such a row is not comparable (NaN * weight in every path) and the finite rows must not notice them."""
    for reverse0 in (False, True):
        flows = [f.to(DEV) for f in _flows(nfa, D, hidden, bins, lu, reverse0, seed=7 * D + bins + reverse0)]
        for B in (33, 257):
            for inverse in (True, False):
                first = _first(flows, inverse)
                cols = first.prqct.identity_features.cpu().numpy()
                tab = _table(first, bins)
                g = torch.Generator().manual_seed(B + inverse)
                x = 1.3 * torch.randn(B, D, generator=g)
                nbad = 0 if lu else 3
                nspec = 2 * bins + 3
                rows = min(B - nbad, nspec)
                met = set()
                for j, c in enumerate(cols):
                    kn = tab[j, :bins + 1] if inverse else tab[j, bins + 1:2 * bins + 2]
                    sp = _specials(kn)
                    idx = (np.arange(rows) + 12 * j) % nspec
                    x[:rows, c] = torch.from_numpy(sp[idx])
                    met.update(idx.tolist())
                assert met == set(range(nspec)), "a knot, an edge or a bin is not met"
                finite = np.ones(B, bool)
                if nbad:
                    x[B - 3, cols[0]], x[B - 2, cols[0]], x[B - 1, cols[0]] = float("inf"), float("-inf"), float("nan")
                    finite[B - 3:] = False
                what = "D=%d hidden=%d K=%d lu=%d reverse=%d B=%d %s" % (D, hidden, bins, lu, reverse0, B,
                                                                        "density" if inverse else "sample")
                _compare(nfa, oracle, flows, x, inverse, bins, finite, what)
                if nbad:
                    xd = x.to(DEV)
                    z1, _ = (first.inverse if inverse else first.forward)(xd)
                    z1u, _ = _layerwise([first], xd, inverse)
                    assert_close(N(z1)[B - 3:][:, cols], N(z1u)[B - 3:][:, cols], what=what + ": identity half of the non-finite rows",
                                 **TOL_LAYER)
                    assert np.array_equal(N(z1)[B - 3:, cols[0]], N(xd)[B - 3:, cols[0]], equal_nan=True)


@pytest.mark.parametrize("lu", [False, True])
@pytest.mark.parametrize("bins", [4, 8, 16])
@pytest.mark.parametrize("D,hidden", SHAPES)
def test_relu_on_zero_negative_zero_denormal_and_large_preactivations(nfa, oracle, D, hidden, bins, lu):
    """Conditioner weights set so that the pre-activations in front of both ReLUs of a residual block include exact 0, -0, denormals
    and large magnitudes (checked on the host for the initial layer's output): hidden unit 0 has zero weights and bias, unit 1 has
    -0 weights and bias (rows 0..3 have positive identity inputs: every product is -0), unit 2 a zero weight row and a denormal bias,
    unit 3 its weight row times 1e4 (its consumers' columns times 1e-4, so the layer stays comparable in float32); the same rows of
    each block's first Linear give the second ReLU the same values.  Same comparison as above.
    The last row carries a NaN in one identity column (its other entries inside the splines' interval).  What the parent commit's
    kernel gives for it, measured on that build (this test passes there) and unchanged here: every entry of the chain's output row is
    NaN in both directions -- NaN * weight reaches every hidden unit through the initial layer (the ReLU's max(NaN, 0) = 0 takes it out
    of the block's branch only, not out of the residual stream), every spline parameter of the row is NaN, and the next layer's mask or
    LU hands the NaN to the other half.  The row's log-det is NaN too, except in the density direction of a chain with LUs: there the
    first LU makes the whole row NaN before any spline sees it, a NaN is outside every spline's interval (identity, log-det 0), and
    the log-det is the finite sum of the LUs' constant log|det|.  The layer-wise path gives the same row and the same log-det."""
    for reverse0 in (False, True):
        flows = [f.to(DEV) for f in _flows(nfa, D, hidden, bins, lu, reverse0, seed=11 * D + bins + reverse0)]
        for f in flows[::2 if lu else 1]:
            net = f.prqct.transform_net
            lins = [net.initial_layer] + [b.linear_layers[0] for b in net.blocks]
            for li, lin in enumerate(lins):
                lin.weight[0].zero_()
                lin.bias[0] = 0.0
                lin.weight[1].fill_(-0.0)
                lin.bias[1] = -0.0
                lin.weight[2].zero_()
                lin.bias[2] = 1e-40
                if li == 0:
                    lin.weight[3] *= 1e4
            for lin in [b.linear_layers[0] for b in net.blocks] + [net.final_layer]:
                lin.weight[:, 3] *= 1e-4
        for B in (33, 257):
            for inverse in (True, False):
                first = _first(flows, inverse)
                cols = first.prqct.identity_features.cpu().numpy()
                g = torch.Generator().manual_seed(3 * B + inverse)
                x = 1.3 * torch.randn(B, D, generator=g)
                x[:4] = x[:4].abs().clamp(0.1, 2.5)
                x[B - 1] = x[B - 1].clamp(-2.0, 2.0)
                lin0 = first.prqct.transform_net.initial_layer
                w0, b0 = N(lin0.weight), N(lin0.bias)
                h0 = np.broadcast_to(b0[:4], (B - 1, 4)).copy()      # as the kernel accumulates: bias first, then the products
                for k, c in enumerate(cols):
                    h0 = h0 + x[:B - 1, c].numpy()[:, None] * w0[None, :4, k]
                assert np.all(h0[:, 0] == 0) and not np.signbit(h0[:, 0]).any()
                assert np.all(h0[:4, 1] == 0) and np.signbit(h0[:4, 1]).all()
                assert np.all((h0[:, 2] > 0) & (h0[:, 2] < np.finfo(np.float32).tiny))
                assert np.abs(h0[:, 3]).max() > 1e3
                x[B - 1, cols[0]] = float("nan")
                finite = np.ones(B, bool)
                finite[B - 1] = False
                what = "D=%d hidden=%d K=%d lu=%d reverse=%d B=%d %s" % (D, hidden, bins, lu, reverse0, B,
                                                                        "density" if inverse else "sample")
                zf, lf, zu, lu_ = _compare(nfa, oracle, flows, x, inverse, bins, finite, what)
                print(what, "NaN row: z NaN %d / %d, ld %r; layer-wise z NaN %d, ld %r" % (
                    int(np.isnan(N(zf)[B - 1]).sum()), D, float(N(lf)[B - 1]), int(np.isnan(N(zu)[B - 1]).sum()), float(N(lu_)[B - 1])))
                assert np.isnan(N(zf)[B - 1]).all() and np.isnan(N(zu)[B - 1]).all(), what + ": the NaN row"
                assert bool(np.isnan(N(lf)[B - 1])) == (not (lu and inverse)), what + ": log-det of the NaN row"
                assert_close(N(lf)[B - 1:], N(lu_)[B - 1:], what=what + ": log-det of the NaN row vs layer-wise", **TOL_CHAIN)
