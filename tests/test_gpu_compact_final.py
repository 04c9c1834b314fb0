"""GPU tests of the compact final layer of the 8-bin fused inference kernels (csrc/rqs_fused.hip: 21 row-blocks, logit 0 of both
softmaxes subtracted at pack time): the fused path against the layer-wise path (fused route off) and the CPU oracle in float32 and
float64, with the tolerances tests/test_gpu_parity.py applies to the same comparisons -- single layers and 3-pair chains, every
early-exit point of the statically unrolled final layer (D = 5 / 16: 2 pairs, 33 / 48: 6, 64: 8), every hidden-width build, both mask
parities, with and without the fused LU, both directions, one-row / ragged / two-workgroup batches, both workgroup sizes bit for bit."""
import numpy as np
import pytest
import torch

from conftest import assert_close

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BATCHES = (1, 31, 257)        # 257 rows: ragged, two workgroups on both builds (128- and 256-row workgroups)


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


def _flows(nfa, D, hidden, lu, n, reverse0, seed, sigma=0.04):
    torch.manual_seed(seed)
    flows = []
    for i in range(n):
        flows.append(nfa.flows.CoupledRationalQuadraticSpline(D, 2, hidden, num_bins=8, init_identity=False,
                                                              reverse_mask=bool(i & 1) != reverse0))
        if lu:
            flows.append(nfa.flows.LULinearPermute(D))
    for f in flows:
        for p_ in f.parameters():
            p_.add_(sigma * torch.randn_like(p_))
    for f in flows[::2 if lu else 1]:
        u = f.prqct.unconditional_transform
        u.unnormalized_widths.normal_()
        u.unnormalized_heights.normal_()
        u.unnormalized_derivatives.normal_()
    return flows


def _state(flows, f64=False):
    st = {}
    for i, f in enumerate(flows):
        st.update({"flows.%d.%s" % (i, k): v.detach().cpu().numpy() for k, v in f.state_dict().items()})
    if f64:
        st = {k: v.astype(np.float64) if v.dtype == np.float32 else v for k, v in st.items()}
    return st


def _oracle(oracle, flows, x, inverse, f64):
    ora = oracle.OracleNSF(_state(flows, f64), num_layers=len(flows))
    z = x.astype(np.float64) if f64 else x
    logq = np.zeros(len(x), z.dtype)
    for i in (range(len(flows) - 1, -1, -1) if inverse else range(len(flows))):
        z = (ora.coupling if ora._is_coupling(i) else ora.lu)(i, z, 0 if inverse else 1, logq, +1)
    return z, logq


def _layerwise(flows, xd, inverse):
    """Every layer on its own launch(es), the fused route off: library GEMMs + the stand-alone spline / LU kernels."""
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


def _fused(nfa, flows, xd, inverse):
    """The fused route (core.run_chain: [coupling, LU] pairs of one shape as ONE persistent launch) on both workgroup sizes."""
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
    assert torch.equal(z1, z0) and torch.equal(l1, l0), "128-row and 256-row workgroups differ"
    return z1, l1


def _check(nfa, oracle, flows, B, inverse, tol_z, tol_ld, what):
    g = torch.Generator().manual_seed(1000 * B + inverse)
    x = 1.3 * torch.randn(B, flows[0].prqct.features, generator=g)
    x.view(-1)[:2] = torch.tensor([3.0, -3.5])          # on the boundary of the splines' interval, in the tail
    xd = x.to(DEV)
    assert all(f.prqct._fused_eligible(xd, None) for f in flows if hasattr(f, "prqct"))
    zf, lf = _fused(nfa, flows, xd, inverse)
    zu, lu_ = _layerwise(flows, xd, inverse)
    assert torch.isfinite(zf).all() and torch.isfinite(lf).all(), what
    assert_close(N(zf), N(zu), what=what + ": fused vs layer-wise z", **tol_z)
    assert_close(N(lf), N(lu_), what=what + ": fused vs layer-wise ld", **tol_ld)
    for f64 in (False, True):
        zo, lo = _oracle(oracle, flows, x.numpy(), inverse, f64)
        tag = what + ": fused vs oracle (%s)" % ("float64" if f64 else "float32")
        assert_close(N(zf).astype(zo.dtype), zo, what=tag + " z", **tol_z)
        assert_close(N(lf).astype(lo.dtype), lo, what=tag + " ld", **tol_ld)


# tests/test_gpu_parity.py: test_fused_layer_vs_unfused_and_oracle (one layer) / test_fused_pair_with_lu_vs_layerwise_and_oracle
TOL_LAYER = (dict(rtol=2e-3, atol=2e-3), dict(rtol=2e-4, atol=2e-3))
TOL_PAIR = (dict(rtol=1e-3, atol=1e-3), dict(rtol=1e-3, atol=2e-3))


@pytest.mark.parametrize("lu", [False, True])
@pytest.mark.parametrize("hidden", [32, 64, 128])
@pytest.mark.parametrize("D", [5, 16, 33, 48, 64])
def test_compact_final_layer_vs_layerwise_and_oracle(nfa, oracle, D, hidden, lu):
    for n in (1, 3):                                   # a single layer (pair); a chain of three
        for reverse0 in (False, True):                 # both mask parities (a chain alternates, starting from either)
            flows = [f.to(DEV) for f in _flows(nfa, D, hidden, lu, n, reverse0, seed=D + hidden + n)]
            tol = TOL_PAIR if (lu or n > 1) else TOL_LAYER
            for B in BATCHES:
                for inverse in (True, False):
                    _check(nfa, oracle, flows, B, inverse, tol[0], tol[1],
                           "D=%d hidden=%d lu=%d layers=%d reverse=%d B=%d %s" % (D, hidden, lu, n, reverse0, B,
                                                                                "density" if inverse else "sample"))


@pytest.mark.parametrize("lu", [False, True])
def test_compact_final_layer_with_logits_spread_over_60_nats(nfa, oracle, lu):
    """Final-layer width / height rows scaled until the softmax logits reach +-60 nats on the test's rows: the subtracted logit 0 is
    then the largest of some features and the smallest of others; maximum, subtraction and exp2 in the epilogue keep every term
    finite and the result with the layer-wise path's and the oracle's."""
    D, hidden, K, M = 64, 128, 8, 23
    flows = _flows(nfa, D, hidden, lu, 1, False, seed=60)
    p = flows[0].prqct
    g = torch.Generator().manual_seed(61)
    x = 1.3 * torch.randn(257, D, generator=g)
    net = p.transform_net
    logits = net(x.index_select(1, p.identity_features)).view(257, D // 2, M)[..., :2 * K] / np.sqrt(hidden)
    s = 60.0 / float(logits.abs().max())
    net.final_layer.weight.view(D // 2, M, hidden)[:, :2 * K] *= s
    net.final_layer.bias.view(D // 2, M)[:, :2 * K] *= s
    logits = net(x.index_select(1, p.identity_features)).view(257, D // 2, M)[..., :2 * K] / np.sqrt(hidden)
    assert 59.0 < float(logits.abs().max()) < 61.0
    first = torch.cat([logits[..., :1] - logits[..., 1:K], logits[..., K:K + 1] - logits[..., K + 1:]], -1)
    assert float(first.max()) > 40.0 and float(first.min()) < -40.0      # logit 0 far above / far below the others somewhere
    flows = [f.to(DEV) for f in flows]
    tol = TOL_PAIR if lu else TOL_LAYER
    for inverse in (True, False):
        xd = x.to(DEV)
        zf, lf = _fused(nfa, flows, xd, inverse)
        zu, lu_ = _layerwise(flows, xd, inverse)
        assert torch.isfinite(zf).all() and torch.isfinite(lf).all()
        assert_close(N(zf), N(zu), what="fused vs layer-wise z", **tol[0])
        assert_close(N(lf), N(lu_), what="fused vs layer-wise ld", **tol[1])
        for f64 in (False, True):
            zo, lo = _oracle(oracle, flows, x.numpy(), inverse, f64)
            assert_close(N(zf).astype(zo.dtype), zo, what="fused vs oracle z (f64=%d)" % f64, **tol[0])
            assert_close(N(lf).astype(lo.dtype), lo, what="fused vs oracle ld (f64=%d)" % f64, **tol[1])
