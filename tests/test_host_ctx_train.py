"""CPU tests of the gated ResidualNet conditioner under autograd (csrc/resnet_ctx_train.hip, flows/ctx_train_pack.py): the padded
blob, table and weight-gradient jobs walked as the kernels walk them reproduce autograd through the float64 network, the packer
declines what the kernels do not cover, the C ABI rejects bad arguments without a GPU, and no kernel uses scratch memory."""
import copy
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT


@pytest.fixture(scope="module")
def nfa():
    import __graft_entry__
    import normflows_amd
    if not os.path.exists(normflows_amd.native_library_path()):
        __graft_entry__.build()
    return normflows_amd


def _net(nfa, nI, C, H, NB, O, seed=0, **kw):
    torch.manual_seed(seed)
    net = nfa.nets.ResidualNet(nI, O, H, context_features=C, num_blocks=NB, **kw)
    with torch.no_grad():
        for p in net.parameters():
            p.add_(0.1 * torch.randn_like(p))
    return net


# boundary widths: nI, C and hidden at and around multiples of 32, PI + PC = 128, NB 1..4, out_features not a multiple of 32
@pytest.mark.parametrize("nI,C,H,NB,O", [(3, 3, 40, 2, 69), (32, 16, 136, 1, 32 * 11), (9, 33, 200, 1, 8 * 47), (1, 1, 1, 1, 1),
                                         (64, 64, 256, 2, 33), (32, 96, 32, 3, 64), (96, 32, 97, 4, 65), (17, 4, 128, 2, 23)])
def test_emulator_matches_float64_autograd(nfa, nI, C, H, NB, O):
    from normflows_amd.flows import ctx_train_pack
    from ctx_train_emulator import emulate
    net = _net(nfa, nI, C, H, NB, O, seed=nI + C + H)
    assert ctx_train_pack.supported(net) is None
    st = ctx_train_pack.structure_for(net)
    params = ctx_train_pack.params_of(net)
    blob = ctx_train_pack.gather_host([p.detach().numpy() for p in params], st)
    g = torch.Generator().manual_seed(5)
    B = 70
    x, c, go = torch.randn(B, nI, generator=g), torch.randn(B, C, generator=g), torch.randn(B, O, generator=g)
    out, gx, gc, flat = emulate(blob, st["table"], st["jobs"], x.numpy(), c.numpy(), go.numpy())
    net64 = copy.deepcopy(net).double()
    x64, c64 = x.double().requires_grad_(True), c.double().requires_grad_(True)
    ref = net64(x64, c64)
    ref.backward(go.double())
    np.testing.assert_allclose(out, ref.detach().numpy(), rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(gx, x64.grad.numpy(), rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(gc, c64.grad.numpy(), rtol=1e-10, atol=1e-10)
    assert flat.size == st["nflat"] and not np.isnan(flat).any()      # every gradient element is written by exactly the jobs
    for k, p in enumerate(ctx_train_pack.params_of(net64)):
        n = p.numel()
        np.testing.assert_allclose(flat[st["poff"][k]:st["poff"][k] + n].reshape(p.shape), p.grad.numpy(), rtol=1e-10, atol=1e-10,
                                   err_msg="parameter %d" % k)


def test_packer_declines_outside_coverage(nfa):
    from normflows_amd.flows import ctx_train_pack
    assert ctx_train_pack.supported(_net(nfa, 4, 3, 32, 2, 10)) is None
    assert "batch norm" in ctx_train_pack.supported(_net(nfa, 4, 3, 32, 2, 10, use_batch_norm=True))
    drop = _net(nfa, 4, 3, 32, 2, 10, dropout_probability=0.1)
    assert "dropout" in ctx_train_pack.supported(drop.train())
    assert ctx_train_pack.supported(drop.eval()) is None               # eval: dropout is the identity
    assert ctx_train_pack.supported(_net(nfa, 4, 3, 32, 2, 10, dropout_probability=0.0).train()) is None
    assert "ReLU" in ctx_train_pack.supported(_net(nfa, 4, 3, 32, 2, 10, activation=torch.tanh))
    assert "preprocessing" in ctx_train_pack.supported(_net(nfa, 4, 3, 32, 2, 10, preprocessing=torch.nn.Identity()))
    assert "float32" in ctx_train_pack.supported(_net(nfa, 4, 3, 32, 2, 10).double())
    assert "128" in ctx_train_pack.supported(_net(nfa, 65, 64, 32, 2, 10))     # 96 + 64 positions
    assert "128" in ctx_train_pack.supported(_net(nfa, 33, 65, 32, 2, 10))
    assert "num_blocks" in ctx_train_pack.supported(_net(nfa, 4, 3, 32, 5, 10))
    assert "hidden" in ctx_train_pack.supported(_net(nfa, 4, 3, 257, 2, 10))
    assert ctx_train_pack.supported(nfa.nets.ResidualNet(4, 10, 32)) is not None    # no context


def test_route_declines_on_host_and_when_switched_off(nfa, monkeypatch):
    """Outside coverage or with the switch off ResidualNet.forward runs the eager modules (on the CPU: no device, no pack)."""
    net = _net(nfa, 4, 3, 32, 2, 10)
    x, c = torch.randn(5, 4, requires_grad=True), torch.randn(5, 3)
    assert net._ctx_train_pack(x, c) is None
    out = net(x, c)
    out.sum().backward()
    assert x.grad is not None
    from normflows_amd import config
    assert config.nsf_context_train is True
    config.set_nsf_context_train(False)
    try:
        assert config.nsf_context_train is False
    finally:
        config.set_nsf_context_train(True)


def test_capi_argument_checks(nfa):
    """Bad shapes give the documented codes before any pointer is touched (nothing is launched: NULL pointers everywhere)."""
    lib = nfa._lib.lib()
    i64, i32, nul = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p(0)

    def fwd(B=10, nI=4, C=3, H=32, O=10, NB=2, ldx=None, ldc=3):
        return lib.nf_resnet_ctx_forward_train(nul, i64(nI if ldx is None else ldx), nul, i64(ldc), nul, nul, nul, nul, i64(B), i32(nI), i32(C), i32(H),
                                               i32(O), i32(NB), nul)

    def bwd(B=10, nI=4, C=3, H=32, O=10, NB=2):
        return lib.nf_resnet_ctx_backward(nul, nul, nul, nul, nul, nul, nul, i64(B), i32(nI), i32(C), i32(H), i32(O), i32(NB), nul)

    def wg(B=10, njobs=4, H=32, NB=2):
        return lib.nf_resnet_ctx_wgrad(nul, nul, nul, nul, nul, nul, i32(njobs), nul, i64(B), i32(H), i32(NB), nul)

    for f in (fwd, bwd):
        assert f() == -14                       # valid shape, NULL pointers
        assert f(B=0) == 0                      # empty batch: OK without touching a pointer
        assert f(B=-1) == -22
        assert f(NB=0) == -22
        assert f(NB=5) == -95
        assert f(H=0) == -22
        assert f(H=257) == -95
        assert f(nI=0) == -22 and f(C=0) == -22 and f(O=0) == -22
        assert f(nI=65, C=64) == -95            # 96 + 64 positions > 128
        assert f(nI=97, C=1) == -95            # 128 + 32 positions
    assert fwd(ldc=0) == -14                    # a stride-0 context is valid
    assert fwd(ldc=-1) == -22 and fwd(ldx=3) == -22
    assert wg() == -14 and wg(B=0) == 0
    assert wg(B=-1) == -22 and wg(njobs=0) == -22 and wg(NB=5) == -95 and wg(H=300) == -95
    lib.nf_resnet_ctx_save_floats.restype = ctypes.c_int64
    assert lib.nf_resnet_ctx_save_floats(i64(65), i32(4), i32(3), i32(40), i32(2)) == 9 * 128 * 64 + 128 * 64
    assert lib.nf_resnet_ctx_save_floats(i64(65), i32(4), i32(3), i32(40), i32(5)) == -22
    assert lib.nf_resnet_ctx_wgrad_chunks(i64(1), i32(10)) == 1 and lib.nf_resnet_ctx_wgrad_chunks(i64(65536), i32(10)) == 64
    assert lib.nf_resnet_ctx_wgrad_chunks(i64(65536), i32(0)) == -22
    # a wide final layer: the partial tiles stay within 2^25 floats (one chunk at least)
    lib.nf_resnet_ctx_scratch_floats.restype = ctypes.c_int64
    from normflows_amd.flows import ctx_train_pack
    njobs = int(ctx_train_pack.structure(32, 16, 256, 65536, 2)["jobs"].shape[0])
    nch = lib.nf_resnet_ctx_wgrad_chunks(i64(16384), i32(njobs))
    assert nch == max(1, (1 << 25) // (njobs * 4160))
    assert lib.nf_resnet_ctx_scratch_floats(i64(16384), i32(njobs)) == nch * njobs * 4160 <= max(1 << 25, njobs * 4160)
    assert lib.nf_resnet_ctx_scratch_floats(i64(16384), i32(100)) == 16 * 100 * 4160


def test_resnet_ctx_kernels_use_no_scratch(nfa):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    obj = os.path.join(ROOT, "normalizing-flows_amd", "lib", "obj", "resnet_ctx_train.o")
    seen = 0
    for name, d in kr.resources(obj).items():
        if "rc_" in name:
            seen += 1
            assert d["vgpr_spill_count"] == 0 and d["private_segment_fixed_size"] == 0, (name, d)
    assert seen == 4, seen


def test_ops_need_a_device(nfa):
    from normflows_amd.flows import ctx_train_pack
    st = ctx_train_pack.structure(4, 3, 32, 10, 2)
    with pytest.raises(RuntimeError, match="MI355X"):
        nfa.ops.resnet_ctx_forward_train(torch.zeros(4, 4), torch.zeros(4, 3), torch.zeros(8), torch.zeros(52, dtype=torch.int32), st)
