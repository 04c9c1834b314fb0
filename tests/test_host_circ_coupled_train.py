"""CPU-side tests of the circular NSF coupling layer's training path (autograd.ResNetFtFn on the dense, periodically fed pack of
flows/made_pack.resnet_train_structure_ft; nf_rqs_coupling_bwd_ft_wave): the packed schedule walked by the existing emulators (feed and
the feed's backward in numpy around them) against torch float64 autograd through the project's own eager modules, the packer's
eligibility, the new symbol's export and argument validation, and the new kernel's code-object resources."""
import copy
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import circ_coupled_train_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def nfa():
    import __graft_entry__
    import normflows_amd
    if not os.path.exists(normflows_amd.native_library_path()):
        __graft_entry__.build()
    return normflows_amd


def emulate_and_compare(nfa, net, x, seed):
    """The packed schedule in float64 against torch float64 autograd through the eager ResidualNet (with its preprocessing) on CPU:
    the output, the input gradient and every parameter gradient, the periodic ones included."""
    from made_bwd_emulator import emulate_chain, emulate_wgrad, slot_forward
    from made_fwd_emulator import emulate_forward
    from normflows_amd.flows import made_pack
    st = made_pack.resnet_train_structure_ft(net)
    assert st is not None
    B, D = x.shape
    MD = net.final_layer.out_features
    tt = st["table"][st["tt_off"]:].reshape(3, D)
    assert np.array_equal(tt[0], np.arange(D))              # the identity column map: position f is input column f
    lins = [net.initial_layer] + [l for b in net.blocks for l in b.linear_layers] + [net.final_layer]
    plist = [p for l in lins for p in (l.weight, l.bias)] + made_pack.periodic_params(net)
    flat32 = np.concatenate([np.zeros(1, np.float32)] + [p.detach().numpy().astype(np.float32).ravel() for p in plist])
    # flat[src] reproduces the value packs
    sl = made_pack._dense_layers(net, preprocessing=True)
    assert np.array_equal(flat32[st["src"][:st["feed_off"]]], made_pack._pack_forward_from(sl)[0])
    assert np.array_equal(flat32[st["bwd"]["src"]], made_pack._pack_backward_from(sl)["blob"])
    assert st["bwd"]["src"].size % 4 == 0 and st["src"].size % 4 == 0          # (16-byte streams behind the feed block)
    flat = flat32.astype(np.float64)
    blob = flat[st["src"]]
    feed = blob[st["feed_off"]:st["feed_off"] + 3 * D].reshape(3, D)
    scale, pidx = tt[1].view(np.float32).astype(np.float64), tt[2]
    per = pidx >= 0
    sn, cs = np.sin(scale * x), np.cos(scale * x)
    fed = np.where(per, feed[0] * sn + feed[1] * cs + feed[2], x)
    out_emu = emulate_forward(blob[:st["feed_off"]], st["table"], fed)
    # the reference: the module in float64 (the periodic scale as the float32 the table holds)
    twin = copy.deepcopy(net).double()
    pre = twin.preprocessing
    if torch.is_tensor(pre.scale):
        pre.scale = pre.scale.float().double()
    else:
        pre.scale = float(np.float32(pre.scale))
    xx = torch.from_numpy(x).clone().requires_grad_(True)
    gen = torch.Generator().manual_seed(seed)
    cp = torch.randn(B, MD, generator=gen, dtype=torch.float64)
    out = twin(xx)
    (out * cp).sum().backward()
    np.testing.assert_allclose(out_emu[:, :MD], out.detach().numpy(), rtol=1e-9, atol=1e-9)
    # backward: chain + weight gradients on the dense tables, the feed's backward around them
    S, prm2 = slot_forward(sl["layers"], sl["NB"], fed, sl["Dp"])
    np.testing.assert_allclose(prm2[:, :MD], out.detach().numpy(), rtol=1e-9, atol=1e-9)
    pack = dict(st["bwd"], blob=flat[st["bwd"]["src"]])
    g_pre, G = emulate_chain(pack, cp.numpy(), S)
    d = np.where(per, scale * (feed[0] * cs - feed[1] * sn), 1.0)
    np.testing.assert_allclose(g_pre * d, xx.grad.numpy(), rtol=1e-9, atol=1e-9)
    grads = emulate_wgrad(pack, cp.numpy(), fed, G, S)
    twin_lins = [twin.initial_layer] + [l for b in twin.blocks for l in b.linear_layers] + [twin.final_layer]
    for lin, (woff, shape, boff, n) in zip(twin_lins, pack["offsets"]):
        assert tuple(lin.weight.shape) == tuple(shape)
        np.testing.assert_allclose(grads[woff:woff + shape[0] * shape[1]].reshape(shape), lin.weight.grad.numpy(), rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(grads[boff:boff + n], lin.bias.grad.numpy(), rtol=1e-9, atol=1e-9)
    n_circ = st["n_circ"]
    assert n_circ == int(per.sum()) and n_circ > 0
    gw = np.zeros((n_circ, 2))
    gw[pidx[per], 0] = (g_pre * sn).sum(0)[per]
    gw[pidx[per], 1] = (g_pre * cs).sum(0)[per]
    np.testing.assert_allclose(gw, pre.weights.grad.numpy(), rtol=1e-9, atol=1e-9)
    if st["has_bias"]:
        gb = np.zeros(n_circ)
        gb[pidx[per]] = g_pre.sum(0)[per]
        np.testing.assert_allclose(gb, pre.bias.grad.numpy(), rtol=1e-9, atol=1e-9)
    return st


def d7_net(nfa):
    g = cases.load_case("grad_circ_cpl_d7_h40")
    layer = cases.make_layer(nfa, "grad_circ_cpl_d7_h40", g)
    ident = g["x"][:, layer.prqct.identity_features.numpy()].astype(np.float64)
    return layer.prqct.transform_net, ident


def test_emulated_schedule_reproduces_float64_autograd(nfa):
    """The D 7 fixture's conditioner (4 inputs of which 3 periodic, 40 hidden units in 256 slots, 75 outputs) on its state and rows."""
    net, ident = d7_net(nfa)
    st = emulate_and_compare(nfa, net, ident, 5)
    assert st["hp"] == 256 and st["n_circ"] == 3 and not st["has_bias"]
    assert st["bwd"]["MD"] == 75 and st["bwd"]["NB"] == 2


def test_emulated_schedule_with_a_periodic_bias(nfa):
    net, ident = d7_net(nfa)
    old = net.preprocessing
    pre = nfa.nets.PeriodicFeaturesElementwise(4, old.ind, old.scale, bias=True)
    with torch.no_grad():
        pre.weights.copy_(old.weights)
        pre.bias.copy_(torch.tensor([0.3, -0.2, 0.5]))
    net.preprocessing = pre
    st = emulate_and_compare(nfa, net, ident, 6)
    assert st["has_bias"] and st["n_circ"] == 3


def test_packer_eligibility(nfa):
    """What the route must leave to the eager modules returns None from the packer (and False from resnet_supported_ft); the three
    fixtures' conditioners are accepted, and a net without a preprocessing never enters this structure."""
    from normflows_amd import nets
    from normflows_amd.flows import made_pack
    ft, ok = made_pack.resnet_train_structure_ft, made_pack.resnet_supported_ft
    P = nets.PeriodicFeaturesElementwise

    def net(D=4, H=40, pre="default", **kw):
        pre = P(D, [0, 2], 1.0) if isinstance(pre, str) else pre
        return nets.ResidualNet(D, 75, H, preprocessing=pre, **kw)
    assert ok(net()) and ft(net()) is not None
    declined = {
        "context": net(context_features=3),
        "tanh": net(pre=P(4, [0, 2], 1.0, activation=torch.nn.Tanh())),
        "batch norm": net(use_batch_norm=True),
        "dropout in train mode": net(dropout_probability=0.1).train(),
        "in_features 1": nets.ResidualNet(1, 25, 40, preprocessing=P(1, [0], 1.0)),
        "hidden 513": net(H=513),
        "float64": net().double(),
        "no preprocessing": net(pre=None),
        "elu": net(activation=torch.nn.functional.elu),
        "preprocessing of another width": net(pre=P(5, [0, 2], 1.0)),
    }
    for what, n in declined.items():
        assert not ok(n) and ft(n) is None, what
    assert ok(net(dropout_probability=0.1).eval())              # dropout is the identity in eval mode
    assert ok(net(D=128, H=512)) and not ok(net(D=129))
    for name in cases.FIXTURES:
        layer = cases.make_layer(nfa, name, cases.load_case(name))
        st = ft(layer.prqct.transform_net)
        assert st is not None and st["hp"] == (512 if name == "grad_circ_cpl_d21_h260" else 256), name
    # the plain structure still refuses a net with a preprocessing (ResidualNet.forward -> MadeFn stays what it was)
    assert made_pack.resnet_train_structure(net(H=200)) is None and made_pack.resnet_train_structure(net(H=200, pre=None)) is not None


def test_switch_and_symbol(nfa):
    """config.nsf_circular_train defaults to on; the new symbol is declared, exported and bound, and rejects NULL and misaligned
    arguments with nf_rqs_coupling_bwd_ft's codes before any launch (the addresses are fake)."""
    assert nfa.config.nsf_circular_train is True
    nfa.config.set_nsf_circular_train(False)
    assert nfa.config.nsf_circular_train is False
    nfa.config.set_nsf_circular_train(True)
    lib = nfa._lib.lib()
    sym = "nf_rqs_coupling_bwd_ft_wave"
    assert sym in nfa._lib.exported_symbols_declared() and hasattr(lib, sym) and hasattr(nfa.ops, "rqs_coupling_bwd_ft_wave")
    assert hasattr(nfa.autograd, "ResNetFtFn") and issubclass(nfa.autograd.ResNetFtFn, nfa.autograd.MadeFtFn)
    vp = ctypes.c_void_p
    null, ok = vp(0), vp(4096)
    names = ["x", "grad_y", "grad_logdet", "cond", "uw", "uh", "ud", "identity_idx", "transform_idx", "grad_x", "grad_cond", "grad_uw",
             "grad_uh", "grad_ud", "tails_t", "bound_t", "tails_i", "bound_i"]

    def call(fn, B=8, nI=4, nT=3, K=8, tails=3, mode=0, dtype=0, **ptrs):
        a = {k: ok for k in names}
        a.update(ptrs)
        return getattr(lib, fn)(a["x"], a["grad_y"], a["grad_logdet"], a["cond"], a["uw"], a["uh"], a["ud"], a["identity_idx"], nI,
                                a["transform_idx"], nT, B, nI + nT, K, tails, 3.0, 1e-3, 1e-3, 1e-3, 1.0, mode, a["grad_x"],
                                a["grad_cond"], a["grad_uw"], a["grad_uh"], a["grad_ud"], dtype, a["tails_t"], a["bound_t"],
                                a["tails_i"], a["bound_i"], None)
    # NULL arguments: the sibling's code for each of them
    for k in ("x", "grad_y", "grad_logdet", "grad_x", "cond", "grad_cond", "transform_idx", "identity_idx", "uh", "ud", "grad_uw", "grad_uh",
              "grad_ud", "tails_t", "tails_i"):
        assert call(sym, **{k: null}) == -14 == call("nf_rqs_coupling_bwd_ft", **{k: null}), k
    # scalar arguments: the sibling's codes
    for kw in (dict(K=0), dict(K=65), dict(tails=4), dict(tails=-1), dict(B=-1), dict(mode=3), dict(nI=-1)):
        assert call(sym, **kw) == call("nf_rqs_coupling_bwd_ft", **kw) < 0, kw
    assert call(sym, B=0) == 0 and call(sym, B=0, nI=0, nT=7) == 0 and call(sym, B=0, nI=7, nT=0) == 0
    # what the kernel does not take goes back to the sibling
    assert call(sym, K=5) == -95 and call(sym, dtype=1) == -95
    assert call(sym, tails=1, tails_t=null, tails_i=null) == -95
    # the LDS fit the op asks for before it allocates anything: the entry point's own computation
    fits = lib.nf_rqs_coupling_bwd_ft_wave_fits
    assert fits(4, 3) == 1 and fits(0, 7) == 1 and fits(32, 32) == 1 and fits(66, 4) == 1 and fits(3, 70) == 1
    assert fits(128, 128) == 0 and fits(-1, 3) == -22 and fits(0, 0) == -22
    assert nfa.ops._ft_wave_fits(4, 3) is True and nfa.ops._ft_wave_fits(128, 128) is False and nfa._lib.ENOTSUP == -95
    # a pointer off its element type's boundary
    for k in names:
        off = 4096 + (4 if k in ("identity_idx", "transform_idx") else 2)
        assert call(sym, **{k: vp(off)}) == -22, k


def test_new_kernel_uses_no_scratch(nfa):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    objdir = os.path.join(ROOT, "normalizing-flows_amd", "lib", "obj")
    seen = 0
    for name, d in kr.resources(os.path.join(objdir, "rqs_bwd_ft.o")).items():
        assert "rqs_coupling_bwd_ft_wave_kernel" in name
        seen += 1
        assert d["vgpr_spill_count"] == 0 and d["private_segment_fixed_size"] == 0, (name, d)
    assert seen == 1, seen
