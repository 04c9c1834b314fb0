"""CPU-side tests of the degree-order AR-NSF training path (autograd.MadeFtFn: nf_made_forward_train_ft, nf_made_feed_ft_bwd on the packs
of flows/made_pack.made_train_structure_ft): symbols and argument validation, the unpermuted structures against digests recorded at
the parent revision, the packed schedule walked by the existing emulators (gather + feed and the feed's backward in numpy around them)
against torch float64 autograd through the project's own eager modules, the packer's eligibility and the code objects' resources."""
import copy
import ctypes
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

import ar_ft_train_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def nfa():
    import __graft_entry__
    import normflows_amd
    if not os.path.exists(normflows_amd.native_library_path()):
        __graft_entry__.build()
    return normflows_amd


def test_symbols_are_declared_exported_bound_and_validate_their_arguments(nfa):
    declared = nfa._lib.exported_symbols_declared()
    lib = nfa._lib.lib()
    for sym, op in (("nf_made_forward_train_ft", "made_forward_train_ft"), ("nf_made_feed_ft_bwd", "made_feed_ft_bwd")):
        assert sym in declared and hasattr(lib, sym) and hasattr(nfa.ops, op)
    assert "nf_made_backward_t64" in declared and hasattr(lib, "nf_made_backward_t64")
    assert nfa.config.arnsf_train_ft is True
    nfa.config.set_arnsf_train_ft(False)
    assert nfa.config.arnsf_train_ft is False
    nfa.config.set_arnsf_train_ft(True)
    i32, i64, vp = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    null, one = vp(0), vp(16)

    def fwd(B=8, D=64, hp=512, mult=25, x=one, x_pad=one, x_pos=one, table=one):
        return lib.nf_made_forward_train_ft(x, one, one, one, x_pad, x_pos, one, table, i64(B), i32(D), i32(hp), i32(mult), null)
    assert fwd(D=1) == -22 and fwd(D=129) == -22 and fwd(B=-1) == -22 and fwd(mult=0) == -22
    assert fwd(hp=128) == -95 and fwd(hp=500) == -95
    assert fwd(x=null) == -14 and fwd(x_pad=null) == -14 and fwd(x_pos=null) == -14 and fwd(table=null) == -14
    assert fwd(B=0) == 0 and fwd(B=0, hp=256) == 0

    def feed(B=8, D=64, n=3, g_pre=one, g_xpos=one, tt=one, fd=one, g_x=one, g_w=one, g_b=one, part=one):
        return lib.nf_made_feed_ft_bwd(g_pre, g_xpos, one, tt, fd, g_x, g_w, g_b, part, i64(B), i32(D), i32(n), null)
    assert feed(D=1) == -22 and feed(D=129) == -22 and feed(B=-1) == -22 and feed(n=-1) == -22 and feed(n=65) == -22
    assert feed(g_pre=null) == -14 and feed(tt=null) == -14 and feed(g_x=null) == -14
    assert feed(fd=null) == -14 and feed(g_w=null) == -14 and feed(part=null) == -14
    assert feed(B=0) == 0 and feed(B=0, n=0, fd=null, g_w=null, part=null) == 0

    def t64(B=8, D=64, hp=512, gp=one):
        return lib.nf_made_backward_t64(gp, one, one, one, one, one, i64(B), i32(D), i32(hp), i32(25), null)
    assert t64(D=1) == -22 and t64(hp=100) == -95 and t64(gp=null) == -14 and t64(B=0) == 0


def test_unpermuted_structures_unchanged(nfa):
    """made_train_structure of unpermuted Identity-preprocessing MADEs: every array byte-identical to what the parent revision built
    (tests/golden/make_made_train_pack_parent.py recorded the digests there) -- and the degree-order structure of the same MADEs holds
    the same streams and tables in front of its feature table."""
    from normflows_amd.flows import made_pack
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_made_train_pack_parent as rec
    want = dict(np.load(os.path.join(ROOT, "tests", "golden", "made_train_pack_parent.npz")))
    got = rec.digests(nfa)
    assert sorted(got) == sorted(want) and len(got) == 21
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    for name, D, H, mult in rec.CASES:
        torch.manual_seed(7)
        made = nfa.nets.MADE(features=D, hidden_features=H, num_blocks=2, output_multiplier=mult)
        a, b = made_pack.made_train_structure(made, mult), made_pack.made_train_structure_ft(made, mult)
        assert np.array_equal(b["table"][:b["tt_off"]], a["table"]) and np.array_equal(b["src"][:b["feed_off"]], a["src"])
        for k in ("table", "src", "wtable", "stable", "mask"):
            assert np.array_equal(a["bwd"][k], b["bwd"][k]), (name, k)
        tt = b["table"][b["tt_off"]:].reshape(3, D)
        assert np.array_equal(tt[0], np.arange(D)) and (tt[2] == -1).all() and not b["src"][b["feed_off"]:].any()
        assert hashlib.sha1(str(a["src"].dtype).encode() + a["src"].tobytes()).digest() == want[name + "__src"].tobytes()


def emulate_and_compare(nfa, layer, x, seed):
    """The packed schedule in float64 against torch float64 autograd through the eager modules (MADE with its preprocessing) on CPU."""
    from made_bwd_emulator import emulate_chain, emulate_wgrad, slot_forward
    from made_fwd_emulator import emulate_forward
    from normflows_amd.flows import made_pack
    t = layer.mprqat
    net, mult = t.autoregressive_net, t._output_dim_multiplier()
    st = made_pack.made_train_structure_ft(net, mult)
    assert st is not None
    D, MD, B = t.features, mult * t.features, x.shape[0]
    col, tt = st["col"], st["table"][st["tt_off"]:].reshape(3, D)
    assert np.array_equal(tt[0], col) and np.array_equal(net.final_layer.degrees.numpy()[::mult][col], np.arange(1, D + 1))
    plist = [p for l in net._linears() for p in (l.weight, l.bias)] + made_pack.periodic_params(net)
    flat32 = np.concatenate([np.zeros(1, np.float32)] + [p.detach().numpy().astype(np.float32).ravel() for p in plist])
    # flat[src] reproduces the value packs
    sl = made_pack._slot_layers(net, mult, ft=True)
    assert np.array_equal(flat32[st["src"][:st["feed_off"]]], made_pack._pack_forward_from(sl)[0])
    assert np.array_equal(flat32[st["bwd"]["src"]], made_pack._pack_backward_from(sl)["blob"])
    flat = flat32.astype(np.float64)
    blob = flat[st["src"]]
    feed = blob[st["feed_off"]:st["feed_off"] + 3 * D].reshape(3, D)
    scale, pidx = tt[1].view(np.float32).astype(np.float64), tt[2]
    per = pidx >= 0
    # gather + feed
    x_pos = x[:, col]
    sn, cs = np.sin(scale * x_pos), np.cos(scale * x_pos)
    fed = np.where(per, feed[0] * sn + feed[1] * cs + feed[2], x_pos)
    params_pos = emulate_forward(blob[:st["feed_off"]], st["table"], fed)
    # the reference: the module in float64 (the periodic scale as the float32 the table holds)
    twin = copy.deepcopy(net).double()
    if not isinstance(twin.preprocessing, torch.nn.Identity) and not torch.is_tensor(twin.preprocessing.scale):
        twin.preprocessing.scale = float(np.float32(twin.preprocessing.scale))
    xx = torch.from_numpy(x).clone().requires_grad_(True)
    gen = torch.Generator().manual_seed(seed)
    cp = torch.randn(B, MD, generator=gen, dtype=torch.float64)
    g_xpos = torch.randn(B, D, generator=gen, dtype=torch.float64).numpy()
    out = twin(xx)
    (out * cp).sum().backward()
    ref_pos = out.detach().numpy().reshape(B, D, mult)[:, col].reshape(B, MD)
    np.testing.assert_allclose(params_pos, ref_pos, rtol=1e-9, atol=1e-9)
    # backward: chain + weight gradients on the degree-order tables, the feed's backward around them
    gp_pos = cp.numpy().reshape(B, D, mult)[:, col].reshape(B, MD)
    S, prm2 = slot_forward(sl["layers"], sl["NB"], fed, sl["Dp"])
    np.testing.assert_allclose(prm2[:, :MD], params_pos, rtol=1e-9, atol=1e-9)
    pack = dict(st["bwd"], blob=flat[st["bwd"]["src"]])
    g_pre, G = emulate_chain(pack, gp_pos, S)
    d = np.where(per, scale * (feed[0] * cs - feed[1] * sn), 1.0)
    g_x = np.zeros((B, D))
    g_x[:, col] = g_pre * d + g_xpos
    ref_gx = xx.grad.numpy().copy()
    ref_gx[:, col] += g_xpos
    np.testing.assert_allclose(g_x, ref_gx, rtol=1e-9, atol=1e-9)
    grads = emulate_wgrad(pack, gp_pos, fed, G, S)
    for lin, (woff, shape, boff, n) in zip(twin._linears(), pack["offsets"]):
        gw = grads[woff:woff + shape[0] * shape[1]].reshape(shape)
        assert tuple(lin.weight.shape) == tuple(shape)
        np.testing.assert_allclose(gw, lin.weight.grad.numpy(), rtol=1e-9, atol=1e-9)
        assert (gw[lin.mask.numpy() == 0] == 0.0).all() and (lin.weight.grad.numpy()[lin.mask.numpy() == 0] == 0.0).all()
        np.testing.assert_allclose(grads[boff:boff + n], lin.bias.grad.numpy(), rtol=1e-9, atol=1e-9)
    n_circ = st["n_circ"]
    assert n_circ == int(per.sum())
    if n_circ:
        gw = np.zeros((n_circ, 2))
        gw[pidx[per], 0] = (g_pre * sn).sum(0)[per]
        gw[pidx[per], 1] = (g_pre * cs).sum(0)[per]
        np.testing.assert_allclose(gw, twin.preprocessing.weights.grad.numpy(), rtol=1e-9, atol=1e-9)
        if st["has_bias"]:
            gb = np.zeros(n_circ)
            gb[pidx[per]] = g_pre.sum(0)[per]
            np.testing.assert_allclose(gb, twin.preprocessing.bias.grad.numpy(), rtol=1e-9, atol=1e-9)
    return st


@pytest.mark.parametrize("name", cases.FIXTURES)
def test_emulated_schedule_reproduces_float64_autograd(nfa, name):
    g = cases.load_case(name)
    layer = cases.make_layer(nfa, name, g)
    st = emulate_and_compare(nfa, layer, g["x"].astype(np.float64), 5)
    assert not np.array_equal(st["col"], np.arange(len(st["col"])))
    assert st["hp"] == (512 if name == "grad_circ_ar_perm_d40_h260" else 256)
    assert st["n_circ"] == {"grad_circ_ar_perm_d21_h40": 5, "grad_circ_ar_perm_d40_h260": 4, "grad_ar_perm_lin_d12_h24": 0}[name]
    assert not st["has_bias"]


def test_emulated_schedule_with_a_periodic_bias(nfa):
    """The first fixture's layer with its preprocessing replaced by one that has a (non-zero) bias parameter."""
    name = cases.FIXTURES[0]
    g = cases.load_case(name)
    layer = cases.make_layer(nfa, name, g)
    net = layer.mprqat.autoregressive_net
    old = net.preprocessing
    pre = nfa.nets.PeriodicFeaturesElementwise(21, old.ind, old.scale, bias=True)
    with torch.no_grad():
        pre.weights.copy_(old.weights)
        pre.bias.copy_(torch.tensor([0.3, -0.2, 0.5, 0.1, -0.4]))
    net.preprocessing = pre
    st = emulate_and_compare(nfa, layer, g["x"].astype(np.float64), 6)
    assert st["has_bias"] and st["n_circ"] == 5


def test_packer_eligibility(nfa):
    """What falls back returns None from the packer; every shape of tests/test_gpu_made_fwd_ft.py::build_case is accepted."""
    from torch.nn import functional as F
    from normflows_amd import nets
    from normflows_amd.flows import made_pack
    C, A = nfa.flows.CircularAutoregressiveRationalQuadraticSpline, nfa.flows.AutoregressiveRationalQuadraticSpline
    M = nfa.flows.autoregressive.MaskedPiecewiseRationalQuadraticAutoregressive
    ft = made_pack.made_train_structure_ft
    pre = nets.PeriodicFeaturesElementwise(5, [1], 1.0, activation=torch.nn.Tanh())
    assert ft(nets.MADE(features=5, hidden_features=12, num_blocks=2, output_multiplier=13, preprocessing=pre), 13) is None
    assert ft(nets.MADE(features=5, hidden_features=12, context_features=3, num_blocks=2, output_multiplier=13), 13) is None
    assert ft(nets.MADE(features=5, hidden_features=12, num_blocks=2, output_multiplier=13, use_batch_norm=True), 13) is None
    assert ft(nets.MADE(features=5, hidden_features=12, num_blocks=2, output_multiplier=13, dropout_probability=0.1).train(), 13) is None
    assert ft(nets.MADE(features=5, hidden_features=12, num_blocks=2, output_multiplier=13, activation=F.elu), 13) is None
    assert ft(nets.MADE(features=5, hidden_features=12, num_blocks=2, output_multiplier=13, use_residual_blocks=False,
                        random_mask=True), 13) is None
    assert ft(nets.MADE(features=5, hidden_features=12, num_blocks=2, output_multiplier=13).double(), 13) is None
    assert ft(nets.MADE(features=129, hidden_features=140, num_blocks=2, output_multiplier=13), 13) is None
    assert ft(nets.MADE(features=5, hidden_features=513, num_blocks=2, output_multiplier=13), 13) is None
    assert ft(nets.MADE(features=5, hidden_features=12, num_blocks=2, output_multiplier=13), 12) is None            # not the net's multiplier
    for bias in (False, True):
        pre = nets.PeriodicFeaturesElementwise(5, [1, 4], 1.0, bias=bias)
        st = ft(nets.MADE(features=5, hidden_features=12, num_blocks=2, output_multiplier=13, permute_mask=True, preprocessing=pre), 13)
        assert st is not None and st["n_circ"] == 2 and st["has_bias"] is bias
    # a permuted or periodic MADE never enters the column-order structure (MADE.forward -> MadeFn stays what it was)
    torch.manual_seed(3)
    t = C(9, 2, 20, ind_circ=[1], num_bins=4, tail_bound=2.0).mprqat
    assert made_pack.made_train_structure(t.autoregressive_net, 13) is None and ft(t.autoregressive_net, 13) is not None
    torch.manual_seed(5)
    for t in (C(2, 2, 4, ind_circ=[1], num_bins=4, tail_bound=2.0).mprqat,
              C(33, 1, 24, ind_circ=[0, 7, 32], num_bins=6, tail_bound=1.5 + 2.0 * torch.rand(33)).mprqat,
              C(128, 2, 300, ind_circ=list(range(0, 128, 5)), num_bins=10, tail_bound=3.0).mprqat,
              C(5, 2, 12, ind_circ=[0, 1, 2, 3, 4], num_bins=10, tail_bound=float(np.pi)).mprqat,
              C(9, 2, 40, ind_circ=[], num_bins=4, tail_bound=2.5, permute_mask=False).mprqat,
              A(33, 2, 96, num_bins=8, tail_bound=2.5, permute_mask=True).mprqat,
              A(7, 2, 24, num_bins=11, tail_bound=2.5, permute_mask=True).mprqat,
              M(6, 16, num_bins=5, tails="linear", tail_bound=1.0 + torch.rand(6)),
              M(6, 16, num_bins=5, tails="circular", tail_bound=1.0 + torch.rand(6))):
        st = ft(t.autoregressive_net, t._output_dim_multiplier())
        assert st is not None
        assert st["bwd"]["src"].size % 4 == 0 and st["src"].size % 4 == 0          # (16-byte streams behind the feed block)


def test_new_kernels_use_no_scratch(nfa):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    objdir = os.path.join(ROOT, "normalizing-flows_amd", "lib", "obj")
    seen = 0
    for name, d in kr.resources(os.path.join(objdir, "made_fwd_train_ft.o")).items():          # 256 / 512 slots, 64-row tiles
        assert "made_fwd_train_ft_kernel" in name
        seen += 1
        assert d["vgpr_spill_count"] == 0 and d["private_segment_fixed_size"] == 0, (name, d)
    for name, d in kr.resources(os.path.join(objdir, "made_feed_ft.o")).items():
        assert "made_feed_ft" in name
        seen += 1
        assert d["vgpr_spill_count"] == 0 and d["private_segment_fixed_size"] == 0, (name, d)
    assert seen == 4, seen
