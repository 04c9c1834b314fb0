"""CPU-side tests of the wide RealNVP coupling layers' training route (autograd.AffineWideFn: flows/affine_wide_pack.train_structure,
csrc/affine_wide_train.hip): the training structure of every fixture walked by the existing MADE emulators with a numpy restatement
of the two new kernels around them, against torch float64 autograd of the same layer and the REFERENCE's stored autograd
(tests/golden/grad_affine_wide_*.npz, make_golden_affine_wide_train.py); the gradient entries that must be exactly 0; the eligibility
table; the switch; the two symbols' export, binding and argument validation; the code objects' resources."""
import copy
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import affine_wide_cases as cases
import affine_wide_train_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def nfa():
    import __graft_entry__
    import normflows_amd
    if not os.path.exists(normflows_amd.native_library_path()):
        __graft_entry__.build()
    return normflows_amd


def scale_err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max()) / max(1.0, float(np.abs(b).max()))


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_train_structure_emulated_against_float64_autograd(nfa, name):
    from made_bwd_emulator import emulate_chain, emulate_wgrad
    from made_fwd_emulator import emulate_forward
    from normflows_amd.flows import affine_wide_pack as awp
    from normflows_amd.flows import made_pack
    layer, g, gold = ref.load_layer(nfa, name)
    d = cases.CASES[name]["d"]
    st = awp.train_structure(layer, d)
    assert isinstance(st, dict)
    sl = awp.slot_layers(layer, d)
    lins = awp.linears(awp.structure(layer, d))
    plist = [t for l in lins for t in (l.weight, l.bias)]
    flat32 = np.concatenate([np.zeros(1, np.float32)] + [p.detach().numpy().astype(np.float32).ravel() for p in plist])
    # flat[src] reproduces the value packs, forward and backward
    assert np.array_equal(flat32[st["src"]], made_pack._pack_forward_from(sl)[0])
    sl_m = dict(sl, masks=awp._train_masks(sl, cases.CASES[name]["kind"]))
    assert np.array_equal(flat32[st["bwd"]["src"]], made_pack._pack_backward_from(sl_m)["blob"])
    assert st["src"].size % 4 == 0 and st["bwd"]["src"].size % 4 == 0
    bw = st["bwd"]
    assert bw["MD"] == 2 * d and bw["NB"] == 1 and int(bw["table"][13]) == 1 and int(st["table"][13]) == 1
    assert int(bw["table"][14]) == bw["Mp"] and int(bw["table"][15]) == 0 and int(st["table"][14]) == 0
    assert np.array_equal(st["modes"], awp.pack(layer, d)[1][-st["modes"].size:])
    flat = flat32.astype(np.float64)
    x = g["x"].astype(np.float64)
    cz, cl = gold["cz"].astype(np.float64), gold["cl"].astype(np.float64)
    modes, smap, nets = sl["modes"], st["smap"], st["nets"]
    Hp, Dp = sl["Hp"], sl["Dp"]
    twin = copy.deepcopy(layer).double()
    order = ref.param_order(nfa, layer, d)
    zeros = ref.exact_zero_entries(layer, name)
    for direction, leg in ((0, "fwd"), (1, "inv")):
        P = emulate_forward(flat[st["src"]], st["table"], x)
        assert P.shape == (cases.ROWS, 2 * d)
        y, ld = ref.apply_np(x, P, modes, smap, nets, direction)
        gz, gP = ref.apply_bwd_np(x, P, cz, cl, modes, smap, nets, direction)
        # the pre-activations in slot space (their signs are the forward's bits)
        xin = np.zeros((cases.ROWS, Dp))
        xin[:, :d] = x
        (W0, _, b0), (W1, _, b1) = sl["layers"][0], sl["layers"][1]
        h = xin @ W0.astype(np.float64).T + b0
        t = np.maximum(h, 0) @ W1.astype(np.float64).T + b1
        S = [h, t, t]
        pack = dict(bw, blob=flat[bw["src"]])
        gx_c, G = emulate_chain(pack, gP, S)
        grads = awp.carve(emulate_wgrad(pack, gP, x, G, S), bw["offsets"], st["carve"])
        gx = gz + gx_c
        # torch float64 autograd of the same layer
        twin.zero_grad(set_to_none=True)
        xx = torch.from_numpy(x).clone().requires_grad_(True)
        yt, ldt = ref.torch_layer(twin, xx, direction)
        ((yt * torch.from_numpy(cz)).sum() + (ldt * torch.from_numpy(cl)).sum()).backward()
        assert scale_err(y, yt.detach().numpy()) < 1e-5 and scale_err(ld, ldt.detach().numpy()) < 1e-5
        assert scale_err(gx, xx.grad.numpy()) < 1e-5
        tp = dict(twin.named_parameters())
        assert len(grads) == len(order) == len(list(layer.parameters()))
        got = {}
        for k, gr in zip(order, grads):
            want = tp[k].grad
            want = np.zeros(tuple(tp[k].shape)) if want is None else want.numpy()
            assert tuple(gr.shape) == tuple(tp[k].shape), k
            assert scale_err(gr, want) < 1e-5, (k, leg, scale_err(gr, want))
            got[k] = gr
        # ... which is the reference's autograd (float64 leg of the fixture) on the same weights and rows
        assert scale_err(y, gold["z_%s_f64" % leg]) < 1e-5 and scale_err(ld, gold["ld_%s_f64" % leg]) < 1e-5
        assert scale_err(gx, gold["gx_%s_f64" % leg]) < 1e-5
        stride = int(gold["stride"])
        for k in order:
            key = k.replace(".", "__")
            assert scale_err(got[k].reshape(-1)[::stride], gold["g_%s_f64__%s" % (leg, key)]) < 1e-5, (k, leg)
            chk = gold["chk_%s_f64__%s" % (leg, key)]
            assert abs(float(got[k].sum()) - chk[0]) <= 1e-5 * max(1.0, chk[1])
        # the entries the reference's autograd leaves exactly 0
        assert bool(zeros) == (cases.CASES[name]["kind"] == "masked")
        for k, m in zeros:
            assert m.any() and not got[k][m].any(), (k, leg)
            assert not tp[k].grad.numpy()[m].any()


def test_eligibility_table_and_switch(nfa):
    """train_structure takes exactly the layers supported() takes, and declines the others with supported()'s reason."""
    from normflows_amd.flows import affine_wide_pack as awp
    MLP, MAF, Block = nfa.nets.MLP, nfa.flows.MaskedAffineFlow, nfa.flows.AffineCouplingBlock
    alt = lambda d: torch.tensor([1.0 if i % 2 == 0 else 0.0 for i in range(d)])      # noqa: E731
    wide = lambda d, **kw: MLP([d, 72, 72, d], **kw)      # noqa: E731
    for layer, d in ((MAF(alt(17), wide(17), wide(17)), 17), (MAF(alt(17), None, wide(17)), 17), (Block(MLP([9, 72, 72, 16])), 17),
                     (Block(MLP([2, 65, 65, 2])), 3), (Block(MLP([9, 72, 72, 8]), scale=False), 17)):
        assert awp.supported(layer, d) is None
        st = awp.train_structure(layer, d)
        assert isinstance(st, dict) and len(st["carve"]) == len(list(layer.parameters()))
    for layer, d, word in (
            (MAF(alt(17), wide(17), wide(17, leaky=0.1)), 17, "slope 0.1"),
            (MAF(alt(17), wide(17), MLP([17, 72, 17])), 17, "1 hidden layers"),
            (MAF(alt(17), MLP([17, 260, 260, 17]), MLP([17, 260, 260, 17])), 17, "548 hidden slots"),
            (MAF(alt(129), wide(129), None), 129, "d = 129"),
            (MAF(alt(16), MLP([16, 64, 64, 16]), MLP([16, 64, 64, 16])), 16, "chain"),
            (Block(MLP([8, 64, 64, 16])), 16, "chain"),
            (MAF(alt(17) * 0.5, wide(17), wide(17)), 17, "not binary"),
            (MAF(alt(17), wide(17), wide(17)).double(), 17, "float64"),
            (Block(MLP([9, 72, 72, 16]), split_mode="checkerboard"), 17, "checkerboard"),
            (MAF(alt(17), wide(17, dropout=0.1), None), 17, "plain nets.MLP"),
            (nfa.flows.ActNorm(17), 17, "neither")):
        got = awp.train_structure(layer, d)
        assert isinstance(got, str) and word in got and got == awp.supported(layer, d), (word, got)
    # layers of one structure share it; another mask is another structure
    a, b = awp.train_structure(MAF(alt(17), wide(17), wide(17)), 17), awp.train_structure(MAF(alt(17), wide(17), wide(17)), 17)
    assert a["src"] is b["src"] and a["bwd"]["mask"] is b["bwd"]["mask"]
    c = awp.train_structure(MAF(1 - alt(17), wide(17), wide(17)), 17)
    assert c["src"] is not a["src"] and not np.array_equal(c["bwd"]["mask"], a["bwd"]["mask"])
    # opt-in
    cfg = nfa.config
    assert cfg.affine_wide_train is False
    gate = cfg.affine_wide_train_capture_min_batch
    assert gate > 0
    cfg.set_affine_wide_train(True, capture_min_batch=0)
    assert cfg.affine_wide_train is True and cfg.affine_wide_train_capture_min_batch == 0
    cfg.set_affine_wide_train(False, capture_min_batch=gate)
    assert cfg.affine_wide_train is False and cfg.affine_wide_train_capture_min_batch == gate
    # on the CPU the route declines (the layer-wise code then refuses the tensor as before)
    cfg.set_affine_wide_train(True)
    try:
        from normflows_amd.flows.affine import _affine_wide_train
        assert _affine_wide_train(MAF(alt(17), wide(17), wide(17)), torch.zeros(4, 17, requires_grad=True), False) is None
    finally:
        cfg.set_affine_wide_train(False)


def test_symbols_are_declared_exported_bound_and_validate_their_arguments(nfa):
    declared = nfa._lib.exported_symbols_declared()
    lib = nfa._lib.lib()
    for sym, wrapper in (("nf_affine_wide_apply", "affine_wide_apply"), ("nf_affine_wide_apply_bwd", "affine_wide_apply_bwd")):
        assert sym in declared and hasattr(lib, sym) and hasattr(nfa.ops, wrapper)
    protos = nfa._lib.prototypes_declared()
    assert protos["nf_affine_wide_apply"][1][5] is ctypes.c_int64
    assert protos["nf_affine_wide_apply_bwd"][1][7] is ctypes.c_int64 and protos["nf_affine_wide_apply_bwd"][1][8] is ctypes.c_int64
    assert hasattr(nfa.autograd, "AffineWideFn")
    i32, i64, vp = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    null, one = vp(0), vp(16)

    def fwd(B=8, D=64, ldp=128, smap=4, nets=3, direction=0, z=one, P=one, modes=one, y=one, ld=one):
        return lib.nf_affine_wide_apply(z, P, modes, y, ld, i64(B), i32(D), i32(ldp), i32(smap), i32(nets), i32(direction), null)
    assert fwd(D=1) == -22 and fwd(D=129, ldp=258) == -22 and fwd(B=-1) == -22
    assert fwd(direction=2) == -22 and fwd(direction=-1) == -22 and fwd(ldp=126) == -22 and fwd(ldp=129) == -22
    assert fwd(nets=4) == -22 and fwd(smap=5) == -95 and fwd(smap=-1) == -95
    assert fwd(z=null) == -14 and fwd(P=null) == -14 and fwd(modes=null) == -14 and fwd(y=null) == -14 and fwd(ld=null) == -14
    assert fwd(B=0) == 0 and fwd(B=0, z=null, P=null, modes=null, y=null, ld=null) == 0 and fwd(B=0, direction=3) == -22
    assert fwd(z=vp(20)) == -22 and fwd(y=vp(24)) == -22 and fwd(P=vp(20)) == -22       # D % 4 == 0: 16-byte rows; P: 8-byte pairs
    assert fwd(D=17, ldp=34, z=null) == -14                                              # (a pointer check comes first)

    def bwd(B=8, Bp=64, D=64, ldp=128, ldg=128, smap=4, nets=3, direction=0, z=one, P=one, gy=one, gld=one, modes=one, gz=one, gP=one):
        return lib.nf_affine_wide_apply_bwd(z, P, gy, gld, modes, gz, gP, i64(B), i64(Bp), i32(D), i32(ldp), i32(ldg), i32(smap),
                                            i32(nets), i32(direction), null)
    assert bwd(D=1) == -22 and bwd(D=129, ldp=258, ldg=384) == -22 and bwd(B=-1) == -22 and bwd(direction=2) == -22
    assert bwd(Bp=7) == -22 and bwd(ldg=124) == -22 and bwd(ldg=130) == -22 and bwd(ldp=126) == -22 and bwd(smap=5) == -95
    assert bwd(z=null) == -14 and bwd(P=null) == -14 and bwd(modes=null) == -14 and bwd(gz=null) == -14 and bwd(gP=null) == -14
    assert bwd(B=0, Bp=0) == 0 and bwd(B=0, Bp=0, z=null, P=null, gy=null, gld=null, modes=null, gz=null, gP=null) == 0
    assert bwd(z=vp(20)) == -22 and bwd(gy=vp(20)) == -22 and bwd(gz=vp(24)) == -22 and bwd(gP=vp(24)) == -22 and bwd(P=vp(12)) == -22


def test_new_kernels_use_no_scratch(nfa):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    seen = []
    for name, d in kr.resources(os.path.join(ROOT, "normalizing-flows_amd", "lib", "obj", "affine_wide_train.o")).items():
        assert "affine_wide_apply" in name
        seen.append(name)
        assert d["vgpr_spill_count"] == 0 and d["private_segment_fixed_size"] == 0 and d["group_segment_fixed_size"] == 0, (name, d)
    assert len(seen) == 4 and sum("bwd" in n for n in seen) == 2, seen      # vector and scalar path of each kernel
