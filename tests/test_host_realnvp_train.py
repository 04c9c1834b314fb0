"""CPU-side tests of the RealNVP training route (csrc/realnvp_train.hip, autograd.RealNVPChainFn, flows/realnvp_pack.py): the device
gather's index map against the inference kernel's host-packed blob, the gradient slices, the eligibility rules, the new entry points'
export and argument validation, the kernels' code-object resources, and the stored fixtures against a float64 restatement of the
formulas (tests/realnvp_train_emulator.py)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import realnvp_train_cases as cases
import realnvp_train_emulator as emu
from conftest import golden_state, load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def nfa():
    import __graft_entry__
    import normflows_amd
    if not os.path.exists(normflows_amd.native_library_path()):
        __graft_entry__.build()
    return normflows_amd


def fixture_model(nfa, name, dtype=torch.float32):
    g = load_golden("grad_realnvp_train_" + name)
    m = cases.model(nfa, name)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in golden_state(g).items()}, strict=True)
    return m.to(dtype), g


@pytest.mark.parametrize("name", list(cases.CASES))
def test_gather_map_reproduces_the_host_blob_and_slices_are_the_parameters(nfa, name):
    """flat[src] (what ops.pack_gather computes, here in torch) == core._pack_realnvp's blob bit for bit; every tensor's (offset,
    shape) slice of the blob is the tensor: the gradient blob has the same layout, so the same slice is its gradient."""
    from normflows_amd import core
    from normflows_amd.flows import realnvp_pack as rp
    m, _ = fixture_model(nfa, name)
    run = list(m.flows)
    d = cases.build(nfa, name)[1]
    st = rp.structure(run, d)
    tl = rp.tensors(run)
    blob = rp.gather_reference(st, [t for t, _, _ in tl])
    ref, hmax = core._pack_realnvp(run, d, "cpu")
    assert torch.equal(blob, ref) and hmax == st["hmax"] and st["nblob"] == ref.numel() and st["nrec"] == len(run)
    assert int(st["src"].min()) >= 1 and int(st["src"].max()) == st["nblob"] + sum(t.numel() for t, _, _ in tl)
    covered = torch.zeros(st["nblob"], dtype=torch.bool)
    for k, (t, r, side) in enumerate(tl):
        assert torch.equal(rp.carve(st, blob, k), t.detach()), k
        off, shape = st["slices"][k]
        assert not covered[off:off + t.numel()].any()
        covered[off:off + t.numel()] = True
        assert st["sides"][k] == (r, side) and (side is None) == (t is run[r].__dict__["_buffers"].get("b"))
    assert torch.equal(st["static"][~covered], ref[~covered]) and not st["static"][covered].any()
    # the gradient mask: one bit per (record, side) with a tensor that needs its gradient; the mask buffer b never
    needs = [side == 1 for _, _, side in tl]
    assert rp.grad_mask(st, needs) == sum(1 << (2 * r + 1) for r in sorted({r for _, r, side in tl if side == 1}))
    assert rp.grad_mask(st, [False] * len(tl)) == 0 and rp.grad_mask(st, [side is None for _, _, side in tl]) == 0
    # the structure depends on the shapes alone
    for p in m.parameters():
        p.data.add_(1.0)
    assert rp.signature(run, d) == rp.signature(list(fixture_model(nfa, name)[0].flows), d)


def test_eligibility(nfa):
    from normflows_amd import core
    MLP, MAF = nfa.nets.MLP, nfa.flows.MaskedAffineFlow
    ok = core._realnvp_train_record_ok
    b2 = torch.tensor([1.0, 0.0])
    assert ok(MAF(b2, MLP([2, 64, 64, 2]), MLP([2, 64, 64, 2])), 2) and ok(MAF(b2), 2) and ok(nfa.flows.AffineConstFlow(2), 2)
    assert ok(MAF(b2, MLP([2, 8, 2], leaky=0.0), None), 2) and ok(MAF(b2, None, MLP([2, 8, 2], leaky=0.2)), 2)
    assert not ok(MAF(b2, MLP([2, 65, 2]), None), 2)                                   # width 65
    b17 = torch.tensor([1.0, 0.0] * 8 + [1.0])
    assert not ok(MAF(b17, MLP([17, 8, 17]), None), 17) and not ok(nfa.flows.AffineConstFlow(17), 17)      # d 17
    assert not ok(MAF(b2, MLP([2, 8, 2], leaky=-0.1), None), 2)                        # negative slope
    assert not ok(MAF(b2, MLP([2, 8, 2], output_fn="tanh"), None), 2)                  # output_fn
    assert not ok(MAF(b2, MLP([2, 8, 2], dropout=0.1), None), 2)                       # dropout
    assert not ok(MAF(b2, MLP([2, 8, 2]).double(), None), 2)                           # float64 weights
    # the LDS budget: one MLP's Linear inputs + two 64-wide gradient columns at 65 floats per column within 160 KB
    deep = lambda n: MLP([2] + [64] * n + [2])      # noqa: E731
    assert nfa.ops.realnvp_rows(64, 2 + 64 * 7) == 64 and nfa.ops.realnvp_rows(64, 2 + 64 * 8) == 0
    assert nfa.ops.realnvp_rows(64, 130) == 128 and nfa.ops.realnvp_rows(16, 21) == 256
    assert ok(MAF(b2, deep(7), None), 2) and not ok(MAF(b2, deep(8), None), 2)
    # ActNorm: only once its data-dependent initialisation is done
    an = nfa.flows.ActNorm(2)
    assert not ok(an, 2)
    an2 = nfa.flows.ActNorm(2)
    an2.data_dep_init_done.fill_(1.0)
    assert ok(an2, 2)
    # the switch, and higher_order_gradients()
    assert nfa.config.realnvp_train is True and core._realnvp_train_enabled()
    with nfa.config.higher_order_gradients():
        assert not core._realnvp_train_enabled()
    assert core._realnvp_train_enabled()
    nfa.config.set_realnvp_train(False)
    try:
        assert nfa.config.realnvp_train is False and not core._realnvp_train_enabled()
    finally:
        nfa.config.set_realnvp_train(True)


def test_symbols_are_declared_exported_bound_and_validate_their_arguments(nfa):
    lib = nfa._lib.lib()
    for sym in ("nf_realnvp_train_rows", "nf_realnvp_train_scratch_floats", "nf_realnvp_chain_train_fwd", "nf_realnvp_chain_bwd"):
        assert sym in nfa._lib.exported_symbols_declared() and hasattr(lib, sym), sym
    assert "nf_realnvp_train_scratch_floats" in nfa._lib.int64_functions_declared()
    for name in ("realnvp_chain_train_fwd", "realnvp_chain_bwd", "realnvp_rows"):
        assert hasattr(nfa.ops, name)
    assert hasattr(nfa.autograd, "RealNVPChainFn")
    EINVAL, ENOTSUP, EFAULT = -22, -95, -14
    vp = ctypes.c_void_p
    null, ok = vp(0), vp(4096)
    assert lib.nf_realnvp_train_rows(0, 4) == EINVAL and lib.nf_realnvp_train_rows(65, 4) == ENOTSUP
    assert lib.nf_realnvp_train_rows(64, 100000) == ENOTSUP
    wg = lib.nf_persistent_workgroups()
    sf = lib.nf_realnvp_train_scratch_floats
    assert sf(1024, 64, 130, 18000) == 8 * 18000 and sf(10 ** 6, 64, 130, 18000) == wg * 18000
    assert sf(10 ** 6, 64, 130, 1 << 17) == (1 << 24) and sf(10 ** 6, 64, 130, (1 << 24) + 1) == EINVAL      # the 64 MiB bound
    assert sf(-1, 64, 130, 100) == EINVAL and sf(8, 65, 130, 100) == ENOTSUP

    def fwd(B=8, d=2, hmax=8, act=10, direction=0, **p):
        a = dict(z=ok, y=ok, logdet=ok, save=ok, blob=ok)
        a.update(p)
        return lib.nf_realnvp_chain_train_fwd(a["z"], a["y"], a["logdet"], a["save"], a["blob"], B, d, hmax, act, direction, None)

    def bwd(B=8, d=2, hmax=8, act=10, nblob=100, direction=0, wmask=1, **p):
        a = dict(save=ok, gy=ok, gld=ok, gz=ok, blob=ok, slabs=ok, grads=ok)
        a.update(p)
        return lib.nf_realnvp_chain_bwd(a["save"], a["gy"], a["gld"], a["gz"], a["blob"], a["slabs"], a["grads"], B, d, hmax, act,
                                        nblob, direction, wmask, None)

    for call in (fwd, bwd):
        assert call(B=-1) == EINVAL and call(d=0) == EINVAL and call(direction=2) == EINVAL and call(hmax=1) == EINVAL
        assert call(act=1) == EINVAL                                  # fewer activation columns than coordinates
        assert call(d=17, hmax=17, act=17) == ENOTSUP and call(hmax=65, act=70) == ENOTSUP and call(hmax=64, act=600) == ENOTSUP
        assert call(B=0) == 0
    for k in ("z", "y", "logdet", "save", "blob"):
        assert fwd(**{k: null}) == EFAULT, k
    for k in ("save", "blob", "slabs", "grads"):
        assert bwd(**{k: null}) == EFAULT, k
    assert bwd(nblob=0) == EINVAL
    assert bwd(wmask=0, gz=null) == 0          # nothing asked for: nothing launched


def test_training_kernels_use_no_scratch(nfa):
    """The coordinates, their cotangents and the per-record temporaries stay in registers (every index into them is static)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    seen = 0
    for name, d in kr.resources(os.path.join(ROOT, "normalizing-flows_amd", "lib", "obj", "realnvp_train.o")).items():
        if "realnvp_train_" in name:
            seen += 1
            assert d["vgpr_spill_count"] == 0 and d["private_segment_fixed_size"] == 0 and d["vgpr_count"] <= 256, (name, d)
    assert seen == 3, seen


@pytest.mark.parametrize("name", list(cases.CASES))
def test_fixtures_equal_the_float64_restatement(nfa, name):
    """The reference's float64 legs against realnvp_train_emulator (plain torch formulas, float64, CPU) on the stored weights: z at 1e-9 of
    scale, log-det and gradients at the float32 rounding the reference itself puts into them (below).  The float32 weights are exactly representable in float64, so the only difference is the order of float64 operations."""
    m, g = fixture_model(nfa, name, torch.float64)
    flows = list(m.flows)
    x, cz, cl = (torch.from_numpy(g[k]).double() for k in ("x", "cz", "cl"))

    def close(got, ref, what, bar=1e-9):
        ref = np.asarray(ref, dtype=np.float64)
        err = float(np.abs(got.detach().numpy() - ref).max()) / max(1.0, float(np.abs(ref).max()))
        assert err < bar, (name, what, err)

    for dname, inverse in (("fwd", False), ("inv", True)):
        z, ld, gx, gp = emu.grads(flows, x, cz, cl, inverse)
        close(z, g["z_%s_f64" % dname], "z " + dname)
        # (the reference sums the layers' log-dets into torch.zeros(len(z)) -- a float32 accumulator whatever the model's dtype,
        # core.py:40-55: its float64 leg of ld carries float32 rounding, 2^-24 relative per layer)
        assert g["ld_%s_f64" % dname].dtype == np.float32
        close(ld, g["ld_%s_f64" % dname], "ld " + dname, bar=len(flows) * 2.0 ** -23)
        # (and the cotangent cl reaches every gradient through that float32 accumulator: autograd rounds it to float32 on the way
        # back, so the float64 leg's gradients carry 2^-24 relative of their log-det term -- 2^-22 of scale bounds it here)
        gbar = 2.0 ** -22
        close(gx, g["gx_%s_f64" % dname], "gx " + dname, bar=gbar)
        n = 0
        for k, p in m.named_parameters():
            close(gp[id(p)], g["g_%s_f64__%s" % (dname, k.replace(".", "__"))], "%s %s" % (dname, k), bar=gbar)
            n += 1
        assert n == len(list(m.flows.parameters())) > 0
    # the float32 legs are float32 evaluations of the same thing
    for k in ("z_fwd", "ld_inv", "gx_inv"):
        assert np.abs(g[k] - g[k + "_f64"]).max() < 1e-3 * max(1.0, np.abs(g[k + "_f64"]).max()), k
    assert g["sd__flows__%d__data_dep_init_done" % (len(flows) - 1)] > 0


# ---- the limit of 32 records ------------------------------------------------------------------------------------------------------
def _records(nfa, n, d=2):
    """n records alternating MaskedAffineFlow(MLP [d, 4, d] s and t) / ActNorm (initialised), every parameter random, on the CPU."""
    g = torch.Generator().manual_seed(n)
    b = torch.tensor([1.0, 0.0] * ((d + 1) // 2))[:d]
    flows = []
    for i in range(n):
        if i % 2 == 0:
            flows.append(nfa.flows.MaskedAffineFlow(b if i % 4 == 0 else 1 - b, nfa.nets.MLP([d, 4, d]), nfa.nets.MLP([d, 4, d], leaky=0.05)))
        else:
            flows.append(nfa.flows.ActNorm(d))
            flows[-1].data_dep_init_done.fill_(1.0)
    with torch.no_grad():
        for f in flows:
            for p in f.parameters():
                p.copy_(0.3 * torch.randn(p.shape, generator=g))
    return flows


def test_structure_mask_and_slices_at_32_records(nfa):
    """MAX_RECORDS records: the gather map still reproduces the host blob; bit 2 * 31 + 1 alone (the t of the last record, an ActNorm)
    is the int64 -(1 << 63), all 64 bits are -1, bit 62 alone stays positive; the last record's tensors are the last slices of the blob."""
    from normflows_amd import core
    from normflows_amd.flows import realnvp_pack as rp
    assert rp.MAX_RECORDS == 32
    run = _records(nfa, 32)
    st = rp.structure(run, 2)
    tl = rp.tensors(run)
    assert st["nrec"] == 32 and len(tl) == len(st["sides"]) == len(st["slices"])
    blob = rp.gather_reference(st, [t for t, _, _ in tl])
    ref, hmax = core._pack_realnvp(run, 2, "cpu")
    assert torch.equal(blob, ref) and hmax == st["hmax"]
    sides = st["sides"]
    assert sides[-2:] == [(31, 0), (31, 1)] and {r for r, _ in sides} == set(range(32))
    assert rp.grad_mask(st, [rs == (31, 1) for rs in sides]) == -(1 << 63)
    assert rp.grad_mask(st, [rs == (31, 0) for rs in sides]) == 1 << 62
    assert rp.grad_mask(st, [r == 31 for r, _ in sides]) == -(1 << 63) + (1 << 62)
    assert rp.grad_mask(st, [True] * len(sides)) == -1                     # every record has an s side and a t side
    assert rp.grad_mask(st, [r == 0 for r, _ in sides]) == 3
    for m in (rp.grad_mask(st, [True] * len(sides)), rp.grad_mask(st, [rs == (31, 1) for rs in sides])):
        assert ctypes.c_int64(m).value == m                                # representable as the C side's int64_t
    # carve: the last record's s and t are the last 2 d floats of a gradient blob, in that order
    grads = torch.arange(st["nblob"], dtype=torch.float32)
    k = len(tl) - 2
    assert torch.equal(rp.carve(st, grads, k).reshape(-1), grads[-4:-2]) and torch.equal(rp.carve(st, grads, k + 1).reshape(-1), grads[-2:])
    assert rp.carve(st, grads, k).shape == run[31].s.shape and rp.carve(st, grads, k + 1).shape == run[31].t.shape
    assert torch.equal(rp.carve(st, blob, k), run[31].s.detach()) and torch.equal(rp.carve(st, blob, k + 1), run[31].t.detach())
    # ... and the first tensor with a gradient of the last MaskedAffineFlow (record 30) lies where its offset says
    k30 = min(i for i, (r, s) in enumerate(sides) if r == 30 and s is not None)
    assert torch.equal(rp.carve(st, blob, k30), tl[k30][0].detach())


def test_the_two_directions_of_a_40_record_stack_share_a_slot_with_two_signatures(nfa):
    """core cuts a run after 32 records in processing order: the forward pass fuses records [0, 32) and [32, 40), the inverse pass
    [8, 40) and [0, 8).  [0, 32) and [0, 8) start with the same flow, which names their cache slot (sub=id(run[0])): the slot's key
    -- signature(run, d) -- must tell them apart, and the structures must differ."""
    from normflows_amd import _keys
    from normflows_amd.flows import realnvp_pack as rp
    flows = _records(nfa, 40)
    fwd, inv = flows[:32], flows[:8]
    assert fwd[0] is inv[0]
    assert rp.signature(fwd, 2) != rp.signature(inv, 2) and rp.signature(fwd, 2)[:9] == rp.signature(inv, 2)
    assert rp.signature(flows[8:40], 2) == rp.signature(fwd, 2)            # same kinds and shapes, other flows: another slot
    assert rp.structure(fwd, 2)["nblob"] != rp.structure(inv, 2)["nblob"]
    holder, built = {"run_struct": {}}, []

    def get(run):
        return _keys.cached(holder, "run_struct", (rp.signature(run, 2), "cpu"), lambda: built.append(len(run)) or rp.structure(run, 2),
                            sub=id(run[0]))
    assert get(fwd)["nrec"] == 32 and get(inv)["nrec"] == 8 and get(fwd)["nrec"] == 32 and get(fwd)["nrec"] == 32
    assert built == [32, 8, 32]                                            # one slot: rebuilt on every change of direction, never stale
