"""CPU-side tests of the coupling block record of the RealNVP chain kernels (csrc/realnvp_block.hpp, realnvp_chain.hip,
realnvp_train.hip; flows/realnvp_pack.py, core._run_chain_impl): one AffineCouplingBlock(nets.MLP) with the Permute directly behind
it as ONE record.  The device gather's index map against the host-packed blob, a reading of that blob the way the kernel reads it
against the reference's fixtures, the eligibility and routing rules, the structure signature and its cached permutation maps, the
stored fixtures against a float64 restatement (tests/realnvp_block_emulator.py), and the inference kernel's code-object resources."""
import os
import sys

import numpy as np
import pytest
import torch

import realnvp_block_cases as cases
import realnvp_block_emulator as emu
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
    g = load_golden("grad_realnvp_block_" + name)
    m = cases.model(nfa, name)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in golden_state(g).items()}, strict=True)
    return m.to(dtype), g


def is_block(nfa, f):
    return isinstance(f, nfa.flows.AffineCouplingBlock)


@pytest.mark.parametrize("name", list(cases.CASES))
def test_gather_map_reproduces_the_host_blob_and_slices_are_the_parameters(nfa, name):
    """flat[src] (what ops.pack_gather computes, here in torch) == core._pack_realnvp's blob bit for bit; a block and its Permute are
    one record; every tensor's (offset, shape) slice of the blob is the tensor; a block's tensors are all side 0."""
    from normflows_amd import core
    from normflows_amd.flows import realnvp_pack as rp
    m, _ = fixture_model(nfa, name)
    run = list(m.flows)
    d = cases.build(nfa, name)[1]
    recs = rp.records(run)
    assert len(recs) == cases.records(name)
    assert sum(1 + (p is not None) for _, p in recs) == len(run) and all(p is None or is_block(nfa, f) for f, p in recs)
    st = rp.structure(run, d)
    tl = rp.tensors(run)
    blob = rp.gather_reference(st, [t for t, _, _ in tl])
    ref, hmax = core._pack_realnvp(run, d, "cpu")
    assert torch.equal(blob, ref) and hmax == st["hmax"] and st["nblob"] == ref.numel() and st["nrec"] == len(recs)
    assert st["act"] >= d and st["hmax"] >= d
    covered = torch.zeros(st["nblob"], dtype=torch.bool)
    for k, (t, r, side) in enumerate(tl):
        assert torch.equal(rp.carve(st, blob, k), t.detach().float()), k
        off, shape = st["slices"][k]
        assert not covered[off:off + t.numel()].any()
        covered[off:off + t.numel()] = True
        assert st["sides"][k] == (r, side)
        f = recs[r][0]
        if is_block(nfa, f):
            assert side == 0 and any(t is p for p in f.parameters())
    assert torch.equal(st["static"][~covered], ref[~covered]) and not st["static"][covered].any()
    # every parameter of the run is in the blob exactly once
    assert {id(t) for t, _, side in tl if side is not None} == {id(p) for f in run for p in f.parameters()}
    # record headers: kind 3, c1, flip + 2 scale_map, has_perm, then the two index maps -- all in `static`
    offs = [int(v) for v in ref[4:4 + len(recs)]]
    for r, (f, p) in enumerate(recs):
        if not is_block(nfa, f):
            assert int(ref[offs[r]]) in (1, 2)
            continue
        c1, flip = ((d + 1) // 2, 0) if f.split_mode == "channel" else (d // 2, 1)
        smap = {"exp": 0, "sigmoid": 1, "sigmoid_inv": 2}[f.flows[1].scale_map] if f.flows[1].scale else 3
        head = ref[offs[r]:offs[r] + 4 + 2 * d].tolist()
        assert head[:4] == [3.0, float(c1), float(flip + 2 * smap), float(p is not None)]
        assert torch.equal(st["static"][offs[r]:offs[r] + 4 + 2 * d], ref[offs[r]:offs[r] + 4 + 2 * d])
        pf, pi = [int(v) for v in head[4:4 + d]], [int(v) for v in head[4 + d:]]
        assert sorted(pf) == sorted(pi) == list(range(d))
        x = torch.arange(float(d)).repeat(2, 1)
        if p is None:
            assert pf == pi == list(range(d))
        else:           # the maps are what Permute._move computes, in both directions
            assert torch.equal(x[:, pf], p._move(x, False)) and torch.equal(x[:, pi], p._move(x, True))
            assert [pf[i] for i in pi] == list(range(d))
    # the gradient mask: bit 2 r for a block record, never bit 2 r + 1
    blocks = [r for r, (f, _) in enumerate(recs) if is_block(nfa, f)]
    needs = [is_block(nfa, recs[r][0]) for _, r, _ in tl]
    assert rp.grad_mask(st, needs) == sum(1 << (2 * r) for r in blocks)
    for r in blocks:
        assert (rp.grad_mask(st, [True] * len(tl)) >> (2 * r)) & 3 == 1


@pytest.mark.parametrize("name", list(cases.CASES))
def test_the_blob_read_like_the_kernel_reads_it_gives_the_fixtures(nfa, name):
    """emu.blob_chain decodes the blob with the kernel's rules (record offsets, header, index maps, MLP layout) in float64: z and
    log-det of both directions equal the reference's float64 legs (float32 weights are exact in float64; the reference's log-det leg
    carries float32 rounding, as test_fixtures_equal_the_float64_restatement explains)."""
    from normflows_amd import core
    m, g = fixture_model(nfa, name)
    run = list(m.flows)
    d = cases.build(nfa, name)[1]
    blob, _ = core._pack_realnvp(run, d, "cpu")
    for dname, inverse in (("fwd", False), ("inv", True)):
        z, ld = emu.blob_chain(blob, torch.from_numpy(g["x"]), inverse)
        zr, lr = g["z_%s_f64" % dname], g["ld_%s_f64" % dname].astype(np.float64)
        assert np.abs(z.numpy() - zr).max() < 1e-9 * max(1.0, np.abs(zr).max()), (name, dname)
        assert np.abs(ld.numpy() - lr).max() < len(run) * 2.0 ** -23 * max(1.0, np.abs(lr).max()), (name, dname)


def test_eligibility(nfa):
    from normflows_amd import core
    MLP, Block, Permute = nfa.nets.MLP, nfa.flows.AffineCouplingBlock, nfa.flows.Permute
    ok, tok, joins = core._realnvp_record_ok, core._realnvp_train_record_ok, core._permute_joins
    assert ok(Block(MLP([1, 64, 64, 2])), 2) and tok(Block(MLP([1, 64, 64, 2])), 2)
    assert tok(Block(MLP([8, 32, 16])), 16) and tok(Block(MLP([8, 32, 8]), scale=False), 16)
    assert tok(Block(MLP([1, 4, 4]), split_mode="channel_inv"), 3) and tok(Block(MLP([2, 4, 2]), True, "sigmoid"), 3)
    assert tok(Block(MLP([1, 8, 2], leaky=0.0), True, "sigmoid_inv"), 2)
    for bad, d in ((Block(MLP([1, 8, 2]), split_mode="checkerboard"), 2),        # checkerboard split
                   (Block(MLP([1, 65, 2])), 2),                                   # width 65
                   (Block(MLP([9, 8, 16])), 17),                                  # d = 17
                   (Block(MLP([2, 8, 2])), 2),                                    # the MLP's input is not z1
                   (Block(MLP([1, 8, 1])), 2),                                    # scale=True needs 2 c2 outputs
                   (Block(MLP([1, 8, 2]), scale=False), 2),                       # scale=False needs c2
                   (Block(MLP([1, 8, 2], output_fn="tanh")), 2),                  # output_fn
                   (Block(MLP([1, 8, 2], dropout=0.1)), 2)):                      # dropout
        assert not ok(bad, d) and not tok(bad, d)
    assert ok(Block(MLP([1, 8, 2], leaky=-0.1)), 2) and not tok(Block(MLP([1, 8, 2], leaky=-0.1)), 2)      # negative slope: inference only
    assert ok(Block(MLP([1, 8, 2]).double()), 2) and not tok(Block(MLP([1, 8, 2]).double()), 2)            # float64 weights
    deep = lambda n: MLP([1] + [64] * n + [2])      # noqa: E731     (the LDS budget of test_host_realnvp_train.test_eligibility)
    assert tok(Block(deep(7)), 2) and not tok(Block(deep(8)), 2)
    # a Permute is never a record of its own, and joins only with the right width and a valid permutation
    assert not ok(Permute(2, "swap"), 2) and not tok(Permute(2, "swap"), 2)
    assert joins(Permute(2, "swap"), 2) and joins(Permute(5, "shuffle"), 5) and joins(Permute(3, "swap"), 3)
    assert not joins(Permute(4, "swap"), 2) and not joins(Permute(4, "shuffle"), 5) and not joins(nfa.flows.ActNorm(2), 2)
    broken = Permute(4, "shuffle")
    broken.perm.copy_(torch.tensor([0, 1, 1, 3]))
    assert not joins(broken, 4)
    # the switch
    assert nfa.config.realnvp_blocks is True
    nfa.config.set_realnvp_blocks(False)
    try:
        assert nfa.config.realnvp_blocks is False and not ok(Block(MLP([1, 8, 2])), 2) and not tok(Block(MLP([1, 8, 2])), 2)
    finally:
        nfa.config.set_realnvp_blocks(True)


def _runs(nfa, flows, d, inverse, train):
    """The fused runs of `flows` as lists of list indices, in processing order: core._run_chain_impl's walk without its launches."""
    from normflows_amd import core
    n = len(flows)
    order = list(range(n - 1, -1, -1)) if inverse else list(range(n))
    k, out = 0, []
    while k < n:
        k2 = core._realnvp_run_end(flows, order, k, d, inverse, train)
        if k2 - k >= (1 if train else 2):
            out.append(sorted(order[k:k2]))
            k = k2
        else:
            k += 1
    return out


def _stack(nfa, d=2):
    MLP, Block, Permute = nfa.nets.MLP, nfa.flows.AffineCouplingBlock, nfa.flows.Permute
    c1 = (d + 1) // 2
    return lambda: Block(MLP([c1, 4, 2 * (d - c1)])), lambda dd=d: Permute(dd, "swap")


def test_routing_a_permute_joins_only_the_block_directly_in_front_of_it(nfa):
    B, P = _stack(nfa)
    b2 = torch.tensor([1.0, 0.0])
    maf = lambda: nfa.flows.MaskedAffineFlow(b2, nfa.nets.MLP([2, 4, 2]), nfa.nets.MLP([2, 4, 2]))  # noqa: E731
    for train in (False, True):
        for inverse in (False, True):
            rev = (lambda runs: list(reversed(runs))) if inverse else (lambda runs: runs)
            # the README shape: everything is one run, in either direction
            assert _runs(nfa, [B(), P(), B(), P(), B(), P()], 2, inverse, train) == [[0, 1, 2, 3, 4, 5]]
            # a Permute that stands behind another Permute, in front of the first block or behind a MaskedAffineFlow ends a run
            flows = [P(), B(), P(), P(), B(), maf(), P(), maf(), B()]
            assert _runs(nfa, flows, 2, inverse, train) == rev([[1, 2], [4, 5], [7, 8]])
            # a Permute of another width does not join: the block in front of it is a run of one layer
            flows = [B(), P(4), B(), P()]
            assert _runs(nfa, flows, 2, inverse, train) == rev(([[0]] if train else []) + [[2, 3]])
            # a lone block: its own kernel at inference (a run needs two layers), a run of one record under autograd
            assert _runs(nfa, [B()], 2, inverse, train) == ([[0]] if train else [])
            assert _runs(nfa, [B(), P()], 2, inverse, train) == [[0, 1]]
            # between two MaskedAffineFlows a Permute ends both runs, as before
            assert _runs(nfa, [maf(), maf(), P(), maf(), maf()], 2, inverse, train) == rev([[0, 1], [3, 4]])


def test_the_cut_after_32_records_never_splits_a_block_from_its_permute(nfa):
    from normflows_amd.flows import realnvp_pack as rp
    B, P = _stack(nfa)
    flows = [f for _ in range(33) for f in (B(), P())]
    assert _runs(nfa, flows, 2, False, True) == [list(range(0, 64)), [64, 65]]
    assert _runs(nfa, flows, 2, True, True) == [list(range(2, 66)), [0, 1]]
    assert _runs(nfa, flows, 2, False, False) == [list(range(66))]              # no cap at inference
    assert _runs(nfa, flows[:64], 2, True, True) == [list(range(64))]           # the README model: one run
    assert len(rp.records(flows[:64])) == rp.MAX_RECORDS == 32
    # blocks without a Permute among them: 32 records are then fewer than 64 layers
    flows = [B(), B()] + flows[:62] + [B()]
    assert _runs(nfa, flows, 2, False, True) == [list(range(0, 62)), [62, 63, 64]]
    assert _runs(nfa, flows, 2, True, True) == [list(range(2, 65)), [0, 1]]      # (the last block + 31 pairs; 34 records in all)


def test_switching_the_blocks_off_restores_the_old_run_boundaries(nfa):
    """With config.realnvp_blocks off no block and no Permute is ever part of a run: the runs are those of the other record kinds."""
    B, P = _stack(nfa)
    b2 = torch.tensor([1.0, 0.0])
    maf = lambda: nfa.flows.MaskedAffineFlow(b2, nfa.nets.MLP([2, 4, 2]), nfa.nets.MLP([2, 4, 2]))  # noqa: E731
    flows = [B(), P(), maf(), maf(), B(), P(), maf(), nfa.flows.AffineConstFlow(2), B()]
    assert _runs(nfa, flows, 2, False, False) == [[0, 1, 2, 3, 4, 5, 6, 7, 8]] and _runs(nfa, flows, 2, True, True) == [[0, 1, 2, 3, 4, 5, 6, 7, 8]]
    nfa.config.set_realnvp_blocks(False)
    try:
        for train in (False, True):
            assert _runs(nfa, flows, 2, False, train) == [[2, 3], [6, 7]] and _runs(nfa, flows, 2, True, train) == [[6, 7], [2, 3]]
            assert _runs(nfa, [B(), P(), B(), P()], 2, False, train) == []
    finally:
        nfa.config.set_realnvp_blocks(True)


def test_signature_is_value_independent_and_follows_the_permutation(nfa, monkeypatch):
    from normflows_amd import _keys
    from normflows_amd.flows import realnvp_pack as rp
    m, _ = fixture_model(nfa, "d5_maps")
    run = list(m.flows)
    shuffle = run[3]
    builds = []
    real_cached = _keys.cached

    def spy(owner, slot, key, build, *a, **k):
        def counted():
            builds.append(slot)
            return build()
        return real_cached(owner, slot, key, counted, *a, **k)
    monkeypatch.setattr(_keys, "cached", spy)
    reads = []
    real_tolist = torch.Tensor.tolist
    monkeypatch.setattr(torch.Tensor, "tolist", lambda t: reads.append(t.data_ptr()) or real_tolist(t))
    sig = rp.signature(run, 5)
    assert builds == ["_maps_cache"] and sorted(reads) == sorted([shuffle.perm.data_ptr(), shuffle.inv_perm.data_ptr()])
    # asked again -- by signature, by structure, by the host packer: the buffers' values are not read a second time
    assert rp.signature(run, 5) == sig
    st = rp.structure(run, 5)
    from normflows_amd import core
    core._pack_realnvp(run, 5, "cpu")
    assert core._permute_joins(shuffle, 5)
    assert builds == ["_maps_cache"] and len(reads) == 2
    # weights do not enter
    with torch.no_grad():
        for p in m.parameters():
            p.add_(1.0)
    assert rp.signature(run, 5) == sig and builds == ["_maps_cache"]
    # a load_state_dict that replaces the permutation does, and the structure's static part follows
    sd = m.state_dict()
    old = sd["flows.3.perm"].clone()
    new = torch.roll(old, 1)
    assert not torch.equal(new, old)
    sd["flows.3.perm"] = new
    sd["flows.3.inv_perm"] = torch.empty_like(new).scatter_(0, new, torch.arange(5))
    m.load_state_dict(sd)
    sig2 = rp.signature(run, 5)
    assert sig2 != sig and builds == ["_maps_cache"] * 2 and len(reads) == 4
    st2 = rp.structure(run, 5)
    assert not torch.equal(st2["static"], st["static"]) and torch.equal(st2["src"], st["src"])
    off = int(st2["static"][4 + 1])         # record 1 = [block 2, the shuffle]
    assert torch.equal(st2["static"][off + 4:off + 9], new.float())
    assert rp.signature(run, 5) == sig2 and len(reads) == 4
    # a swap has nothing to read
    m2, _ = fixture_model(nfa, "readme_d2")
    n = len(reads)
    rp.signature(list(m2.flows), 2)
    assert len(reads) == n


@pytest.mark.parametrize("name", list(cases.CASES))
def test_fixtures_equal_the_float64_restatement(nfa, name):
    """The reference's float64 legs against realnvp_block_emulator (plain torch formulas, float64, CPU) on the stored weights, at the
    bars of test_host_realnvp_train.test_fixtures_equal_the_float64_restatement: z at 1e-9 of scale, the log-det at the float32
    rounding of the reference's float32 accumulator (2^-23 per layer), gradients at 2^-22 of scale (the cotangent of that
    accumulator is rounded to float32 on the way back)."""
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
        assert g["ld_%s_f64" % dname].dtype == np.float32
        close(ld, g["ld_%s_f64" % dname], "ld " + dname, bar=len(flows) * 2.0 ** -23)
        gbar = 2.0 ** -22
        close(gx, g["gx_%s_f64" % dname], "gx " + dname, bar=gbar)
        n = 0
        for k, p in m.named_parameters():
            close(gp[id(p)], g["g_%s_f64__%s" % (dname, k.replace(".", "__"))], "%s %s" % (dname, k), bar=gbar)
            n += 1
        assert n == len(list(m.flows.parameters())) > 0
    for k in ("z_fwd", "ld_inv", "gx_inv"):
        assert np.abs(g[k] - g[k + "_f64"]).max() < 1e-3 * max(1.0, np.abs(g[k + "_f64"]).max()), k


def test_inference_kernel_uses_no_scratch(nfa):
    """The coordinates and the record's temporaries stay in registers: c1, the flip and the permutation are run-time values, and
    every move between columns goes through LDS."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    seen = 0
    for name, d in kr.resources(os.path.join(ROOT, "normalizing-flows_amd", "lib", "obj", "realnvp_chain.o")).items():
        if "realnvp_chain_kernel" in name:
            seen += 1
            assert d["vgpr_spill_count"] == 0 and d["private_segment_fixed_size"] == 0 and d["vgpr_count"] <= 256, (name, d)
    assert seen == 1, seen
