"""CPU-side tests of the one-launch wide RealNVP coupling layer (nf_affine_wide: csrc/affine_wide.hip, flows/affine_wide_pack.py): the
packed schedule walked by tests/affine_wide_emulator.py in float32 against the REFERENCE's stored outputs (tests/golden/
affine_wide_*.npz, make_golden_affine_wide.py) in both directions, where every weight lands, the wrap-around copies, the prefix
k-group counts of the stacked nets, the packer's eligibility with its reasons, the C ABI's argument validation, the switch and the
code objects' resources."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import affine_wide_cases as cases
from conftest import assert_close, golden_state, ld_tol, load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = dict(rtol=1e-4, atol=1e-4)


@pytest.fixture(scope="module")
def nfa():
    import __graft_entry__
    import normflows_amd
    if not os.path.exists(normflows_amd.native_library_path()):
        __graft_entry__.build()
    return normflows_amd


def load_layer(nfa, name):
    g = load_golden("affine_wide_" + name)
    layer = cases.build(nfa, name)
    layer.load_state_dict({k: torch.from_numpy(v) for k, v in golden_state(g).items()})
    return layer, g


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_emulated_schedule_reproduces_the_reference(nfa, name):
    from affine_wide_emulator import emulate
    from normflows_amd.flows import affine_wide_pack as awp
    layer, g = load_layer(nfa, name)
    d = cases.CASES[name]["d"]
    assert g["x"].shape == (cases.ROWS, d) and awp.supported(layer, d) is None
    blob, table = awp.pack(layer, d)
    assert blob.dtype == np.float32 and table.dtype == np.int32
    assert int(table[3]) == {"a": 256, "b": 512, "c": 512, "d": 256, "e": 256, "f": 256, "g": 256, "h": 256}[name]
    for direction, leg in ((0, "fwd"), (1, "inv")):
        y, ld = emulate(blob, table, g["x"], direction)
        assert_close(y, g["y_" + leg], what="%s y %s" % (name, leg), **TOL)
        assert_close(ld, g["ld_" + leg], what="%s ld %s" % (name, leg), **ld_tol(np.float32))
        idt = np.nonzero(awp.slot_layers(layer, d)["modes"] == 0)[0]
        assert idt.size and np.array_equal(y[:, idt], g["x"][:, idt])            # identity features: bit for bit
    if name in ("d", "h"):                                                       # no scale parameter: the log-det is exactly 0
        assert not ld.any() and not g["ld_fwd"].any()
    # the register weight ring over two tiles of a persistent workgroup: every entry it multiplies with is the one the schedule
    # means, and no request leaves the wave's stream
    from made_fwd_emulator import two_tile_ring_walk
    groups = two_tile_ring_walk(blob, table)
    assert len(groups) == 8 and min(groups) > 0


def _index_weights(layer):
    """{id(Linear): (weight, bias)} holding distinct positive integers (exact in float32), and the Linears."""
    lins = [m for m in layer.modules() if isinstance(m, torch.nn.Linear)]
    wb, off = {}, 1
    for l in lins:
        o, i = l.weight.shape
        w = off + np.arange(o * i, dtype=np.int64).reshape(o, i)
        off += o * i
        b = off + np.arange(o, dtype=np.int64)
        off += o
        wb[id(l)] = (w.astype(np.float32), b.astype(np.float32))
    assert off < 2 ** 24
    return wb, lins


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_every_weight_lands_once_and_the_streams_wrap(nfa, name):
    """The pack of index-valued weights: every weight and bias the layer uses appears exactly once in the streams (a masked flow's
    first-layer columns of transformed features are multiplied by b_f = 0 and never appear; a bias group repeats a bias for the 32
    lanes of a half), nothing else does, and every wave's stream ends with the copy of its first 8 entries."""
    from affine_wide_emulator import items_of
    from normflows_amd.flows import affine_wide_pack as awp
    layer, _ = load_layer(nfa, name)
    c = cases.CASES[name]
    d = c["d"]
    wb, lins = _index_weights(layer)
    blob, table = awp.pack(layer, d, wb=wb)
    tab = items_of(table)
    total = int(table[9])
    assert blob.size == total
    # an item = one row-block of one layer for the sample blocks its wave owns: a 512-slot hidden row-block has one owner (both sample
    # blocks), a 256-slot hidden row-block and every final row-block two (one per sample block), which hold the same entries
    owners = {}
    for w in range(8):
        pos, end = int(table[16 + w]), (int(table[16 + w + 1]) if w < 7 else total)
        start = pos
        for i, (nkg, rb) in enumerate(tab[w]):
            if rb < 0:
                continue
            n = 1024 + 256 * int(nkg)
            owners.setdefault((i // 2, int(rb)), []).append(blob[pos:pos + n])
            pos += n
        assert end - pos == 8 * 256 and np.array_equal(blob[pos:end], np.resize(blob[start:pos], 8 * 256))      # the wrap-around copy
    nsb = int(table[4])
    weights, biases = [], []
    for (layer_i, rb), copies in sorted(owners.items()):
        assert len(copies) == (1 if (layer_i < 3 and nsb == 2) else 2), (layer_i, rb, len(copies))
        assert all(np.array_equal(c_, copies[0]) for c_ in copies)
        biases.append(copies[0][:1024].reshape(4, 2, 32, 4)[:, :, 0, :].reshape(-1))
        weights.append(copies[0][1024:])
    got_w = np.concatenate(weights)
    got_b = np.concatenate(biases)
    want_w, want_b = [], []
    b = cases.mask(c) if c["kind"] == "masked" else None
    for l in lins:
        w_, b_ = wb[id(l)]
        first = any(l is net[0] for net in _nets(layer))
        want_w.append((w_[:, b == 1.0] if (first and b is not None) else w_).reshape(-1))
        want_b.append(b_)
    want_w, want_b = np.concatenate(want_w), np.concatenate(want_b)
    assert np.array_equal(np.sort(got_w[got_w != 0]), np.sort(want_w))
    assert np.array_equal(np.sort(got_b[got_b != 0]), np.sort(want_b))


def _nets(layer):
    out = []
    for m in layer.modules():
        if type(m).__name__ == "MLP":
            out.append([l for l in m.net if isinstance(l, torch.nn.Linear)])
    return out


def test_s_row_blocks_stop_at_the_s_columns(nfa):
    """The stacked pack's hidden-to-hidden items: the s row-blocks' k-group counts end at the s columns, the t row-blocks' at the t
    columns (prefix skipping over a block-diagonal weight), row-blocks beyond the nets carry none; a block's single MLP is dense."""
    from affine_wide_emulator import items_of
    from normflows_amd.flows import affine_wide_pack as awp

    def hidden_nkg(name):
        layer, _ = load_layer(nfa, name)
        blob, table = awp.pack(layer, cases.CASES[name]["d"])
        tab, hrb = items_of(table), int(table[3]) // 32
        out = np.zeros(hrb, dtype=np.int64)
        for w in range(8):
            out[w], out[hrb - 1 - w] = tab[w, 2, 0], tab[w, 3, 0]
            assert tab[w, 2, 1] == w and tab[w, 3, 1] == hrb - 1 - w
        return out, awp.slot_layers(layer, cases.CASES[name]["d"])
    nkg, sl = hidden_nkg("a")              # s: slots [0, 72) of a 96-slot block, t: [96, 168) reading h1 slots [96, 168); t's second layer is 40 wide
    assert sl["offs"] == {"s": 0, "t": 96} and sl["H"] == 168
    assert nkg.tolist() == [12, 12, 12, 24, 24, 0, 0, 0]       # 72 s columns -> 9 k-groups -> 12; 168 columns -> 21 -> 24; t rows [96, 136)
    nkg, sl = hidden_nkg("b")              # s: [0, 160), t: [160, 320)
    assert sl["offs"] == {"s": 0, "t": 160}
    assert nkg.tolist() == [20] * 5 + [40] * 5 + [0] * 6
    nkg, sl = hidden_nkg("c")              # one net of 264 units: dense over its own columns
    assert nkg.tolist() == [36] * 9 + [0] * 7
    nkg, sl = hidden_nkg("e")
    assert nkg.tolist() == [20] * 5 + [0] * 3


def test_eligibility_table(nfa):
    from normflows_amd.flows import affine_wide_pack as awp
    MLP, MAF, Block = nfa.nets.MLP, nfa.flows.MaskedAffineFlow, nfa.flows.AffineCouplingBlock
    alt = lambda d: torch.tensor([1.0 if i % 2 == 0 else 0.0 for i in range(d)])      # noqa: E731
    wide = lambda d, **kw: MLP([d, 72, 72, d], **kw)      # noqa: E731
    why = awp.supported
    assert why(MAF(alt(17), wide(17), wide(17)), 17) is None
    assert why(Block(MLP([9, 72, 72, 16])), 17) is None and why(Block(MLP([2, 65, 65, 2])), 3) is None       # narrow d, wide net
    for layer, d, word in (
            (MAF(alt(17), wide(17), wide(17, leaky=0.1)), 17, "slope 0.1"),
            (MAF(alt(17), wide(17), MLP([17, 72, 17])), 17, "1 hidden layers"),
            (MAF(alt(17), MLP([17, 72, 72, 72, 17]), None), 17, "3 hidden layers"),
            (MAF(alt(17), wide(17), wide(17)), 18, "17 entries"),
            (MAF(alt(17), MLP([17, 260, 260, 17]), MLP([17, 260, 260, 17])), 17, "548 hidden slots"),
            (MAF(alt(129), wide(129), None), 129, "d = 129"),
            (MAF(alt(16), MLP([16, 64, 64, 16]), MLP([16, 64, 64, 16])), 16, "chain"),
            (Block(MLP([8, 64, 64, 16])), 16, "chain"),
            (MAF(alt(17) * 0.5, wide(17), wide(17)), 17, "not binary"),
            (MAF(alt(17), wide(17), wide(17)).double(), 17, "float64"),
            (MAF(alt(17), wide(17).double(), wide(17)), 17, "float64"),
            (Block(MLP([9, 72, 72, 16]), split_mode="checkerboard"), 17, "checkerboard"),
            (MAF(alt(17), wide(17, output_fn="tanh"), None), 17, "plain nets.MLP"),
            (MAF(alt(17), wide(17, dropout=0.1), None), 17, "plain nets.MLP"),
            (Block(MLP([9, 72, 72, 8])), 17, "9 -> 16"),
            (Block(MLP([9, 72, 72, 16]), scale=False), 17, "9 -> 8"),
            (nfa.flows.ActNorm(17), 17, "neither")):
        got = why(layer, d)
        assert isinstance(got, str) and word in got, (word, got)
        assert awp.pack(layer, d) is None
    nobias = MAF(alt(17), wide(17), wide(17))
    nobias.s.net[2] = torch.nn.Linear(72, 72, bias=False)
    assert "without bias" in why(nobias, 17)
    x64 = torch.zeros(4, 17, dtype=torch.float64)
    assert "float64" in why(MAF(alt(17), wide(17), wide(17)), 17, x64)
    assert "shape" in why(MAF(alt(17), wide(17), wide(17)), 17, torch.zeros(4, 17, 1, 1))
    assert "GPU" in why(MAF(alt(17), wide(17), wide(17)), 17, torch.zeros(4, 17))


def test_symbol_is_declared_exported_bound_and_validates_its_arguments(nfa):
    declared = nfa._lib.exported_symbols_declared()
    lib = nfa._lib.lib()
    assert "nf_affine_wide" in declared and hasattr(lib, "nf_affine_wide") and hasattr(nfa.ops, "affine_wide")
    assert nfa._lib.prototypes_declared()["nf_affine_wide"][1][5] is ctypes.c_int64
    assert nfa.config.affine_wide is True
    nfa.config.set_affine_wide(False)
    assert nfa.config.affine_wide is False
    nfa.config.set_affine_wide(True)
    assert nfa.config.affine_wide is True
    gate = nfa.config.affine_wide_graph_min_batch
    assert gate == 16384 and nfa.config._graph_recording == 0
    nfa.config.set_affine_wide(True, graph_min_batch=0)
    assert nfa.config.affine_wide_graph_min_batch == 0
    nfa.config.set_affine_wide(True, graph_min_batch=gate)
    i32, i64, vp = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    null, one = vp(0), vp(16)

    def call(B=8, D=64, hp=512, direction=0, acc=0, z=one, y=one, ld=one, blob=one, table=one):
        return lib.nf_affine_wide(z, y, ld, blob, table, i64(B), i32(D), i32(hp), i32(direction), i32(acc), null)
    assert call(D=1) == -22 and call(D=129) == -22 and call(B=-1) == -22
    assert call(direction=2) == -22 and call(direction=-1) == -22 and call(acc=2) == -22 and call(acc=-2) == -22
    assert call(hp=128) == -95 and call(hp=384) == -95
    assert call(z=null) == -14 and call(y=null) == -14 and call(ld=null) == -14 and call(blob=null) == -14 and call(table=null) == -14
    assert call(B=0) == 0 and call(B=0, z=null, y=null, ld=null, blob=null, table=null) == 0 and call(B=0, hp=100) == -95
    assert call(z=vp(20)) == -22 and call(y=vp(24)) == -22            # D % 4 == 0: 16-byte rows
    assert call(D=17, z=null) == -14                                   # (a pointer check comes first whatever the row length)


def test_new_kernels_use_no_scratch(nfa):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    seen = 0
    for name, d in kr.resources(os.path.join(ROOT, "normalizing-flows_amd", "lib", "obj", "affine_wide.o")).items():
        assert "affine_wide_kernel" in name
        seen += 1
        assert d["vgpr_spill_count"] == 0 and d["private_segment_fixed_size"] == 0, (name, d)
    assert seen == 2, seen
