"""CPU tests of tests/wgrad_cases.py, the case table behind tests/test_gpu_wgrad_kernels.py: the restated launcher agrees with the
built library's own chunk arithmetic (nf_linear_wgrad_chunks / nf_linear_wgrad_scratch_floats are host-only queries) on every case
and on a sweep of shapes around every threshold; the table holds every path, every class of last chunk, every reduction regime and
every option on every path that accepts it; the restated reduction order sums what it is given; and the float32 yardstick's error,
printed per case as a fraction of the bar the GPU test will use, stays inside the existing bar."""
import os

import pytest
import torch

import wgrad_cases as wc


@pytest.fixture(scope="module")
def nfa():
    import __graft_entry__
    import normflows_amd
    if not os.path.exists(normflows_amd.native_library_path()):
        __graft_entry__.build()
    return normflows_amd


def test_issue_shapes_take_the_stated_plans():
    """SHAPES states (path, chunk rows, chunks, rows of the last chunk) per shape; the restated launcher gives exactly that."""
    for (B, M, N), want in wc.SHAPES.items():
        pl = wc.plan(B, M, N)
        assert (pl.path, pl.rows, pl.chunks, pl.last) == want, ((B, M, N), pl, want)
        assert B <= wc.MAX_ROWS
    assert all(c.B <= wc.MAX_ROWS and (c.B, c.M, c.N) in wc.SHAPES for c in wc.CASES)
    assert len({c.id for c in wc.CASES}) == len(wc.CASES)


def test_table_is_pinned_to_the_library_chunk_arithmetic(nfa):
    L = nfa._lib
    for c in wc.CASES:
        pl = c.plan()
        assert L.query("nf_linear_wgrad_chunks", c.B, c.M, c.N) == pl.chunks, c
        assert L.query("nf_linear_wgrad_scratch_floats", c.B, c.M, c.N) == pl.chunks * (c.M * c.N + c.M) == wc.scratch_floats(c.B, c.M, c.N), c
    # ... and around every threshold of the launcher: ring / tile / vec / general, the chunk-row roundings, the slot counts
    n = 0
    for M in (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 252, 255, 256, 257, 260, 384, 512, 768, 1024, 70000):
        for N in (1, 3, 4, 31, 32, 33, 64, 65, 92, 95, 96, 97, 100, 124, 127, 128):
            for B in (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 144, 1023, 1024, 1025, 4096, 8208, 16384, 16400, 50000, 65536, 65537, 131072, 1 << 20):
                pl = wc.plan(B, M, N)
                assert L.query("nf_linear_wgrad_chunks", B, M, N) == pl.chunks, (B, M, N, pl)
                assert L.query("nf_linear_wgrad_scratch_floats", B, M, N) == pl.chunks * (M * N + M), (B, M, N, pl)
                assert 1 <= pl.last <= pl.rows and (pl.chunks - 1) * pl.rows + pl.last == B
                n += 1
    assert n > 5000
    pl = wc.plan(65536, 768, 128)        # the one shape the ring ran at before: 82 chunks of 800 rows, the last 736 rows = 46 steps
    assert (pl.path, pl.rows, pl.chunks, pl.last, wc.ring_last_steps(pl)) == ("ring", 800, 82, 736, 46)


def test_every_path_last_chunk_class_and_reduction_regime_is_held():
    plain = [c for c in wc.CASES if c.opt == wc.DEFAULTS]
    assert {c.plan().path for c in plain} == set(wc.PATHS)
    for fam in wc.FAMILIES:
        pls = [c.plan() for c in plain if c.plan().family == fam]
        classes = {wc.last_class(pl) for pl in pls}
        # the ring takes B % 16 == 0 only: its last chunk holds whole 16-row steps
        assert classes >= ({"even", "full"} if fam == "ring" else {"one", "odd", "full"}), (fam, classes)
        assert any(pl.chunks == 1 for pl in pls) and any(pl.chunks > 1 for pl in pls), fam
        assert any(pl.chunks > 1 and wc.last_class(pl) == "full" for pl in pls), fam
    ring = [c.plan() for c in plain if c.plan().path == "ring"]
    steps = {wc.ring_last_steps(pl) for pl in ring}
    assert steps >= {1, 2, 3, 8}, steps                                   # fewer than, exactly and more than the W3_NR - 1 steps of look-ahead
    assert any(pl.chunks == 1 and wc.ring_last_steps(pl) < wc.W3_NR - 1 for pl in ring)        # a whole launch shorter than the ring is deep
    assert any(pl.chunks > 1 and wc.ring_last_steps(pl) == 1 for pl in ring)
    full = [c for c in wc.CASES if c.route == "full"]
    for bias in (0, 1):
        assert {c.plan().regime for c in full if c.want_bias == bias} == set(wc.REGIMES), bias
    # the unrolled loop taken four times plus a tail; one trip on SOME lanes only (49..63 chunks); one on every lane plus a tail
    assert any(c.plan().chunks > 4 * 64 and c.plan().chunks % 64 for c in plain)
    assert any(48 < c.plan().chunks < 64 for c in plain) and any(64 < c.plan().chunks < 80 for c in plain)
    # skip_every and accumulate inside the unrolled regime
    assert any(c.skip_every and c.accumulate and c.plan().regime == ">64" for c in full)


def test_every_option_runs_on_every_path_that_accepts_it():
    for fam in wc.FAMILIES:
        cs = wc.cases_of(fam)
        for multi in (False, True):
            sub = [c for c in cs if (c.plan().chunks > 1) == multi and not c.nonfinite]
            alone = lambda **o: any(c.opt == dict(wc.DEFAULTS, **o) for c in sub)
            assert alone(relu_x=1) and alone(want_bias=0) and alone(accumulate=1) and alone(pair=1), (fam, multi)
            assert alone(route="partials") and any(c.route == "partials" and not c.want_bias for c in sub), (fam, multi)
            if fam != "vec-odd" or multi:
                assert any(alone(skip_every=k) for k in (2, 3)), (fam, multi)
                assert any(c.relu_x and c.skip_every and c.accumulate for c in sub), (fam, multi)
        if fam != "vec-odd":      # (an odd M has no multiple of 24)
            assert any(c.skip_every == 24 and c.opt == dict(wc.DEFAULTS, skip_every=24) for c in cs), fam
        assert {c.nonfinite for c in cs} >= {"x_inf", "dy_nan", "x_nan"}, fam
        assert all(c.relu_x for c in cs if c.nonfinite == "x_nan")
    for c in wc.CASES:      # the issue's skip_every shapes
        if c.skip_every:
            assert c.M % c.skip_every == 0 and c.rows_out == c.M - c.M // c.skip_every
    assert {(c.M, c.N) for c in wc.CASES if c.skip_every} >= {(6, 8), (48, 64), (9, 5), (48, 33), (768, 128)}
    assert {(c.B, c.plan().path) for c in wc.CASES if c.skip_every == 24 and c.M == 768} == {(129, "tile"), (144, "ring")}


def test_relu_inputs_carry_both_zeros_and_negatives_in_the_last_row_of_every_chunk():
    for c in wc.CASES:
        if not c.relu_x:
            continue
        x = c.inputs()
        for b0, b1 in c.chunk_bounds():
            row = x["X"][b1 - 1]
            assert float(row[0]) == 0.0 and not bool(torch.signbit(row[0]))
            if c.N > 1:
                assert float(row[1]) == 0.0 and bool(torch.signbit(row[1]))
            if c.N > 2:
                assert bool((row[2:min(c.N, 6)] < 0).all())
    # cases of one shape share dY and X apart from those entries: the option identities compare like with like
    a, b = wc.Case(97, 48, 64).inputs(), wc.Case(97, 48, 64, accumulate=1, skip_every=24).inputs()
    assert torch.equal(a["dY"], b["dY"]) and torch.equal(a["X"], b["X"]) and b["prevW"].shape == (46, 64)


@pytest.mark.parametrize("chunks", [1, 2, 15, 16, 17, 33, 48, 49, 50, 63, 64, 65, 80, 127, 128, 129, 313])
def test_reduction_order_restated_sums_its_partial_tiles(chunks):
    """reduce_in_order is the documented order of wgrad_reduce_group in float32.  Here: it agrees with the float64 sum of random
    partial tiles to rounding (each element is a sum of `chunks` terms along chains of at most ceil(chunks / 64) + 3 + 2 + 16
    additions: |error| <= that many half-ulps of the running sums, bounded by the sum of |terms|), it reads every chunk exactly once
    (integer tiles sum exactly), and the chunk -> (lane, accumulator) map is the documented one."""
    g = torch.Generator().manual_seed(chunks)
    parts = torch.randn(chunks, 257, generator=g, dtype=torch.float64).float()
    got = wc.reduce_in_order(parts)
    assert got.dtype == torch.float32
    ref = parts.double().sum(0)
    depth = -(-chunks // 64) + 3 + 2 + wc.RL
    bound = depth * 2.0 ** -24 * parts.double().abs().sum(0)
    assert bool(((got.double() - ref).abs() <= bound).all()), float(((got.double() - ref).abs() / bound).max())
    ints = torch.randint(-1000, 1000, (chunks, 65), generator=g).float()
    old = torch.randint(-1000, 1000, (65,), generator=g).float()
    assert torch.equal(wc.reduce_in_order(ints), ints.sum(0)) and torch.equal(wc.reduce_in_order(ints, old), old + ints.sum(0))
    # the order itself, written out a second way: per lane, chunk c = q + 16 j goes to accumulator j % 4 while its group of four
    # (j - j % 4 .. + 3) is complete below `chunks`, to accumulator 0 otherwise
    total = torch.zeros(257)
    for q in range(wc.RL):
        mine = list(range(q, chunks, wc.RL))
        acc = [torch.zeros(257) for _ in range(4)]
        for j, c in enumerate(mine):
            whole = (j - j % 4) + 3 < len(mine)
            acc[j % 4 if whole else 0] = acc[j % 4 if whole else 0] + parts[c]
        total = total + ((acc[0] + acc[1]) + (acc[2] + acc[3]))
    assert torch.equal(got, total)
    assert wc.reduce_regime(chunks) == ("<=16" if chunks <= 16 else "17..48" if chunks <= 48 else "49..64" if chunks <= 64 else ">64")


def test_yardstick_error_as_a_fraction_of_the_bar():
    """Per case: the float64 reference is finite and the float32 yardstick's own error, printed in units of the existing bar (2e-5
    max|ref| + 1e-3 for dW, 1e-4 max|ref| + 1e-3 for db), stays below 1: the bar max(1, 4 x yardstick error) of the GPU test is at
    most 4 x the existing bar, and where the yardstick is below 0.25 the existing bar decides."""
    worst, decides = {}, []
    for c in wc.CASES:
        x = c.inputs()
        ref, yard = c.reference(x), c.yardstick(x)
        for what, r, y in zip(("dW", "db"), ref, yard):
            assert r.dtype == torch.float64 and y.dtype == torch.float32 and bool(torch.isfinite(r).all()), (c, what)
            assert r.shape == ((c.rows_out, c.N) if what == "dW" else (c.rows_out,))
            e = wc.scaled_error(y, r, what)
            print("WGRAD-YARD %s %s yardstick error / existing bar %.4f" % (c.id, what, e))
            assert e < 1.0, (c, what, e)
            fam = c.plan().family
            worst[fam, what] = max(worst.get((fam, what), 0.0), e)
            if wc.allowed(e) > 1.0:
                decides.append((c.id, what, e))
    print("worst float32 yardstick error / existing bar per path:", {"%s %s" % k: "%.4f" % v for k, v in sorted(worst.items())})
    print("cases whose bar the yardstick decides:", decides or "none")
