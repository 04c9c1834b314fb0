"""GPU tests (-m gpu) of the weight-gradient kernels of csrc/wgrad.hip on every path, option and chunk edge: the four split-K partial
kernels the launcher picks among, and the fixed-order reduction train_reduce.hpp::wgrad_reduce_group.  The cases, their float64
references and float32 yardsticks live in tests/wgrad_cases.py (pinned to the library's own chunk arithmetic on the CPU by
tests/test_host_wgrad_cases.py); this module runs them through the C ABI with buffers it owns, and through the `ops` wrappers where
they can express the case.

Inventory, re-derived from the launcher (wgrad.hip:551-609; "before": what a GPU test held to values before this module -- the nine
plain-option shapes of test_linear_wgrad_kernel, the three of test_linear_wgrad_pair_equals_two_single_launches, and whole-layer
tests at 1e-3 of each gradient's scale; "here": the shapes as (B, M, N) -> chunks x chunk rows, rows of the last chunk):

| kernel | condition | before | here |
|---|---|---|---|
| wgrad_ring_kernel (LDS-DMA ring, 16-row steps, 2 steps of look-ahead) | N == 128, M % 128 == 0, M >= 256, B % 16 == 0 | (65 536, 768, 128) only: 82 chunks of 800 rows, the last 46 steps | last chunks of 1, 2, 3 and 8 steps; a whole launch of ONE step (16, 256, 128); 1, 2, 17, 65 chunks; M 256 .. 768; every option, pairs at 2 and 65 chunks |
| wgrad_tile_kernel (LDS tiles, 32-row steps) | N in [96, 128], N % 4 == 0, M % 4 == 0, M >= 256, not the ring | (65 536, 736, 128), (4 099, 300, 100), (777, 768, 128), (33, 256, 96), pair (3 000, 768, 128) | B = 1 and 129 beside the ring's shapes; a third M-tile of 4 rows with N = 100; last chunks of 1, 33, 52, 128 rows; 1, 2, 17, 33 chunks; every option |
| wgrad_partial_vec_kernel<true, .> (8-byte dY loads) | N % 4 == 0, M even, otherwise | (65 536, 128, 128 or 32), pair (4 099, 64, 32) | M 4 .. 192, a second M-group of 2 rows, last chunks of 1, 7, 12, 33, 63, 64 rows; 1, 2, 18, 25, 34 chunks; every option |
| wgrad_partial_vec_kernel<false, .> (odd M: odd chunk stride, partial tiles off 16-byte alignment) | N % 4 == 0, M odd | (1 025, 5, 128) | M 7, 9, 33; last chunks of 1, 33, 64 rows; 1, 2, 50 chunks; every option |
| wgrad_partial_kernel<NT>, NT = 1 .. 4 | N % 4 != 0 | (4 099, 70, 33): NT = 2 | N 1 .. 127 on all four NT; idle waves; pair tail with an odd last row; last chunks of 1, 2, 4, 5, 7, 9, 12, 13, 64, 80 rows; 1 .. 313 chunks; every option; a pair is declined |
| wgrad_reduce_group | chunk-lane loop: <= 16 chunks (idle lanes), 17 .. 48 (tail loop only), 49 .. 64 (one unrolled trip on some lanes), > 64 | whatever the shapes above gave, accumulate = 0, skip_every at one shape inside a layer | 1, 2, 3, 17, 18, 25, 33, 34, 50, 65, 313 chunks with and without db; accumulate (never run on a GPU before: ops.py passes 0); skip_every 2, 3, 24; every result against the restated order, bit for bit |

Harness: scratch, dW and db live inside NaN-filled storages.  dW and db start 20 bytes into theirs (4-byte, not 8- or 16-byte
aligned: the header promises "any address") with guard floats on both sides, and the storage behind dW / db is as long as the
un-skipped output, so a row written at its un-compacted place shows.  Scratch is 16-byte aligned with a guard behind
chunks x (M N + M) floats (twice that for a pair).

Every case asserts
(a) dW and db against the float64 reference on all elements.  The bar is the larger of the bar test_linear_wgrad_kernel holds the
    kernel to (2e-5 max|ref| + 1e-3 for dW, 1e-4 max|ref| + 1e-3 for db) and 4 x the float32 yardstick's own error on that case
    (another summation order: split-K chunks, MFMA accumulation, a 16-lane tree);
(b) per chunk, on the `partials` route: every chunk's tile [c][0 : M N] against dY64[b0:b1].T @ f(X64[b0:b1]) and its bias part
    against dY64[b0:b1].sum(0), the same rule scaled to that chunk's own max|ref| -- a row counted in the wrong chunk, twice or not
    at all shows at the chunk; the bias part stays NaN with want_bias = 0;
(c) the guards of scratch, dW and db are untouched; with skip_every the outputs have M - M / skip_every rows and nothing behind
    them is written; with accumulate = 0 no NaN is left in dW / db;
(d) dW and db of the full route equal, bit for bit, wgrad_cases.reduce_in_order (the documented order of wgrad_reduce_group, in
    float32) applied to the partial tiles of the `partials` route on the same inputs, with the skip_every row mapping and the
    accumulate add; the scratch the full route leaves equals the `partials` route's;
(e) bit for bit: accumulate = 1 onto a random previous buffer = previous + result(accumulate = 0); skip_every = k = the skip_every
    = 0 result with rows m % k == k - 1 deleted; relu_x = 1 on X = relu_x = 0 on X.clamp_min(0) (-0.0 == 0.0); a pair = two single
    calls on the four pair-capable paths, NF_ENOTSUP with nothing written on the general path; two identical calls give identical
    bits; ops.linear_wgrad / ops.linear_wgrad_pair give the C ABI's bits;
(f) non-finite containment, one case per path: a +Inf in X[b*, n*] (b* the last row of the first chunk) makes column n* of dW
    non-finite and leaves every other column and all of db bit-equal to the finite run; a NaN in dY[b*, m*] likewise for row m* and
    db[m*]; with relu_x = 1 a NaN in X is consumed as 0 by fmaxf on ALL paths (torch.relu would keep it): bit-equal to the run with
    0.0 there;
(g) routing: nf_linear_wgrad_chunks gives the table's chunk count, and (b) holds with the table's chunk rows -- the ring at
    (144, 256, 128) and the tile kernel at (129, 256, 128) write the same partial layout.

Worst case of each path on an MI355X against the float64 reference: kernel error / bar, then kernel error / the float32
yardstick's own error (dW, db: (a); chunk: (b), the worse of tile and bias part).

| path     | dW error / bar | at                          | db error / bar | at                | chunk error / bar | at               | error / yardstick dW, db, chunk |
|----------|----------------|-----------------------------|----------------|-------------------|-------------------|------------------|---------------------------------|
| ring     | 0.015          | (144, 768, 128) accumulate  | 0.002          | (144, 768, 128) pair | 0.016          | (8 208, 512, 128) | 1.3, 2.1, 3.4                  |
| tile     | 0.014          | (129, 768, 128)             | 0.002          | (161, 260, 100)   | 0.015             | (4 129, 256, 96) | 1.0, 2.8, 3.1                   |
| vec even | 0.009          | (1 600, 24, 32)             | 0.001          | (1 600, 24, 32)   | 0.009             | (1 100, 64, 64)  | 1.5, 1.7, 3.3                   |
| vec odd  | 0.007          | (3 137, 33, 64)             | 0.001          | (3 137, 33, 64)   | 0.007             | (3 137, 33, 64)  | 1.2, 2.1, 4.2                   |
| general  | 0.009          | (50 000, 96, 70)            | 0.002          | (50 000, 96, 70)  | 0.022             | (50 000, 96, 70) | 1.4, 1.9, 4.5                   |

The existing bar decides on every case but one: dW of (50 000, 96, 70), where the host's float32 matrix product over 50 000 rows is
itself a little over 0.25 of the existing bar from float64 (the kernel: 0.036 of the yardstick's error), so 4 x the yardstick is
just above 1.  Against the existing bar alone every case stays below 0.03: these sums are short, and the 1e-3 absolute term is wide at
this scale -- what holds the kernels here is (b) at the chunk's own scale and the bit-for-bit checks (d) and (e).  Where a chunk is
3 to 4.5 times the yardstick's error, both are a few float32 ulps of a sum of 64 .. 160 products in different orders.

Run time on an MI355X: 161 tests in 4.3 to 4.7 s (slowest: the 65-chunk ring pair, 0.43 s).

Sensitivity: one-line mutations that only skip work or change a value, each built into a library of its own outside the
repository, run once and not kept.  New cases that fail; then what tests/test_gpu_training.py as it was before this module (187
tests) did on the same library:
  1 ring, the last step of a chunk with fewer than W3_NR - 1 steps skipped: 31 -- every ring case whose last chunk is one step
    (B = 16, 144, 2 064, 8 208, with every option) and the ring-versus-tile layout test.  Before: all 187 passed.
  2 vec, `live` tested against B instead of b1: 0, and 0 before -- the mutation changes no value: chunk rows are a multiple of the
    loop's 32-row trip (wgrad.hip:466), so only the LAST chunk has rows past its end, and there b1 == B.  In its place
  2b vec, `live` tested for the pair's first row only (b + 2 j < b1: the row behind an odd last row is counted): 53 -- every vec
    case, even and odd M, whose last chunk has an odd number of rows.  Before: 4 failed (test_linear_wgrad_kernel[1025-5-128] and
    three ragged-batch tests).
  3 general, the odd last row of the pair tail dropped: 29 -- every general-path case with an odd last chunk, on all four NT.
    Before: 1 failed (test_linear_wgrad_kernel[4099-70-33]).
  4 tile, ReLU not applied to xv[3]: 10 -- every tile case with relu_x, through the clamp identity (e), the references (a), (b)
    and the NaN-as-zero rule (f).  Before: all 187 passed.
  5 reduce, s3 left out of (s0 + s1) + (s2 + s3): 10 -- every case with more than 48 chunks (50, 65, 313; ring, vec odd, general;
    with and without db, pair, accumulate + skip_every).  Before: 14 failed (the 65 536-row shapes).
  6 reduce, accumulate ignored for elements e >= nW: 21 -- every accumulate case with a db, on all five paths.  Before: all 187
    passed.
"""
import ctypes

import pytest
import torch

import wgrad_cases as wc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
OFF = 5            # floats in front of dW / db inside their storages: 20 bytes
GUARD = 64         # NaN floats behind scratch; behind dW / db on top of the rows skip_every leaves out
NAN = float("nan")


@pytest.fixture(scope="module")
def nfa():
    import normflows_amd
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    assert normflows_amd.native_library_path().endswith("normalizing-flows_amd/lib/libnf_mi355x.so")
    normflows_amd._lib.lib()
    return normflows_amd


def same(a, b):
    """Bit equality that lets NaN equal NaN (and -0.0 equal 0.0)."""
    return (a.shape == b.shape and a.dtype == b.dtype and torch.equal(torch.isnan(a), torch.isnan(b))
            and torch.equal(torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0)))


def _p(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _sync():
    if DEV != "cpu":
        torch.cuda.synchronize()


# ---- the three calls of the C ABI, on tensors ---------------------------------------------------------------------------------------
def abi_partials(L, dY, X, scratch, B, M, N, relu, wb):
    return L.call_rc("nf_linear_wgrad_partials", _p(dY), _p(X), _p(scratch), B, M, N, relu, wb, L.stream())


def abi_single(L, dY, X, dW, db, scratch, B, M, N, acc, relu, skip):
    """nf_linear_wgrad_skip, or the narrower entry point that can express the call (all three are exercised)."""
    if skip:
        return L.call_rc("nf_linear_wgrad_skip", _p(dY), _p(X), _p(dW), _p(db), _p(scratch), B, M, N, acc, relu, skip, L.stream())
    if relu:
        return L.call_rc("nf_linear_wgrad_act", _p(dY), _p(X), _p(dW), _p(db), _p(scratch), B, M, N, acc, relu, L.stream())
    return L.call_rc("nf_linear_wgrad", _p(dY), _p(X), _p(dW), _p(db), _p(scratch), B, M, N, acc, L.stream())


def abi_pair(L, dY0, X0, dW0, db0, dY1, X1, dW1, db1, scratch, B, M, N, acc, relu):
    return L.call_rc("nf_linear_wgrad_pair", _p(dY0), _p(X0), _p(dW0), _p(db0), _p(dY1), _p(X1), _p(dW1), _p(db1), _p(scratch), B, M, N,
                     acc, relu, L.stream())


def _scratch(L, shape, problems):
    B, M, N = shape
    chunks = L.query("nf_linear_wgrad_chunks", B, M, N)
    n = L.query("nf_linear_wgrad_scratch_floats", B, M, N)
    assert n == chunks * (M * N + M)
    buf = torch.full((problems * n + GUARD,), NAN, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    return buf, chunks, n


def partials(L, shape, dY, X, relu, wb):
    """The (chunks, M N + M) partial tiles nf_linear_wgrad_partials writes; (c) for the scratch."""
    B, M, N = shape
    buf, chunks, n = _scratch(L, shape, 1)
    rc = abi_partials(L, dY, X, buf, B, M, N, relu, wb)
    _sync()
    assert rc == 0, rc
    out = buf.cpu()
    assert bool(torch.isnan(out[n:]).all()), "%s: a write behind the scratch's chunks x (M N + M) floats" % (shape,)
    return out[:n].view(chunks, M * N + M)


def full(L, shape, probs, relu=0, wb=1, acc=0, skip=0, prev=None, expect_rc=0):
    """One full-route call (partial launch + reduction) on one problem or a pair; (c) for scratch, dW and db.
    -> dict(dW=[(Mo, N) per problem], db=[(Mo) or None], parts=(problems, chunks, M N + M)), all on the CPU."""
    B, M, N = shape
    npb = len(probs)
    Mo = len(wc.keep_rows(M, skip))
    buf, chunks, n = _scratch(L, shape, npb)
    wbuf = [torch.full((OFF + M * N + GUARD,), NAN, dtype=torch.float32, device=DEV) for _ in probs]
    bbuf = [torch.full((OFF + M + GUARD,), NAN, dtype=torch.float32, device=DEV) for _ in probs]
    dW = [w[OFF:OFF + Mo * N] for w in wbuf]
    db = [b[OFF:OFF + Mo] if wb else None for b in bbuf]
    for t in dW + [b for b in db if b is not None]:
        assert t.data_ptr() % 4 == 0 and t.data_ptr() % 8 != 0       # "any address"
    if acc:
        for p in range(npb):
            dW[p].copy_(prev[p][0].reshape(-1))
            if wb:
                db[p].copy_(prev[p][1])
    if npb == 1:
        rc = abi_single(L, probs[0][0], probs[0][1], dW[0], db[0], buf, B, M, N, acc, relu, skip)
    else:
        assert not skip
        rc = abi_pair(L, probs[0][0], probs[0][1], dW[0], db[0], probs[1][0], probs[1][1], dW[1], db[1], buf, B, M, N, acc, relu)
    _sync()
    assert rc == expect_rc, (shape, rc, expect_rc)
    sc = buf.cpu()
    wcpu, bcpu = [w.cpu() for w in wbuf], [b.cpu() for b in bbuf]
    if rc != 0:          # declined: nothing may have been written anywhere
        assert bool(torch.isnan(sc).all()) and all(bool(torch.isnan(w).all()) for w in wcpu) and all(bool(torch.isnan(b).all()) for b in bcpu)
        return None
    assert bool(torch.isnan(sc[npb * n:]).all()), "%s: a write behind the scratch" % (shape,)
    for w, b in zip(wcpu, bcpu):
        assert bool(torch.isnan(w[:OFF]).all()) and bool(torch.isnan(w[OFF + Mo * N:]).all()), "%s: a write outside dW's %d rows" % (shape, Mo)
        assert bool(torch.isnan(b[:OFF]).all()) and bool(torch.isnan(b[OFF + Mo:]).all()), "%s: a write outside db's %d rows" % (shape, Mo)
        assert wb or bool(torch.isnan(b).all()), "%s: db written without a db" % (shape,)
    return dict(dW=[w[OFF:OFF + Mo * N].view(Mo, N) for w in wcpu], db=[b[OFF:OFF + Mo] if wb else None for b in bcpu],
                parts=sc[:npb * n].view(npb, chunks, M * N + M))


def same_result(a, b):
    return all(same(x, y) for x, y in zip(a["dW"], b["dW"])) and all((x is None and y is None) or same(x, y) for x, y in zip(a["db"], b["db"]))


def via_ops(nfa, c, probs):
    """The same case through ops.linear_wgrad / ops.linear_wgrad_pair (accumulate = 0 only; the pair wrapper always wants db)."""
    ops = nfa.ops
    if c.pair:
        w0, b0, w1, b1 = ops.linear_wgrad_pair(probs[0][0], probs[0][1], probs[1][0], probs[1][1], relu_x=bool(c.relu_x))
        _sync()
        return dict(dW=[w0.cpu(), w1.cpu()], db=[b0.cpu(), b1.cpu()])
    w, b = ops.linear_wgrad(probs[0][0], probs[0][1], want_bias=bool(c.want_bias), relu_x=bool(c.relu_x), skip_every=c.skip_every)
    _sync()
    return dict(dW=[w.cpu()], db=[None if b is None else b.cpu()])


# ---- (b) ------------------------------------------------------------------------------------------------------------------------------
def check_chunks(c, x, problem, parts):
    """Every chunk's tile and bias part against the float64 product of that chunk's rows; -> worst (error / bar, error / yardstick)."""
    M, N, pl = c.M, c.N, c.plan()
    assert parts.shape == (pl.chunks, M * N + M), (c, parts.shape)
    refW, refb = c.chunk_formula(x, torch.float64, problem)
    yW, yb = c.chunk_formula(x, torch.float32, problem)
    worst = [0.0, 0.0]
    for what, got, ref, yard, rel in (("dW", parts[:, :M * N].reshape(pl.chunks, -1), refW.reshape(pl.chunks, -1), yW.reshape(pl.chunks, -1), 2e-5),
                                      ("db", parts[:, M * N:], refb, yb, 1e-4)):
        if what == "db" and not c.want_bias:
            assert bool(torch.isnan(got).all()), "%s: the bias part of a partial tile was written with want_bias = 0" % c
            continue
        bar = rel * ref.abs().amax(1) + 1e-3                       # the existing rule at the chunk's own scale
        err = torch.nan_to_num((got.double() - ref).abs(), nan=float("inf")).amax(1) / bar
        yerr = (yard.double() - ref).abs().amax(1) / bar
        ok = err <= torch.clamp(wc.MARGIN * yerr, min=1.0)
        assert bool(ok.all()), "%s problem %d: %s part of chunk %d (rows %s) is %.3g x its bar from the float64 product of its rows" % (
            c, problem, what, int((~ok).nonzero()[0]), c.chunk_bounds()[int((~ok).nonzero()[0])], float(err[~ok][0]))
        worst[0] = max(worst[0], float((err / torch.clamp(wc.MARGIN * yerr, min=1.0)).max()))
        worst[1] = max(worst[1], float(torch.where(yerr > 0, err / yerr.clamp_min(1e-30), torch.zeros_like(err)).max()))
    return worst


def check_reference(c, x, problem, got):
    """(a): -> {what: (error / bar, error / yardstick, whether the yardstick decided the bar)}."""
    ref, yard = c.reference(x, problem), c.yardstick(x, problem)
    out = {}
    for what, g, r, y in (("dW", got["dW"][problem], ref[0], yard[0]), ("db", got["db"][problem], ref[1], yard[1])):
        if g is None:
            continue
        assert g.shape == r.shape and g.dtype == torch.float32, (c, what, g.shape, r.shape)
        assert not bool(torch.isnan(g).any()), "%s: NaN left in %s" % (c, what)                                   # (c)
        err, yerr = wc.scaled_error(g, r, what), wc.scaled_error(y, r, what)
        bar = wc.allowed(yerr)
        print("WGRAD %s problem %d %s err/bar %.4f err/yardstick %s%s" % (c.id, problem, what, err / bar, "%.3f" % (err / yerr) if yerr > 0 else "-",
                                                                          " (the yardstick decides)" if bar > 1.0 else ""))
        assert err <= bar, "%s %s: error %.3f x the existing bar, allowed %.3f (float32 yardstick %.3f)" % (c, what, err, bar, yerr)
        out[what] = (err / bar, err / yerr if yerr > 0 else 0.0, bar > 1.0)
    return out


def restated(c, x, problem, parts):
    """(d): the documented reduction order applied to one problem's partial tiles -> (dW, db or None)."""
    M, N = c.M, c.N
    keep = wc.keep_rows(M, c.skip_every)
    red = wc.reduce_in_order(parts[:, :M * N + (M if c.want_bias else 0)].contiguous())
    dW, db = red[:M * N].view(M, N)[keep], (red[M * N:][keep] if c.want_bias else None)
    if c.accumulate:
        sfx = "1" if problem else ""
        dW = x["prevW" + sfx] + dW
        db = None if db is None else x["prevb" + sfx] + db
    return dW, db


@pytest.mark.parametrize("c", wc.CASES, ids=lambda c: c.id)
def test_wgrad_case(nfa, c):
    L = nfa._lib
    B, M, N, pl = c.B, c.M, c.N, c.plan()
    shape = (B, M, N)
    assert L.query("nf_linear_wgrad_chunks", B, M, N) == pl.chunks                                                # (g)
    x = c.inputs()
    xd = {k: v.to(DEV) for k, v in x.items()}
    sfxs = ("", "1") if c.pair else ("",)
    probs = [(xd["dY" + s], xd["X" + s]) for s in sfxs]
    prev = [(x["prevW" + s], x["prevb" + s]) for s in sfxs] if c.accumulate else None

    # the `partials` route, per problem: (b), (g)
    parts = [partials(L, shape, dY, X, c.relu_x, c.want_bias) for dY, X in probs]
    for p in range(len(probs)):
        w = check_chunks(c, x, p, parts[p])
        print("WGRAD %s problem %d chunks: worst err/bar %.4f err/yardstick %.3f" % (c.id, p, w[0], w[1]))
    if c.route == "partials":
        assert same(partials(L, shape, probs[0][0], probs[0][1], c.relu_x, c.want_bias), parts[0]), "%s: two calls differ" % c
        return
    if c.pair and pl.family not in wc.PAIR_FAMILIES:
        full(L, shape, probs, relu=c.relu_x, wb=c.want_bias, expect_rc=wc.ENOTSUP)
        with pytest.raises(NotImplementedError):
            via_ops(nfa, c, probs)
        return

    memo = {}

    def R(relu=c.relu_x, skip=c.skip_every, acc=c.accumulate, pair=c.pair, clamp=False, only=None, inputs=None):
        """The full route with some options taken back (memoised): the right-hand sides of the identities (e)."""
        key = (relu, skip, acc, pair, clamp, only, id(inputs))
        if key not in memo:
            pr = probs if inputs is None else inputs
            if only is not None:
                pr = [pr[only]]
            if clamp:
                pr = [(dY, X.clamp_min(0)) for dY, X in pr]
            pv = None if not acc else (prev if only is None else [prev[only]])
            memo[key] = full(L, shape, pr, relu=relu, wb=c.want_bias, acc=acc, skip=skip, prev=pv)
        return memo[key]

    got = R()
    assert same_result(got, full(L, shape, probs, relu=c.relu_x, wb=c.want_bias, acc=c.accumulate, skip=c.skip_every, prev=prev)), \
        "%s: two identical calls differ" % c                                                                      # (e)
    for p in range(len(probs)):
        assert same(got["parts"][p], parts[p]), "%s problem %d: the full route's partial tiles differ from the partials route's" % (c, p)
        wantW, wantb = restated(c, x, p, parts[p])                                                                # (d)
        assert torch.equal(got["dW"][p], wantW), "%s problem %d: %d elements of dW differ from the documented reduction order" % (
            c, p, int((got["dW"][p] != wantW).sum()))
        assert (wantb is None and got["db"][p] is None) or torch.equal(got["db"][p], wantb), "%s problem %d: db differs from the documented reduction order" % (c, p)
        check_reference(c, x, p, got)                                                                             # (a), (c)

    # (e) option identities, each taking ONE option back
    if c.accumulate:
        base = R(acc=0)
        for p in range(len(probs)):
            assert torch.equal(got["dW"][p], prev[p][0] + base["dW"][p]), "%s: accumulate != previous + result" % c
            assert got["db"][p] is None or torch.equal(got["db"][p], prev[p][1] + base["db"][p]), "%s: accumulate (db) != previous + result" % c
    if c.skip_every:
        keep = wc.keep_rows(M, c.skip_every)
        a, b = R(acc=0), R(acc=0, skip=0)
        assert a["dW"][0].shape == (len(keep), N) and torch.equal(a["dW"][0], b["dW"][0][keep]), "%s: skip_every != rows deleted" % c
        assert a["db"][0] is None or torch.equal(a["db"][0], b["db"][0][keep]), "%s: skip_every (db) != rows deleted" % c
    if c.relu_x:
        assert same_result(R(acc=0, skip=0), R(acc=0, skip=0, relu=0, clamp=True)), "%s: relu_x = 1 on X != relu_x = 0 on X.clamp_min(0)" % c
    if c.pair:
        for p in range(2):
            one = R(acc=0, pair=0, only=p)
            two = R(acc=0)
            assert torch.equal(two["dW"][p], one["dW"][0]) and (one["db"][0] is None or torch.equal(two["db"][p], one["db"][0])), \
                "%s: problem %d of the pair != the single call" % (c, p)
            assert same(two["parts"][p], one["parts"][0])
    if not c.accumulate and (c.want_bias or not c.pair):
        assert same_result(got, via_ops(nfa, c, probs)), "%s: the ops wrapper's bits differ from the C ABI's" % c

    # (f) non-finite containment
    if c.nonfinite:
        bs, ms, ns = c.bad_entry()
        assert 0 <= bs < B and 0 <= ms < M and 0 <= ns < N and bool((x["dY"][bs] != 0).all()) and bool((x["X"][bs] != 0).any())
        dYb, Xb = probs[0][0].clone(), probs[0][1].clone()
        if c.nonfinite == "dy_nan":
            dYb[bs, ms] = NAN
        else:
            Xb[bs, ns] = float("inf") if c.nonfinite == "x_inf" else NAN
        badp = [(dYb, Xb)] + probs[1:]
        bad = R(inputs=badp)
        if c.nonfinite == "x_nan":        # fmaxf(NaN, 0) = 0: the NaN is consumed as a zero, on every path alike
            assert c.relu_x
            Xz = probs[0][1].clone()
            Xz[bs, ns] = 0.0
            zero = [(probs[0][0], Xz)] + probs[1:]
            assert same_result(bad, R(inputs=zero)), "%s: a NaN under relu_x is not consumed as 0" % c
            assert not any(bool(torch.isnan(t).any()) for t in bad["dW"])
        else:
            gW, gb, fW, fb = bad["dW"][0], bad["db"][0], got["dW"][0], got["db"][0]
            if c.nonfinite == "x_inf":
                hit = torch.zeros(M, N, dtype=torch.bool)
                hit[:, ns] = True
                assert torch.equal(gb, fb), "%s: db moved with an Inf in X" % c
            else:
                hit = torch.zeros(M, N, dtype=torch.bool)
                hit[ms] = True
                assert bool(torch.isnan(gb[ms])) and torch.equal(gb[torch.arange(M) != ms], fb[torch.arange(M) != ms]), "%s: db outside row m*" % c
            assert not bool(torch.isfinite(gW[hit]).any()), "%s: finite entries where the non-finite operand entered" % c
            assert torch.equal(gW[~hit], fW[~hit]), "%s: %d entries outside the non-finite operand's row / column moved" % (c, int((gW[~hit] != fW[~hit]).sum()))
            for p in range(1, len(probs)):      # the pair's other problem
                assert torch.equal(bad["dW"][p], got["dW"][p]) and torch.equal(bad["db"][p], got["db"][p]), "%s: the second problem moved" % c


def test_ring_and_tile_write_the_same_partial_layout(nfa):
    """(g): (144, 256, 128) takes the ring, (129, 256, 128) the tile kernel (B % 16 != 0); both split into 128-row chunks and pass
    (b).  On their shared first 128 rows the chunk-0 tiles of the two kernels agree to the bar of (b) (not bit for bit: K-steps of 16
    against 32 rows)."""
    L = nfa._lib
    ring, tile = wc.Case(144, 256, 128), wc.Case(129, 256, 128)
    assert (ring.plan().path, tile.plan().path, ring.plan().rows, tile.plan().rows) == ("ring", "tile", 128, 128)
    x = ring.inputs()
    xr = {k: v.to(DEV) for k, v in x.items()}
    pr = partials(L, (144, 256, 128), xr["dY"], xr["X"], 0, 1)
    check_chunks(ring, x, 0, pr)
    xt = {k: v[:129].contiguous() for k, v in x.items()}
    pt = partials(L, (129, 256, 128), xt["dY"].to(DEV), xt["X"].to(DEV), 0, 1)
    check_chunks(tile, xt, 0, pt)          # (the tile case on the ring case's first 129 rows)
    ref = xt["dY"][:128].double().t() @ xt["X"][:128].double()
    for got in (pr[0, :256 * 128], pt[0, :256 * 128]):
        assert wc.scaled_error(got.view(256, 128), ref, "dW") <= 1.0
    assert L.query("nf_linear_wgrad_chunks", 144, 256, 128) == 2 == L.query("nf_linear_wgrad_chunks", 129, 256, 128)
