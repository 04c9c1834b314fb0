"""Case table of the weight-gradient kernels (csrc/wgrad.hip: nf_linear_wgrad, _act, _skip, _pair, _partials, and the fixed-order
reduction train_reduce.hpp::wgrad_reduce_group), importable without a GPU: tests/test_host_wgrad_cases.py checks the table against
the built library's own chunk arithmetic, tests/test_gpu_wgrad_kernels.py runs it.

A Case is (B, M, N, options).  From it follow
  plan()        Plan(path, family, rows, chunks, last, regime): which of the hand-specialised split-K kernels the launcher picks, its
                chunk rows, the number of chunks, the rows of the last chunk and the regime of the reduction's chunk-lane loop -- the
                launcher's conditions restated in pure Python below;
  inputs()      seeded CPU tensors, generated in float64 and rounded ONCE to float32, so that the float64 reference, the float32
                yardstick and the kernel read the same numbers (ReLU has no kink problem: all three clamp the same float32 values);
  reference()   dY64.T @ f(X64) and dY64.sum(0) in float64, f = clamp_min(0) under relu_x, rows m % skip_every == skip_every - 1
                deleted under skip_every, the previous contents added under accumulate;
  yardstick()   the same formula in float32 on the CPU: what a straightforward float32 evaluation loses.
reduce_in_order() is the documented summation order of wgrad_reduce_group in float32, one IEEE add at a time.

Options: relu_x, want_bias, accumulate, skip_every, pair (two problems in one launch), route ("full": partial launch + reduction;
"partials": nf_linear_wgrad_partials alone) and nonfinite ("x_inf": one +Inf in X, "dy_nan": one NaN in dY, "x_nan": one NaN in X
-- with relu_x, fmaxf turns it into 0 -- all three in the last row of the first chunk)."""
import zlib
from collections import namedtuple

import torch

# ---- launch constants, each with the line it was read from ---------------------------------------------------------------------------
W2_KS = 32            # wgrad.hip:214  batch rows per LDS tile of the tile kernel
W2_T = 128            # wgrad.hip:215  tile edge (M and N)
W3_KS = 16            # wgrad.hip:324  batch rows per ring step
W3_NR = 3             # wgrad.hip:316  ring slots: NR - 1 steps of look-ahead
W2_SLOTS = 512        # wgrad.hip:423  workgroups the tile / ring launch aims at
TILE_MIN_ROWS = 4 * W2_KS   # wgrad.hip:429
WG_MT = 4             # wgrad.hip:129  m-tiles (waves) per workgroup of the general kernel
VEC_STEP = 32         # wgrad.hip:90, :466  rows per trip of the vec kernel's loop; chunk rows are a multiple of it
MIN_ROWS = 64         # wgrad.hip:467
RING_MIN_M = 256      # wgrad.hip:480
TILE_MIN_M = 256      # wgrad.hip:490
N_MAX = 128           # wgrad.hip:556
RL = 16               # train_reduce.hpp:16  chunk lanes of a 64-element reduction group
ENOTSUP = -95         # nf_mi355x.h NF_ENOTSUP: what a pair launch on the general path returns (wgrad.hip:571)

Plan = namedtuple("Plan", "path family rows chunks last regime")
FAMILIES = ("ring", "tile", "vec-even", "vec-odd", "general")
PATHS = ("ring", "tile", "vec-even", "vec-odd", "general/NT=1", "general/NT=2", "general/NT=3", "general/NT=4")
REGIMES = ("<=16", "17..48", "49..64", ">64")
PAIR_FAMILIES = ("ring", "tile", "vec-even", "vec-odd")      # wgrad.hip:571: np == 2 && !tile && !vec -> NF_ENOTSUP


def _cdiv(a, b):
    return -(-a // b)


def wgrad_use_ring(B, M, N):
    """wgrad.hip:473-484."""
    return N == 128 and M % 128 == 0 and M >= RING_MIN_M and B % 16 == 0


def wgrad_use_tile(M, N):
    """wgrad.hip:486-492."""
    return 96 <= N <= 128 and N % 4 == 0 and M % 4 == 0 and M >= TILE_MIN_M


def wgrad_tile_chunk_rows(B, M):
    """wgrad.hip:420-431."""
    mt = _cdiv(M, W2_T)
    want = max(1, W2_SLOTS // mt)
    rows = _cdiv(_cdiv(B, want), W2_KS) * W2_KS
    return max(rows, TILE_MIN_ROWS)


def wgrad_chunk_rows(B, M, vec):
    """wgrad.hip:459-469."""
    mgroups = _cdiv(M, 64) if vec else _cdiv(M, 32)
    want = _cdiv(2048 if (vec and M > 256) else 1024, mgroups)
    rows = _cdiv(_cdiv(B, want), VEC_STEP) * VEC_STEP
    return max(rows, MIN_ROWS)


def reduce_regime(chunks):
    """The chunk-lane loop of wgrad_reduce_group (train_reduce.hpp:32-39) with RL = 16: lane q starts at chunk q; the 4-way unrolled
    loop runs while c + 48 < chunks, the tail loop takes the rest.  <= 16: lanes q >= chunks idle, one tail step at most; 17..48: the
    tail loop alone, up to three steps; 49..64: one unrolled trip on lanes q < chunks - 48 and a three-step tail on the others;
    > 64: the unrolled trip on every lane, then a tail (or a second trip) on some."""
    return REGIMES[0] if chunks <= RL else (REGIMES[1] if chunks <= 3 * RL else (REGIMES[2] if chunks <= 4 * RL else REGIMES[3]))


def plan(B, M, N):
    """wgrad.hip:559-601: the launcher's path choice, chunk rows and chunk count."""
    assert B >= 1 and M >= 1 and 1 <= N <= N_MAX
    vec = N % 4 == 0
    ring = wgrad_use_ring(B, M, N)
    tile = ring or wgrad_use_tile(M, N)
    rows = wgrad_tile_chunk_rows(B, M) if tile else wgrad_chunk_rows(B, M, vec)
    chunks = _cdiv(B, rows)
    if ring:
        path = "ring"
    elif tile:
        path = "tile"
    elif vec:
        path = "vec-even" if M % 2 == 0 else "vec-odd"
    else:
        path = "general/NT=%d" % _cdiv(N, 32)
    return Plan(path, path.split("/")[0], rows, chunks, B - (chunks - 1) * rows, reduce_regime(chunks))


def last_class(pl):
    """The class of the last chunk: `one` row, an `odd` count, a `full` chunk, or an `even` partial count."""
    return "one" if pl.last == 1 else ("full" if pl.last == pl.rows else ("odd" if pl.last % 2 else "even"))


def ring_last_steps(pl):
    """K-steps of the ring kernel's last chunk (wgrad.hip:341)."""
    assert pl.path == "ring" and pl.last % W3_KS == 0
    return pl.last // W3_KS


def scratch_floats(B, M, N):
    """wgrad.hip:494-503: what nf_linear_wgrad_scratch_floats returns."""
    return plan(B, M, N).chunks * (M * N + M)


# ---- the reduction order -----------------------------------------------------------------------------------------------------------
def reduce_in_order(parts, old=None):
    """wgrad_reduce_group (train_reduce.hpp:28-57) restated: parts (chunks, n) float32 -> (n) float32.  Lane q in 0..15 keeps four
    accumulators over chunks q, q + 16, q + 32, q + 48, stepping by 64 while c + 48 < chunks; the remaining chunks, stepping by 16,
    go into the first accumulator; the lane's sum is (s0 + s1) + (s2 + s3); the total is the sequential sum over lanes 0..15 from
    0.0f; the output is old + total when accumulating.  Every `+` below is one float32 addition of torch on the CPU."""
    assert parts.dtype == torch.float32 and parts.dim() == 2
    chunks, n = parts.shape
    total = torch.zeros(n, dtype=torch.float32)
    for q in range(RL):
        s = [torch.zeros(n, dtype=torch.float32) for _ in range(4)]
        c = q
        while c + 3 * RL < chunks:
            for k in range(4):
                s[k] = s[k] + parts[c + k * RL]
            c += 4 * RL
        while c < chunks:
            s[0] = s[0] + parts[c]
            c += RL
        total = total + ((s[0] + s[1]) + (s[2] + s[3]))
    return total if old is None else old + total


def keep_rows(M, skip_every):
    """Rows of the M that have an output row: m % skip_every != skip_every - 1 (train_reduce.hpp:48-51)."""
    return [m for m in range(M) if not skip_every or m % skip_every != skip_every - 1]


# ---- the case -----------------------------------------------------------------------------------------------------------------------
DEFAULTS = dict(relu_x=0, want_bias=1, accumulate=0, skip_every=0, pair=0, route="full", nonfinite=None)


class Case:
    def __init__(self, B, M, N, **opt):
        assert set(opt) <= set(DEFAULTS), opt
        self.B, self.M, self.N = B, M, N
        self.opt = dict(DEFAULTS, **opt)
        o = self.opt
        assert o["route"] in ("full", "partials") and o["nonfinite"] in (None, "x_inf", "dy_nan", "x_nan")
        assert not o["skip_every"] or (o["skip_every"] > 1 and M % o["skip_every"] == 0)
        if o["route"] == "partials":     # nf_linear_wgrad_partials has neither a reduction nor a second problem
            assert not (o["accumulate"] or o["skip_every"] or o["pair"])
        assert not (o["pair"] and o["skip_every"])      # nf_linear_wgrad_pair has no skip_every

    def __getattr__(self, k):
        if k != "opt" and k in self.opt:
            return self.opt[k]
        raise AttributeError(k)

    @property
    def id(self):
        o = self.opt
        tags = [k for k in ("relu_x", "accumulate", "pair") if o[k]]
        tags += ["nobias"] if not o["want_bias"] else []
        tags += ["skip%d" % o["skip_every"]] if o["skip_every"] else []
        tags += ["partials"] if o["route"] == "partials" else []
        tags += [o["nonfinite"]] if o["nonfinite"] else []
        return "-".join([self.plan().path.replace("/", "_"), "B%d" % self.B, "M%d" % self.M, "N%d" % self.N] + tags)

    def __repr__(self):
        return self.id

    def plan(self):
        return plan(self.B, self.M, self.N)

    @property
    def rows_out(self):
        return len(keep_rows(self.M, self.skip_every))

    def bad_entry(self):
        """(b*, m*, n*) of option `nonfinite`: the last row of the first chunk, a row and a column inside the tiles."""
        pl = self.plan()
        return min(pl.rows, self.B) - 1, (2 * self.M) // 3, (2 * self.N) // 3

    def inputs(self):
        """{dY, X (, dY1, X1) (, prevW, prevb (, prevW1, prevb1))}: float32 CPU tensors; the non-finite entry is NOT placed here (the
        GPU test places it, and compares with the run on these finite inputs)."""
        B, M, N, o = self.B, self.M, self.N, self.opt
        # (the seed leaves the options out: cases of one shape share their inputs, so that the option identities compare like with like)
        g = torch.Generator().manual_seed(zlib.crc32(("wgrad-%d-%d-%d" % (B, M, N)).encode()))
        rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).float()
        x = dict(dY=rn(B, M), X=rn(B, N), dY1=rn(B, M), X1=rn(B, N), prevW=rn(M, N), prevb=rn(M), prevW1=rn(M, N), prevb1=rn(M))
        if o["relu_x"]:
            pl = self.plan()
            for X in (x["X"], x["X1"]):
                for c in range(pl.chunks):              # the last row of every chunk: exact zeros of both signs and negative entries
                    r = min((c + 1) * pl.rows, B) - 1
                    X[r, 0] = 0.0
                    X[r, 1 % N] = -0.0 if N > 1 else X[r, 0]
                    for n in range(2, min(N, 6)):
                        X[r, n] = -X[r, n].abs() - 0.25
        Mo = self.rows_out
        for k in ("prevW", "prevW1"):
            x[k] = x[k][:Mo].contiguous()
        for k in ("prevb", "prevb1"):
            x[k] = x[k][:Mo].contiguous()
        drop = [k for k in x if (k.endswith("1") and not o["pair"]) or (k.startswith("prev") and not o["accumulate"])]
        return {k: v for k, v in x.items() if k not in drop}

    def _formula(self, x, dtype, problem=0):
        sfx = "1" if problem else ""
        dY, X = x["dY" + sfx].to(dtype), x["X" + sfx].to(dtype)
        if self.relu_x:
            X = X.clamp_min(0)
        keep = keep_rows(self.M, self.skip_every)
        dW, db = (dY.t() @ X)[keep], dY.sum(0)[keep]
        if self.accumulate:
            dW, db = x["prevW" + sfx].to(dtype) + dW, x["prevb" + sfx].to(dtype) + db
        return dW, db

    def reference(self, x, problem=0):
        """(dW, db) in float64."""
        return self._formula(x, torch.float64, problem)

    def yardstick(self, x, problem=0):
        """(dW, db) of the same formula in float32 on the CPU."""
        return self._formula(x, torch.float32, problem)

    def chunk_bounds(self):
        pl = self.plan()
        return [(c * pl.rows, min((c + 1) * pl.rows, self.B)) for c in range(pl.chunks)]

    def chunk_formula(self, x, dtype, problem=0):
        """Per chunk c: (dY[b0:b1].T @ f(X[b0:b1]), dY[b0:b1].sum(0)) as (chunks, M, N) and (chunks, M) in `dtype`."""
        sfx = "1" if problem else ""
        pl = self.plan()
        dY, X = x["dY" + sfx].to(dtype), x["X" + sfx].to(dtype)
        if self.relu_x:
            X = X.clamp_min(0)
        pad = pl.chunks * pl.rows - self.B      # zero rows add nothing to a chunk's sums
        dY = torch.cat([dY, dY.new_zeros(pad, self.M)]).view(pl.chunks, pl.rows, self.M)
        X = torch.cat([X, X.new_zeros(pad, self.N)]).view(pl.chunks, pl.rows, self.N)
        return torch.bmm(dY.transpose(1, 2), X), dY.sum(1)


# ---- bars ----------------------------------------------------------------------------------------------------------------------------
MARGIN = 4.0       # another summation order than the yardstick's: split-K chunks, MFMA accumulation, a 16-lane tree


def existing_bar(ref, what):
    """The bar tests/test_gpu_training.py::test_linear_wgrad_kernel holds the kernel to: 2e-5 max|ref| + 1e-3 (dW), 1e-4 max|ref| +
    1e-3 (db)."""
    scale = float(ref.abs().max()) if ref.numel() else 0.0
    return (2e-5 if what == "dW" else 1e-4) * scale + 1e-3


def scaled_error(got, ref, what):
    """max |got - ref| in units of the existing bar; a NaN in `got` counts as infinite."""
    e = (got.double() - ref).abs()
    return float(torch.nan_to_num(e, nan=float("inf")).max()) / existing_bar(ref, what)


def allowed(yard_err):
    """The bar of one output in units of the existing bar: the larger of that bar (1) and MARGIN x the float32 yardstick's own error."""
    return max(1.0, MARGIN * yard_err)


# ---- the table -----------------------------------------------------------------------------------------------------------------------
# (B, M, N) -> what the launcher is expected to do with it: (path, chunk rows, chunks, rows of the last chunk)
SHAPES = {
    # ring: last chunks of 1, 2 and 3 steps (fewer than, as many as and more than the NR - 1 = 2 steps of look-ahead), a single chunk
    (16, 256, 128): ("ring", 128, 1, 16), (144, 256, 128): ("ring", 128, 2, 16), (160, 256, 128): ("ring", 128, 2, 32),
    (176, 384, 128): ("ring", 128, 2, 48), (2064, 256, 128): ("ring", 128, 17, 16), (8208, 512, 128): ("ring", 128, 65, 16),
    (144, 768, 128): ("ring", 128, 2, 16),
    (256, 256, 128): ("ring", 128, 2, 128),        # added: no ring shape above ends on a FULL chunk behind another one
    # tile: B % 16 != 0 beside the ring's shapes; a third M-tile of 4 rows with N < 128
    (1, 256, 128): ("tile", 128, 1, 1), (129, 256, 128): ("tile", 128, 2, 1), (161, 260, 100): ("tile", 128, 2, 33),
    (4129, 256, 96): ("tile", 128, 33, 33), (2100, 256, 124): ("tile", 128, 17, 52),
    (129, 768, 128): ("tile", 128, 2, 1), (33, 256, 100): ("tile", 128, 1, 33),       # the option shapes
    (256, 256, 96): ("tile", 128, 2, 128),         # added: full last chunk
    # vec, even M
    (1, 4, 4): ("vec-even", 64, 1, 1), (7, 6, 8): ("vec-even", 64, 1, 7), (63, 64, 4): ("vec-even", 64, 1, 63),
    (64, 66, 124): ("vec-even", 64, 1, 64), (65, 130, 128): ("vec-even", 64, 2, 1), (1100, 64, 64): ("vec-even", 64, 18, 12),
    (1600, 24, 32): ("vec-even", 64, 25, 64), (2113, 192, 36): ("vec-even", 64, 34, 1),
    (97, 48, 64): ("vec-even", 64, 2, 33),                                             # the multi-chunk option shape
    # vec, odd M: with N % 4 == 0 the chunk stride M N + M is odd, every second partial tile starts off 16-byte alignment
    (97, 7, 12): ("vec-odd", 64, 2, 33), (3137, 33, 64): ("vec-odd", 64, 50, 1),
    (33, 7, 12): ("vec-odd", 64, 1, 33), (97, 9, 12): ("vec-odd", 64, 2, 33),          # the option shapes (M = 9: skip_every = 3)
    (128, 7, 12): ("vec-odd", 64, 2, 64),          # added: full last chunk
    # general, NT = 1..4
    (1, 1, 1): ("general/NT=1", 64, 1, 1), (2, 3, 5): ("general/NT=1", 64, 1, 2), (9, 31, 31): ("general/NT=1", 64, 1, 9),
    (3141, 32, 1): ("general/NT=1", 64, 50, 5), (71, 33, 33): ("general/NT=2", 64, 2, 7), (130, 129, 65): ("general/NT=3", 64, 3, 2),
    (77, 40, 97): ("general/NT=4", 64, 2, 13), (1100, 130, 127): ("general/NT=4", 64, 18, 12),
    (50000, 96, 70): ("general/NT=3", 160, 313, 80),
    (9, 9, 5): ("general/NT=1", 64, 1, 9), (71, 48, 33): ("general/NT=2", 64, 2, 7),   # the option shapes
    (128, 9, 5): ("general/NT=1", 64, 2, 64),      # added: full last chunk
    (7, 3, 65): ("general/NT=3", 64, 1, 7),        # added: the issue's NT = 3 shapes end on even chunks; the pair tail's odd last row
    (4100, 9, 5): ("general/NT=1", 64, 65, 4),     # added: the smallest tensors that reach > 64 chunks (with skip_every = 3 too)
}

# per family: (single-chunk shape, multi-chunk shape) the options run at, and the skip_every values of each
OPTION_SHAPES = {
    "ring": (((16, 256, 128), (2,)), ((144, 768, 128), (3, 24))),
    "tile": (((33, 256, 100), (2,)), ((129, 768, 128), (3, 24))),
    "vec-even": (((7, 6, 8), (3,)), ((97, 48, 64), (2, 24))),
    "vec-odd": (((33, 7, 12), ()), ((97, 9, 12), (3,))),
    "general": (((9, 9, 5), (3,)), ((71, 48, 33), (2, 24))),
}
NONFINITE_SHAPES = {"ring": (144, 256, 128), "tile": (129, 256, 128), "vec-even": (65, 130, 128), "vec-odd": (97, 7, 12),
                    "general": (71, 33, 33)}


def _table():
    T, seen = [], set()

    def add(shape, **opt):
        c = Case(*shape, **opt)
        if c.id not in seen:
            seen.add(c.id)
            T.append(c)

    for shape in SHAPES:
        add(shape)
    for fam, pairs in OPTION_SHAPES.items():
        for shape, skips in pairs:
            add(shape, relu_x=1)
            add(shape, want_bias=0)
            add(shape, accumulate=1)
            for k in skips:
                add(shape, skip_every=k)
            add(shape, pair=1)       # (the general path: the launcher must decline with NF_ENOTSUP and write nothing)
            add(shape, route="partials")
            add(shape, route="partials", want_bias=0, relu_x=1)
            if skips:
                add(shape, relu_x=1, skip_every=skips[-1], accumulate=1)
                add(shape, relu_x=1, skip_every=skips[-1], accumulate=1, want_bias=0)
    # the reduction regimes without db (and with skip_every / accumulate in the unrolled loop)
    add((2064, 256, 128), want_bias=0)                    # 17 chunks
    add((3137, 33, 64), want_bias=0)                      # 50
    add((3141, 32, 1), accumulate=1)                      # 50
    add((4100, 9, 5), want_bias=0)                        # 65
    add((4100, 9, 5), skip_every=3, accumulate=1, relu_x=1)
    add((8208, 512, 128), relu_x=1, pair=1)               # 65 chunks x 2 problems on the ring
    for fam, shape in NONFINITE_SHAPES.items():
        add(shape, nonfinite="x_inf")
        add(shape, nonfinite="dy_nan")
        add(shape, nonfinite="x_nan", relu_x=1)
        if fam in PAIR_FAMILIES:
            add(shape, nonfinite="x_inf", pair=1, relu_x=1)
    return T


CASES = _table()
MAX_ROWS = 50000      # the 65 536-row shapes are test_linear_wgrad_kernel's


def cases_of(family):
    return [c for c in CASES if c.plan().family == family]
