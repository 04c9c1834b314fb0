"""Builders of the mixed layer stacks of tests/test_gpu_mixed_stacks.py.  Test infrastructure; importing it needs no GPU.

Every builder returns (model, expected).  `expected` is written by hand from the router's rules ("The chain router's
rules", R1-R9 below refer to that table) and never from a run:

  inference stacks   {"fwd": segments, "inv": segments}; a segment is (lo, hi, [C-ABI entry points]) -- the flows [lo, hi) of the
                     list as the router hands them to ONE kernel family, in PROCESSING order (the inverse pass walks the list from
                     its end), with the compute entry points (COMPUTE below) that segment calls, in order;
  RealNVP training   {"fwd": [[indices of a fused run] ...], "inv": ..., "layerwise": (MaskedAffineFn calls, ActNormFn calls)};
  pair training      {"packs": [...], "pass": [...]}: the C-ABI calls (TRAIN below) of one forward_kld forward pass.
"""
import torch

from test_gpu_realnvp_train import small_model
from test_gpu_views import DEV, perturbed

CHAIN, CHAIN_X3, PAIR1, WIDE, CIRC = "nf_rqs_fused_chain", "nf_rqs_fused_x3_chain", "nf_rqs_fused", "nf_nsf_wide_k", "nf_nsf_wide_ft"
LU1, RNVP, MAF1, ACT1 = "nf_rows_matvec_affine", "nf_realnvp_chain", "nf_masked_affine", "nf_actnorm"
MADE_AFFINE, MAF_INV, MADE_SPLINE, ARNSF_INV = "nf_made_forward_affine", "nf_maf_inverse", "nf_made_forward_spline", "nf_arnsf_inverse"
# the three kernels behind ops.maf_inverse (one launch each; which one is the pack's business, not the router's)
ALIAS = {"nf_maf_inverse_h": MAF_INV, "nf_maf_inverse_h_tri": MAF_INV}
# every entry point that computes a layer (or several) at inference: one-launch ones and what the layer-wise paths call instead
COMPUTE = {CHAIN, CHAIN_X3, PAIR1, "nf_rqs_fused_x3", WIDE, CIRC, LU1, "nf_lu_linear_permute", RNVP, MAF1, ACT1, MADE_AFFINE, MAF_INV,
           MADE_SPLINE, ARNSF_INV, "nf_made_forward_spline_ft", "nf_arnsf_inverse_ft", "nf_rqs_coupling", "nf_rqs_coupling_ft",
           "nf_made_forward", "nf_maf_affine", "nf_rows_matvec", "nf_rows_matvec2", "nf_nsf_wide_ctx"}
# ... and of a differentiable density pass of spline pairs
TRAIN = {"nf_rqs_fused_pack_all_multi", "nf_lu_factors_multi", "nf_lu_pack_train_multi", "nf_rqs_fused_train_pair_fwd",
         "nf_rqs_fused_train_full_fwd", "nf_rqs_fused_pack_all", "nf_lu_factors", "nf_lu_fwd", "nf_rows_matvec2", "nf_rqs_coupling",
         "nf_rqs_fused_train_fwd", "nf_lu_linear_permute", LU1}


def names(segments):
    return [n for _, _, ns in segments for n in ns]


def reversed_segments(segments):
    return [(lo, hi, list(ns)) for lo, hi, ns in reversed(segments)]


def _model(nfa, D, flows, seed, sigma):
    m = nfa.NormalizingFlow(nfa.distributions.DiagGaussian(D, trainable=False), flows)
    return perturbed(m, seed, sigma).to(DEV).eval()


def _initialised(flows):
    for f in flows:
        if hasattr(f, "data_dep_init_done"):
            f.data_dep_init_done.fill_(1.0)
    return flows


def _pair(nfa, D, blocks, hidden, K=8, reverse=False):
    """Identity initialisation; the builders perturb every parameter afterwards (sigma 0.03 .. 0.05).  A stack of tens of layers
    stays well conditioned this way: with random LU factors the sampling direction of 66 pairs amplifies a float32 rounding error by
    1e17 and a round trip says nothing."""
    return [nfa.flows.CoupledRationalQuadraticSpline(D, blocks, hidden, num_bins=K, init_identity=True, reverse_mask=reverse),
            nfa.flows.LULinearPermute(D, identity_init=True)]


# ---- inference ---------------------------------------------------------------------------------------------------------------------
def narrow_pairs(nfa, pairs=66, seed=41):
    """I1 / I2: `pairs` x [CRQS(6, 1 block, 32 hidden, 8 bins), LU(6)], alternating mask parity.  R1, R2: consecutive pairs of one
    signature are one segment, cut every 64 pairs IN PROCESSING ORDER -- the inverse pass takes the LAST 64 pairs first."""
    torch.manual_seed(seed)
    flows = [f for i in range(pairs) for f in _pair(nfa, 6, 1, 32, reverse=bool(i & 1))]
    return _model(nfa, 6, flows, seed + 1, 0.05), narrow_pairs_expected(pairs)


def narrow_pairs_expected(pairs, entry=CHAIN):
    n = 2 * pairs
    cut = 2 * 64
    if pairs <= 64:
        fwd = [(0, n, [entry])]
        return {"fwd": fwd, "inv": reversed_segments(fwd)}
    assert pairs == 66      # 64 + 2: both chunks have two pairs or more, so both are chains (R3: a chunk of one pair would not be)
    return {"fwd": [(0, cut, [entry]), (cut, n, [entry])], "inv": [(n - cut, n, [entry]), (0, n - cut, [entry])]}


def prefix(nfa, model, pairs):
    """The first `pairs` pairs of `model` as a model of their own (the same modules)."""
    return nfa.NormalizingFlow(model.q0, list(model.flows)[:2 * pairs]).eval()


def signature_changes(nfa, seed=43):
    """I3, D = 64.  R1: `pending` is flushed where _pair_signature changes; R3: a segment of one pair is nf_rqs_fused with the LU stage;
    R4: pairs beyond the benchmark kernel (hidden 256) go pair by pair to nf_nsf_wide_k."""
    torch.manual_seed(seed)
    flows = (_pair(nfa, 64, 2, 128) + _pair(nfa, 64, 2, 128, reverse=True) + _pair(nfa, 64, 1, 64) + _pair(nfa, 64, 1, 64, reverse=True)
             + _pair(nfa, 64, 1, 64, K=4) + _pair(nfa, 64, 2, 256) + _pair(nfa, 64, 2, 256, reverse=True))
    fwd = [(0, 4, [CHAIN]), (4, 8, [CHAIN]), (8, 10, [PAIR1]), (10, 14, [WIDE, WIDE])]
    return _model(nfa, 64, flows, seed + 1, 0.03), {"fwd": fwd, "inv": reversed_segments(fwd)}


def orphans(nfa, seed=47):
    """I4, D = 16: [LU, CRQS, LU, CRQS, CRQS, LU, Permute, CRQS].  R5: a pair is a CRQS with the LU BEHIND it in list order, whichever
    end the walk starts from: (1, 2) and (4, 5) in both directions; the LU at 0, the CRQS at 3 and 7 and the Permute run alone (R9)."""
    torch.manual_seed(seed)
    c = lambda rev=False: _pair(nfa, 16, 1, 32, reverse=rev)[0]  # noqa: E731
    lu = lambda: _pair(nfa, 16, 1, 32)[1]  # noqa: E731
    flows = [lu(), c(), lu(), c(True), c(), lu(), nfa.flows.Permute(16, mode="shuffle"), c(True)]
    fwd = [(0, 1, [LU1]), (1, 3, [PAIR1]), (3, 4, [PAIR1]), (4, 6, [PAIR1]), (6, 7, []), (7, 8, [PAIR1])]
    return _model(nfa, 16, flows, seed + 1, 0.05), {"fwd": fwd, "inv": reversed_segments(fwd)}


def _maf(nfa, d, width, i, leaky=0.05):
    b = torch.tensor([1.0, 0.0] * ((d + 1) // 2))[:d]
    return nfa.flows.MaskedAffineFlow(b if i % 2 == 0 else 1 - b, nfa.nets.MLP([d, width, d], init_zeros=True),
                                      nfa.nets.MLP([d, width, d], leaky=leaky, init_zeros=True))


def realnvp_runs(nfa, seed=53):
    """I5, d = 4.  R6: maximal runs of records; R7: a run of fewer than two records (the ActNorm at 9) and an ineligible layer (an MLP
    of width 65) go layer by layer; the Permute ends a run."""
    torch.manual_seed(seed)
    A, C = nfa.flows.ActNorm, nfa.flows.AffineConstFlow
    flows = _initialised([_maf(nfa, 4, 8, 0), A(4), _maf(nfa, 4, 65, 1), _maf(nfa, 4, 8, 2), A(4), nfa.flows.Permute(4, mode="swap"),
                          _maf(nfa, 4, 8, 3), C(4), _maf(nfa, 4, 65, 4), A(4), _maf(nfa, 4, 65, 5)])
    fwd = [(0, 2, [RNVP]), (2, 3, [MAF1]), (3, 5, [RNVP]), (5, 6, []), (6, 8, [RNVP]), (8, 9, [MAF1]), (9, 10, [ACT1]), (10, 11, [MAF1])]
    return _model(nfa, 4, flows, seed + 1, 0.05), {"fwd": fwd, "inv": reversed_segments(fwd)}


def families(nfa, seed=59):
    """I6, D = 16: two narrow spline pairs, an autoregressive spline layer, a Permute, a MAF layer, three RealNVP records, a circular
    coupling layer (coordinates 1, 6, 11 circular) and a trailing LU (R5: no pair, the layer in front is no CoupledRQS).  The
    autoregressive layers take their one-pass kernel in one direction and their one-launch sampler in the other."""
    torch.manual_seed(seed)
    fl = nfa.flows
    flows = (_pair(nfa, 16, 1, 32) + _pair(nfa, 16, 1, 32, reverse=True)
             + [fl.AutoregressiveRationalQuadraticSpline(16, 2, 40, num_bins=8, init_identity=True), fl.Permute(16, mode="shuffle"),
                fl.MaskedAffineAutoregressive(16, 40)]
             + _initialised([_maf(nfa, 16, 24, 0), fl.ActNorm(16), _maf(nfa, 16, 24, 1)])
             + [fl.CircularCoupledRationalQuadraticSpline(16, 2, 64, ind_circ=[1, 6, 11], num_bins=8, tail_bound=3.0, init_identity=True),
                fl.LULinearPermute(16, identity_init=False)])
    fwd = [(0, 4, [CHAIN]), (4, 5, [ARNSF_INV]), (5, 6, []), (6, 7, [MADE_AFFINE]), (7, 10, [RNVP]), (10, 11, [CIRC]), (11, 12, [LU1])]
    inv = [(11, 12, [LU1]), (10, 11, [CIRC]), (7, 10, [RNVP]), (6, 7, [MAF_INV]), (5, 6, []), (4, 5, [MADE_SPLINE]), (0, 4, [CHAIN])]
    return _model(nfa, 16, flows, seed + 1, 0.03), {"fwd": fwd, "inv": inv}


def pairs_around_records(nfa, seed=79):
    """I7, D = 6: two narrow pairs, [MaskedAffineFlow, ActNorm], two narrow pairs.  R1: a RealNVP run flushes `pending` first -- without
    that flush the two pairs in front of the run would be computed behind it.  (No other stack has pairs next to a run: in I6 another
    layer's flush always comes first.)"""
    torch.manual_seed(seed)
    flows = [f for i in range(2) for f in _pair(nfa, 6, 1, 32, reverse=bool(i & 1))]
    flows += _initialised([_maf(nfa, 6, 8, 0), nfa.flows.ActNorm(6)])
    flows += [f for i in range(2) for f in _pair(nfa, 6, 1, 32, reverse=bool(i & 1))]
    fwd = [(0, 4, [CHAIN]), (4, 6, [RNVP]), (6, 10, [CHAIN])]
    return _model(nfa, 6, flows, seed + 1, 0.05), {"fwd": fwd, "inv": reversed_segments(fwd)}


# ---- training ----------------------------------------------------------------------------------------------------------------------
def realnvp_records(nfa, records, seed=61):
    """T1: `records` records alternating MaskedAffineFlow(MLP [2, 4, 2] s and t) / ActNorm, d = 2.  R8: under autograd a run is cut
    after 32 records IN PROCESSING ORDER, so the inverse pass fuses the LAST 32 records first; record 31 of a 32-record run is an
    ActNorm, whose t is bit 63 of the backward's gradient mask."""
    m = small_model(nfa, d=2, widths=(4,), n=(records + 1) // 2, seed=seed)
    m = nfa.NormalizingFlow(m.q0, list(m.flows)[:records])
    with torch.no_grad():           # (0.12 x N(0, 1): at small_model's 0.3 twenty coupling layers overflow float32 on the way back)
        for p in m.parameters():
            p.mul_(0.4)
    cut = 32
    fwd = [list(range(0, min(cut, records)))] + ([list(range(cut, records))] if records > cut else [])
    inv = [list(range(max(records - cut, 0), records))] + ([list(range(0, records - cut))] if records > cut else [])
    return m, {"fwd": fwd, "inv": inv, "layerwise": (0, 0)}


def realnvp_train_mix(nfa, seed=67):
    """T2, d = 3: [AffineConst, ActNorm, Permute, MAF, ActNorm, MAF(width 65), ActNorm, MAF].  R8: a run without an MLP-conditioned
    layer (0, 1) is not fused and there is no inference kernel under autograd, so both layers run alone; (3, 4) is a fused run; the
    width-65 layer runs alone; (6, 7) -- an ActNorm with an eligible MaskedAffineFlow behind it -- is a run of two with an
    MLP-conditioned layer, and so a fused run as well."""
    torch.manual_seed(seed)
    A, C = nfa.flows.ActNorm, nfa.flows.AffineConstFlow
    flows = _initialised([C(3), A(3), nfa.flows.Permute(3, mode="swap"), _maf(nfa, 3, 8, 0), A(3), _maf(nfa, 3, 65, 1), A(3),
                          _maf(nfa, 3, 8, 2)])
    m = nfa.NormalizingFlow(nfa.distributions.DiagGaussian(3, trainable=False), flows)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(0.3 * torch.randn(p.shape, generator=g))
    return m.to(DEV), {"fwd": [[3, 4], [6, 7]], "inv": [[6, 7], [3, 4]], "layerwise": (1, 2)}


PACK_NSF, PACK_LU, PACK_PAIR, PAIR_FWD = "nf_rqs_fused_pack_all_multi", "nf_lu_factors_multi", "nf_lu_pack_train_multi", "nf_rqs_fused_train_pair_fwd"
FULL_FWD, PACK_ONE, LU_FWD, FACTORS_ONE = "nf_rqs_fused_train_full_fwd", "nf_rqs_fused_pack_all", "nf_lu_fwd", "nf_lu_factors"


def pair_training(nfa, seed=71):
    """T3, D = 64: 0-3 two [CRQS(2 blocks, 128), LU]; 4-5 [CRQS(1 block, 128), LU]; 6 LU; 7-8 [CRQS(2 blocks, 128) FROZEN, LU];
    9-10 [CRQS(2 blocks, 256), LU].  _prepack._plan: "nsf" groups {0, 2} (2 blocks) and {4} (1 block) -- 7 is frozen, 9 is beyond the
    training kernels --, one "lu" group of all six LU layers, "pair" groups {(0, 1), (2, 3)} and {(4, 5)}: the launches go out in the
    order the groups were first met.  The density pass walks from the end: 10 and 8 and 6 read the factors the "lu" launch left
    (nf_lu_fwd, no nf_lu_factors); 9 runs its conditioner as modules and nf_rqs_coupling; 7 packs for itself (nf_rqs_fused_pack_all)
    in front of its one-launch forward; the three pairs run as PairTrainFn."""
    torch.manual_seed(seed)
    flows = (_pair(nfa, 64, 2, 128) + _pair(nfa, 64, 2, 128, reverse=True) + _pair(nfa, 64, 1, 128)
             + [nfa.flows.LULinearPermute(64, identity_init=False)] + _pair(nfa, 64, 2, 128, reverse=True) + _pair(nfa, 64, 2, 256))
    m = _model(nfa, 64, flows, seed + 1, 0.03).train()
    for p in m.flows[7].parameters():
        p.requires_grad_(False)
    packs = [PACK_NSF, PACK_LU, PACK_NSF, PACK_PAIR, PACK_PAIR]
    walk = [LU_FWD, "nf_rqs_coupling", LU_FWD, PACK_ONE, FULL_FWD, LU_FWD, PAIR_FWD, PAIR_FWD, PAIR_FWD]
    return m, {"packs": packs, "pass": packs + walk}


def shared_pair(nfa, seed=73):
    """T4, D = 64: [A, LUa, C, LUc, A, LUa] -- the pair (A, LUa) is in the list twice.  A module that is in the list twice is in no
    group (its layer-owned images serve one use per token): "nsf" {C}, "lu" {LUc}, "pair" {(C, LUc)}.  Both uses of (A, LUa) find no
    token: the LU assembles its factors and A packs for itself, twice with the same weights."""
    torch.manual_seed(seed)
    a, c = _pair(nfa, 64, 2, 128), _pair(nfa, 64, 2, 128, reverse=True)
    m = _model(nfa, 64, a + c + a, seed + 1, 0.03).train()
    packs = [PACK_NSF, PACK_LU, PACK_PAIR]
    alone = [FACTORS_ONE, LU_FWD, PACK_ONE, FULL_FWD]
    return m, {"packs": packs, "pass": packs + alone + [PAIR_FWD] + alone}
