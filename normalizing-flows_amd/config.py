"""Run-time switches of normflows_amd.

fused_gemm: how the fused NSF coupling-layer kernel evaluates its GEMMs
  "f32"    exact fp32 MFMA (v_mfma_f32_32x32x2_f32), the default;
  "bf16x3" error-compensated split-bf16 MFMA (csrc/rqs_fused_x3.hip): fp32 operands as hi+mid+lo bf16, six products
           accumulated in fp32 -- fp32-equivalent results (same parity tests), ~2x the throughput on gfx950.
"""
fused_gemm = "f32"


def set_fused_gemm(mode):
    global fused_gemm
    if mode not in ("f32", "bf16x3"):
        raise ValueError("fused_gemm must be 'f32' or 'bf16x3'")
    fused_gemm = mode


# Runs of GlowBlocks of one shape inside MultiscaleFlow go out as ONE persistent launch per level (nf_glow_level, Squeeze /
# Split / Merge folded in).  False: one launch per GlowBlock plus the glue kernels (ablation / debugging).
glow_level_chains = True


def set_glow_level_chains(mode=True):
    global glow_level_chains
    glow_level_chains = bool(mode)


def set_roctx(mode=True):
    """roctx ranges per layer type around every layer call of the containers (also NF_ROCTX=1); see _prof.py."""
    from . import _prof
    _prof.enabled = bool(mode)


# The two weight gradients of a residual block as ONE pair launch (nf_linear_wgrad_pair); False = two single launches (ablation).
wgrad_pair = True


def set_wgrad_pair(mode=True):
    global wgrad_pair
    wgrad_pair = bool(mode)


# Consecutive fused [CoupledRQS + LULinearPermute] pairs of one shape as ONE persistent launch (nf_rqs_fused_chain /
# nf_rqs_fused_x3_chain); False = one launch per pair (ablation, tests).
fused_chain = True


# Training forward of an eligible NSF coupling layer as ONE launch (autograd.CouplingTrainFn) instead of per-module Functions.
train_full = True


def set_train_full(mode=True):
    global train_full
    train_full = bool(mode)


# Backward of a residual block (and the initial layer behind the first one) as one pass over the rows (nf_resblock_bwd).
resblock_bwd = True


def set_resblock_bwd(mode=True):
    global resblock_bwd
    resblock_bwd = bool(mode)


# The coupling transform's backward + the final Linear's input gradient as one pass over the rows (nf_final_bwd); False = the
# stand-alone spline backward (nf_rqs_coupling_bwd_p24) + a library GEMM on the padded rows (round 2; ablation / differential tests).
final_bwd_fused = True


def set_final_bwd_fused(mode=True):
    global final_bwd_fused
    final_bwd_fused = bool(mode)


# The whole backward of a benchmark-shaped coupling layer behind one C-ABI call with ONE reduction launch for all of its partial
# tiles (nf_coupling_train_bwd, round 6); False = the kernels issued one by one from autograd.CouplingTrainFn.backward, each with
# its own reduction launch (rounds 3-5; ablation / differential tests: the gradients are bit-identical).
train_bwd_onecall = True


def set_train_bwd_onecall(mode=True):
    global train_bwd_onecall
    train_bwd_onecall = bool(mode)


# A benchmark-shaped [CoupledRQS, LULinearPermute] pair under autograd as ONE forward launch and the composed LU's one-product
# backward (autograd.PairTrainFn, round 6); False = LULinearPermuteFn + CouplingTrainFn (rounds 3-5; ablation / differential tests).
train_pair = True


def set_train_pair(mode=True):
    global train_pair
    train_pair = bool(mode)


# The pair backward's last two launches (the reduction of the partial tiles, the LU's factor gradients: parameter gradients only, 46 us
# of latency-bound work per pair) on a SIDE stream, under the next pair's MFMA-bound kernels (round 6, late; nf_pair_train_bwd_head /
# _tail, _sidestream.py).  Taken only when nothing can read those gradients before the join at the end of the backward pass: every
# parameter of the pair writes into a registered gradient buffer (dp.FlatParameters) handed to this call while .grad is unset (autograd
# adopts the view, no accumulation kernel), had one training forward since zero_grad (no second contribution in the graph) and carries no hooks other than join-aware ones (dp.OverlappedGradientAverager's).
# OFF by default -- measured (tools/train_bench.py --flat [--async], alternating on one box): without those two launches at all the step
# is 1.46 ms shorter (25.28 -> 23.82 ms), but on the side stream only 0.2-0.3 ms of that came back (25.25 -> 25.0), and nothing once the
# reduction launch issued its longest blocks first (25.1 either way): every heavy kernel of the step allocates the whole register file of
# a CU (2 waves per SIMD x 219-256 registers), so a second kernel gets no wave slot while one runs -- the side stream only fills the
# drain / ramp at kernel boundaries.
train_reduce_async = False


def set_train_reduce_async(mode=True):
    global train_reduce_async
    train_reduce_async = bool(mode)


# Glow's training step (BASELINE configs[3]): the launches of a GlowBlock's backward that only produce PARAMETER gradients -- the conditioner's
# weight gradients (made_wgrad + its reduction + the last bias sum), the 1x1 convolution's weight gradient and its LU factors' -- on the
# side stream (_sidestream.fork), joined at the end of the backward pass.  Unlike the benchmark model's pair (above) the Glow step is
# made of kernels that do not fill the chip: the 8x8 / 4x4 levels give the row-tile kernels 256 / 64 workgroups, the LU-factor and
# reduction kernels are one-workgroup launches.  Taken per Function only when every parameter it feeds has no .grad to accumulate into
# and no hooks (autograd adopts the tensor without a kernel); anything else joins first.
# OFF by default -- measured (tools/glow_leaf_ab.py, alternating on one box, config 4): the step recorded as one hipGraph 44.57 / 44.40 ms
# without, 43.98 / 44.13 ms with (same gradient bits): 12.5 ms of leaf launches per step move to a parallel branch of the graph and 0.4 ms
# comes back -- the replayed graph does not run the branches side by side to any useful degree.
train_leaf_async = False


def set_train_leaf_async(mode=True):
    global train_leaf_async
    train_leaf_async = bool(mode)


# Glow's training step: the Invertible1x1Convs of a level assemble their matrices (and, in the backward, their LU factors' gradients) in
# ONE launch per level (autograd.Inv1x1WeightsFn) instead of one single-workgroup launch per block and direction.  False = per block.
glow_weights_batched = True


def set_glow_weights_batched(mode=True):
    global glow_weights_batched
    glow_weights_batched = bool(mode)


# The 256-slot training kernels (nf_made_forward_train / nf_made_backward: GlowBlock's conv conditioner at the 16x16 level, ResidualNets /
# MADEs of hidden width <= 256 on <= 64 features) on 128-row tiles at batches that are a multiple of 128 rows where the persistent workgroups' rounds come out shorter (csrc/mlp_tile.hpp
# mf_tr128: a weight fragment feeds eight MFMAs instead of four; same bits).  Lives in the library (nf_config_made_tr128).
def set_made_tr128(mode=True):
    """Returns the previous setting.  A forward and its backward must run under the same setting."""
    from . import _lib
    return bool(_lib.lib().nf_config_made_tr128(1 if mode else 0))


# MultiscaleFlow under autograd: the per-layer `log_q += log_det` statements of a level are collected and applied as one launch in the same
# order (flows/affine.lazy_ld, nf_ld_fold_multi: same bits).  False = one launch per layer.
lazy_logdet = True


def set_lazy_logdet(mode=True):
    global lazy_logdet
    lazy_logdet = bool(mode)


# A differentiable density pass of a benchmark-shaped model on a batch that is NOT a multiple of 64 rows (>= 1024) is run on the batch
# padded with zero rows to the next multiple (NormalizingFlow._log_prob_impl) and sliced back: the one-call / pair training kernels need
# whole 64-row tiles, and the slice's backward hands the padding rows a zero cotangent, so they contribute exactly nothing to any
# gradient.  65 537 rows: 44.4 -> 34.4 ms per step of the benchmark model (what 65 600 rows cost).  False = the general kernels.
train_pad_batch = True


def set_train_pad_batch(mode=True):
    global train_pad_batch
    train_pad_batch = bool(mode)


def set_fused_small_batch(mode=True):
    """nf_rqs_fused_chain on 128-row workgroups for batches of at most 32 768 rows (the default; csrc/rqs_fused_nw4.hip: 5.4 -> 3.0 ms
    per pass of the benchmark chain).  False = every batch on the 256-row workgroups (differential tests).  Returns the old setting."""
    from . import _lib as L
    return bool(L.lib().nf_rqs_fused_small_batch(1 if mode else 0))


# LULinearPermute's density-direction backward (D = 64) as one pass over the rows (nf_lu_bwd).
lu_bwd_fused = True


def set_lu_bwd_fused(mode=True):
    global lu_bwd_fused
    lu_bwd_fused = bool(mode)


# Training: every eligible layer's weights packed by ONE launch per kind at the start of a differentiable density pass (_prepack.py).
train_prepack = True


def set_train_prepack(mode=True):
    global train_prepack
    train_prepack = bool(mode)


# MAF inverse (nf_maf_inverse): the mapping with 32 samples per wave and the lane-halves sharing a sample's hidden units (two waves
# per SIMD, csrc/maf_inverse_h.hip); False = round 2's 64-samples-per-wave kernel (csrc/maf_inverse.hip; ablation).
maf_halves = True


def set_maf_halves(mode=True):
    global maf_halves
    maf_halves = bool(mode)


# MAF inverse, round 5: format-1 packs (flows/maf_pack.pack_made(tri=True)) -- regular tiles (<= 8 degrees of <= 4 hidden units) run
# nf_maf_inverse_h_tri's statically unrolled triangular sequential part and 8-deep activation ring; False = format 0 on
# nf_maf_inverse_h (round 3/4; ablation).  Only with maf_halves.
maf_tri = True


def set_maf_tri(mode=True):
    global maf_tri
    maf_tri = bool(mode)


def set_fused_chain(mode=True):
    global fused_chain
    fused_chain = bool(mode)


# LULinearPermute under autograd: its two batch-side products per direction as ONE launch (nf_rows_matvec2); False = two
# nf_rows_matvec launches (ablation).
lu_matvec2 = True


def set_lu_matvec2(mode=True):
    global lu_matvec2
    lu_matvec2 = bool(mode)


# MADE's single pass as ONE launch (nf_made_forward / nf_made_forward_affine, csrc/made_fwd.hip) where flows/made_pack.py takes the
# structure; False = layer by layer (library GEMMs on the pre-masked weights; ablation / differential tests).
made_fused = True


def set_made_fused(mode=True):
    global made_fused
    made_fused = bool(mode)


# MADE under autograd (core.py:87-102 through an autoregressive flow's single-pass direction): forward nf_made_forward_train, backward
# nf_made_backward + nf_made_wgrad (csrc/made_bwd.hip); False = torch autograd through library GEMMs on the pre-masked weights.
made_train = True


def set_made_train(mode=True):
    global made_train
    made_train = bool(mode)


# MaskedAffineAutoregressive.inverse (the reference's DENSITY direction of MAF: D sequential MADE passes, autoregressive.py:29-38) under
# autograd by implicit differentiation (autograd.MafInverseFn): the one-pass inverse kernel forward, the triangular system of the
# backward solved with the MADE input-gradient chain, ONE weight-gradient launch; False = torch autograd through the D-pass loop.
maf_implicit = True
# stop the sweeps once max |v_new - v| <= rtol * max |v| (0.0 = until v stops changing bit for bit: the exact solution of the triangular
# system; 1e-6 saves the last ~15 % of the sweeps at float32-noise-level gradient changes)
maf_implicit_rtol = 0.0


# Autoregressive.inverse under autograd for the other element-wise transforms (AR-NSF sampling, circular splines, MAF structures
# outside the one-pass kernels): implicit differentiation on the layer's own density-direction graph (autograd.ArInverseImplicitFn:
# <= D backward sweeps of the net + one weight-gradient pass).  False = the reference's D recorded passes.
# Restriction: the implicit Functions are once_differentiable -- FIRST-order gradients only.  Double backward through
# an autoregressive layer's inverse (create_graph=True: gradient penalties, Hessian-vector products through sampling) needs the D
# recorded passes, which support it like the reference's loop: `with normflows_amd.config.higher_order_gradients():` (or
# set_ar_implicit(False) / set_maf_implicit(False)) around the forward pass.
ar_implicit = True
# MaskedAffineAutoregressive's element-wise map under autograd as torch formulas (affine/autoregressive.py:98-128 verbatim in torch
# ops: differentiable to any order) instead of nf_maf_affine + nf_maf_affine_bwd; set by higher_order_gradients().
torch_elementwise = False


class higher_order_gradients:
    """Context manager: inside it Autoregressive.inverse / MaskedAffineAutoregressive.inverse run the reference's D recorded passes
    under autograd instead of the once-differentiable implicit Functions, and MADE runs as plain torch modules: as differentiable
    as the element-wise transform's own backward allows (the affine transform of MAF: any order)."""

    def __enter__(self):
        global ar_implicit, maf_implicit, made_train, torch_elementwise
        self.saved = (ar_implicit, maf_implicit, made_train, torch_elementwise)
        # (MADE itself then runs as torch modules on library GEMMs and MAF's element-wise affine map as torch formulas: the
        # hand-written MadeFn / MafAffineFn backwards are sets of kernels, first-order as well)
        ar_implicit = maf_implicit = made_train = False
        torch_elementwise = True
        return self

    def __exit__(self, *exc):
        global ar_implicit, maf_implicit, made_train, torch_elementwise
        ar_implicit, maf_implicit, made_train, torch_elementwise = self.saved
        return False


def set_ar_implicit(mode=True):
    global ar_implicit
    ar_implicit = bool(mode)


def set_maf_implicit(mode=True, rtol=None):
    global maf_implicit, maf_implicit_rtol
    maf_implicit = bool(mode)
    if rtol is not None:
        maf_implicit_rtol = float(rtol)


# CoupledRationalQuadraticSpline beyond the benchmark kernel's shapes (D <= 128, hidden <= 512, 8 bins) as ONE launch (nf_nsf_wide,
# csrc/nsf_wide.hip); False = library GEMMs for the conditioner + nf_rqs_coupling (ablation / differential tests).
nsf_wide = True


def set_nsf_wide(mode=True):
    global nsf_wide
    nsf_wide = bool(mode)


# Conditional CoupledRationalQuadraticSpline (num_context_channels, ResidualNet with a GLU context gate) at inference as ONE launch
# (nf_nsf_wide_ctx, csrc/nsf_ctx.hip); False = the conditioner as eager modules + nf_rqs_coupling (A/B runs, differential tests).
nsf_context = True


def set_nsf_context(mode=True):
    global nsf_context
    nsf_context = bool(mode)


# CircularCoupledRationalQuadraticSpline (list tails, periodic preprocessing of the circular identity coordinates) at inference as ONE
# launch (nf_nsf_wide_ft, csrc/nsf_circ.hip); False = library GEMMs for the conditioner + nf_rqs_coupling_ft (A/B runs, differential tests).
nsf_circular = True


def set_nsf_circular(mode=True):
    global nsf_circular
    nsf_circular = bool(mode)


# The density direction of the autoregressive spline layers with list tails (circular coordinates), a tensor tail bound or a permuted
# mask at inference as ONE launch (nf_made_forward_spline_ft, csrc/made_fwd_ft.hip); False = eager MaskedLinear modules +
# nf_rqs_coupling_ft (A/B runs, differential tests).
arnsf_density_ft = True


def set_arnsf_density_ft(mode=True):
    global arnsf_density_ft
    arnsf_density_ft = bool(mode)


# The same layers UNDER AUTOGRAD in the density direction on the MADE training kernels (autograd.MadeFtFn: nf_made_forward_train_ft,
# nf_made_backward, nf_made_feed_ft_bwd, nf_made_wgrad on a degree-order pack); False = eager MaskedLinear modules + torch.sin /
# torch.cos in front of SplineFn.  The route also follows made_train and made_fused, so inside higher_order_gradients() the torch
# modules run and double backward keeps working.
arnsf_train_ft = True


def set_arnsf_train_ft(mode=True):
    global arnsf_train_ft
    arnsf_train_ft = bool(mode)


# CircularCoupledRationalQuadraticSpline UNDER AUTOGRAD, both directions: the conditioner (a ResidualNet behind the periodic
# preprocessing of the circular identity coordinates) on the MADE training kernels through a dense pack (autograd.ResNetFtFn:
# nf_made_forward_train_ft, nf_made_backward, nf_made_feed_ft_bwd, nf_made_wgrad; flows/made_pack.resnet_train_structure_ft), and the
# spline's backward of an 8-bin layer on wave-private tiles (nf_rqs_coupling_bwd_ft_wave, csrc/rqs_bwd_ft.hip); False = eager torch
# modules (indexing, sin / cos, cat, one library GEMM per Linear) + nf_rqs_coupling_bwd_ft (A/B runs, differential tests).  The
# conditioner route also follows made_train and made_fused, so inside higher_order_gradients() the torch modules run and double
# backward keeps working.
nsf_circular_train = True


def set_nsf_circular_train(mode=True):
    global nsf_circular_train
    nsf_circular_train = bool(mode)


# The GLU-gated conditioner of a conditional CoupledRationalQuadraticSpline (ResidualNet with context_features) under autograd on
# HIP kernels (autograd.ResNetCtxFn, csrc/resnet_ctx_train.hip); False = the conditioner as eager torch modules.  The route also
# follows made_train, so inside higher_order_gradients() the torch modules run and double backward keeps working.
nsf_context_train = True


def set_nsf_context_train(mode=True):
    global nsf_context_train
    nsf_context_train = bool(mode)


# Runs of MaskedAffineFlow(MLP s, MLP t) / ActNorm / AffineConstFlow layers (the inference kernel nf_realnvp_chain's records) under
# autograd as one forward and one backward launch (autograd.RealNVPChainFn, csrc/realnvp_train.hip: nf_realnvp_chain_train_fwd /
# nf_realnvp_chain_bwd); False = layer by layer: library GEMMs + LeakyReLU launches for the MLPs, MaskedAffineFn / ActNormFn on top
# (A/B runs, differential tests).  The Function is once-differentiable: inside higher_order_gradients() the route is not taken.
realnvp_train = True
# While a stream is being CAPTURED (torch.cuda.graph) the route is taken from this many rows on.  Replayed from a graph the
# layer-by-layer route has no launch overhead left, and below this size its many small kernels finish sooner than the two long
# ones (profiles/realnvp_train_bench.json: `capture_min_batch`, tools/realnvp_train_bench.py).  Eager steps take the route at every
# batch size (2.4x faster or more at 1024 and at 65 536 rows).
realnvp_train_capture_min_batch = 4096


def set_realnvp_train(mode=True, capture_min_batch=None):
    global realnvp_train, realnvp_train_capture_min_batch
    realnvp_train = bool(mode)
    if capture_min_batch is not None:
        realnvp_train_capture_min_batch = int(capture_min_batch)


# AffineCouplingBlock(MLP) layers, each with the Permute directly behind it, as "coupling block" records of those same runs -- at
# inference (nf_realnvp_chain) and under autograd (RealNVPChainFn): the reference's quick-start model, 32 x [AffineCouplingBlock(MLP),
# Permute(2, 'swap')], is one launch / one forward and one backward launch.  False = the record kind is never formed: every block runs
# its own conditioner modules + nf_affine_coupling and every Permute its torch indexing, as before the record existed (A/B runs,
# differential tests).  Under autograd the record follows realnvp_train and realnvp_train_capture_min_batch like the other kinds.
realnvp_blocks = True
# At inference the record is formed at every batch size, captured or not.  lane = sample: a launch lasts as long as one lane needs
# for all the MLPs of the run, so replayed from a graph -- where the layer-by-layer kernels have no launch overhead left -- a small
# batch is faster with the switch off (profiles/realnvp_block_bench.json: `log_prob_graph`, `inference_graph_not_slower_from`).


def set_realnvp_blocks(mode=True):
    global realnvp_blocks
    realnvp_blocks = bool(mode)


# MaskedAffineFlow(MLP s, MLP t) and AffineCouplingBlock(MLP) layers beyond the chain kernels' shapes (d > 16 or a width > 64; d <= 128,
# <= 512 hidden slots, two hidden layers, LeakyReLU(0)) at inference as ONE launch (nf_affine_wide, csrc/affine_wide.hip); False = the
# conditioners as library GEMMs + LeakyReLU launches with nf_masked_affine / nf_affine_coupling behind them (A/B runs, differential
# tests).  Layers the chain kernels can take never come here, whatever realnvp_blocks says.
affine_wide = True
# While NormalizingFlow.use_graphs records a pass (its warm-up call and the capture alike, so both take one route) the launch is taken
# from this many rows on.  Replayed from a graph the layer-wise kernels have no launch overhead left, and a small batch fills few of
# the persistent workgroups: at 1 024 rows the one launch lasts 0.09-0.11 ms against 0.05-0.06 ms; replayed, it is no slower from
# 8 192 rows on (d 64, two nets of 256) resp. 16 384 (d 128, one net of 512) (profiles/affine_wide_bench.json:
# `graph_not_slower_from`, tools/affine_wide_bench.py); the gate is the larger of the two.  Eager calls, and a capture the caller makes with torch.cuda.graph directly,
# take the launch at every size: such a caller warms up eagerly, and a gate on the capture alone would then record library GEMMs that
# were never initialised outside it.  set_affine_wide(False) is the faster setting for those captures of small batches.
affine_wide_graph_min_batch = 16384
_graph_recording = 0          # > 0 inside core._GraphCache's warm-up + capture


def set_affine_wide(mode=True, graph_min_batch=None):
    global affine_wide, affine_wide_graph_min_batch
    affine_wide = bool(mode)
    if graph_min_batch is not None:
        affine_wide_graph_min_batch = int(graph_min_batch)


# The same layers UNDER AUTOGRAD on HIP kernels (autograd.AffineWideFn: nf_pack_gather, nf_made_forward_train in plain-MLP mode on the
# stacked [s | t] conditioner, nf_affine_wide_apply; backward nf_affine_wide_apply_bwd, nf_made_backward, nf_made_wgrad) instead of
# b * z, one library GEMM per Linear, one LeakyReLU launch per activation and MaskedAffineFn / AffineCouplingFn on top.  OPT-IN,
# default False: with the switch off these layers' gradients are bit for bit what the layer-wise route gives (the MFMA kernels sum
# in another order than the library GEMMs), which tests/test_gpu_affine_wide.py pins for the default configuration.  The route also
# follows made_train and made_fused, so inside higher_order_gradients() the torch modules run and double backward keeps working.
affine_wide_train = False
# While a stream is being CAPTURED (NormalizingFlow.use_graphs' recording, or a caller's own torch.cuda.graph) the route is taken from
# this many rows on: replayed from a graph the layer-wise route has no launch overhead left, and at 1 024 rows its step lasts 0.18 ms
# against 0.30 ms (d 128, one net of 512).  Replayed, the route is not slower from 2 048 rows on (d 64, two nets of 256) resp. 8 192
# (d 128, one net of 512) (profiles/affine_wide_train_bench.json: `capture_not_slower_from`, tools/affine_wide_train_bench.py); the
# gate is the larger of the two.  Eager steps take the route at every size (1.3x - 2.2x faster over the swept sizes).
affine_wide_train_capture_min_batch = 8192


def set_affine_wide_train(mode=True, capture_min_batch=None):
    global affine_wide_train, affine_wide_train_capture_min_batch
    affine_wide_train = bool(mode)
    if capture_min_batch is not None:
        affine_wide_train_capture_min_batch = int(capture_min_batch)


# Runs of Planar / Radial layers (exact types, float32 CUDA inputs of <= 128 elements per row, <= 64 layers per launch) on the rank-1
# chain kernels (csrc/rank1_chain.hip): ONE launch at inference (nf_rank1_chain), one forward and one backward launch under
# autograd (autograd.Rank1ChainFn), the u- and beta-constraints computed on the stacked parameters in front of them
# (flows/rank1_pack.py); False = every layer's torch formulas, the reference's arithmetic (A/B runs, differential tests).  The
# Function is once-differentiable: inside higher_order_gradients() the torch formulas run.
# Default on: eager, the kernels' median lies below the formulas' minimum for every measured model, leg and batch size; replayed from
# a captured graph they are not slower at any swept size either (1 024 .. 65 536 rows), so there is no batch-size gate for recorded
# passes (profiles/rank1_bench.json: `default_on_criterion`, `graph_not_slower_from`; tools/rank1_bench.py).
rank1_chain = True


def set_rank1_chain(mode=True):
    global rank1_chain
    rank1_chain = bool(mode)


# The densities a model is trained against or starts from: the closed-form 2-D targets and priors (TwoMoons, CircularGaussianMixture,
# RingMixture, TwoModes, Sinusoidal, Sinusoidal_gap, Sinusoidal_split, Smiley: exact types, contiguous float32 CUDA (B, 2) input) as ONE
# launch that writes log p and, under autograd, d log p / d z (nf_density2d, autograd.Density2dFn), and GaussianMixture.log_prob
# (exact type, float32 parameters, contiguous float32 CUDA (B, d) input, d <= 128, M <= 64, M d <= 4096) as one forward launch and one
# backward launch plus a fixed-order slab reduction (nf_gmm_log_prob / _bwd, autograd.GmmLogProbFn; the record is built by torch in
# dist_mixture.record).  False = the torch formulas, the reference's arithmetic op for op (A/B runs, differential tests).  Both
# Functions are once-differentiable: inside higher_order_gradients() the torch formulas run.
# Default OFF.  Measured (tools/target_bench.py, profiles/target_bench.json): eager, the kernels' median lies below the formulas'
# minimum in 29 of the 30 cases (every density, leg and batch size: 2.0x - 20x; the reverse-KL step of 32 Planar layers at 65 536
# rows), but not for that step at 1 024 rows, which is host-bound (off 2.78 ms median, 2.11 minimum; on 2.48) -- and the project's
# rule is default on only when it holds in every case (`default_on_criterion`).  Replayed from a captured graph the step is faster
# on the kernels at every swept size, 1 024 .. 65 536 rows (`graph_not_slower_from`): no batch-size gate.
target_density = False


def set_target_density(mode=True):
    global target_density
    target_density = bool(mode)


# The stochastic flow layers: flows.HamiltonianMonteCarlo (exact type) and flows.MetropolisHastings (exact type, with an exact-type
# DiagGaussianProposal of shape (2,)) on contiguous float32 CUDA (B, 2) inputs against one of the eight closed-form 2-D densities, a
# 2-D DiagGaussian (float32, no temperature, no gradient wanted) or a LinearInterpolation of two of them with a host-side alpha: ONE
# launch per layer call (nf_hmc2d / nf_mh2d, csrc/hmc2d.hip; stochastic_route.py) with the random numbers drawn by torch in front of
# it in the reference's order, and under autograd autograd.Hmc2dFn / Mh2dFn (one backward launch plus a fixed-order slab reduction
# for log_step_size / log_mass).  False = the torch formulas, the reference's arithmetic op for op (A/B runs, differential tests).
# The route evaluates the densities itself: it does not depend on target_density.  Both Functions are once-differentiable: inside
# higher_order_gradients() the torch formulas run.
# Default on: eager, the kernels' median lies below the formulas' minimum in every measured case (HMC with 5 leapfrog steps against
# TwoModes and CircularGaussianMixture(8), MH with 10 steps, a 10-layer HAIS chain; forward, and forward + backward to log_step_size /
# log_mass; 1 024 and 65 536 rows: 11x - 256x); replayed from a captured graph the explicit-noise transitions are faster at every swept
# size (1 024 .. 65 536 rows), so there is no batch-size gate for recorded passes (profiles/stochastic_bench.json:
# `default_on_criterion`, `graph_not_slower_from`; tools/stochastic_bench.py).
stochastic_kernels = True


def set_stochastic_kernels(mode=True):
    global stochastic_kernels
    stochastic_kernels = bool(mode)


# Residual flows on 2-D rows (exact type, a LipschitzMLP of 1 .. 3 hidden layers of width <= 128, `brute_force or not training`, CUDA
# float32, no gradient needed) on the kernels of csrc/lipmlp.hip: the density direction of a maximal run of [Residual | initialised
# ActNorm | AffineConstFlow] layers with at least one Residual as ONE launch (nf_lipmlp_chain; value, exact 2 x 2 Jacobian by
# forward-mode tangents and log|det| per Residual record), the fixed-point direction as one launch and one read-back per iteration
# (nf_lipmlp_apply) and one Jacobian launch at the point found; effective weights packed in front of them with torch
# (flows/lipmlp_pack.py).  False = the torch formulas, the reference's arithmetic (A/B runs, differential tests).
# Default on: eager, the kernels' median lies below the formulas' minimum in every measured case (`log_prob` of the 16-layer example model
# at 1 024 and 65 536 rows, `sample` at 1 024 rows); replayed from a captured graph they are not slower at any swept size either
# (1 024 .. 65 536 rows), so there is no batch-size gate for recorded passes (profiles/residual_bench.json: `default_on_criterion`,
# `graph_not_slower_from`; tools/residual_bench.py).
residual_chain = True


def set_residual_chain(mode=True):
    global residual_chain
    residual_chain = bool(mode)


# Training of 2-D Residual layers on the kernels of csrc/lipmlp_train.hip: a density-direction pass that needs a gradient, or a
# training-mode pass on a stochastic log-det estimator, runs as one forward launch (value, estimate and the estimate's cotangent of
# the exact 2 x 2 Jacobian) and one backward launch plus a fixed-order reduction (autograd.LipMlpTrainFn, flows/lipmlp_pack.py:
# train_eligible has the conditions; residual_chain must be on as well); False = the torch formulas, the reference's arithmetic.  The
# random draws come in the reference's order in front of the launch, so one seed gives both routes the same numbers.  The Function is
# once-differentiable: inside higher_order_gradients() the torch formulas run.
# Default OFF whatever tools/residual_train_bench.py says (profiles/residual_train_bench.json: `default_on_criterion`); turning it on
# is a change of its own.
residual_train = False


def set_residual_train(mode=True):
    global residual_train
    residual_train = bool(mode)


# Residual layers on (B, d) rows with 3 <= d <= 64 at inference (evaluation mode, exact_trace=False, CUDA float32, no gradient needed)
# on the kernels of csrc/lipmlp_nd.hip: the density direction of a maximal run of [Residual | initialised ActNorm | AffineConstFlow]
# layers as ONE launch (nf_lipmlp_nd_chain: value pass, then one forward-mode tangent pass per term of Hutchinson's power series),
# the fixed-point direction as one launch and one read-back per iteration (nf_lipmlp_nd_apply) and one series launch at the point
# found (flows/lipmlp_nd_pack.py: eligible has the conditions; residual_chain must be on as well).  Every layer's truncation and
# noise are drawn in the reference's order, from the same generators, in front of the launch.  False = the torch formulas, the
# reference's arithmetic: one autograd pass through the network per series term.
# Default OFF whatever tools/residual_nd_bench.py says: the route changes which float32 rounding a seeded evaluation gets (forward-
# mode tangents against the reference's vector-Jacobian products), the d > 2 workloads have no soak run behind them yet, and
# training at d > 2 still takes the formulas; turning it on is a change of its own (profiles/residual_nd_bench.json).
residual_nd = False


def set_residual_nd(mode=True):
    global residual_nd
    residual_nd = bool(mode)


# Debug mode of the element-wise spline API (utils.splines): after every call a check launch (nf_rqs_spline_check)
# sets device-side flags and the shim reads them back -- a host synchronisation per call, which is why it is off by default -- and
# raises what the reference raises: AssertionError for a negative discriminant in the inverse direction (utils/splines.py:181),
# RuntimeError for tails=None inputs outside the domain (the reference's gather index error, utils/splines.py:154-160; without
# debug mode the kernels clamp the bin).
debug_checks = False


def set_debug_checks(mode=True):
    global debug_checks
    debug_checks = bool(mode)


# The implicit backward of the MAF inverse (autograd.MafInverseFn): True = ONE pass of nf_maf_solve_t per layer (round 5: back-
# substitution on the transposed pack, no host read-back); False = round 4's sweeps of nf_made_backward until v stops changing
# (15-25 passes per layer; ablation / cross-check).
maf_onepass = True


def set_maf_onepass(mode=True):
    global maf_onepass
    maf_onepass = bool(mode)


# The weight-gradient launch of the one-pass implicit backward reads MADE's hidden gradients from the SOLVE's scratch (nf_maf_scratch_rows:
# the solve finalises every unit of the transposed network once from final values = the input-gradient chain at the solution) instead of
# running nf_made_backward once more.  False = the extra chain pass.
maf_solve_grads = True


def set_maf_solve_grads(mode=True):
    global maf_solve_grads
    maf_solve_grads = bool(mode)


# Round 6 (late): the one-pass solve runs the regular-8 tiles of a format-1 transposed pack on a statically unrolled sequential part
# (nf_maf_solve_t_tri; bit-identical to the generic part).  False = every tile on the generic part.
maf_solve_fast = True


def set_maf_solve_fast(mode=True):
    global maf_solve_fast
    maf_solve_fast = bool(mode)


# Round 6: that weight-gradient launch reads BOTH scratches where the one-pass kernels left them (nf_made_wgrad_pos: problems, tiles and
# scatter maps over scratch positions; batches that are a multiple of 64 rows, position counts that are a multiple of 128) instead of two
# nf_maf_scratch_rows rearrangements per layer (2 x 245 us and 2.7 GB of traffic per config-5 layer at B = 65 536).  False = rearrange.
maf_wgrad_in_place = True


def set_maf_wgrad_in_place(mode=True):
    global maf_wgrad_in_place
    maf_wgrad_in_place = bool(mode)
