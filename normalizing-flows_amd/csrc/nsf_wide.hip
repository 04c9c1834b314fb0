// nsf_wide.hip -- CoupledRationalQuadraticSpline (normflows/flows/neural_spline/wrapper.py:14-85 -> nsf/coupling.py:71-128, 150-164,
// 221-253, 329-362 over nets/resnet.py:37-50, 92-104 and utils/splines.py:16-219) as ONE launch for the shapes beyond the benchmark
// kernel's (rqs_fused.hip: D <= 64, hidden <= 128): up to 128 features and 512 hidden units, 4 / 8 / 16 bins, linear tails, float32.  Round 3
// ran these as library GEMMs + nf_rqs_coupling on a materialised conditioner output (2944 B per row and 32 transform features).
//
// The engine is mlp_tile.hpp's (made_fwd.hip describes it): 8 waves own 64 rows for the whole layer, pre-activations in accumulator
// registers, the next layer's B operand in LDS in MFMA order, one contiguous weight stream per wave through a register ring,
// persistent over the tiles.  What is specific here (host packer: flows/nsf_wide_pack.py; the stages the conditional layer's kernel
// nsf_ctx.hip runs as they are live in nsf_tile.hpp and the nsf_tile_*.hpp fragments it describes):
//   * the x tile is held with its columns SORTED (B-operand order over POSITIONS: identity feature i at position i < PI, transform
//     feature j at PI + j; PI = the identity count rounded up to 32, zeros at the padding positions): the initial layer contracts
//     over the first PI positions only -- the conditioner sees the identity features alone (nsf/coupling.py:83-84), so a NaN / inf in
//     a transform column passes through its own element (utils/splines.py:40-41) without reaching the conditioner through a zero
//     weight; the LU matrix is packed in position order;
//   * the final layer runs in GROUPS of four transform features = 3 row-blocks for both sample blocks (6 accumulators); the packed
//     row order makes a lane's 48 accumulator values of a sample block the 2 x 24 parameter lists (8 widths, 8 heights, 7
//     derivatives, pad) of features 4 g + 2 hh + {0, 1}: the spline runs on them in registers (fused_common.hpp rqs_regs: branch-
//     free, hardware transcendentals, log2(e) / sqrt(hidden) folded into the packed rows), reads x from the tile and writes y into it;
//   * the identity features go through the batch-shared spline (nsf/coupling.py:221-253) from knot tables staged in the activation
//     region while it is free: AFTER the network in the density direction (the conditioner sees the raw features, :83-92), BEFORE
//     it in the sampling direction (:112-118);
//   * per-row log-det: the lane-halves' sums, the groups' and the identity columns' partials through LDS in a fixed order.
// Bound: fp32 MFMA.  FLOP per row: 2 (nI H + 4 H^2 + 23 nT H) algorithmic (executed: full-width initial layer, padded hidden
// units, 24 rows per feature); HBM: 8 D + 4 bytes per row.
#include "nsf_tile.hpp"

namespace nf {

// knot tables of the batch-shared spline, once per parameter version (same arithmetic as rqs_fused.hip's pack_tables_kernel)
__global__ void nsf_wide_tables_kernel(const float *__restrict__ uw, const float *__restrict__ uh, const float *__restrict__ ud,
                                       float *__restrict__ tab, int nI, RqsParams<float> p) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nI) return;
    const int K = p.K;
    const float *wj = uw + j * K, *hj = uh + j * K, *dj = ud + j * (K - 1);
    auto wacc = [=](int k) { return wj[k]; };
    auto hacc = [=](int k) { return hj[k]; };
    auto dacc = [=](int k) { return dj[k]; };
    rqs_build_table<float>(p, wacc, hacc, dacc, tab + j * 3 * (K + 1));
}

// The adjacent LULinearPermute (mixing.py:535-563) as one dense product on the tile, in place: every wave computes its 32 output
// columns of one sample block from the tile (B operand as it stands), all waves meet, then the columns are written back in B-operand
// order (the accumulator quads ARE 16-byte groups of that order).
template <int TR>
__device__ __forceinline__ void nw_lu_stage(MfRing &ring, const int *it, float *xreg, int lane_b, int hh, int n) {
    constexpr int NSL = TR / 64;           // sample blocks per LU item: 4 row-blocks x TR / 32 sample blocks over 8 waves
    const int rb = it[1];
    f32x16 o1[NSL];
    if (rb >= 0) mf_item<NSL, false, TR>(ring, it[0], xreg + lane_b + 128 * it[2], o1);
    MF_BARRIER();
    if (rb >= 0) mf_publish<NSL, false, TR>(xreg, rb, it[2], hh, n, o1);
    MF_BARRIER();
}

// NHI hidden items per wave with NS sample blocks each, TR rows per tile: (1, 2, 128) Hp = 128 -- the activations of a 128-wide
// network leave room for 128-row tiles: half the barriers, tile prologues and weight-stream traffic per row --, (1, 2, 64) Hp = 256,
// (2, 2, 64) Hp = 512.
// DIR 0: density direction = prqct.forward (nsf/coupling.py:71-98); DIR 1: sampling direction = prqct.inverse (:100-128).
// LU: with the adjacent LULinearPermute -- applied BEFORE the coupling layer in the density direction (core.py:193-195 walks the
// flows backwards: the LU layer behind a coupling layer comes first), AFTER it in the sampling direction (core.py:177-179).
// KB bins (round 5: 4 and 16 beside 8): a lane-half's 48 accumulator values per sample block are FPL = 16 / KB whole parameter lists of
// MP = 3 KB slots, so a final-layer group holds FPG = 2 FPL transform features (8 / 4 / 2).
template <int NHI, int NS, int DIR, bool LU, int TR, int KB = F_K>
__global__ void __launch_bounds__(64 * MF_NW, 1)
nsf_wide_kernel(const float *__restrict__ x, float *__restrict__ y, float *__restrict__ logdet, const float *__restrict__ blob,
                const int *__restrict__ table, const float *__restrict__ tabs, const float *__restrict__ lu_lad, int64_t B,
                int acc_mode, RqsParams<float> p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, n = lane & 31, hh = lane >> 5;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int D = table[0], Dp = table[1], Hp = table[3], NB = table[4], nI = table[5], nT = table[6], par_i = table[7],
              par_t = table[8], G = table[9], nfi = table[10], PI = table[15];
    constexpr int KGS = 8 * TR, NIG = 64 * MF_NW / TR;       // floats per k-group of activations; identity-feature residues
    constexpr int MP = 3 * KB, FPL = 16 / KB, FPG = 2 * FPL;
    constexpr int NFI = nsf_nfi(KB);
    float *acts = lds;                                       // [Hp / 8 k-groups][2][TR][4]
    float *xreg = lds + (size_t)(Hp / 8) * KGS;              // [Dp / 8][2][TR][4]
    float *ldp = acts + nsf_tab_floats(KB);                   // log-det partials [G + NIG][TR], behind the staged tables
    const int nitems = (1 + 2 * NB) * NHI + nfi + (LU ? 1 : 0);
    const int *items_all = table + MF_HDR + w * nitems * 3;  // [nitems][nkg, rb | g, sb0]
    const int *items = items_all + ((LU && DIR == 0) ? 3 : 0);   // the network's items (the density direction's LU entry comes first)
    const int fin0 = (1 + 2 * NB) * NHI;                     // index of the wave's first final entry
    const float ld_const = LU ? (DIR == 0 ? lu_lad[0] : -lu_lad[0]) : 0.0f;
    const float *stream = blob + table[16 + w];
    const int lane_b = (TR * hh + n) * 4;
    const int64_t ntiles = (B + TR - 1) / TR;
    MfRing ring;
    mf_ring_start(ring, stream, lane);

    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t row0 = tile * TR;
        const int nrows = (int)((B - row0) < TR ? (B - row0) : TR);
        ring.ap = stream + lane * 4;
        // the tile's prologue / epilogue address arithmetic from a thread index the compiler cannot hoist out of the tile loop: as loop
        // invariants those values stayed live across the products (the last 1-4 spilled registers of the 64-row instantiations)
        int tq = tid;
        asm volatile("" : "+v"(tq));
#include "nsf_tile_load.hpp"
        float ld_ident = 0.0f;
        if constexpr (LU && DIR == 0) {
            MF_BARRIER();
            nw_lu_stage<TR>(ring, items_all, xreg, lane_b, hh, n);
        }
        if constexpr (DIR == 1) {                            // sampling: the identity half's inverse spline comes first (:112-114)
#pragma unroll 1
            for (int i = tq; i < nI * nsf_tabw(KB); i += 64 * MF_NW) acts[i] = tabs[i];
            MF_BARRIER();
            ld_ident = nsf_identity<true, TR, KB>(xreg, acts, p, nI, tq);
        }
        f32x16 h[NHI][NS], t[NHI][NS];
        MF_BARRIER();
        // ---- initial layer: h = b0 + W0 x over the identity positions [0, PI) of the tile ----------------------------------------------
#pragma unroll
        for (int s = 0; s < NHI; ++s) mf_item<NS, false, TR>(ring, items[3 * s], xreg + lane_b + 128 * items[3 * s + 2], h[s]);
        // ---- residual blocks (nets/resnet.py:37-50): t = b1 + W1 relu(h);  h += b2 + W2 relu(t) ----------------------------------
        for (int b = 0; b < NB; ++b) {
            MF_BARRIER();
#pragma unroll
            for (int s = 0; s < NHI; ++s) mf_publish<NS, true, TR>(acts, items[3 * s + 1], items[3 * s + 2], hh, n, h[s]);
            MF_BARRIER();
#pragma unroll
            for (int s = 0; s < NHI; ++s) {
                const int *it = items + 3 * ((1 + 2 * b) * NHI + s);
                mf_item<NS, false, TR>(ring, it[0], acts + lane_b + 128 * it[2], t[s]);
            }
            MF_BARRIER();
#pragma unroll
            for (int s = 0; s < NHI; ++s) mf_publish<NS, true, TR>(acts, items[3 * s + 1], items[3 * s + 2], hh, n, t[s]);
            MF_BARRIER();
#pragma unroll
            for (int s = 0; s < NHI; ++s) {
                const int *it = items + 3 * ((2 + 2 * b) * NHI + s);
                mf_item<NS, true, TR>(ring, it[0], acts + lane_b + 128 * it[2], h[s]);
            }
        }
        // ---- final layer on the raw block output (:104) in groups of four transform features + the spline ----------------------------
#include "nsf_tile_final.hpp"
        if constexpr (LU && DIR == 1) nw_lu_stage<TR>(ring, items_all + 3 * (nitems - 1), xreg, lane_b, hh, n);
#include "nsf_tile_store.hpp"
        MF_BARRIER();                                        // the next tile overwrites the x tile and the activations
    }
}

template <int NHI, int NS, int DIR, bool LU, int TR, int KB>
static int nsf_wide_launch(const void *x, void *y, void *logdet, const void *blob, const int32_t *table, const void *tabs,
                           const void *lu_lad, int64_t B, int Hp, int acc, const RqsParams<float> &p, hipStream_t st) {
    const int64_t ntiles = (B + TR - 1) / TR;
    const int grid = persistent_grid(ntiles);
    const size_t act_floats = (size_t)(Hp / 8) * 8 * TR;       // (>= the staged tables + the log-det partials: 2048 + 24 TR floats)
    const size_t lds = sizeof(float) * (act_floats + (size_t)16 * 8 * TR);
    static LdsOptIn opted;
    if (opt_in_lds(reinterpret_cast<const void *>(&nsf_wide_kernel<NHI, NS, DIR, LU, TR, KB>), lds, opted) != NF_OK) return NF_ENOTSUP;
    hipLaunchKernelGGL((nsf_wide_kernel<NHI, NS, DIR, LU, TR, KB>), dim3((unsigned)grid), dim3(64 * MF_NW), lds, st, (const float *)x, (float *)y,
                       (float *)logdet, (const float *)blob, (const int *)table, (const float *)tabs, (const float *)lu_lad, B, acc, p);
    NF_CHECK_LAUNCH();
    return NF_OK;
}

}  // namespace nf

// Knot tables (cumulative widths | cumulative heights | derivatives, 27 floats per identity feature) of the batch-shared spline
// PiecewiseRationalQuadraticCDF (nsf/coupling.py:170-259), once per parameter version.
extern "C" int nf_nsf_wide_tables(const void *uw, const void *uh, const void *ud, void *tabs, int n_identity, int K, double tail_bound,
                                  double min_bin_width, double min_bin_height, double min_derivative, nf_stream_t stream) {
    if (K != 4 && K != 8 && K != 16) return NF_ENOTSUP;
    if (n_identity < 1 || n_identity > 64 || min_bin_width * K > 1.0 || min_bin_height * K > 1.0) return NF_EINVAL;
    if (!uw || !uh || !ud || !tabs) return NF_EFAULT;
    auto p = nf::make_rqs_params<float>(K, NF_TAILS_LINEAR, tail_bound, 0, 1, 0, 1, min_bin_width, min_bin_height, min_derivative, 1.0);
    hipLaunchKernelGGL(nf::nsf_wide_tables_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const float *)uw, (const float *)uh,
                       (const float *)ud, (float *)tabs, n_identity, p);
    NF_CHECK_LAUNCH();
    return NF_OK;
}

template <int DIR, bool LU, int KB>
static int nsf_wide_dispatch_k(const void *x, void *y, void *logdet, const void *blob, const int32_t *table, const void *tabs,
                               const void *lu_lad, int64_t B, int Hp, int acc, const nf::RqsParams<float> &p, hipStream_t st) {
    if (Hp == 128) return nf::nsf_wide_launch<1, 2, DIR, LU, 128, KB>(x, y, logdet, blob, table, tabs, lu_lad, B, Hp, acc, p, st);
    if (Hp == 256) return nf::nsf_wide_launch<1, 2, DIR, LU, 64, KB>(x, y, logdet, blob, table, tabs, lu_lad, B, Hp, acc, p, st);
    return nf::nsf_wide_launch<2, 2, DIR, LU, 64, KB>(x, y, logdet, blob, table, tabs, lu_lad, B, Hp, acc, p, st);
}

template <int DIR, bool LU>
static int nsf_wide_dispatch(const void *x, void *y, void *logdet, const void *blob, const int32_t *table, const void *tabs,
                             const void *lu_lad, int64_t B, int Hp, int acc, const nf::RqsParams<float> &p, hipStream_t st) {
    if (p.K == 4) return nsf_wide_dispatch_k<DIR, LU, 4>(x, y, logdet, blob, table, tabs, lu_lad, B, Hp, acc, p, st);
    if (p.K == 16) return nsf_wide_dispatch_k<DIR, LU, 16>(x, y, logdet, blob, table, tabs, lu_lad, B, Hp, acc, p, st);
    return nsf_wide_dispatch_k<DIR, LU, 8>(x, y, logdet, blob, table, tabs, lu_lad, B, Hp, acc, p, st);
}

// The coupling layer in one launch; blob / table: flows/nsf_wide_pack.pack_nsf_wide (packed for THIS direction when it carries the
// adjacent LULinearPermute); tabs: nf_nsf_wide_tables; lu_logdet: device scalar log|det| of the LU layer, or NULL (no LU in the pack).
// ... with K bins (4 | 8 | 16; pack and tables built for the same K: flows/nsf_wide_pack.pack_nsf_wide writes it to table[24])
extern "C" int nf_nsf_wide_k(const void *x, void *y, void *logdet, const void *blob, const int32_t *table, const void *tabs,
                             const void *lu_logdet, int64_t B, int D, int hidden_padded, int K, int direction, int acc, double tail_bound,
                             double min_bin_width, double min_bin_height, double min_derivative, nf_stream_t stream) {
    if (B < 0 || D < 2 || D > 128 || direction < 0 || direction > 1) return NF_EINVAL;
    if (acc < NF_LD_SUB || acc > NF_LD_ADD) return NF_EINVAL;
    if (hidden_padded != 128 && hidden_padded != 256 && hidden_padded != 512) return NF_ENOTSUP;
    if (K != 4 && K != 8 && K != 16) return NF_ENOTSUP;
    if (min_bin_width * K > 1.0 || min_bin_height * K > 1.0) return NF_EINVAL;
    if (B == 0) return NF_OK;
    if (!x || !y || !logdet || !blob || !table || !tabs) return NF_EFAULT;
    if ((D & 3) == 0 && nf_misaligned16(x, y)) return NF_EINVAL;        // rows a multiple of 4 floats long move as 16-byte vectors
    auto p = nf::make_rqs_params<float>(K, NF_TAILS_LINEAR, tail_bound, 0, 1, 0, 1, min_bin_width, min_bin_height, min_derivative, 1.0);
    hipStream_t st = (hipStream_t)stream;
    const int Hp = hidden_padded;
    if (direction == 0) {
        if (lu_logdet) return nsf_wide_dispatch<0, true>(x, y, logdet, blob, table, tabs, lu_logdet, B, Hp, acc, p, st);
        return nsf_wide_dispatch<0, false>(x, y, logdet, blob, table, tabs, nullptr, B, Hp, acc, p, st);
    }
    if (lu_logdet) return nsf_wide_dispatch<1, true>(x, y, logdet, blob, table, tabs, lu_logdet, B, Hp, acc, p, st);
    return nsf_wide_dispatch<1, false>(x, y, logdet, blob, table, tabs, nullptr, B, Hp, acc, p, st);
}

extern "C" int nf_nsf_wide(const void *x, void *y, void *logdet, const void *blob, const int32_t *table, const void *tabs,
                           const void *lu_logdet, int64_t B, int D, int hidden_padded, int direction, int acc, double tail_bound,
                           double min_bin_width, double min_bin_height, double min_derivative, nf_stream_t stream) {
    return nf_nsf_wide_k(x, y, logdet, blob, table, tabs, lu_logdet, B, D, hidden_padded, nf::F_K, direction, acc, tail_bound, min_bin_width,
                         min_bin_height, min_derivative, stream);
}
