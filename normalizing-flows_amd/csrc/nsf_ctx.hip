// nsf_ctx.hip -- the CONDITIONAL CoupledRationalQuadraticSpline (wrapper.py:14-85 with num_context_channels = C; ResidualNet with
// context_features, nets/resnet.py:37-50, 92-104; ConditionalNormalizingFlow, core.py:216-366) as ONE launch per layer, inference only.
// Until now every layer that received a context ran its conditioner as eager modules (cat -> Linear -> per block relu / Linear / relu /
// Linear / context_layer / cat / glu / add -> Linear) and handed a materialised (B, (3K - 1) nT) output to nf_rqs_coupling.
//
// The engine and the layer are nsf_wide.hip's (mlp_tile.hpp; read its header first), the tile's load, final stage and store are the
// fragments both kernels include (nsf_tile.hpp); the context changes the network in two places:
//   * the initial layer reads cat(identity features, context): the row's C context values sit in the x tile at positions
//     [Dp, Dp + PC) (PC = C rounded up to 32, the padding zero; Dp + PC <= 128, so the LDS size does not change), and the layer is two
//     items: the identity positions [0, PI) as in nsf_wide, then an ADD item over the context positions (zero bias group);
//   * every residual block ends in a GLU gate (resnet.py:46-49): h += (b2 + W2 relu(t)) * sigmoid(bc + Wc ctx).  After relu(t) is
//     published, t is free: per hidden item the gate item (over the context positions) goes into t, sigmoid in place; then
//     b2 + W2 relu(t) goes into ONE extra accumulator set u and h += u * t.  Gate and W2 alternate per hidden item (one gate and one u live
//     next to h when a wave owns two items).
// The context is read with a row stride `ldc` (0: one observation for every row, context.expand(B, C) without a copy).  A context row
// only reaches its own tile column (B operand = row), so a NaN in one row's context stays in that row; the transform columns still never
// reach the conditioner.  Extra work: (1 + NB) C H MACs per row.
#include "nsf_tile.hpp"

namespace nf {

// Instantiated as nsf_wide_kernel's first two shapes without the LU: (NHI, NS, TR) = (1, 2, 128) Hp 128, (1, 2, 64) Hp 256.  Hp 512
// ((2, 2, 64)) compiles but spills 26-31 registers (108-120 bytes of scratch) even with gate and W2 alternating: not built.
// Items per wave (flows/nsf_ctx_pack.py): NHI identity items, NHI context items, per block NHI W1 items then per hidden item its gate
// and W2 items, nfi finals.
template <int NHI, int NS, int DIR, int TR, int KB>
__global__ void __launch_bounds__(64 * MF_NW, 1)
nsf_ctx_kernel(const float *__restrict__ x, const float *__restrict__ ctx, float *__restrict__ y, float *__restrict__ logdet,
               const float *__restrict__ blob, const int *__restrict__ table, const float *__restrict__ tabs, int64_t B, int64_t ldc,
               int C, int PC, int Dp, int acc_mode, RqsParams<float> p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, n = lane & 31, hh = lane >> 5;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int D = table[0], Hp = table[3], NB = table[4], nI = table[5], nT = table[6], par_i = table[7], G = table[9], nfi = table[10],
              PI = table[15];
    constexpr int KGS = 8 * TR, NIG = 64 * MF_NW / TR;
    constexpr int MP = 3 * KB, FPL = 16 / KB, FPG = 2 * FPL;
    constexpr int NFI = nsf_nfi(KB);
    float *acts = lds;                                       // [Hp / 8 k-groups][2][TR][4]
    float *xreg = lds + (size_t)(Hp / 8) * KGS;              // [128 / 8][2][TR][4]: identity | transform | context positions
    float *ldp = acts + nsf_tab_floats(KB);
    const int nitems = (2 + 3 * NB) * NHI + nfi;
    const int *items = table + MF_HDR + w * nitems * 3;
    const int fin0 = (2 + 3 * NB) * NHI;
    const float ld_const = 0.0f;
    const float *stream = blob + table[16 + w];
    const int lane_b = (TR * hh + n) * 4;
    const float *xctx = xreg + (size_t)(Dp / 8) * KGS;       // B operand of the context positions (Dp is a multiple of 32)
    const int64_t ntiles = (B + TR - 1) / TR;
    MfRing ring;
    mf_ring_start(ring, stream, lane);

    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t row0 = tile * TR;
        const int nrows = (int)((B - row0) < TR ? (B - row0) : TR);
        ring.ap = stream + lane * 4;
        int tq = tid;
        asm volatile("" : "+v"(tq));
#define NSF_TILE_CONTEXT                                     // the fragment also loads the context row
#include "nsf_tile_load.hpp"
#undef NSF_TILE_CONTEXT
        float ld_ident = 0.0f;
        if constexpr (DIR == 1) {                            // sampling: the identity half's inverse spline first (nsf/coupling.py:112-114)
#pragma unroll 1
            for (int i = tq; i < nI * nsf_tabw(KB); i += 64 * MF_NW) acts[i] = tabs[i];
            MF_BARRIER();
            ld_ident = nsf_identity<true, TR, KB>(xreg, acts, p, nI, tq);
        }
        f32x16 h[NHI][NS], t[NHI][NS], u[NS];
        MF_BARRIER();
        // ---- initial layer on cat(identity, context): h = b0 + W0[:, :nI] x_ident, then h += W0[:, nI:] ctx ----------------------------
#pragma unroll
        for (int s = 0; s < NHI; ++s) mf_item<NS, false, TR>(ring, items[3 * s], xreg + lane_b + 128 * items[3 * s + 2], h[s]);
#pragma unroll
        for (int s = 0; s < NHI; ++s) {
            const int *it = items + 3 * (NHI + s);
            mf_item<NS, true, TR>(ring, it[0], xctx + lane_b + 128 * it[2], h[s]);
        }
        // ---- residual blocks with the GLU gate (nets/resnet.py:37-50): t = b1 + W1 relu(h);  h += (b2 + W2 relu(t)) sigmoid(bc + Wc ctx)
        for (int b = 0; b < NB; ++b) {
            const int *blk = items + 3 * (2 + 3 * b) * NHI;
            MF_BARRIER();
#pragma unroll
            for (int s = 0; s < NHI; ++s) mf_publish<NS, true, TR>(acts, items[3 * s + 1], items[3 * s + 2], hh, n, h[s]);
            MF_BARRIER();
#pragma unroll
            for (int s = 0; s < NHI; ++s) {
                const int *it = blk + 3 * s;
                mf_item<NS, false, TR>(ring, it[0], acts + lane_b + 128 * it[2], t[s]);
            }
            MF_BARRIER();
#pragma unroll
            for (int s = 0; s < NHI; ++s) mf_publish<NS, true, TR>(acts, items[3 * s + 1], items[3 * s + 2], hh, n, t[s]);
            MF_BARRIER();
#pragma unroll
            for (int s = 0; s < NHI; ++s) {                  // t is free: per hidden item the gate into t[s], then W2 into u
                const int *it = blk + 3 * (NHI + 2 * s);
                mf_item<NS, false, TR>(ring, it[0], xctx + lane_b + 128 * it[2], t[s]);
#pragma unroll
                for (int q = 0; q < NS; ++q)
#pragma unroll
                    for (int r = 0; r < 16; ++r) t[s][q][r] = 1.0f / (1.0f + __expf(-t[s][q][r]));
                mf_item<NS, false, TR>(ring, it[3], acts + lane_b + 128 * it[5], u);
#pragma unroll
                for (int q = 0; q < NS; ++q)
#pragma unroll
                    for (int r = 0; r < 16; ++r) h[s][q][r] += u[q][r] * t[s][q][r];
            }
        }
        // ---- final layer on the raw block output in groups of transform features + the spline (= nsf_wide.hip) ----------------------
#include "nsf_tile_final.hpp"
#include "nsf_tile_store.hpp"
        MF_BARRIER();
    }
}

template <int NHI, int NS, int DIR, int TR, int KB>
static int nsf_ctx_launch(const void *x, const void *ctx, void *y, void *logdet, const void *blob, const int32_t *table, const void *tabs,
                          int64_t B, int64_t ldc, int C, int PC, int Dp, int Hp, int acc, const RqsParams<float> &p, hipStream_t st) {
    const int64_t ntiles = (B + TR - 1) / TR;
    const int grid = persistent_grid(ntiles);
    const size_t act_floats = (size_t)(Hp / 8) * 8 * TR;
    const size_t lds = sizeof(float) * (act_floats + (size_t)16 * 8 * TR);      // x tile: 128 positions (Dp + PC <= 128)
    static LdsOptIn opted;
    if (opt_in_lds(reinterpret_cast<const void *>(&nsf_ctx_kernel<NHI, NS, DIR, TR, KB>), lds, opted) != NF_OK) return NF_ENOTSUP;
    hipLaunchKernelGGL((nsf_ctx_kernel<NHI, NS, DIR, TR, KB>), dim3((unsigned)grid), dim3(64 * MF_NW), lds, st, (const float *)x,
                       (const float *)ctx, (float *)y, (float *)logdet, (const float *)blob, (const int *)table, (const float *)tabs, B, ldc,
                       C, PC, Dp, acc, p);
    NF_CHECK_LAUNCH();
    return NF_OK;
}

template <int DIR, int KB>
static int nsf_ctx_dispatch_k(const void *x, const void *ctx, void *y, void *logdet, const void *blob, const int32_t *table,
                              const void *tabs, int64_t B, int64_t ldc, int C, int PC, int Dp, int Hp, int acc, const RqsParams<float> &p,
                              hipStream_t st) {
    if (Hp == 128) return nsf_ctx_launch<1, 2, DIR, 128, KB>(x, ctx, y, logdet, blob, table, tabs, B, ldc, C, PC, Dp, Hp, acc, p, st);
    return nsf_ctx_launch<1, 2, DIR, 64, KB>(x, ctx, y, logdet, blob, table, tabs, B, ldc, C, PC, Dp, Hp, acc, p, st);
}

template <int DIR>
static int nsf_ctx_dispatch(const void *x, const void *ctx, void *y, void *logdet, const void *blob, const int32_t *table,
                            const void *tabs, int64_t B, int64_t ldc, int C, int PC, int Dp, int Hp, int acc, const RqsParams<float> &p,
                            hipStream_t st) {
    if (p.K == 4) return nsf_ctx_dispatch_k<DIR, 4>(x, ctx, y, logdet, blob, table, tabs, B, ldc, C, PC, Dp, Hp, acc, p, st);
    if (p.K == 16) return nsf_ctx_dispatch_k<DIR, 16>(x, ctx, y, logdet, blob, table, tabs, B, ldc, C, PC, Dp, Hp, acc, p, st);
    return nsf_ctx_dispatch_k<DIR, 8>(x, ctx, y, logdet, blob, table, tabs, B, ldc, C, PC, Dp, Hp, acc, p, st);
}

}  // namespace nf

// The conditional coupling layer in one launch (include/nf_mi355x.h); blob / table: flows/nsf_ctx_pack.pack_nsf_ctx, tabs:
// nf_nsf_wide_tables (the batch-shared spline does not see the context).
extern "C" int nf_nsf_wide_ctx(const void *x, const void *context, void *y, void *logdet, const void *blob, const int32_t *table,
                               const void *tabs, int64_t B, int64_t ldc, int D, int C, int hidden_padded, int K, int direction, int acc,
                               double tail_bound, double min_bin_width, double min_bin_height, double min_derivative,
                               nf_stream_t stream) {
    if (B < 0 || D < 2 || D > 128 || C < 1 || ldc < 0 || direction < 0 || direction > 1) return NF_EINVAL;
    if (acc < NF_LD_SUB || acc > NF_LD_ADD) return NF_EINVAL;
    // Hp 512 (two hidden items per wave) is not built: with the gate and u next to h it spills 26-31 registers
    if (hidden_padded != 128 && hidden_padded != 256) return NF_ENOTSUP;
    if (K != 4 && K != 8 && K != 16) return NF_ENOTSUP;
    if (min_bin_width * K > 1.0 || min_bin_height * K > 1.0) return NF_EINVAL;
    // positions of the x tile: identity (D / 2 rounded either way, padded to 32) + transform (likewise) + context (C padded to 32)
    const int Dp = (D / 2 + 31) / 32 * 32 + ((D + 1) / 2 + 31) / 32 * 32;
    if (C > 128) return NF_ENOTSUP;
    const int PC = (C + 31) / 32 * 32;
    if (Dp + PC > 128) return NF_ENOTSUP;
    if (B == 0) return NF_OK;
    if (!x || !context || !y || !logdet || !blob || !table || !tabs) return NF_EFAULT;
    if ((D & 3) == 0 && nf_misaligned16(x, y)) return NF_EINVAL;        // rows a multiple of 4 floats long move as 16-byte vectors
    auto p = nf::make_rqs_params<float>(K, NF_TAILS_LINEAR, tail_bound, 0, 1, 0, 1, min_bin_width, min_bin_height, min_derivative, 1.0);
    hipStream_t st = (hipStream_t)stream;
    if (direction == 0) return nf::nsf_ctx_dispatch<0>(x, context, y, logdet, blob, table, tabs, B, ldc, C, PC, Dp, hidden_padded, acc, p, st);
    return nf::nsf_ctx_dispatch<1>(x, context, y, logdet, blob, table, tabs, B, ldc, C, PC, Dp, hidden_padded, acc, p, st);
}
