// nsf_circ.hip -- CircularCoupledRationalQuadraticSpline (normflows/flows/neural_spline/wrapper.py:88-185 -> nsf/coupling.py:71-128,
// 283-318 with per-feature tails, utils/splines.py:28-66 and the PeriodicFeaturesElementwise preprocessing of utils/nn.py:64-129 in
// front of the ResidualNet, nets/resnet.py:92-104) as ONE launch per layer, inference only, float32.  Until now this layer ran as
// library GEMMs + torch.sin / torch.cos + nf_rqs_coupling_ft on a materialised (B, (3K + 1) nT) conditioner output.
//
// The engine and the layer are nsf_wide.hip's (mlp_tile.hpp; read nsf_wide.hip's header first), the tile's load, final stage and store
// are the fragments all three kernels include (nsf_tile.hpp).  What may differ per feature is read from the per-feature table
// (ft_table.hpp: the FT_* rows of nf_arnsf_inverse_ft) laid out in the tile's POSITION order -- identity positions [0, PI), transform
// positions [PI, Dp) -- and copied into LDS behind the x tile once per workgroup (no vector-memory request joins the weight ring's):
//   * tails and bound of every feature (list tails, utils/splines.py:48-57): a linear feature's end derivatives are the constant, a
//     circular one's last derivative is its first; OUTSIDE its interval a coordinate gives output 0 and log-det 0 (not the identity:
//     the list branch never copies the outside inputs), in both halves.  The final Linear has 3K + 1 rows per feature; the last one is
//     always overwritten and the packer drops it, derivative 0 travels in the slot the linear-tails layout pads (slot 3K - 1), so the
//     lane's parameter list is rqs_regs_h's with the edge logit chosen per feature (nsf_regs_ft);
//   * the conditioner's input: the initial layer contracts over the FED identity positions, w_sin sin(s x) + w_cos cos(s x) + bias for
//     a circular identity feature and the value itself otherwise (ft_feed).  The feed is written into the activation region (free until
//     the first publish) in B-operand order and the initial item reads it there; the x tile keeps the raw values: in the density
//     direction the identity output is the batch-shared spline of the RAW value (nsf/coupling.py:83-92), in the sampling direction the
//     feed is taken of the identity half after its inverse spline (:112-118).  Only identity positions are fed: a NaN in a transform
//     column still never reaches the conditioner.
// No LU, no context.  Extra work against nsf_wide: PI values fed per row (one sinf / cosf pair per circular identity feature) and one
// more barrier per tile.
#include "nsf_tile.hpp"
#include "ft_table.hpp"

#define NSF_FT_STRIDE 128                                    // row stride of the LDS copy of the per-feature table (Dp <= 128)

namespace nf {

// knot tables of the batch-shared spline with per-feature tails and bounds: K + 1 derivative logits per feature, the edge ones
// overwritten by type (rqs_dlogit's dfull branch)
__global__ void nsf_circ_tables_kernel(const float *__restrict__ uw, const float *__restrict__ uh, const float *__restrict__ ud,
                                       const int *__restrict__ tails_i, const float *__restrict__ bound_i, float *__restrict__ tab,
                                       int nI, RqsParams<float> p) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nI) return;
    const int K = p.K;
    const RqsParams<float> q = rqs_feature_params(p, tails_i, bound_i, j);
    const float *wj = uw + j * K, *hj = uh + j * K, *dj = ud + j * (K + 1);
    auto wacc = [=](int k) { return wj[k]; };
    auto hacc = [=](int k) { return hj[k]; };
    auto dacc = [=](int k) { return dj[k]; };
    rqs_build_table<float>(q, wacc, hacc, dacc, tab + j * 3 * (K + 1));
}

// rqs_regs_h on the lane's parameter list of a list-tails feature: K widths | K heights | derivatives 1 .. K - 1 | derivative 0.
template <bool INVERSE, int KB>
__device__ __forceinline__ void nsf_regs_ft(const RqsParams<float> &p, float bound, int tails, float x, const float (&prm)[3 * KB],
                                            float &y, float &lad) {
    RqsParams<float> q = p;
    q.left = q.bottom = -bound;
    q.right = q.top = bound;
    q.edge_logit = tails == NF_TAILS_CIRCULAR ? prm[3 * KB - 1] : p.edge_logit;
    float yy, ll;
    rqs_regs_h<INVERSE, KB>(q, x, prm, yy, ll);              // (identity and log-det 0 outside)
    y = (x >= -bound && x <= bound) ? yy : 0.0f;             // false for NaN: 0 (utils/splines.py:31)
    lad = ll;
}

// nsf_identity with every feature's interval read from its own knot table (cumw[0] = -bound, cumw[K] = bound): 0 / 0 outside
template <bool INV, int TR, int KB>
__device__ __forceinline__ float nsf_identity_ft(float *xreg, const float *tabs, int nI, int tid) {
    const int n = tid % TR;
    float ld = 0.0f;
#pragma unroll 1
    for (int i = tid / TR; i < nI; i += 64 * MF_NW / TR) {
        float *xp = xreg + nsf_xidx<TR>(i, n);
        const float *tab = tabs + i * nsf_tabw(KB);
        const float x = *xp;
        const float *srch = INV ? tab + (KB + 1) : tab;
        int bin = 0;
#pragma unroll
        for (int k = 1; k < KB; ++k) bin = (x >= srch[k]) ? k : bin;
        const float cw0 = tab[bin], cw1 = tab[bin + 1], ch0 = tab[KB + 1 + bin], ch1 = tab[KB + 2 + bin];
        const float d0 = tab[2 * (KB + 1) + bin], d1 = tab[2 * (KB + 1) + bin + 1];
        float yy, ll;
        rqs_eval_bin_fast<INV>(x, cw0, cw1 - cw0, ch0, ch1 - ch0, d0, d1, yy, ll);
        const bool inside = x >= tab[0] && x <= tab[KB];
        *xp = inside ? yy : 0.0f;
        ld += inside ? ll : 0.0f;
    }
    return ld;
}

// Instantiated as nsf_wide_kernel's first two shapes without the LU: (NHI, NS, TR) = (1, 2, 128) Hp 128, (1, 2, 64) Hp 256 (Hp 512 is
// not built: nsf_wide's (2, 2, 64) instantiations sit at the register limit).  Items per wave: nsf_wide's (flows/nsf_circ_pack.py).
template <int NHI, int NS, int DIR, int TR, int KB>
__global__ void __launch_bounds__(64 * MF_NW, 1)
nsf_circ_kernel(const float *__restrict__ x, float *__restrict__ y, float *__restrict__ logdet, const float *__restrict__ blob,
                const int *__restrict__ table, const float *__restrict__ ftable, const float *__restrict__ tabs, int64_t B,
                int acc_mode, RqsParams<float> p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, n = lane & 31, hh = lane >> 5;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int D = table[0], Dp = table[1], Hp = table[3], NB = table[4], nI = table[5], nT = table[6], par_i = table[7], G = table[9],
              nfi = table[10], PI = table[15];
    constexpr int KGS = 8 * TR, NIG = 64 * MF_NW / TR;
    constexpr int MP = 3 * KB, FPL = 16 / KB, FPG = 2 * FPL;
    constexpr int NFI = nsf_nfi(KB);
    float *acts = lds;                                       // [Hp / 8 k-groups][2][TR][4]; first the fed identity positions
    float *xreg = lds + (size_t)(Hp / 8) * KGS;              // [128 / 8][2][TR][4]
    float *ftl = xreg + (size_t)16 * KGS;                    // [8][NSF_FT_STRIDE]: the per-feature table by position
    float *ldp = acts + nsf_tab_floats(KB);
    const int *items = table + MF_HDR + w * ((1 + 2 * NB) * NHI + nfi) * 3;
    const int fin0 = (1 + 2 * NB) * NHI;
    const float ld_const = 0.0f;
    const float *stream = blob + table[16 + w];
    const int lane_b = (TR * hh + n) * 4;
    const int64_t ntiles = (B + TR - 1) / TR;
    for (int i = tid; i < 8 * NSF_FT_STRIDE; i += 64 * MF_NW) {
        const int c = i % NSF_FT_STRIDE;
        ftl[i] = c < Dp ? ftable[(i / NSF_FT_STRIDE) * Dp + c] : 0.0f;
    }
    MfRing ring;
    mf_ring_start(ring, stream, lane);

    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t row0 = tile * TR;
        const int nrows = (int)((B - row0) < TR ? (B - row0) : TR);
        ring.ap = stream + lane * 4;
        int tq = tid;
        asm volatile("" : "+v"(tq));
#include "nsf_tile_load.hpp"
        float ld_ident = 0.0f;
        if constexpr (DIR == 1) {                            // sampling: the identity half's inverse spline first (nsf/coupling.py:112-114)
#pragma unroll 1
            for (int i = tq; i < nI * nsf_tabw(KB); i += 64 * MF_NW) acts[i] = tabs[i];
            MF_BARRIER();
            ld_ident = nsf_identity_ft<true, TR, KB>(xreg, acts, nI, tq);
        }
        MF_BARRIER();                                        // the tile (and ftl, first tile) is complete, the staged tables are free
        {   // the conditioner's input: the fed identity positions in B-operand order at the start of the activation region
            const int r = tq % TR, cg = tq / TR;
#pragma unroll 1
            for (int ps = cg; ps < PI; ps += NIG) acts[nsf_xidx<TR>(ps, r)] = ft_feed(ftl, NSF_FT_STRIDE, ps, xreg[nsf_xidx<TR>(ps, r)]);
        }
        f32x16 h[NHI][NS], t[NHI][NS];
        MF_BARRIER();
        // ---- initial layer: h = b0 + W0 feed(x) over the identity positions [0, PI) --------------------------------------------------
#pragma unroll
        for (int s = 0; s < NHI; ++s) mf_item<NS, false, TR>(ring, items[3 * s], acts + lane_b + 128 * items[3 * s + 2], h[s]);
        // ---- residual blocks (nets/resnet.py:37-50): t = b1 + W1 relu(h);  h += b2 + W2 relu(t) (= nsf_wide.hip) ------------------
        for (int b = 0; b < NB; ++b) {
            MF_BARRIER();                                    // (first block: every wave has read the fed positions)
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
        // ---- final layer in groups of transform features + the per-feature spline; the identity half's spline in the density direction
#define NSF_TILE_FT
#include "nsf_tile_final.hpp"
#undef NSF_TILE_FT
#include "nsf_tile_store.hpp"
        MF_BARRIER();
    }
}

template <int NHI, int NS, int DIR, int TR, int KB>
static int nsf_circ_launch(const void *x, void *y, void *logdet, const void *blob, const int32_t *table, const void *ftable,
                           const void *tabs, int64_t B, int Hp, int acc, const RqsParams<float> &p, hipStream_t st) {
    const int64_t ntiles = (B + TR - 1) / TR;
    const int grid = persistent_grid(ntiles);
    const size_t act_floats = (size_t)(Hp / 8) * 8 * TR;
    const size_t lds = sizeof(float) * (act_floats + (size_t)16 * 8 * TR + 8 * NSF_FT_STRIDE);
    static LdsOptIn opted;
    if (opt_in_lds(reinterpret_cast<const void *>(&nsf_circ_kernel<NHI, NS, DIR, TR, KB>), lds, opted) != NF_OK) return NF_ENOTSUP;
    hipLaunchKernelGGL((nsf_circ_kernel<NHI, NS, DIR, TR, KB>), dim3((unsigned)grid), dim3(64 * MF_NW), lds, st, (const float *)x,
                       (float *)y, (float *)logdet, (const float *)blob, (const int *)table, (const float *)ftable, (const float *)tabs, B,
                       acc, p);
    NF_CHECK_LAUNCH();
    return NF_OK;
}

template <int DIR, int KB>
static int nsf_circ_dispatch_k(const void *x, void *y, void *logdet, const void *blob, const int32_t *table, const void *ftable,
                               const void *tabs, int64_t B, int Hp, int acc, const RqsParams<float> &p, hipStream_t st) {
    if (Hp == 128) return nsf_circ_launch<1, 2, DIR, 128, KB>(x, y, logdet, blob, table, ftable, tabs, B, Hp, acc, p, st);
    return nsf_circ_launch<1, 2, DIR, 64, KB>(x, y, logdet, blob, table, ftable, tabs, B, Hp, acc, p, st);
}

template <int DIR>
static int nsf_circ_dispatch(const void *x, void *y, void *logdet, const void *blob, const int32_t *table, const void *ftable,
                             const void *tabs, int64_t B, int Hp, int acc, const RqsParams<float> &p, hipStream_t st) {
    if (p.K == 4) return nsf_circ_dispatch_k<DIR, 4>(x, y, logdet, blob, table, ftable, tabs, B, Hp, acc, p, st);
    if (p.K == 16) return nsf_circ_dispatch_k<DIR, 16>(x, y, logdet, blob, table, ftable, tabs, B, Hp, acc, p, st);
    return nsf_circ_dispatch_k<DIR, 8>(x, y, logdet, blob, table, ftable, tabs, B, Hp, acc, p, st);
}

}  // namespace nf

// Knot tables of the batch-shared spline under list tails (include/nf_mi355x.h): derivatives (n_identity, K + 1), type and bound per
// identity feature.
extern "C" int nf_nsf_wide_tables_ft(const void *uw, const void *uh, const void *ud, const int32_t *tails_i, const void *bound_i,
                                     void *tabs, int n_identity, int K, double min_bin_width, double min_bin_height,
                                     double min_derivative, nf_stream_t stream) {
    if (K != 4 && K != 8 && K != 16) return NF_ENOTSUP;
    if (n_identity < 1 || n_identity > 64 || min_bin_width * K > 1.0 || min_bin_height * K > 1.0) return NF_EINVAL;
    if (!uw || !uh || !ud || !tails_i || !bound_i || !tabs) return NF_EFAULT;
    auto p = nf::make_rqs_params<float>(K, NF_TAILS_FEATURE, 1.0, 0, 1, 0, 1, min_bin_width, min_bin_height, min_derivative, 1.0);
    hipLaunchKernelGGL(nf::nsf_circ_tables_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const float *)uw, (const float *)uh,
                       (const float *)ud, (const int *)tails_i, (const float *)bound_i, (float *)tabs, n_identity, p);
    NF_CHECK_LAUNCH();
    return NF_OK;
}

// The circular coupling layer in one launch (include/nf_mi355x.h); blob / table / ftable: flows/nsf_circ_pack.pack_nsf_circ, tabs:
// nf_nsf_wide_tables_ft.
extern "C" int nf_nsf_wide_ft(const void *x, void *y, void *logdet, const void *blob, const int32_t *table, const void *ftable,
                              const void *tabs, int64_t B, int D, int hidden_padded, int K, int direction, int acc,
                              double min_bin_width, double min_bin_height, double min_derivative, nf_stream_t stream) {
    if (B < 0 || D < 2 || D > 128 || direction < 0 || direction > 1) return NF_EINVAL;
    if (acc < NF_LD_SUB || acc > NF_LD_ADD) return NF_EINVAL;
    // Hp 512 (two hidden items per wave) is not built: nsf_wide's instantiations of that shape leave no register for the per-feature reads
    if (hidden_padded != 128 && hidden_padded != 256) return NF_ENOTSUP;
    if (K != 4 && K != 8 && K != 16) return NF_ENOTSUP;
    if (min_bin_width * K > 1.0 || min_bin_height * K > 1.0) return NF_EINVAL;
    if (B == 0) return NF_OK;
    if (!x || !y || !logdet || !blob || !table || !ftable || !tabs) return NF_EFAULT;
    if ((D & 3) == 0 && nf_misaligned16(x, y)) return NF_EINVAL;        // rows a multiple of 4 floats long move as 16-byte vectors
    // bounds and types come from the table; the launch-wide interval is never read
    auto p = nf::make_rqs_params<float>(K, NF_TAILS_LINEAR, 1.0, 0, 1, 0, 1, min_bin_width, min_bin_height, min_derivative, 1.0);
    hipStream_t st = (hipStream_t)stream;
    if (direction == 0) return nf::nsf_circ_dispatch<0>(x, y, logdet, blob, table, ftable, tabs, B, hidden_padded, acc, p, st);
    return nf::nsf_circ_dispatch<1>(x, y, logdet, blob, table, ftable, tabs, B, hidden_padded, acc, p, st);
}
