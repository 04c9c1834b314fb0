// made_fwd_ft.hip -- the density direction of the autoregressive rational-quadratic spline layers whose features differ from one
// another (neural_spline/autoregressive.py:94-134 over affine/autoregressive.py:24-27: ONE pass of MADE, nets/made.py:296-304, then
// utils/splines.py:16-219 element-wise) as ONE launch: CircularAutoregressiveRationalQuadraticSpline (neural_spline/wrapper.py:247-311:
// list tails, the periodic preprocessing of utils/nn.py:64-129 in front of the MADE, a tensor tail bound) and
// AutoregressiveRationalQuadraticSpline(permute_mask=True) (:186-244).  The sampling direction of the same layers is
// nf_arnsf_inverse_ft (maf_inverse.hip); until now their density ran as eager MaskedLinear modules + torch.sin / torch.cos +
// nf_rqs_coupling_ft.
//
// The engine, the hidden layers and their items are made_fwd.hip's (mlp_tile.hpp; read made_fwd.hip's header first).  What differs:
//   * DEGREE ORDER.  Position f of the x tile holds the input column of degree f + 1 (col[f] of the per-feature table, ft_table.hpp,
//     in degree order as for nf_arnsf_inverse_ft): the tile is gathered on the way in and scattered on the way out, the initial
//     layer's columns and the final layer's items are packed in that order, so the masks are block lower-triangular whatever the
//     permutation (flows/made_pack.pack_made_forward_ft).
//   * PERIODIC FEED.  The initial layer contracts over ft_feed of the tile (w_sin sin(s x) + w_cos cos(s x) + bias for a circular
//     coordinate, the value otherwise), written into the activation region, which is free until the first publish (nsf_circ.hip's
//     arrangement); the x tile keeps the raw values for the spline.
//   * THE TABLE IS READ THROUGH THE SCALAR CACHE.  Every index into it is wave-uniform (wave w loads / feeds / stores positions
//     w, w + 8, ...; a final item is one feature) and every read is unconditional, so they are s_load's on the constant cache
//     (checked in the disassembly: the only vector loads with other than ring or x addresses are ld_store's read of the caller's
//     accumulator): no vector-memory request joins the weight ring's, and no LDS is needed (at 512 hidden slots the activations
//     and the x tile fill the 160 KB).
//   * FINAL LAYER: ONE ITEM PER FEATURE, any K with mult <= 32 (K <= 11 with scalar linear tails, K <= 10 otherwise).  A feature's rows fill one 32-row block in FIXED slots -- widths
//     0..K-1, heights 11..11+K-1, derivative logit j (0..K) in slot 21 + j -- for both sample blocks of the tile (NS = 2: a weight
//     fragment feeds two MFMAs at either width).  The two lane-halves then exchange sixteen registers so that lane = row of the tile
//     holds all 32 slots, and the spline runs on them with static register indices and wave-uniform guards k < K (ftd_spline).  Rows
//     per feature: 3K - 1 | 3K | 3K + 1 (scalar linear | circular | no tails), 3K + 1 with list tails, whose last derivative row is
//     always overwritten (utils/splines.py:48-57) and whose outside inputs give 0 / log-det 0.
//   * log-det: a lane sums its row over the wave's features, the eight waves' sums are added in a fixed order (deterministic).
// No 1 / sqrt(hidden) scaling: the reference tests hasattr(net, "hidden_features"), which its MADE never has.
#include "mlp_tile.hpp"
#include "ft_table.hpp"

namespace nf {

constexpr int FTD_KMAX = 11;                 // bins: 3K - 1 <= 32 (scalar linear tails), 3K + 1 <= 32 otherwise (K <= 10)
constexpr int FTD_H0 = 11, FTD_D0 = 21;      // first slot of the heights / slot of derivative logit 0 (flows/made_pack.FT_SLOT_*)

// The density-direction spline of common.hpp rqs_element on a register-resident slot list; K, the tails type and the interval are
// wave-uniform.  p.dfull: list tails (0 / 0 outside); otherwise the identity outside.
__device__ __forceinline__ void ftd_spline(const RqsParams<float> &p, float x, const float (&prm)[32], float &y, float &lad) {
    int K = p.K;
    asm volatile("" : "+s"(K));      // (not loop-invariant for the compiler: hoisted, the ~40 guards k < K cost a hundred SGPRs and spills)
    // branch-free: every guard k < K is a select on a wave-uniform condition
    float mw = prm[0], mh = prm[FTD_H0];
#pragma unroll
    for (int k = 1; k < FTD_KMAX; ++k) {
        mw = k < K ? fmaxf(mw, prm[k]) : mw;
        mh = k < K ? fmaxf(mh, prm[FTD_H0 + k]) : mh;
    }
    float ew[FTD_KMAX], eh[FTD_KMAX], sw = 0.0f, sh = 0.0f;
#pragma unroll
    for (int k = 0; k < FTD_KMAX; ++k) {
        ew[k] = k < K ? fexp(prm[k] - mw) : 0.0f;
        eh[k] = k < K ? fexp(prm[FTD_H0 + k] - mh) : 0.0f;
        sw += ew[k];
        sh += eh[k];
    }
    const float rw = p.scale_w * frcp(sw), rh = p.scale_h * frcp(sh);
    // cumulative sums = knots; the bin search of utils/splines.py:146-157 on the way (the knots increase: `x >= knot` holds for a prefix)
    float cw = 0.0f, ch = 0.0f, kx = p.left, ky = p.bottom;
    float blo = p.left, bhi = p.left, olo = p.bottom, ohi = p.bottom;
    int bin = 0;
#pragma unroll
    for (int k = 0; k < FTD_KMAX; ++k) {
        cw += p.min_w + rw * ew[k];
        ch += p.min_h + rh * eh[k];
        const float nx = k == K - 1 ? p.right : (p.right - p.left) * cw + p.left;
        const float ny = k == K - 1 ? p.top : (p.top - p.bottom) * ch + p.bottom;
        const bool take = k == 0 || (k < K && x >= kx);
        bin = take ? k : bin;
        blo = take ? kx : blo;
        bhi = take ? nx : bhi;
        olo = take ? ky : olo;
        ohi = take ? ny : ohi;
        kx = nx;
        ky = ny;
    }
    // derivative logit j sits in slot 21 + j (the packer moves the rows of every tails type there); the edges by type (:34-57)
    float l0 = p.edge_logit, l1 = p.edge_logit;
#pragma unroll
    for (int j = 0; j <= FTD_KMAX; ++j) {
        float lj = FTD_D0 + j < 32 ? prm[FTD_D0 + j < 32 ? FTD_D0 + j : 0] : p.edge_logit;      // (logit 11: scalar linear tails only, an edge)
        lj = (p.tails == NF_TAILS_LINEAR && (j == 0 || j == K)) ? p.edge_logit : lj;
        lj = (p.tails == NF_TAILS_CIRCULAR && j == K) ? prm[FTD_D0] : lj;
        l0 = j == bin ? lj : l0;
        l1 = j == bin + 1 ? lj : l1;
    }
    const float d0 = p.min_d + fsoftplus(l0), d1 = p.min_d + fsoftplus(l1);
    float yy, ll;
    rqs_eval_bin_fast<false>(x, blo, bhi - blo, olo, ohi - olo, d0, d1, yy, ll);
    const bool inside = rqs_inside(p, x);                  // (false for NaN)
    y = inside ? yy : (p.dfull ? 0.0f : x);
    lad = inside ? ll : 0.0f;
}

// position f of a [Dp / 8][2][64 rows][4] tile (B-operand order), row r
__device__ __forceinline__ int ftd_xidx(int f, int r) { return ((f >> 2) * 64 + r) * 4 + (f & 3); }

template <int NSB>
__global__ void __launch_bounds__(64 * MF_NW, 1)
made_fwd_ft_kernel(const float *__restrict__ x, float *__restrict__ y, float *__restrict__ logdet, const float *__restrict__ blob,
                   const int *__restrict__ table, const float *__restrict__ ftable, int64_t B, int acc_mode, RqsParams<float> p) {
    constexpr int TR = MF_ROWS, NS = NSB;
    constexpr int HRB = 8 * NSB;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *acts = lds;                                  // [HRB * 4 k-groups][2][64][4]; first the fed tile
    float *xreg = lds + (size_t)HRB * 4 * 8 * TR;       // [Dp / 8][2][64][4]: the raw tile in degree order, then y
    const int tid = threadIdx.x, lane = tid & 63, n = lane & 31, hh = lane >> 5;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int D = table[0], Dp = table[1], NB = table[5], nfi = table[8], nitems = table[10];
    const int *items = table + MF_HDR + w * nitems * 2;       // [nitems][nkg, rb | feature]
    const int *fit = items + 2 * (2 + 4 * NB);
    const float *stream = blob + table[16 + w];
    const int *ftc = reinterpret_cast<const int *>(ftable) + FT_COL * D;
    const int *ftt = reinterpret_cast<const int *>(ftable) + FT_TAILS * D;
    const float *ftb = ftable + FT_BOUND * D;
    const int rbs[2] = {w, HRB - 1 - w};
    const int sb0s[2] = {0, NSB == 2 ? 0 : 1};
    const int lane_b = (TR * hh + n) * 4;
    const int64_t ntiles = (B + TR - 1) / TR;
    MfRing ring;
    mf_ring_start(ring, stream, lane);

    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t row0 = tile * TR;
        const int nrows = (int)((B - row0) < TR ? (B - row0) : TR);
        ring.ap = stream + lane * 4;
        int tq = tid;
        asm volatile("" : "+v"(tq));
        asm volatile("" : "+v"(ring.ap));
        const int r = tq & 63;
        // ---- x tile -> LDS in degree order: wave w gathers positions w, w + 8, ...; raw into the tile, fed into the activation region
        {
            const float *xr = x + (row0 + r) * D;
#pragma unroll 1
            for (int f = w; f < Dp; f += MF_NW) {
                float v = 0.0f, g = 0.0f;
                if (f < D) {
                    if (r < nrows) v = xr[ftc[f]];
                    g = ft_feed(ftable, D, f, v);
                }
                xreg[ftd_xidx(f, r)] = v;
                acts[ftd_xidx(f, r)] = g;
            }
        }
        f32x16 h[2][NS], t[2][NS];
        MF_BARRIER();
        // ---- initial layer: h = b0 + W0 feed(x) ---------------------------------------------------------------------------------------
#pragma unroll
        for (int s = 0; s < 2; ++s) mf_item<NS, false, TR>(ring, items[2 * s], acts + lane_b + 128 * sb0s[s], h[s]);
        // ---- residual blocks (= made_fwd.hip) -----------------------------------------------------------------------------------------
        for (int b = 0; b < NB; ++b) {
            MF_BARRIER();        // (b = 0: every wave has read the fed tile)
#pragma unroll
            for (int s = 0; s < 2; ++s) mf_publish<NS, true, TR>(acts, rbs[s], sb0s[s], hh, n, h[s]);
            MF_BARRIER();
#pragma unroll
            for (int s = 0; s < 2; ++s) mf_item<NS, false, TR>(ring, items[2 * (2 + 4 * b + s)], acts + lane_b + 128 * sb0s[s], t[s]);
            MF_BARRIER();
#pragma unroll
            for (int s = 0; s < 2; ++s) mf_publish<NS, true, TR>(acts, rbs[s], sb0s[s], hh, n, t[s]);
            MF_BARRIER();
#pragma unroll
            for (int s = 0; s < 2; ++s) mf_item<NS, true, TR>(ring, items[2 * (4 + 4 * b + s)], acts + lane_b + 128 * sb0s[s], h[s]);
        }
        MF_BARRIER();
#pragma unroll
        for (int s = 0; s < 2; ++s) mf_publish<NS, false, TR>(acts, rbs[s], sb0s[s], hh, n, h[s]);
        MF_BARRIER();
        // ---- final layer: one item per feature, both sample blocks; lane = row 32 hh + n evaluates the spline ---------------------------
        float ldrow = 0.0f;
#pragma nounroll
        for (int j = 0; j < nfi; ++j) {
            const int f = fit[2 * j + 1];
            if (f < 0) continue;
            f32x16 o[2];
            mf_item<2, false, TR>(ring, fit[2 * j], acts + lane_b, o);
            // o[sb][4 q + i] = slot 8 q + 4 hh + i of sample block sb.  v_permlane32_swap trades the upper lanes of o[0] for the lower
            // lanes of o[1]: afterwards the first register holds slot 8 q + i and the second slot 8 q + 4 + i of the lane's own row
            // (lower half: sample block 0, upper half: sample block 1) -- no select, no LDS
            float prm[32];
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(o[0][4 * q + i]), __float_as_uint(o[1][4 * q + i]),
                                                                     false, false);
                    prm[8 * q + i] = __uint_as_float(sw[0]);
                    prm[8 * q + 4 + i] = __uint_as_float(sw[1]);
                }
            // type and bound of the feature: unconditional reads at a wave-uniform index (scalar loads; selected against a null pointer
            // they became vector loads with a full vmcnt wait each, which drained the weight ring twice per feature)
            const int tcode = ftt[f];
            const float tb = ftb[f];
            RqsParams<float> q = p;
            q.tails = p.dfull ? tcode : p.tails;
            if (p.tails != NF_TAILS_NONE) {
                q.left = q.bottom = -tb;
                q.right = q.top = tb;
            }
            float *xp = xreg + ftd_xidx(f, r);                 // (row of the tile = lane)
            float yv, lad;
            ftd_spline(q, *xp, prm, yv, lad);
            *xp = yv;
            ldrow += lad;
        }
        MF_BARRIER();                      // every wave is done with the activations: their region now holds the partial sums
        acts[w * 64 + r] = ldrow;
        MF_BARRIER();
        if (tq < nrows) {
            float v = 0.0f;
#pragma unroll
            for (int k = 0; k < MF_NW; ++k) v += acts[k * 64 + tq];      // fixed order: deterministic
            ld_store(logdet + row0 + tq, v, acc_mode);
        }
        if (r < nrows) {
            float *yr = y + (row0 + r) * D;
#pragma unroll 1
            for (int f = w; f < D; f += MF_NW) yr[ftc[f]] = xreg[ftd_xidx(f, r)];
        }
        MF_BARRIER();                      // the next tile overwrites the x tile and the activations
    }
}

template <int NSB>
static int made_fwd_ft_launch(const void *x, void *y, void *logdet, const void *blob, const int32_t *table, const void *ftable,
                              int64_t B, int acc, const RqsParams<float> &p, hipStream_t st) {
    const int64_t ntiles = (B + MF_ROWS - 1) / MF_ROWS;
    const int grid = persistent_grid(ntiles);        // persistent: one workgroup per CU
    const size_t lds = sizeof(float) * ((size_t)8 * NSB * 4 * 8 * MF_ROWS + MF_XFLOATS);
    static LdsOptIn opted;
    if (opt_in_lds(reinterpret_cast<const void *>(&made_fwd_ft_kernel<NSB>), lds, opted) != NF_OK) return NF_ENOTSUP;
    hipLaunchKernelGGL((made_fwd_ft_kernel<NSB>), dim3((unsigned)grid), dim3(64 * MF_NW), lds, st, (const float *)x, (float *)y,
                       (float *)logdet, (const float *)blob, (const int *)table, (const float *)ftable, B, acc, p);
    NF_CHECK_LAUNCH();
    return NF_OK;
}

}  // namespace nf

// MaskedPiecewiseRationalQuadraticAutoregressive.forward with a per-feature table in one launch (include/nf_mi355x.h);
// blob / table / ftable: flows/made_pack.pack_made_forward_ft.
extern "C" int nf_made_forward_spline_ft(const void *x, void *y, void *logdet, const void *blob, const int32_t *table,
                                         const void *ftable, int64_t B, int D, int hidden_padded, int K, int tails,
                                         double min_bin_width, double min_bin_height, double min_derivative, int acc,
                                         nf_stream_t stream) {
    if (K < 1 || tails < NF_TAILS_NONE || tails > NF_TAILS_FEATURE) return NF_EINVAL;
    if (min_bin_width * K > 1.0 || min_bin_height * K > 1.0) return NF_EINVAL;   // utils/splines.py:121-124
    const int R = tails == NF_TAILS_LINEAR ? 3 * K - 1 : (tails == NF_TAILS_CIRCULAR ? 3 * K : 3 * K + 1);
    if (R > 32) return NF_ENOTSUP;
    if (B < 0 || D < 2 || D > 128) return NF_EINVAL;
    if (hidden_padded != 256 && hidden_padded != 512) return NF_ENOTSUP;
    if (acc < NF_LD_SUB || acc > NF_LD_ADD) return NF_EINVAL;
    if (B == 0) return NF_OK;
    if (!x || !y || !logdet || !blob || !table || !ftable) return NF_EFAULT;
    // the bound is the table's for every feature (rqs_feature_params); 1.0 only fills the launch-wide fields
    auto p = nf::make_rqs_params<float>(K, tails, 1.0, 0, 1, 0, 1, min_bin_width, min_bin_height, min_derivative, 1.0);
    hipStream_t st = (hipStream_t)stream;
    if (hidden_padded == 256) return nf::made_fwd_ft_launch<1>(x, y, logdet, blob, table, ftable, B, acc, p, st);
    return nf::made_fwd_ft_launch<2>(x, y, logdet, blob, table, ftable, B, acc, p, st);
}
