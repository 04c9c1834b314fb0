// lipmlp_nd.hip -- residual flows x + g(x), g a LipschitzMLP on d-dimensional rows (3 <= d <= 64), at inference, for gfx950: the
// density direction of a run of [Residual | ActNorm | AffineConstFlow] layers as ONE launch (value and Hutchinson's power-series
// estimate of log|det(I + J)| per Residual record), and one launch per call for a single network (x + g(x), or the fixed-point step
// y - g(x) with a device-side count of the elements that have not converged).  The formula route spends one autograd pass through
// the network per series term -- at least 21 in evaluation mode -- each of them three weight rescalings, three library GEMMs, three
// Swish backward chains and a row dot.
//
// Reference semantics: normflows/flows/residual.py:118-124 (iResBlock.forward), :133-142 (_inverse_fixed_point's step and stop
// test), :188-228 (_logdetgrad's power-series branch without exact_trace, in evaluation mode) and :355-365 (basic_logdet_estimator),
// normflows/nets/lipschitz.py:66-67, :272-274, :647-648 (LipschitzMLP / InducedNormLinear / Swish forward),
// normflows/flows/affine/coupling.py:38-54 (AffineConstFlow).
//
// Per Residual record and row, with J the Jacobian of g at x, v the row of vareps and a_k = (-1)^(k+1) coef(k) / k:
//     y = x + g(x),     ld = sum_{k = 1 .. n} a_k  v . w_k,     w_0 = v,  w_k = J w_{k-1}.
// FORWARD mode: the reference's v^T J^k (one vector-Jacobian product per term) and w_k = J^k v give the same scalar v^T J^k v, and
// the tangent J w goes through the weights in the layout the value pass reads.  One value pass keeps every Swish derivative of the
// row in LDS (d for the input Swish, HP per hidden layer); each of the n tangent passes is then
//     t = w o f'(x);  t <- (t W_0^T) o f'(p_1);  t <- (t W_m^T) o f'(p_m) ...;  w <- t W_last^T
// followed by the row dot v . w.  Plain fp32 FMAs in a fixed order: bit-identical from run to run.
//
// Blob (flows/lipmlp_nd_pack.py; the table is in include/nf_mi355x.h), dp = d rounded up to 4: K headers of 16 floats, K affine
// slots of 2 dp floats (e | t), then one weight block of 2 HP^2 + 2 dp HP + 3 HP + dp floats per Residual record, widths
// zero-padded to HP in {32, 64, 128} and to dp.  A padded unit has pre-activation 0, value f(0) = 0 and zero outgoing weights; a
// padded input column carries x = v = 0 and zero weights both ways.
//
// Mapping (template <HP>): 256 lanes own a tile of R = nf_lipmlp_nd_rows(HP, d) rows: R <= 4096 / HP, halved until the tile's
// activation plane, its three derivative planes and the four d-wide arrays (x, v, w, f'(x)) fit the 160 KiB of LDS of one CU.  In the
// first (dp -> HP) and the hidden (HP -> HP) products lane (rg, cg) = (tid / (HP / 4), tid % (HP / 4)) owns a 4 x 4 register tile,
// reads its activations from LDS as float4 along k (a broadcast within a row group) and its weight columns from the blob as float4,
// as lm_net does.  The last product (HP -> dp) has dp / 4 column groups: 4 x 4 tiles where those fill half the lanes, 1 x 4 tiles
// otherwise.  A persistent grid of <= NF_PERSISTENT_WORKGROUPS workgroups walks the row tiles.
#include "lipmlp_net.hpp"

namespace nf {

constexpr int LN_RESMAX = 8;       // Residual records per launch
constexpr int LN_MAXTERMS = 48;    // series terms per record
constexpr int LN_DMIN = 3, LN_DMAX = 64;
constexpr size_t LN_LDS_BUDGET = 160 * 1024;

struct LnTerms {                   // by value in the launch arguments: coef(k) of term k = 1 .. n[r] of Residual record r
    float c[LN_RESMAX][LN_MAXTERMS];
    int n[LN_RESMAX];
};

static inline int ln_dp(int d) { return (d + 3) & ~3; }
static inline int64_t ln_rstride(int hp, int d) { return (int64_t)2 * hp * hp + (int64_t)2 * ln_dp(d) * hp + 3 * hp + ln_dp(d); }
static inline size_t ln_lds_bytes(int hp, int d, int rows, bool chain) {
    return sizeof(float) * (size_t)rows * ((chain ? 4 : 1) * (hp + 4) + (chain ? 4 : 2) * (ln_dp(d) + 4));
}
static inline int ln_rows(int hp, int d) {
    int r = 4096 / hp;
    while (ln_lds_bytes(hp, d, r, true) > LN_LDS_BUDGET) r /= 2;
    return r;
}
static inline int64_t ln_blob_floats(int K, int nres, int hp, int d) {
    return (int64_t)K * LM_HDR + (int64_t)K * 2 * ln_dp(d) + nres * ln_rstride(hp, d);
}

// The products below end with a barrier; every lane reaches it, lanes without a tile only wait.
// (kdim -> HP) on 4 x 4 tiles.  A: the input plane (R, lda); MUL: A is multiplied element-wise by Am first (the tangent's f'(x)).
// EPI 0: out = f(acc + b), its derivative to Dp (EPI 2: not kept).  EPI 1: out = acc o Dp (a tangent: no bias).
// IN_PLACE: A is H itself, so a barrier separates the reads from the writes.
template <int HP, bool VEC, bool MUL, int EPI, bool IN_PLACE>
__device__ __forceinline__ void ln_prod(float *__restrict__ H, float *__restrict__ Dp, const float *A, int lda,
                                        const float *__restrict__ Am, int kdim, const float *__restrict__ W,
                                        const float *__restrict__ b, float c, int R) {
    constexpr int CT = HP / 4, LDH = HP + 4;
    const int tid = threadIdx.x, cg = tid % CT, rg = tid / CT;
    const bool active = 4 * rg < R;
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.0f;
    if (active) {
        for (int k = 0; k < kdim; k += 4) {
            float4 w[4];
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) w[kk] = lm_ld4<VEC>(W + (size_t)(k + kk) * HP + 4 * cg);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float4 a = *reinterpret_cast<const float4 *>(A + (4 * rg + i) * lda + k);
                if (MUL) {
                    const float4 m = *reinterpret_cast<const float4 *>(Am + (4 * rg + i) * lda + k);
                    a.x *= m.x, a.y *= m.y, a.z *= m.z, a.w *= m.w;
                }
                const float av[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) {
                    acc[i][0] = fmaf(av[kk], w[kk].x, acc[i][0]);
                    acc[i][1] = fmaf(av[kk], w[kk].y, acc[i][1]);
                    acc[i][2] = fmaf(av[kk], w[kk].z, acc[i][2]);
                    acc[i][3] = fmaf(av[kk], w[kk].w, acc[i][3]);
                }
            }
        }
    }
    if (IN_PLACE) __syncthreads();         // every lane has read the layer's input: H is free to take its output
    if (active) {
        float bv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (EPI != 1) {
            const float4 b4 = lm_ld4<VEC>(b + 4 * cg);
            bv[0] = b4.x, bv[1] = b4.y, bv[2] = b4.z, bv[3] = b4.w;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int off = (4 * rg + i) * LDH + 4 * cg;
            if (EPI == 1) {
                const float4 dv = *reinterpret_cast<const float4 *>(Dp + off);
                *reinterpret_cast<float4 *>(H + off) = make_float4(acc[i][0] * dv.x, acc[i][1] * dv.y, acc[i][2] * dv.z, acc[i][3] * dv.w);
            } else {
                float hv[4], dv[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) lm_swish(acc[i][j] + bv[j], c, hv[j], dv[j]);
                *reinterpret_cast<float4 *>(H + off) = make_float4(hv[0], hv[1], hv[2], hv[3]);
                if (EPI == 0) *reinterpret_cast<float4 *>(Dp + off) = make_float4(dv[0], dv[1], dv[2], dv[3]);
            }
        }
    }
    __syncthreads();
}

// (HP -> dp) on RT x 4 tiles: out (R, ldo) = H W (+ b).  W: (HP, dp), k-major.
template <int HP, bool VEC, int RT, bool BIAS>
__device__ __forceinline__ void ln_last_tiles(float *__restrict__ out, int ldo, const float *__restrict__ H, const float *__restrict__ W,
                                              const float *__restrict__ b, int dp, int R) {
    constexpr int LDH = HP + 4;
    const int ncg = dp / 4, items = (R / RT) * ncg;
    for (int it = threadIdx.x; it < items; it += LM_THREADS) {
        const int cg = it % ncg, rg = it / ncg;
        float acc[RT][4];
#pragma unroll
        for (int i = 0; i < RT; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = 0.0f;
        for (int k = 0; k < HP; k += 4) {
            float4 w[4];
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) w[kk] = lm_ld4<VEC>(W + (size_t)(k + kk) * dp + 4 * cg);
#pragma unroll
            for (int i = 0; i < RT; ++i) {
                const float4 a = *reinterpret_cast<const float4 *>(H + (RT * rg + i) * LDH + k);
                const float av[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) {
                    acc[i][0] = fmaf(av[kk], w[kk].x, acc[i][0]);
                    acc[i][1] = fmaf(av[kk], w[kk].y, acc[i][1]);
                    acc[i][2] = fmaf(av[kk], w[kk].z, acc[i][2]);
                    acc[i][3] = fmaf(av[kk], w[kk].w, acc[i][3]);
                }
            }
        }
        float4 b4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (BIAS) b4 = lm_ld4<VEC>(b + 4 * cg);
#pragma unroll
        for (int i = 0; i < RT; ++i)
            *reinterpret_cast<float4 *>(out + (RT * rg + i) * ldo + 4 * cg) =
                make_float4(acc[i][0] + b4.x, acc[i][1] + b4.y, acc[i][2] + b4.z, acc[i][3] + b4.w);
    }
    __syncthreads();
}

template <int HP, bool VEC, bool BIAS>
__device__ __forceinline__ void ln_last(float *__restrict__ out, int ldo, const float *__restrict__ H, const float *__restrict__ W,
                                        const float *__restrict__ b, int dp, int R) {
    if ((R / 4) * (dp / 4) >= LM_THREADS / 2) ln_last_tiles<HP, VEC, 4, BIAS>(out, ldo, H, W, b, dp, R);
    else ln_last_tiles<HP, VEC, 1, BIAS>(out, ldo, H, W, b, dp, R);
}

// The weight block of one Residual record; hidden product m reads Wm(m) and bm(m) (no array of pointers: an index that is not
// static would put the struct into private memory).
template <int HP> struct LnBlock {
    const float *W0, *b0, *W1, *Wl, *bl;
    __device__ __forceinline__ const float *Wm(int m) const { return W1 + (size_t)m * (HP * HP + HP); }
    __device__ __forceinline__ const float *bm(int m) const { return Wm(m) + HP * HP; }
};
template <int HP> __device__ __forceinline__ LnBlock<HP> ln_block(const float *__restrict__ W, int dp) {
    LnBlock<HP> k;
    k.W0 = W, k.b0 = W + (size_t)dp * HP;
    k.W1 = k.b0 + HP;
    k.Wl = k.W1 + 2 * (HP * HP + HP), k.bl = k.Wl + (size_t)HP * dp;
    return k;
}

// The value pass of one network on the tile's rows xs (R, ldd): g(x) to ws (R, ldd); KEEP: f'(x) to d0 and f'(p_m) to D_m.
template <int HP, bool VEC, bool KEEP>
__device__ __forceinline__ void ln_value(float *__restrict__ H, float *__restrict__ D, float *__restrict__ ws, float *__restrict__ d0,
                                         const float *__restrict__ xs, const float *__restrict__ hdr, const LnBlock<HP> &k, int nmid, int dp,
                                         int ldd, int R) {
    constexpr int PL_STEP = HP + 4;
    const int PL = R * PL_STEP;
    const float c0 = hdr[2];
    for (int idx = threadIdx.x; idx < R * dp; idx += LM_THREADS) {
        const int o = (idx / dp) * ldd + idx % dp;
        float a, da;
        lm_swish(xs[o], c0, a, da);
        ws[o] = a;
        if (KEEP) d0[o] = da;
    }
    __syncthreads();
    ln_prod<HP, VEC, false, KEEP ? 0 : 2, false>(H, D, ws, ldd, nullptr, dp, k.W0, k.b0, hdr[3], R);
    for (int m = 0; m < nmid; ++m)
        ln_prod<HP, VEC, false, KEEP ? 0 : 2, true>(H, D + (1 + m) * PL, H, PL_STEP, nullptr, HP, k.Wm(m), k.bm(m), hdr[4 + m], R);
    ln_last<HP, VEC, true>(ws, ldd, H, k.Wl, k.bl, dp, R);
}

// The density direction of K records on z (B, d): y (B, d), logdet (B) combined by acc.
template <int HP, bool VEC>
__global__ void __launch_bounds__(LM_THREADS)
lipmlp_nd_chain_kernel(const float *__restrict__ z, const float *__restrict__ vareps, float *__restrict__ y, float *__restrict__ logdet,
                       const float *__restrict__ blob, int64_t B, int d, int K, int nres, int R, int acc, LnTerms terms) {
    constexpr int LDH = HP + 4;
    const int dp = (d + 3) & ~3, ldd = dp + 4, PL = R * LDH, PD = R * ldd;
    extern __shared__ __attribute__((aligned(16))) float ln_lds[];
    float *H = ln_lds, *D = H + PL, *xs = D + 3 * PL, *vs = xs + PD, *ws = vs + PD, *d0 = ws + PD;
    const int tid = threadIdx.x;
    const float *aff = blob + (int64_t)K * LM_HDR, *wts = aff + (int64_t)K * 2 * dp;
    const int64_t rstride = (int64_t)2 * HP * HP + (int64_t)2 * dp * HP + 3 * HP + dp;
    const int64_t ntiles = (B + R - 1) / R;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t row0 = tile * R;
        for (int idx = tid; idx < R * dp; idx += LM_THREADS) {        // a row past the batch and a column past d run on zeros
            const int r = idx / dp, j = idx % dp;
            xs[r * ldd + j] = (row0 + r < B && j < d) ? z[(row0 + r) * d + j] : 0.0f;
        }
        float ld = 0.0f;                                             // lane tid < R: the log-det of row tid
        __syncthreads();
        for (int q = 0; q < K; ++q) {
            const float *hdr = blob + q * LM_HDR;
            const int kind = __builtin_amdgcn_readfirstlane((int)hdr[0]);
            if (kind == 0) {
                int ri = __builtin_amdgcn_readfirstlane((int)hdr[11]);
                ri = ri < 0 ? 0 : (ri >= nres ? nres - 1 : ri);
                ri = ri >= LN_RESMAX ? LN_RESMAX - 1 : ri;
                int nmid = __builtin_amdgcn_readfirstlane((int)hdr[1]);
                nmid = nmid < 0 ? 0 : (nmid > 2 ? 2 : nmid);
                int n = terms.n[ri];
                n = n < 1 ? 1 : (n > LN_MAXTERMS ? LN_MAXTERMS : n);
                const LnBlock<HP> k = ln_block<HP>(wts + ri * rstride, dp);
                for (int idx = tid; idx < R * dp; idx += LM_THREADS) {
                    const int r = idx / dp, j = idx % dp;
                    vs[r * ldd + j] = (row0 + r < B && j < d) ? vareps[((int64_t)ri * B + row0 + r) * d + j] : 0.0f;
                }
                ln_value<HP, VEC, true>(H, D, ws, d0, xs, hdr, k, nmid, dp, ldd, R);
                for (int idx = tid; idx < R * dp; idx += LM_THREADS) {
                    const int o = (idx / dp) * ldd + idx % dp;
                    xs[o] += ws[o];
                    ws[o] = vs[o];
                }
                __syncthreads();
                float sgn = 1.0f;
                for (int t = 1; t <= n; ++t, sgn = -sgn) {           // w <- J w, then v . w
                    ln_prod<HP, VEC, true, 1, false>(H, D, ws, ldd, d0, dp, k.W0, nullptr, 0.0f, R);
                    for (int m = 0; m < nmid; ++m)
                        ln_prod<HP, VEC, false, 1, true>(H, D + (1 + m) * PL, H, LDH, nullptr, HP, k.Wm(m), nullptr, 0.0f, R);
                    ln_last<HP, VEC, false>(ws, ldd, H, k.Wl, nullptr, dp, R);
                    if (tid < R) {
                        float dot = 0.0f;
                        for (int j = 0; j < dp; j += 4) {
                            const float4 a = *reinterpret_cast<const float4 *>(vs + tid * ldd + j);
                            const float4 w = *reinterpret_cast<const float4 *>(ws + tid * ldd + j);
                            dot = fmaf(a.w, w.w, fmaf(a.z, w.z, fmaf(a.y, w.y, fmaf(a.x, w.x, dot))));
                        }
                        ld = fmaf(sgn * terms.c[ri][t - 1] / (float)t, dot, ld);
                    }
                }
                __syncthreads();                                     // the last dot has read v and w: the next record may overwrite them
            } else {                                                 // ActNorm / AffineConstFlow: e = exp(+-s) and the log-det come packed
                const float *e = aff + (int64_t)q * 2 * dp, *t = e + dp;
                for (int idx = tid; idx < R * dp; idx += LM_THREADS) {
                    const int j = idx % dp, o = (idx / dp) * ldd + j;
                    xs[o] = kind == 1 ? fmaf(xs[o], e[j], t[j]) : (xs[o] - t[j]) * e[j];
                }
                ld += hdr[10];
                __syncthreads();
            }
        }
        for (int idx = tid; idx < R * d; idx += LM_THREADS) {
            const int r = idx / d, j = idx % d;
            if (row0 + r < B) y[(row0 + r) * d + j] = xs[r * ldd + j];
        }
        if (tid < R && row0 + tid < B) {
            const int64_t row = row0 + tid;
            logdet[row] = acc == NF_LD_WRITE ? ld : (acc == NF_LD_ADD ? logdet[row] + ld : logdet[row] - ld);
        }
        __syncthreads();
    }
}

// One network: mode 0: out = x + g(x).  mode 1: out = yin - g(x), and *count += the number of elements of this call with
// !((out - x)^2 / (atol + |yin| rtol) < 1) (residual.py:136-137; a NaN counts).
template <int HP, bool VEC>
__global__ void __launch_bounds__(LM_THREADS)
lipmlp_nd_apply_kernel(const float *__restrict__ x, const float *__restrict__ yin, float *__restrict__ out, int *__restrict__ count,
                       const float *__restrict__ blob, int64_t B, int d, int R, int mode, float atol, float rtol) {
    constexpr int LDH = HP + 4;
    const int dp = (d + 3) & ~3, ldd = dp + 4, PL = R * LDH, PD = R * ldd;
    extern __shared__ __attribute__((aligned(16))) float ln_lds[];
    float *H = ln_lds, *xs = H + PL, *ws = xs + PD;
    const int tid = threadIdx.x;
    int nmid = __builtin_amdgcn_readfirstlane((int)blob[1]);
    nmid = nmid < 0 ? 0 : (nmid > 2 ? 2 : nmid);
    const LnBlock<HP> k = ln_block<HP>(blob + LM_HDR + 2 * dp, dp);
    const int64_t ntiles = (B + R - 1) / R;
    int bad = 0;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t row0 = tile * R;
        for (int idx = tid; idx < R * dp; idx += LM_THREADS) {
            const int r = idx / dp, j = idx % dp;
            xs[r * ldd + j] = (row0 + r < B && j < d) ? x[(row0 + r) * d + j] : 0.0f;
        }
        __syncthreads();
        ln_value<HP, VEC, false>(H, nullptr, ws, nullptr, xs, blob, k, nmid, dp, ldd, R);
        for (int idx = tid; idx < R * d; idx += LM_THREADS) {
            const int r = idx / d, j = idx % d;
            if (row0 + r >= B) continue;
            const int64_t at = (row0 + r) * d + j;
            const float g = ws[r * ldd + j], xv = xs[r * ldd + j];
            if (mode == 0) {
                out[at] = xv + g;
            } else {
                const float yv = yin[at], o = yv - g, dl = o - xv;
                out[at] = o;
                bad += !(dl * dl / (atol + fabsf(yv) * rtol) < 1.0f);
            }
        }
        __syncthreads();
    }
    if (mode != 0) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) bad += __shfl_xor(bad, o, 64);
        if ((tid & 63) == 0 && bad > 0) atomicAdd(count, bad);
    }
}

static int ln_check(int64_t B, int hp, int d, int K, int nres, int64_t nblob) {
    if (hp != 32 && hp != 64 && hp != 128) return NF_ENOTSUP;
    if (d < LN_DMIN || d > LN_DMAX) return NF_ENOTSUP;
    if (K > LM_KMAX || nres > LN_RESMAX) return NF_ERANGE;
    if (K < 1 || B < 0 || nres < 1 || nres > K) return NF_EINVAL;
    if (nblob != ln_blob_floats(K, nres, hp, d)) return NF_EINVAL;
    return NF_OK;
}

}  // namespace nf

extern "C" int nf_lipmlp_nd_rows(int hp, int d) {
    if ((hp != 32 && hp != 64 && hp != 128) || d < nf::LN_DMIN || d > nf::LN_DMAX) return NF_ENOTSUP;
    return nf::ln_rows(hp, d);
}

extern "C" int64_t nf_lipmlp_nd_blob_floats(int K, int nres, int hp, int d) {
    if ((hp != 32 && hp != 64 && hp != 128) || d < nf::LN_DMIN || d > nf::LN_DMAX) return NF_ENOTSUP;
    if (K > nf::LM_KMAX || nres > nf::LN_RESMAX) return NF_ERANGE;
    if (K < 1 || nres < 1 || nres > K) return NF_EINVAL;
    return nf::ln_blob_floats(K, nres, hp, d);
}

extern "C" int nf_lipmlp_nd_chain(const void *z, const void *vareps, void *y, void *logdet, const void *blob, int64_t nblob, int64_t B,
                                  int d, int hp, int K, int nres, const int *nterms_host, const float *coef_host, int acc,
                                  nf_stream_t stream) {
    using namespace nf;
    const int rc = ln_check(B, hp, d, K, nres, nblob);
    if (rc != NF_OK) return rc;
    if (acc < NF_LD_SUB || acc > NF_LD_ADD) return NF_EINVAL;
    if (!nterms_host || !coef_host) return NF_EFAULT;
    for (int r = 0; r < nres; ++r) {
        if (nterms_host[r] > LN_MAXTERMS) return NF_ERANGE;
        if (nterms_host[r] < 1) return NF_EINVAL;
    }
    if (B == 0) return NF_OK;
    if (!z || !vareps || !y || !logdet || !blob) return NF_EFAULT;
    LnTerms terms;
    for (int r = 0; r < LN_RESMAX; ++r) {
        terms.n[r] = r < nres ? nterms_host[r] : 1;
        for (int k = 0; k < LN_MAXTERMS; ++k) terms.c[r][k] = (r < nres && k < nterms_host[r]) ? coef_host[r * LN_MAXTERMS + k] : 0.0f;
    }
    hipStream_t st = (hipStream_t)stream;
    const int R = ln_rows(hp, d);
    const int grid = persistent_grid((B + R - 1) / R);
    const size_t lds = ln_lds_bytes(hp, d, R, true);
    const bool vec = !nf_misaligned16(blob);
#define NF_LN_CHAIN(HP, VEC)                                                                                                     \
    do {                                                                                                                         \
        static LdsOptIn opted;                                                                                                   \
        if (opt_in_lds(reinterpret_cast<const void *>(&lipmlp_nd_chain_kernel<HP, VEC>), lds, opted) != NF_OK) return NF_ENOTSUP; \
        hipLaunchKernelGGL((lipmlp_nd_chain_kernel<HP, VEC>), dim3(grid), dim3(LM_THREADS), lds, st, (const float *)z,           \
                           (const float *)vareps, (float *)y, (float *)logdet, (const float *)blob, B, d, K, nres, R, acc, terms); \
    } while (0)
    if (hp == 32) { if (vec) NF_LN_CHAIN(32, true); else NF_LN_CHAIN(32, false); }
    else if (hp == 64) { if (vec) NF_LN_CHAIN(64, true); else NF_LN_CHAIN(64, false); }
    else { if (vec) NF_LN_CHAIN(128, true); else NF_LN_CHAIN(128, false); }
#undef NF_LN_CHAIN
    NF_CHECK_LAUNCH();
    return NF_OK;
}

extern "C" int nf_lipmlp_nd_apply(const void *x, const void *yin, void *out, void *count, const void *blob, int64_t nblob, int64_t B,
                                  int d, int hp, int mode, double atol, double rtol, nf_stream_t stream) {
    using namespace nf;
    const int rc = ln_check(B, hp, d, 1, 1, nblob);
    if (rc != NF_OK) return rc;
    if (mode != 0 && mode != 1) return NF_EINVAL;
    if (mode == 1 && !(atol >= 0.0 && rtol >= 0.0 && atol + rtol > 0.0)) return NF_EINVAL;
    if (B == 0) return NF_OK;
    if (!x || !out || !blob || (mode == 1 && (!yin || !count))) return NF_EFAULT;
    hipStream_t st = (hipStream_t)stream;
    const int R = ln_rows(hp, d);
    const int grid = persistent_grid((B + R - 1) / R);
    const size_t lds = ln_lds_bytes(hp, d, R, false);
    const bool vec = !nf_misaligned16(blob);
#define NF_LN_APPLY(HP, VEC)                                                                                                     \
    do {                                                                                                                         \
        static LdsOptIn opted;                                                                                                   \
        if (opt_in_lds(reinterpret_cast<const void *>(&lipmlp_nd_apply_kernel<HP, VEC>), lds, opted) != NF_OK) return NF_ENOTSUP; \
        hipLaunchKernelGGL((lipmlp_nd_apply_kernel<HP, VEC>), dim3(grid), dim3(LM_THREADS), lds, st, (const float *)x,           \
                           (const float *)yin, (float *)out, (int *)count, (const float *)blob, B, d, R, mode, (float)atol,      \
                           (float)rtol);                                                                                         \
    } while (0)
    if (hp == 32) { if (vec) NF_LN_APPLY(32, true); else NF_LN_APPLY(32, false); }
    else if (hp == 64) { if (vec) NF_LN_APPLY(64, true); else NF_LN_APPLY(64, false); }
    else { if (vec) NF_LN_APPLY(128, true); else NF_LN_APPLY(128, false); }
#undef NF_LN_APPLY
    NF_CHECK_LAUNCH();
    return NF_OK;
}
