// gmm.hip -- log-density of a diagonal Gaussian mixture and its backward for gfx950: one launch forward, one launch plus a fixed-order
// slab reduction backward, where the formula route materialises (B, M, d) intermediates several times over in each direction (168 MB
// apiece at 65 536 rows, 10 modes, d = 64).
//
// Reference semantics: normflows/distributions/base.py:645-659 (GaussianMixture.log_prob; :634-641 is the same formula in forward);
// the gradients are what PyTorch autograd derives from those lines.
//
//   lp_b = logsumexp_m( -d/2 log 2 pi + logw_m - 1/2 sum_j ((z_bj - loc_mj) e^{-ls_mj})^2 - sum_j ls_mj )
//
// Record: R is one float32 vector [loc (M, d) | log_scale (M, d) | logw (M)], logw = log_softmax(weight_scores), built on the host
// side of the launch with differentiable torch operations (distributions: dist_mixture.record); the backward returns gR in the same
// layout and torch's autograd carries it to the leaves, the softmax's backward included.
//
// LDS: loc (M d), e^{-ls} (M d) and the per-mode constant c_m = -d/2 log 2 pi + logw_m - sum_j ls_mj (M): at most 32 KB + 256 B.
// Row layouts as in rank1_chain.hip (template <G, NE>): d <= 16 lane = row, 256 rows per workgroup; 16 < d <= 128 sixteen lanes per
// row, lane j of the group holds elements j, j + 16, ...; the squared distance is summed over the group with four xor-shuffle steps.
// The log-sum-exp streams over the modes in registers.  A persistent grid of <= NF_PERSISTENT_WORKGROUPS workgroups walks the row tiles.
//
// Backward: the responsibilities r_bm = exp(lp_bm - lp_b) are recomputed from z, the record and the saved lp.
//   gz_bj   = -g_b sum_m r_bm (z_bj - loc_mj) e^{-2 ls_mj}
//   gloc_mj =  sum_b g_b r_bm (z_bj - loc_mj) e^{-2 ls_mj}
//   gls_mj  =  sum_b g_b r_bm (eps_bmj^2 - 1)
//   glogw_m =  sum_b g_b r_bm
// Parameter gradients: every wave sums its rows' contributions with shuffles (a fixed tree) into a slab that only this wave writes
// (first tile writes, later tiles add), one reduction launch sums the slabs in a fixed order (train_reduce.hpp).  No atomics:
// bit-identical from run to run.  `want` switches the three parameter sums off one by one (bit 0 loc, 1 log_scale, 2 logw); want == 0:
// no slab work, one launch.
#include "common.hpp"
#include "train_reduce.hpp"

namespace nf {

constexpr int GM_DMAX = 128;
constexpr int GM_MMAX = 64;
constexpr int GM_MDMAX = 4096;
constexpr int GM_WAVES = 4;
constexpr int64_t GM_SCRATCH_MAX_FLOATS = (int64_t)1 << 24;        // 64 MiB of slabs
constexpr float GM_HALF_LOG_2PI = 0.91893853320467274178f;

template <int G> __device__ __forceinline__ float gm_group_sum(float x) {
    if (G == 16) {
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    }
    return x;
}

// Sum over the rows of a wave of a value that lane (lane % G) of every row holds.
template <int G> __device__ __forceinline__ float gm_rows_sum(float x) {
#pragma unroll
    for (int o = 32; o >= G; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

template <int G> __device__ __forceinline__ int gm_idx(int j, int e) { return G == 1 ? e : j + G * e; }

// sL = loc, sI = e^{-ls}, sC = c_m
__device__ __forceinline__ void gm_stage(float *sL, float *sI, float *sC, const float *__restrict__ R, int M, int d) {
    const int md = M * d;
    for (int i = threadIdx.x; i < md; i += blockDim.x) {
        sL[i] = R[i];
        sI[i] = ::expf(-R[md + i]);
    }
    for (int m = threadIdx.x; m < M; m += blockDim.x) {
        float s = 0.0f;
        for (int i = 0; i < d; ++i) s += R[md + m * d + i];
        sC[m] = R[2 * md + m] - (float)d * GM_HALF_LOG_2PI - s;
    }
    __syncthreads();
}

template <int G, int NE>
__global__ void __launch_bounds__(256)
gmm_fwd_kernel(const float *__restrict__ z, const float *__restrict__ R, float *__restrict__ out, int64_t B, int M, int d, int acc) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float *sL = reinterpret_cast<float *>(smem_raw), *sI = sL + M * d, *sC = sI + M * d;
    gm_stage(sL, sI, sC, R, M, d);
    constexpr int rows = 256 / G;
    const int j = threadIdx.x % G, sub = threadIdx.x / G;
    const int64_t ntiles = (B + rows - 1) / rows;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t r = tile * rows + sub;
        const bool valid = r < B;          // a row past the batch runs on zeros (every lane takes part in the shuffles)
        float v[NE];
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const int i = gm_idx<G>(j, e);
            v[e] = (valid && i < d) ? z[r * d + i] : 0.0f;
        }
        float mx = 0.0f, S = 0.0f;
        for (int m = 0; m < M; ++m) {
            const float *lo = sL + m * d, *is = sI + m * d;
            float q = 0.0f;
#pragma unroll
            for (int e = 0; e < NE; ++e) {
                const int i = gm_idx<G>(j, e);
                if (i < d) {
                    const float u = (v[e] - lo[i]) * is[i];
                    q = fmaf(u, u, q);
                }
            }
            const float t = sC[m] - 0.5f * gm_group_sum<G>(q);
            if (m == 0 || t > mx) {
                S = (m == 0 ? 0.0f : S * ::expf(mx - t)) + 1.0f;
                mx = t;
            } else {
                S += ::expf(t - mx);
            }
        }
        if (valid && j == 0) ld_store(out + r, mx + ::logf(S), acc);
    }
}

template <int G, int NE>
__global__ void __launch_bounds__(256)
gmm_bwd_kernel(const float *__restrict__ z, const float *__restrict__ R, const float *__restrict__ lp, const float *__restrict__ g,
               float *__restrict__ gz, float *__restrict__ slabs, int64_t B, int M, int d, int want) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float *sL = reinterpret_cast<float *>(smem_raw), *sI = sL + M * d, *sC = sI + M * d;
    gm_stage(sL, sI, sC, R, M, d);
    constexpr int rows = 256 / G;
    const int j = threadIdx.x % G, sub = threadIdx.x / G, lane = threadIdx.x & 63;
    const int md = M * d;
    float *slab = want ? slabs + ((size_t)blockIdx.x * GM_WAVES + (threadIdx.x >> 6)) * ((size_t)2 * md + M) : nullptr;
    const bool wl = want & 1, ws = want & 2, ww = want & 4;
    bool first = true;
    const int64_t ntiles = (B + rows - 1) / rows;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t r = tile * rows + sub;
        const bool valid = r < B;
        float v[NE], a[NE];
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const int i = gm_idx<G>(j, e);
            v[e] = (valid && i < d) ? z[r * d + i] : 0.0f;
            a[e] = 0.0f;
        }
        const float gb = valid ? g[r] : 0.0f, lpb = valid ? lp[r] : 0.0f;
        for (int m = 0; m < M; ++m) {
            const float *lo = sL + m * d, *is = sI + m * d;
            float u[NE], q = 0.0f;
#pragma unroll
            for (int e = 0; e < NE; ++e) {
                const int i = gm_idx<G>(j, e);
                u[e] = i < d ? (v[e] - lo[i]) * is[i] : 0.0f;
                q = fmaf(u[e], u[e], q);
            }
            const float t = sC[m] - 0.5f * gm_group_sum<G>(q);
            const float w = valid ? gb * ::expf(t - lpb) : 0.0f;       // (a row past the batch contributes exactly nothing)
            if (ww) {
                const float sw = gm_rows_sum<G>(w);
                if (lane == 0) {
                    if (first) slab[2 * md + m] = sw;
                    else slab[2 * md + m] += sw;
                }
            } else if (want && first && lane == 0) slab[2 * md + m] = 0.0f;
#pragma unroll
            for (int e = 0; e < NE; ++e) {
                if (G * e < d) {           // wave-uniform
                    const int i = gm_idx<G>(j, e);
                    const float gl = i < d ? w * u[e] * is[i] : 0.0f;           // w (z - loc) e^{-2 ls}
                    a[e] -= gl;
                    if (want) {
                        const float sa = wl ? gm_rows_sum<G>(gl) : 0.0f;
                        const float sb = ws ? gm_rows_sum<G>(w * (u[e] * u[e] - 1.0f)) : 0.0f;
                        if (lane < G && i < d) {
                            if (first || !wl) slab[m * d + i] = sa;
                            else slab[m * d + i] += sa;
                            if (first || !ws) slab[md + m * d + i] = sb;
                            else slab[md + m * d + i] += sb;
                        }
                    }
                }
            }
        }
        first = false;
        if (gz && valid) {
#pragma unroll
            for (int e = 0; e < NE; ++e) {
                const int i = gm_idx<G>(j, e);
                if (i < d) gz[r * d + i] = a[e];
            }
        }
    }
}

// gR[e] = sum over the waves' slabs in a fixed order (train_reduce.hpp: chunk lanes, then lane order).
__global__ void __launch_bounds__(64 * RL)
gmm_reduce_kernel(const float *__restrict__ slabs, float *__restrict__ gR, int64_t n, int chunks) {
    __shared__ float sm[RL][64];
    for (int64_t e0 = (int64_t)blockIdx.x * 64; e0 < n; e0 += (int64_t)gridDim.x * 64)
        wgrad_reduce_group(slabs, gR, nullptr, n, n, n, chunks, 0, 1, 0, nullptr, 0, e0, sm);
}

static inline int gm_rows(int d) { return d <= 16 ? 256 : 16; }
static inline size_t gm_lds(int M, int d) { return ((size_t)2 * M * d + M) * sizeof(float); }

static inline int gm_grid(int64_t B, int M, int d, bool slabs) {
    int grid = persistent_grid((B + gm_rows(d) - 1) / gm_rows(d));
    const int64_t per = (int64_t)GM_WAVES * (2 * M * d + M);
    if (slabs && grid * per > GM_SCRATCH_MAX_FLOATS) grid = (int)(GM_SCRATCH_MAX_FLOATS / per);
    return grid < 1 ? 1 : grid;
}

static inline int gm_check(int64_t B, int M, int d) {
    if (d < 1 || d > GM_DMAX || M < 1 || M > GM_MMAX || M * d > GM_MDMAX) return NF_ENOTSUP;
    if (B < 0) return NF_EINVAL;
    return NF_OK;
}

}  // namespace nf

extern "C" int nf_gmm_rows(int d) { return d < 1 || d > nf::GM_DMAX ? NF_ENOTSUP : nf::gm_rows(d); }

extern "C" int64_t nf_gmm_scratch_floats(int64_t B, int M, int d) {
    const int rc = nf::gm_check(B, M, d);
    if (rc != NF_OK) return rc;
    return (int64_t)nf::gm_grid(B, M, d, true) * nf::GM_WAVES * (2 * M * d + M);
}

extern "C" int nf_gmm_log_prob(const void *z, const void *R, void *out, int64_t B, int M, int d, int acc, nf_stream_t stream) {
    const int rc = nf::gm_check(B, M, d);
    if (rc != NF_OK) return rc;
    if (acc < NF_LD_SUB || acc > NF_LD_ADD) return NF_EINVAL;
    if (B == 0) return NF_OK;
    if (!z || !R || !out) return NF_EFAULT;
    hipStream_t st = (hipStream_t)stream;
    const int grid = nf::gm_grid(B, M, d, false);
    const size_t lds = nf::gm_lds(M, d);
    if (d <= 16)
        hipLaunchKernelGGL((nf::gmm_fwd_kernel<1, 16>), dim3(grid), dim3(256), lds, st, (const float *)z, (const float *)R, (float *)out,
                           B, M, d, acc);
    else
        hipLaunchKernelGGL((nf::gmm_fwd_kernel<16, 8>), dim3(grid), dim3(256), lds, st, (const float *)z, (const float *)R, (float *)out,
                           B, M, d, acc);
    NF_CHECK_LAUNCH();
    return NF_OK;
}

extern "C" int nf_gmm_log_prob_bwd(const void *z, const void *R, const void *lp, const void *g, void *gz, void *slabs, void *gR,
                                   int64_t B, int M, int d, int want, nf_stream_t stream) {
    const int rc = nf::gm_check(B, M, d);
    if (rc != NF_OK) return rc;
    if (want < 0 || want > 7) return NF_EINVAL;
    if (B == 0) return NF_OK;
    if (!z || !R || !lp || !g || (want && (!slabs || !gR))) return NF_EFAULT;
    if (!gz && !want) return NF_OK;
    hipStream_t st = (hipStream_t)stream;
    const int grid = nf::gm_grid(B, M, d, want != 0);
    const size_t lds = nf::gm_lds(M, d);
    if (d <= 16)
        hipLaunchKernelGGL((nf::gmm_bwd_kernel<1, 16>), dim3(grid), dim3(256), lds, st, (const float *)z, (const float *)R,
                           (const float *)lp, (const float *)g, (float *)gz, (float *)slabs, B, M, d, want);
    else
        hipLaunchKernelGGL((nf::gmm_bwd_kernel<16, 8>), dim3(grid), dim3(256), lds, st, (const float *)z, (const float *)R,
                           (const float *)lp, (const float *)g, (float *)gz, (float *)slabs, B, M, d, want);
    NF_CHECK_LAUNCH();
    if (want) {
        const int64_t n = (int64_t)2 * M * d + M;
        hipLaunchKernelGGL(nf::gmm_reduce_kernel, dim3(nf::grid_for(n, 64)), dim3(64 * nf::RL), 0, st, (const float *)slabs,
                           (float *)gR, n, grid * nf::GM_WAVES);
        NF_CHECK_LAUNCH();
    }
    return NF_OK;
}
