// rqs_bwd_ft.hip -- nf_rqs_coupling_bwd_ft_wave: the wave-private backward of the NSF coupling transform for PER-FEATURE tails (list
// tails and / or a tensor bound: utils/splines.py:48-66 under nsf/coupling.py:71-128), the counterpart of rqs_bwd.hip's
// rqs_coupling_bwd_wave_kernel for the layers whose features differ in tails type and interval (the circular-coordinate coupling
// layer of wrapper.py:88-185).  float32, 8 bins, cond / grad_cond rows of 3 K + 1 = 25 floats per (sample, transform feature): K
// widths, K heights, K + 1 derivative logits, of which a feature's tails type overrides the two ends (rqs_regs_bwd_ft in
// rqs_bwd_common.hpp, the register routine; statement for statement the arithmetic of rqs_element_bwd under rqs_feature_params).
//
// Shape of the kernel, as rqs_coupling_bwd_wave_kernel: a wave owns SPW samples per pass; their conditioner rows, x and grad_y rows
// are staged into the wave's own LDS region with unit-stride global loads, every row is turned into its gradient row in registers
// and leaves with unit-stride stores (25-float rows are not 16-byte aligned: element by element, as the 23-float rows there).  The
// tails code and the bound of every feature of both halves are copied into LDS once per workgroup.  The identity half's batch-shared
// parameters: a lane that keeps one feature for the whole launch (SPW nI <= 64) sums its gradients in lane-private LDS words, which
// meet the other lanes' once, at the end, in workgroup LDS by atomics; the workgroup's sums then go to global memory by atomics
// (summation order across workgroups is not deterministic; grad_x and grad_cond are).
#include "common.hpp"
#include "rqs_bwd_common.hpp"

constexpr int NF_BWD_FT_WAVES = 8;    // waves per workgroup: one workgroup per CU (rqs_bwd.hip NF_BWD_WAVE_WAVES)

namespace nf {

__global__ void __launch_bounds__(64 * NF_BWD_FT_WAVES, 2)
rqs_coupling_bwd_ft_wave_kernel(const float *__restrict__ x, const float *__restrict__ gy, const float *__restrict__ gld,
                                const float *__restrict__ cond, const float *__restrict__ uw, const float *__restrict__ uh,
                                const float *__restrict__ ud, const int64_t *__restrict__ iidx, int nI,
                                const int64_t *__restrict__ tidx, int nT, int64_t B, int D, RqsParams<float> p, int mode,
                                float *__restrict__ gx, float *__restrict__ gcond, float *__restrict__ guw,
                                float *__restrict__ guh, float *__restrict__ gud, int SPW, const int *__restrict__ tails_t,
                                const float *__restrict__ bound_t, const int *__restrict__ tails_i,
                                const float *__restrict__ bound_i) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    constexpr int K = F_K, M = F_MFT, nd = F_K + 1;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, nwv = blockDim.x >> 6;
    const int per_wave = SPW * nT * M + 3 * SPW * D;
    float *s_acc = reinterpret_cast<float *>(smem_raw);           // nI * M: the workgroup's sums of the shared parameters
    float *s_prm = s_acc + (size_t)nI * M;                       // nI * M: shared parameters in rqs_regs order (w, h x log2 e; 9 logits)
    float *s_bt = s_prm + (size_t)nI * M;                        // nT bounds of the transform half
    float *s_bi = s_bt + nT;                                     // nI bounds of the identity half
    float *w_base = s_bi + nI;
    float *w_cond = w_base + (size_t)wid * per_wave;
    float *w_x = w_cond + (size_t)SPW * nT * M, *w_gy = w_x + (size_t)SPW * D, *w_gx = w_gy + (size_t)SPW * D;
    // lane-private running sums of the identity half: 25 words per lane (odd stride: conflict-free)
    float *w_racc = w_base + (size_t)nwv * per_wave + (size_t)wid * 64 * M + (size_t)lane * M;
    int *s_iidx = reinterpret_cast<int *>(w_base + (size_t)nwv * per_wave + (size_t)nwv * 64 * M);
    int *s_tidx = s_iidx + nI, *s_tt = s_tidx + nT, *s_ti = s_tt + nT;
    const bool do_t = mode != NF_RQS_SAMPLE_IDENTITY, do_i = mode != NF_RQS_SAMPLE_TRANSFORM;
    const bool inverse = mode != NF_RQS_DENSITY;
    const bool has_uncond = uw != nullptr;

    if (do_i)
        for (int j = tid; j < nI; j += blockDim.x) {
            s_iidx[j] = (int)iidx[j];
            s_ti[j] = tails_i ? tails_i[j] : NF_TAILS_LINEAR;
            s_bi[j] = bound_i ? bound_i[j] : p.right;
        }
    if (do_t)
        for (int j = tid; j < nT; j += blockDim.x) {
            s_tidx[j] = (int)tidx[j];
            s_tt[j] = tails_t ? tails_t[j] : NF_TAILS_LINEAR;
            s_bt[j] = bound_t ? bound_t[j] : p.right;
        }
    if (do_i && has_uncond) {
        for (int i = tid; i < nI * M; i += blockDim.x) {
            const int j = i / M, c = i - M * j;
            s_acc[i] = 0.0f;
            s_prm[i] = c < K ? uw[(size_t)j * K + c] * 1.44269504088896340736f
                             : (c < 2 * K ? uh[(size_t)j * K + c - K] * 1.44269504088896340736f : ud[(size_t)j * nd + c - 2 * K]);
        }
    }
    __syncthreads();

    const float sc = 1.44269504088896340736f / p.wh_div, inv_div = 1.0f / p.wh_div;
    const int64_t gw = (int64_t)blockIdx.x * nwv + wid, GW = (int64_t)gridDim.x * nwv;
    // one pass covers the identity half with one lane per element: a lane keeps the same shared feature for the whole launch
    const bool lane_acc = do_i && has_uncond && SPW * nI <= 64;
#pragma unroll
    for (int k = 0; k < M; ++k) w_racc[k] = 0.0f;
    for (int64_t b0 = gw * SPW; b0 < B; b0 += GW * SPW) {
        const int ns = (int)((B - b0) < SPW ? (B - b0) : SPW);
        for (int i = lane; i < ns * D; i += 64) {
            w_x[i] = x[b0 * D + i];
            w_gy[i] = gy[b0 * D + i];
            w_gx[i] = 0.0f;
        }
        if (do_t) {
            const float *src = cond + b0 * (int64_t)nT * M;
            for (int i = lane; i < ns * nT * M; i += 64) w_cond[i] = src[i];
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (do_t) {
            for (int e = lane; e < ns * nT; e += 64) {
                const int s_ = e / nT, j = e - s_ * nT, col = s_tidx[j];
                float *row = w_cond + (size_t)e * M;
                float prm[M], g[M];
#pragma unroll
                for (int k = 0; k < 2 * K; ++k) prm[k] = row[k] * sc;
#pragma unroll
                for (int k = 2 * K; k < M; ++k) prm[k] = row[k];
                const float xv = w_x[s_ * D + col], gyv = w_gy[s_ * D + col], gl = gld[b0 + s_];
                const float tb = s_bt[j];
                const bool circ = s_tt[j] == NF_TAILS_CIRCULAR;
                const float gxv = inverse ? rqs_regs_bwd_ft<true>(p, tb, circ, xv, prm, gyv, gl, g, inv_div)
                                          : rqs_regs_bwd_ft<false>(p, tb, circ, xv, prm, gyv, gl, g, inv_div);
#pragma unroll
                for (int k = 0; k < M; ++k) row[k] = g[k];      // (a lane's own row: parameters in, gradients out)
                w_gx[s_ * D + col] = gxv;
            }
        }
        if (do_i) {
            for (int e = lane; e < ns * nI; e += 64) {
                const int s_ = e / nI, j = e - s_ * nI, col = s_iidx[j];
                const float xv = w_x[s_ * D + col], gyv = w_gy[s_ * D + col];
                if (!has_uncond) {
                    w_gx[s_ * D + col] = gyv;
                    continue;
                }
                float prm[M], g[M];
                const float *pr = s_prm + (size_t)j * M;
#pragma unroll
                for (int k = 0; k < M; ++k) prm[k] = pr[k];
                const float gl = gld[b0 + s_];
                const float tb = s_bi[j];
                const bool circ = s_ti[j] == NF_TAILS_CIRCULAR;
                // the unconditional transform is not scaled (nsf/coupling.py:224-232): wh_div = 1
                w_gx[s_ * D + col] = inverse ? rqs_regs_bwd_ft<true>(p, tb, circ, xv, prm, gyv, gl, g, 1.0f)
                                             : rqs_regs_bwd_ft<false>(p, tb, circ, xv, prm, gyv, gl, g, 1.0f);
                if (lane_acc) {
#pragma unroll
                    for (int k = 0; k < M; ++k) w_racc[k] += g[k];      // lane-private LDS words: plain read-add-write
                } else {
                    float *accj = s_acc + (size_t)j * M;
#pragma unroll
                    for (int k = 0; k < M - 1; ++k)
                        if (g[k] != 0.0f) atomicAdd(accj + k, g[k]);
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (do_t) {
            float *dst = gcond + b0 * (int64_t)nT * M;
            for (int i = lane; i < ns * nT * M; i += 64) dst[i] = w_cond[i];
        }
        if (mode == NF_RQS_DENSITY) {
            for (int i = lane; i < ns * D; i += 64) gx[b0 * D + i] = w_gx[i];
        } else {
            const int nown = do_t ? nT : nI;
            const int *own = do_t ? s_tidx : s_iidx;
            for (int e = lane; e < ns * nown; e += 64) {
                const int s_ = e / nown, j = e - s_ * nown;
                gx[(b0 + s_) * D + own[j]] = w_gx[s_ * D + own[j]];
            }
        }
        // the next pass stages over the words this write-back has just read
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    if (lane_acc && lane < SPW * nI) {
        float *accj = s_acc + (size_t)(lane % nI) * M;
#pragma unroll
        for (int k = 0; k < M - 1; ++k) atomicAdd(accj + k, w_racc[k]);
    }
    __syncthreads();
    if (do_i && has_uncond) {
        for (int i = tid; i < nI * M; i += blockDim.x) {
            const int j = i / M, c = i - j * M;
            const float v = s_acc[i];
            if (v != 0.0f) {
                if (c < K) atomicAdd(guw + (size_t)j * K + c, v);
                else if (c < 2 * K) atomicAdd(guh + (size_t)j * K + (c - K), v);
                else atomicAdd(gud + (size_t)j * nd + (c - 2 * K), v);
            }
        }
    }
}

}  // namespace nf

// Samples a wave takes per pass and the launch's dynamic LDS (bytes) for a split of D = nI + nT features.
static size_t rqs_bwd_ft_wave_lds(int nI, int nT, int *spw) {
    const int D = nI + nT, nmax = nT > nI ? nT : nI;
    int SPW = nmax > 0 ? 64 / nmax : 1;
    if (SPW < 1) SPW = 1;
    *spw = SPW;
    const size_t per_wave = (size_t)SPW * nT * nf::F_MFT + 3 * (size_t)SPW * D;
    return (2 * (size_t)nI * nf::F_MFT + (size_t)D + NF_BWD_FT_WAVES * (per_wave + 64 * nf::F_MFT)) * sizeof(float) +
           2 * (size_t)D * sizeof(int) + 16;
}

// include/nf_mi355x.h: 1 when nf_rqs_coupling_bwd_ft_wave's tile of this split fits the LDS, 0 when it returns NF_ENOTSUP for it.
extern "C" int nf_rqs_coupling_bwd_ft_wave_fits(int nI, int nT) {
    if (nI < 0 || nT < 0 || nI + nT < 1) return NF_EINVAL;
    int spw;
    return rqs_bwd_ft_wave_lds(nI, nT, &spw) <= 150 * 1024 ? 1 : 0;
}

// include/nf_mi355x.h.  The arguments of nf_rqs_coupling_bwd_ft; what this kernel does not take is NF_ENOTSUP.
extern "C" int nf_rqs_coupling_bwd_ft_wave(const void *x, const void *grad_y, const void *grad_logdet, const void *cond,
                                           const void *uw, const void *uh, const void *ud, const int64_t *identity_idx, int nI,
                                           const int64_t *transform_idx, int nT, int64_t B, int D, int K, int tails,
                                           double tail_bound, double min_bin_width, double min_bin_height,
                                           double min_derivative, double wh_div, int mode, void *grad_x, void *grad_cond,
                                           void *grad_uw, void *grad_uh, void *grad_ud, int dtype, const int32_t *tails_t,
                                           const void *bound_t, const int32_t *tails_i, const void *bound_i,
                                           nf_stream_t stream) {
    using namespace nf;
    if (K < 1 || K > NF_MAX_BINS) return NF_ERANGE;
    if (tails < NF_TAILS_NONE || tails > NF_TAILS_FEATURE) return NF_EINVAL;
    if (B < 0 || D < 1 || nI < 0 || nT < 0 || nI + nT != D || mode < 0 || mode > 2) return NF_EINVAL;
    if (tails == NF_TAILS_FEATURE && ((nT && mode != NF_RQS_SAMPLE_IDENTITY && !tails_t) ||
                                      (nI && uw && mode != NF_RQS_SAMPLE_TRANSFORM && !tails_i))) return NF_EFAULT;
    if (tails != NF_TAILS_FEATURE && (tails_t || tails_i)) return NF_EINVAL;
    if (tails == NF_TAILS_NONE && (bound_t || bound_i)) return NF_EINVAL;
    // rows of 3 K + 1 floats (list tails), 8 bins, float32: everything else stays with nf_rqs_coupling_bwd_ft
    if (K != F_K || tails != NF_TAILS_FEATURE || dtype != NF_F32) return NF_ENOTSUP;
    if (B == 0) return NF_OK;
    if (!x || !grad_y || !grad_logdet || !grad_x) return NF_EFAULT;
    if (mode != NF_RQS_SAMPLE_IDENTITY && nT && (!cond || !grad_cond || !transform_idx)) return NF_EFAULT;
    if (mode != NF_RQS_SAMPLE_TRANSFORM && nI && !identity_idx) return NF_EFAULT;
    if (uw && (!uh || !ud || !grad_uw || !grad_uh || !grad_ud)) return NF_EFAULT;
    // every array is moved element by element: its element type's alignment is all the kernel asks for
    if ((((uintptr_t)x | (uintptr_t)grad_y | (uintptr_t)grad_logdet | (uintptr_t)cond | (uintptr_t)uw | (uintptr_t)uh |
          (uintptr_t)ud | (uintptr_t)grad_x | (uintptr_t)grad_cond | (uintptr_t)grad_uw | (uintptr_t)grad_uh |
          (uintptr_t)grad_ud | (uintptr_t)tails_t | (uintptr_t)bound_t | (uintptr_t)tails_i | (uintptr_t)bound_i) & 3) ||
        (((uintptr_t)identity_idx | (uintptr_t)transform_idx) & 7))
        return NF_EINVAL;
    const auto p = make_rqs_params<float>(K, tails, tail_bound, 0, 1, 0, 1, min_bin_width, min_bin_height, min_derivative, wh_div);
    int SPW;
    const size_t lds = rqs_bwd_ft_wave_lds(nI, nT, &SPW);
    if (lds > 150 * 1024) return NF_ENOTSUP;
    const int64_t nwaves = (B + SPW - 1) / SPW, gq = (nwaves + NF_BWD_FT_WAVES - 1) / NF_BWD_FT_WAVES;
    const int grid = (int)(gq < 2048 / NF_BWD_FT_WAVES ? gq : 2048 / NF_BWD_FT_WAVES);
    static LdsOptIn opted = {};
    if (opt_in_lds(reinterpret_cast<const void *>(&rqs_coupling_bwd_ft_wave_kernel), lds, opted) != NF_OK) return NF_ENOTSUP;
    hipLaunchKernelGGL(rqs_coupling_bwd_ft_wave_kernel, dim3(grid), dim3(64 * NF_BWD_FT_WAVES), lds, (hipStream_t)stream,
                       (const float *)x, (const float *)grad_y, (const float *)grad_logdet, (const float *)cond, (const float *)uw,
                       (const float *)uh, (const float *)ud, identity_idx, nI, transform_idx, nT, B, D, p, mode, (float *)grad_x,
                       (float *)grad_cond, (float *)grad_uw, (float *)grad_uh, (float *)grad_ud, SPW, (const int *)tails_t,
                       (const float *)bound_t, (const int *)tails_i, (const float *)bound_i);
    NF_CHECK_LAUNCH();
    return NF_OK;
}
