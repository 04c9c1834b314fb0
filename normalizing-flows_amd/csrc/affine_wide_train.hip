// affine_wide_train.hip -- the element-wise half of a wide RealNVP coupling layer UNDER AUTOGRAD (autograd.AffineWideFn): the
// conditioner -- MaskedAffineFlow's stacked [s | t] MLPs or an AffineCouplingBlock's param_map, flows/affine_wide_pack.py -- runs on
// the MADE training kernels in plain-MLP mode (nf_made_forward_train / nf_made_backward / nf_made_wgrad), and these two kernels are
// the coupling map in front of / behind it, reading the raw conditioner output P in the pack's own layout (row 2 f = feature f's scale
// parameter, 2 f + 1 = its shift parameter, for all d features):
//   nf_affine_wide_apply      (z, P) -> (y, log-det): the formulas of EPI 4 (made_fwd_body.hpp) = affine.hip's masked_affine_kernel /
//                             affine_coupling_kernel (affine/coupling.py:209-229, :117-171)
//   nf_affine_wide_apply_bwd  (z, P, gy, gld) -> (gz through the element-wise map only, gP in the padded shape nf_made_backward /
//                             nf_made_wgrad take): the closed forms of affine_bwd.hip
// One 2-D grid-stride kernel each: threadIdx.x walks a row's features (quads of them as 16-byte vectors when d % 4 == 0), threadIdx.y /
// blockIdx.x the rows.  A row belongs to `blockDim.x` (a power of two <= 64) consecutive lanes of one wave: the log-det is summed per
// lane in feature order and then over the lanes by a butterfly -- a fixed order, no atomics, bit-repeatable.  HBM-bound: every operand
// element is read once and every result element written once.  No LDS, no scratch memory (tests/test_host_affine_wide_train.py).
#include "common.hpp"

namespace nf {

typedef float aw_f4 __attribute__((ext_vector_type(4)));
typedef float aw_f2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ unsigned aw_mode(const int *__restrict__ modes, int f) {
    return ((unsigned)modes[f >> 4] >> (2 * (f & 15))) & 3u;
}

// One feature of the forward map: y and its log-det term (before the direction's sign).  mode: 0 identity, 1 / 2 transformed.
__device__ __forceinline__ float aw_apply_one(float v, float sc, float sh, unsigned mode, int smap, int nets, int direction, float &ld) {
    if (smap == 4) {                     // masked_affine_kernel with b = 1 (identity) / 0
        const float bi = mode == 0u ? 1.0f : 0.0f;
        if (!(nets & 1)) sc = 0.0f;      // a missing net is the constant 0
        if (!(nets & 2)) sh = 0.0f;
        if (!M<float>::finite(sc)) sc = M<float>::nan();
        if (!M<float>::finite(sh)) sh = M<float>::nan();
        const float zm = bi * v;
        ld += (1.0f - bi) * sc;
        if (direction == 0) return zm + (1.0f - bi) * (v * M<float>::exp(sc) + sh);
        return zm + (1.0f - bi) * (v - sh) * M<float>::exp(-sc);
    }
    if (mode == 0u) return v;
    if (smap == NF_SCALE_NONE) return direction == 0 ? v + sh : v - sh;          // affine_coupling_kernel
    if (smap == NF_SCALE_EXP) {
        ld += sc;
        return direction == 0 ? v * M<float>::exp(sc) + sh : (v - sh) * M<float>::exp(-sc);
    }
    const float sg = sigmoid(sc + 2.0f);
    const float lg = M<float>::log(sg);
    if (smap == NF_SCALE_SIGMOID) {
        ld -= lg;
        return direction == 0 ? v / sg + sh : (v - sh) * sg;
    }
    ld += lg;
    return direction == 0 ? v * sg + sh : (v - sh) / sg;
}

// One feature of the backward: gz through the element-wise map, (g scale parameter, g shift parameter).
__device__ __forceinline__ float aw_bwd_one(float v, float sc, float sh, float g, float gl, unsigned mode, int smap, int nets,
                                            int direction, float &gsc, float &gsh) {
    gsc = 0.0f;
    gsh = 0.0f;
    if (smap == 4) {                     // masked_affine_bwd_kernel
        const float bi = mode == 0u ? 1.0f : 0.0f, nb = 1.0f - bi;
        if (!(nets & 1)) sc = 0.0f;
        if (!(nets & 2)) sh = 0.0f;
        if (!M<float>::finite(sc)) sc = M<float>::nan();
        if (!M<float>::finite(sh)) sh = M<float>::nan();
        if (direction == 0) {
            const float e = M<float>::exp(sc);
            if (nets & 1) gsc = nb * (g * v * e + gl);
            if (nets & 2) gsh = nb * g;
            return g * (bi + nb * e);
        }
        const float e = M<float>::exp(-sc);
        if (nets & 1) gsc = -nb * (g * (v - sh) * e + gl);
        if (nets & 2) gsh = -nb * g * e;
        return g * (bi + nb * e);
    }
    if (mode == 0u) return g;            // affine_coupling_bwd_kernel: the identity half is copied
    if (smap == NF_SCALE_NONE) {
        gsh = direction == 0 ? g : -g;
        return g;
    }
    if (smap == NF_SCALE_EXP) {
        if (direction == 0) {            // y = v e^sc + sh, ld = +sum sc
            const float e = M<float>::exp(sc);
            gsh = g;
            gsc = g * v * e + gl;
            return g * e;
        }
        const float e = M<float>::exp(-sc);   // y = (v - sh) e^-sc, ld = -sum sc
        gsh = -g * e;
        gsc = -(g * (v - sh) * e + gl);
        return g * e;
    }
    const float sg = sigmoid(sc + 2.0f), om = 1.0f - sg;      // d sg / d sc = sg (1 - sg), d log sg / d sc = 1 - sg
    const bool mult = (smap == NF_SCALE_SIGMOID_INV) == (direction == 0);      // y uses * sg (else / sg)
    if (direction == 0) {
        gsh = g;
        if (mult) { gsc = g * v * sg * om + gl * om; return g * sg; }
        gsc = -(g * v * om / sg + gl * om);
        return g / sg;
    }
    if (mult) { gsh = -g * sg; gsc = g * (v - sh) * sg * om + gl * om; return g * sg; }
    gsh = -g / sg;
    gsc = -(g * (v - sh) * om / sg + gl * om);
    return g / sg;
}

// The row's lanes are blockDim.x consecutive lanes of one wave (blockDim.x a power of two <= 64): butterfly in a fixed order.
__device__ __forceinline__ float aw_row_sum(float v) {
    for (int o = (int)blockDim.x >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

template <bool VEC>
__global__ void __launch_bounds__(256)
affine_wide_apply_kernel(const float *__restrict__ z, const float *__restrict__ P, const int *__restrict__ modes, float *__restrict__ y,
                         float *__restrict__ logdet, int64_t B, int D, int ldp, int smap, int nets, int direction) {
    const int64_t rstep = (int64_t)gridDim.x * blockDim.y;
    const int64_t rows = (B + blockDim.y - 1) / blockDim.y * blockDim.y;       // (whole row groups: every lane reaches the shuffles)
    for (int64_t r = (int64_t)blockIdx.x * blockDim.y + threadIdx.y; r < rows; r += rstep) {
        const bool live = r < B;
        float ld = 0.0f;
        if (live) {
            const float *zr = z + r * D, *pr = P + r * ldp;
            float *yr = y + r * D;
            if constexpr (VEC) {
                for (int q = threadIdx.x; 4 * q < D; q += blockDim.x) {
                    const aw_f4 v = *reinterpret_cast<const aw_f4 *>(zr + 4 * q);
                    aw_f4 o;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int f = 4 * q + i;
                        const aw_f2 p = *reinterpret_cast<const aw_f2 *>(pr + 2 * f);      // (scale, shift): one 8-byte load
                        o[i] = aw_apply_one(v[i], p[0], p[1], aw_mode(modes, f), smap, nets, direction, ld);
                    }
                    *reinterpret_cast<aw_f4 *>(yr + 4 * q) = o;
                }
            } else {
                for (int f = threadIdx.x; f < D; f += blockDim.x) {
                    const aw_f2 p = *reinterpret_cast<const aw_f2 *>(pr + 2 * f);
                    yr[f] = aw_apply_one(zr[f], p[0], p[1], aw_mode(modes, f), smap, nets, direction, ld);
                }
            }
        }
        ld = aw_row_sum(ld);
        if (live && threadIdx.x == 0) logdet[r] = direction == 0 ? ld : -ld;
    }
}

template <bool VEC>
__global__ void __launch_bounds__(256)
affine_wide_apply_bwd_kernel(const float *__restrict__ z, const float *__restrict__ P, const float *__restrict__ gy,
                             const float *__restrict__ gld, const int *__restrict__ modes, float *__restrict__ gz,
                             float *__restrict__ gP, int64_t B, int64_t Bp, int D, int ldp, int ldg, int smap, int nets, int direction) {
    const int64_t rstep = (int64_t)gridDim.x * blockDim.y;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.y + threadIdx.y; r < Bp; r += rstep) {
        float *gpr = gP + r * ldg;
        if (r >= B) {                    // the padding rows of g_params: zeros
            if constexpr (VEC) {
                for (int c = 4 * threadIdx.x; c < ldg; c += 4 * blockDim.x) *reinterpret_cast<aw_f4 *>(gpr + c) = aw_f4{0.0f, 0.0f, 0.0f, 0.0f};
            } else {
                for (int c = threadIdx.x; c < ldg; c += blockDim.x) gpr[c] = 0.0f;
            }
            continue;
        }
        const float *zr = z + r * D, *pr = P + r * ldp, *gyr = gy ? gy + r * D : nullptr;
        float *gzr = gz + r * D;
        const float gl = gld ? gld[r] : 0.0f;
        if constexpr (VEC) {
            for (int q = threadIdx.x; 4 * q < D; q += blockDim.x) {
                const aw_f4 v = *reinterpret_cast<const aw_f4 *>(zr + 4 * q);
                const aw_f4 g = gyr ? *reinterpret_cast<const aw_f4 *>(gyr + 4 * q) : aw_f4{0.0f, 0.0f, 0.0f, 0.0f};
                aw_f4 o, lo, hi;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int f = 4 * q + i;
                    const aw_f2 p = *reinterpret_cast<const aw_f2 *>(pr + 2 * f);
                    float gsc, gsh;
                    o[i] = aw_bwd_one(v[i], p[0], p[1], g[i], gl, aw_mode(modes, f), smap, nets, direction, gsc, gsh);
                    if (i < 2) { lo[2 * i] = gsc; lo[2 * i + 1] = gsh; }
                    else { hi[2 * (i - 2)] = gsc; hi[2 * (i - 2) + 1] = gsh; }
                }
                *reinterpret_cast<aw_f4 *>(gzr + 4 * q) = o;
                *reinterpret_cast<aw_f4 *>(gpr + 8 * q) = lo;
                *reinterpret_cast<aw_f4 *>(gpr + 8 * q + 4) = hi;
            }
            for (int c = 2 * D + 4 * threadIdx.x; c < ldg; c += 4 * blockDim.x)
                *reinterpret_cast<aw_f4 *>(gpr + c) = aw_f4{0.0f, 0.0f, 0.0f, 0.0f};
        } else {
            for (int f = threadIdx.x; f < D; f += blockDim.x) {
                const aw_f2 p = *reinterpret_cast<const aw_f2 *>(pr + 2 * f);
                float gsc, gsh;
                gzr[f] = aw_bwd_one(zr[f], p[0], p[1], gyr ? gyr[f] : 0.0f, gl, aw_mode(modes, f), smap, nets, direction, gsc, gsh);
                *reinterpret_cast<aw_f2 *>(gpr + 2 * f) = aw_f2{gsc, gsh};
            }
            for (int c = 2 * D + threadIdx.x; c < ldg; c += blockDim.x) gpr[c] = 0.0f;
        }
    }
}

// Lanes per row: the power of two that covers the row's work items (quads on the vector path), at most one wave.
static inline int aw_lanes(int D, bool vec) {
    const int items = vec ? D / 4 : D;
    int t = 1;
    while (t < items && t < 64) t <<= 1;
    return t;
}

}  // namespace nf

static int affine_wide_train_check(int64_t B, int D, int ldp, int smap, int nets, int direction) {
    if (B < 0 || D < 2 || D > 128 || (direction != 0 && direction != 1)) return NF_EINVAL;
    if (ldp < 2 * D || (ldp & 1) || nets < 0 || nets > 3) return NF_EINVAL;
    if (smap < NF_SCALE_EXP || smap > 4) return NF_ENOTSUP;
    return NF_OK;
}

// include/nf_mi355x.h
extern "C" int nf_affine_wide_apply(const void *z, const void *P, const int32_t *modes, void *y, void *logdet, int64_t B, int D, int ldp,
                                    int smap, int nets, int direction, nf_stream_t stream) {
    const int rc = affine_wide_train_check(B, D, ldp, smap, nets, direction);
    if (rc != NF_OK) return rc;
    if (B == 0) return NF_OK;
    if (!z || !P || !modes || !y || !logdet) return NF_EFAULT;
    if (((uintptr_t)P & 7) != 0) return NF_EINVAL;                              // (scale, shift) pairs are 8-byte loads
    const bool vec = (D & 3) == 0;
    if (vec && nf_misaligned16(z, y)) return NF_EINVAL;                         // rows a multiple of 4 floats long move as 16-byte vectors
    const int lanes = nf::aw_lanes(D, vec);
    const dim3 block((unsigned)lanes, (unsigned)(256 / lanes));
    const int grid = nf::grid_for(B, (int)block.y, 256 * 16);
    hipStream_t st = (hipStream_t)stream;
    if (vec)
        hipLaunchKernelGGL(nf::affine_wide_apply_kernel<true>, dim3((unsigned)grid), block, 0, st, (const float *)z, (const float *)P,
                           (const int *)modes, (float *)y, (float *)logdet, B, D, ldp, smap, nets, direction);
    else
        hipLaunchKernelGGL(nf::affine_wide_apply_kernel<false>, dim3((unsigned)grid), block, 0, st, (const float *)z, (const float *)P,
                           (const int *)modes, (float *)y, (float *)logdet, B, D, ldp, smap, nets, direction);
    NF_CHECK_LAUNCH();
    return NF_OK;
}

// include/nf_mi355x.h
extern "C" int nf_affine_wide_apply_bwd(const void *z, const void *P, const void *gy, const void *gld, const int32_t *modes, void *gz,
                                        void *gP, int64_t B, int64_t Bp, int D, int ldp, int ldg, int smap, int nets, int direction,
                                        nf_stream_t stream) {
    const int rc = affine_wide_train_check(B, D, ldp, smap, nets, direction);
    if (rc != NF_OK) return rc;
    if (Bp < B || ldg < 2 * D || (ldg & 3)) return NF_EINVAL;
    if (B == 0) return NF_OK;
    if (!z || !P || !modes || !gz || !gP) return NF_EFAULT;                     // (gy, gld may be NULL: zeros)
    if (((uintptr_t)P & 7) != 0 || nf_misaligned16(gP)) return NF_EINVAL;       // 8-byte pair loads; g_params rows move as 16-byte vectors
    const bool vec = (D & 3) == 0;
    if (vec && nf_misaligned16(z, gy, gz)) return NF_EINVAL;
    const int lanes = nf::aw_lanes(D, vec);
    const dim3 block((unsigned)lanes, (unsigned)(256 / lanes));
    const int grid = nf::grid_for(Bp, (int)block.y, 256 * 16);
    hipStream_t st = (hipStream_t)stream;
    if (vec)
        hipLaunchKernelGGL(nf::affine_wide_apply_bwd_kernel<true>, dim3((unsigned)grid), block, 0, st, (const float *)z, (const float *)P,
                           (const float *)gy, (const float *)gld, (const int *)modes, (float *)gz, (float *)gP, B, Bp, D, ldp, ldg, smap,
                           nets, direction);
    else
        hipLaunchKernelGGL(nf::affine_wide_apply_bwd_kernel<false>, dim3((unsigned)grid), block, 0, st, (const float *)z, (const float *)P,
                           (const float *)gy, (const float *)gld, (const int *)modes, (float *)gz, (float *)gP, B, Bp, D, ldp, ldg, smap,
                           nets, direction);
    NF_CHECK_LAUNCH();
    return NF_OK;
}
