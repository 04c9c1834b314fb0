// hmc2d.hip -- the stochastic flow layers on (B, 2) batches for gfx950: ONE launch per HamiltonianMonteCarlo transition (leapfrog
// trajectory, Metropolis correction, output selection, log-det; in training also the parameter tangents), one launch for the
// `steps` random-walk steps of MetropolisHastings with a DiagGaussianProposal, and the HMC backward with a fixed-order reduction.
// The formula route evaluates target.log_prob 2 L + 4 times per HMC layer (each of them a dozen to seventy element-wise launches)
// plus 2 L torch.autograd.grad calls.
//
// Reference semantics: normflows/flows/stochastic.py:27-47 (MetropolisHastings.forward), :73-108 (HamiltonianMonteCarlo.forward,
// gradlogP), normflows/distributions/mh_proposal.py:77-82 (DiagGaussianProposal.forward), normflows/distributions/
// linear_interpolation.py:25-28.  The random numbers are the CALLER's (torch draws them in the reference's order in front of the
// launch).
//
// lane = row, grid-stride loop over the rows.  The target is w0 log p_0 + w1 log p_1 with one or two terms; a term is one of
// density2d's seven kinds (density2d_row.hpp: value and gradient in registers) or a diagonal Gaussian (kind 7) whose loc /
// log_scale are read from device memory.  The kind is a wave-uniform run-time switch; the loops are arranged so that the target
// is evaluated at ONE place of each kernel.  gradlogP detaches its argument: the force is a constant to autograd, the
// trajectory is element-wise per dimension, and d z_new / d log_step_size, d z_new / d log_mass are running scalars per row.
#include "density2d_row.hpp"

namespace nf {

constexpr int H2_GAUSS = 7;             // the diagonal-Gaussian term (HAIS's prior): a0 = loc (2), a1 = log_scale (2)
constexpr int H2_SIDE = 8;              // floats per row of the training sidecar
constexpr int H2_BWD_MAX_BLOCKS = 256;
constexpr int H2_NPAR = 4;              // log_step_size (2) | log_mass (2)

struct H2Term {
    int kind, n;
    float w;
    float p[D2_NP];
    const float *a0, *a1;               // kind 6: a0 = scale (1); kind 7: a0 = loc (2), a1 = log_scale (2)
};
struct H2Target {
    int nterms;
    H2Term t[2];
};
struct H2Ctx { float c0, c1, c2, c3, c4; };   // kind 6: 1 / (2 s^2), log normaliser; kind 7: loc, exp(-log_scale), constant

// CircularGaussianMixture's centres as the formulas hold them: 2 sin / cos(2 pi / n_modes * i) evaluated in double and rounded
// once.  (d2_circ_setup evaluates them in float32 from a float32 phase, up to five float32 roundings off; one density evaluation does
// not notice, a leapfrog trajectory through the mixture's narrow modes multiplies it up.)  Every thread of the workgroup calls it.
__device__ __forceinline__ void h2_circ_setup(const H2Term &t, float *cx, float *cy, H2Ctx &c) {
    const double w = 6.283185307179586 / (double)t.n;
    for (int i = threadIdx.x; i < t.n; i += blockDim.x) {
        cx[i] = (float)(2.0 * ::sin(w * (double)i));
        cy[i] = (float)(2.0 * ::cos(w * (double)i));
    }
    __syncthreads();
    const float s = t.a0[0];
    c.c0 = 1.0f / (2.0f * s * s);
    c.c1 = -M<float>::log(t.p[1] * s * s * (float)t.n);         // p[1] = 2 pi
}

__device__ __forceinline__ void h2_setup(const H2Term &t, float *cx, float *cy, H2Ctx &c) {
    c.c0 = c.c1 = c.c2 = c.c3 = c.c4 = 0.0f;
    if (t.kind == D2_CIRC_GMM) h2_circ_setup(t, cx, cy, c);     // (wave- and workgroup-uniform branch)
    else if (t.kind == H2_GAUSS) {
        const float ls0 = t.a1[0], ls1 = t.a1[1];
        c.c0 = t.a0[0];
        c.c1 = t.a0[1];
        c.c2 = M<float>::exp(-ls0);
        c.c3 = M<float>::exp(-ls1);
        c.c4 = -1.8378770664093453f - (ls0 + ls1);              // -0.5 d log(2 pi) - sum log_scale, d = 2
    }
}

__device__ __forceinline__ float h2_term(const H2Term &t, const H2Ctx &c, const float *cx, const float *cy, float z0, float z1,
                                         float &g0, float &g1) {
    switch (t.kind) {
        case D2_TWO_MODES: return d2_row<D2_TWO_MODES>(z0, z1, t.p, t.n, cx, cy, 0.0f, 0.0f, g0, g1);
        case D2_SINUSOIDAL: return d2_row<D2_SINUSOIDAL>(z0, z1, t.p, t.n, cx, cy, 0.0f, 0.0f, g0, g1);
        case D2_SIN_GAP: return d2_row<D2_SIN_GAP>(z0, z1, t.p, t.n, cx, cy, 0.0f, 0.0f, g0, g1);
        case D2_SIN_SPLIT: return d2_row<D2_SIN_SPLIT>(z0, z1, t.p, t.n, cx, cy, 0.0f, 0.0f, g0, g1);
        case D2_SMILEY: return d2_row<D2_SMILEY>(z0, z1, t.p, t.n, cx, cy, 0.0f, 0.0f, g0, g1);
        case D2_RINGS: return d2_row<D2_RINGS>(z0, z1, t.p, t.n, cx, cy, 0.0f, 0.0f, g0, g1);
        case D2_CIRC_GMM: return d2_row<D2_CIRC_GMM>(z0, z1, t.p, t.n, cx, cy, c.c0, c.c1, g0, g1);
        default: {
            const float u0 = (z0 - c.c0) * c.c2, u1 = (z1 - c.c1) * c.c3;
            g0 = -u0 * c.c2;
            g1 = -u1 * c.c3;
            return c.c4 - 0.5f * (u0 * u0 + u1 * u1);
        }
    }
}

// w0 log p_0(z) + w1 log p_1(z) and its gradient
__device__ __forceinline__ float h2_eval(const H2Target &T, const H2Ctx &c0, const H2Ctx &c1, const float *cx, const float *cy, float z0,
                                         float z1, float &g0, float &g1) {
    float a0, a1;
    float v = T.t[0].w * h2_term(T.t[0], c0, cx, cy, z0, z1, a0, a1);
    g0 = T.t[0].w * a0;
    g1 = T.t[0].w * a1;
    if (T.nterms == 2) {
        v += T.t[1].w * h2_term(T.t[1], c1, cx, cy, z0, z1, a0, a1);
        g0 += T.t[1].w * a0;
        g1 += T.t[1].w * a1;
    }
    return v;
}

// torch.clamp(g, min=-c, max=c); a NaN stays a NaN.  c == 0: no clipping (the reference tests `if self.max_abs_grad`).
__device__ __forceinline__ float h2_clip(float g, float c) { return c > 0.0f ? (g < -c ? -c : (g > c ? c : g)) : g; }

template <bool TRAIN>
__global__ void __launch_bounds__(256)
hmc2d_kernel(const float *__restrict__ z, const float *__restrict__ eps, const float *__restrict__ u, const float *__restrict__ lss,
             const float *__restrict__ lm, H2Target T, int steps, float clip, float *__restrict__ z_out, float *__restrict__ log_det,
             float *__restrict__ accept, float *__restrict__ side, int64_t B) {
    __shared__ float cx[D2_MAX_MODES], cy[D2_MAX_MODES];
    H2Ctx c0, c1;
    h2_setup(T.t[0], cx, cy, c0);
    c1 = c0;
    if (T.nterms == 2) h2_setup(T.t[1], cx, cy, c1);
    // stochastic.py:75, :80: exp(0.5 log_mass), exp(log_step_size), exp(log_mass)
    const float lm0 = lm[0], lm1 = lm[1];
    const float sq0 = M<float>::exp(0.5f * lm0), sq1 = M<float>::exp(0.5f * lm1);
    const float em0 = M<float>::exp(lm0), em1 = M<float>::exp(lm1);
    const float s0 = M<float>::exp(lss[0]), s1 = M<float>::exp(lss[1]);
    const float hs0 = s0 / 2.0f, hs1 = s1 / 2.0f;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < B; r += (int64_t)gridDim.x * blockDim.x) {
        const float zi0 = z[2 * r], zi1 = z[2 * r + 1];
        const float p0 = eps[2 * r] * sq0, p1 = eps[2 * r + 1] * sq1;
        float zn0 = zi0, zn1 = zi1, pn0 = p0, pn1 = p1, ph0 = 0.0f, ph1 = 0.0f;
        float lp0 = 0.0f, lpn = 0.0f, gi0 = 0.0f, gi1 = 0.0f, gn0 = 0.0f, gn1 = 0.0f;
        // tangents of z_new and of the momentum: d / d log_step_size (zs, ps), d / d log_mass (zm, pm); p = eps exp(0.5 log_mass)
        float zs0 = 0.0f, zs1 = 0.0f, zm0 = 0.0f, zm1 = 0.0f, ps0 = 0.0f, ps1 = 0.0f, pm0 = 0.5f * p0, pm1 = 0.5f * p1;
        for (int i = 0;; ++i) {
            lpn = h2_eval(T, c0, c1, cx, cy, zn0, zn1, gn0, gn1);
            const float gc0 = h2_clip(gn0, clip), gc1 = h2_clip(gn1, clip);
            if (i == 0) {
                lp0 = lpn; gi0 = gn0; gi1 = gn1;
            } else {                                    // :85  p_new = p_half - (step_size / 2) * -gradlogP(z_new)
                pn0 = ph0 - hs0 * -gc0;
                pn1 = ph1 - hs1 * -gc1;
                if (TRAIN) { ps0 += hs0 * gc0; ps1 += hs1 * gc1; }
            }
            if (i == steps) break;
            ph0 = pn0 - hs0 * -gc0;                     // :83
            ph1 = pn1 - hs1 * -gc1;
            const float q0 = ph0 / em0, q1 = ph1 / em1;
            zn0 = zn0 + s0 * q0;                        // :84
            zn1 = zn1 + s1 * q1;
            if (TRAIN) {
                ps0 += hs0 * gc0; ps1 += hs1 * gc1;
                zs0 += s0 * q0 + s0 * (ps0 / em0); zs1 += s1 * q1 + s1 * (ps1 / em1);
                zm0 += s0 * (pm0 / em0 - q0); zm1 += s1 * (pm1 / em1 - q1);
            }
        }
        // :88-96
        const float prob = M<float>::exp(lpn - lp0 - 0.5f * (pn0 * pn0 / em0 + pn1 * pn1 / em1) + 0.5f * (p0 * p0 / em0 + p1 * p1 / em1));
        const bool acc = u[r] < prob;                   // false for a NaN probability
        z_out[2 * r] = acc ? zn0 : zi0;
        z_out[2 * r + 1] = acc ? zn1 : zi1;
        log_det[r] = acc ? lp0 - lpn : 0.0f;
        accept[r] = acc ? 1.0f : 0.0f;
        if (TRAIN) {
            float *sr = side + (size_t)r * H2_SIDE;
            sr[0] = zs0; sr[1] = zs1; sr[2] = zm0; sr[3] = zm1;
            sr[4] = gi0; sr[5] = gi1;
            sr[6] = acc ? gn0 : gi0; sr[7] = acc ? gn1 : gi1;
        }
    }
}

// gz = gz_out + gld (grad_lp(z) - grad_lp(z_out)); v = accept (gz_out - gld grad_lp(z_out)); slab of this wave = sum_rows v * tangent
__global__ void __launch_bounds__(256)
hmc2d_bwd_kernel(const float *__restrict__ gzo, const float *__restrict__ gld, const float *__restrict__ accept,
                 const float *__restrict__ side, float *__restrict__ gz, float *__restrict__ slabs, int want, int64_t B) {
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < B; r += (int64_t)gridDim.x * blockDim.x) {
        const float *sr = side + (size_t)r * H2_SIDE;
        const float o0 = gzo ? gzo[2 * r] : 0.0f, o1 = gzo ? gzo[2 * r + 1] : 0.0f;
        const float l = gld ? gld[r] : 0.0f;
        if (gz) {
            gz[2 * r] = o0 + l * (sr[4] - sr[6]);
            gz[2 * r + 1] = o1 + l * (sr[5] - sr[7]);
        }
        if (want) {
            const float ac = accept[r];
            const float v0 = ac * (o0 - l * sr[6]), v1 = ac * (o1 - l * sr[7]);
            if (want & 1) { a0 = fmaf(v0, sr[0], a0); a1 = fmaf(v1, sr[1], a1); }
            if (want & 2) { a2 = fmaf(v0, sr[2], a2); a3 = fmaf(v1, sr[3], a3); }
        }
    }
    if (want) {
        a0 = wave_sum(a0); a1 = wave_sum(a1); a2 = wave_sum(a2); a3 = wave_sum(a3);
        if ((threadIdx.x & 63) == 0) {
            float *s = slabs + ((size_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * H2_NPAR;
            s[0] = a0; s[1] = a1; s[2] = a2; s[3] = a3;
        }
    }
}

// gpar[c] = the waves' slabs summed in a fixed order: thread t takes slabs t, t + 256, ... in turn, then the workgroup's fixed tree
__global__ void __launch_bounds__(256)
hmc2d_reduce_kernel(const float *__restrict__ slabs, float *__restrict__ gpar, int nslabs) {
    __shared__ float sm[16];
    for (int c = 0; c < H2_NPAR; ++c) {
        float a = 0.0f;
        for (int w = threadIdx.x; w < nslabs; w += 256) a += slabs[(size_t)w * H2_NPAR + c];
        a = block_sum(a, sm);
        if (threadIdx.x == 0) gpar[c] = a;
    }
}

template <bool SIDE>
__global__ void __launch_bounds__(256)
mh2d_kernel(const float *__restrict__ z, const float *__restrict__ eps, const float *__restrict__ u, const float *__restrict__ scale,
            int nscale, H2Target T, int steps, float *__restrict__ z_out, float *__restrict__ log_det, float *__restrict__ gside,
            int64_t B) {
    __shared__ float cx[D2_MAX_MODES], cy[D2_MAX_MODES];
    H2Ctx c0, c1;
    h2_setup(T.t[0], cx, cy, c0);
    c1 = c0;
    if (T.nterms == 2) h2_setup(T.t[1], cx, cy, c1);
    const float sc0 = scale[0], sc1 = scale[nscale - 1];
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < B; r += (int64_t)gridDim.x * blockDim.x) {
        float z0 = z[2 * r], z1 = z[2 * r + 1];
        float q0 = z0, q1 = z1;                         // the point under evaluation: z itself, then each proposal
        float lp = 0.0f, g0 = 0.0f, g1 = 0.0f, gi0 = 0.0f, gi1 = 0.0f, ld = 0.0f;
        for (int i = 0;; ++i) {
            float h0, h1;
            const float lq = h2_eval(T, c0, c1, cx, cy, q0, q1, h0, h1);
            if (i == 0) {
                lp = lq; g0 = gi0 = h0; g1 = gi1 = h1;
            } else {                                    // stochastic.py:36-45 of step i - 1
                const float e = M<float>::exp(lq - lp + 0.0f);
                const float wa = e > 1.0f ? 1.0f : e;   // torch.clamp(., max=1): a NaN stays a NaN and rejects
                if (u[(size_t)(i - 1) * B + r] <= wa) {
                    z0 = q0; z1 = q1;
                    ld = ld + (lp - lq);
                    lp = lq; g0 = h0; g1 = h1;
                }
            }
            if (i == steps) break;
            const float *e = eps + ((size_t)i * B + r) * 2;
            q0 = e[0] * sc0 + z0;                       // mh_proposal.py:80
            q1 = e[1] * sc1 + z1;
        }
        z_out[2 * r] = z0;
        z_out[2 * r + 1] = z1;
        log_det[r] = ld;
        if (SIDE) {
            float *sr = gside + (size_t)r * 4;
            sr[0] = gi0; sr[1] = gi1; sr[2] = g0; sr[3] = g1;
        }
    }
}

// the target of a launch from the host tables: tkind (nterms x 2: kind, n), trec (nterms x 9: weight, record), aux device pointers
static int h2_target(H2Target &T, const int *tkind, const float *trec, const void *a00, const void *a01, const void *a10, const void *a11,
                     int nterms) {
    if (nterms < 1 || nterms > 2 || !tkind || !trec) return NF_EINVAL;
    const void *aux[2][2] = {{a00, a01}, {a10, a11}};
    int ncirc = 0;
    T.nterms = nterms;
    for (int i = 0; i < 2; ++i) {
        H2Term &t = T.t[i];
        const bool on = i < nterms;
        t.kind = on ? tkind[2 * i] : H2_GAUSS;
        t.n = on ? tkind[2 * i + 1] : 0;
        t.w = on ? trec[9 * i] : 0.0f;
        for (int k = 0; k < D2_NP; ++k) t.p[k] = on ? trec[9 * i + 1 + k] : 0.0f;
        t.a0 = on ? (const float *)aux[i][0] : nullptr;
        t.a1 = on ? (const float *)aux[i][1] : nullptr;
        if (!on) continue;
        if (t.kind < D2_TWO_MODES || t.kind > H2_GAUSS) return NF_ENOTSUP;
        if (t.kind == D2_RINGS && (t.n < 1 || t.n > D2_MAX_RINGS)) return NF_ERANGE;
        if (t.kind == D2_CIRC_GMM && (t.n < 1 || t.n > D2_MAX_MODES)) return NF_ERANGE;
        if (t.kind == D2_CIRC_GMM && ++ncirc > 1) return NF_ENOTSUP;        // one set of centres in LDS
        if (t.kind == D2_CIRC_GMM && !t.a0) return NF_EFAULT;
        if (t.kind == H2_GAUSS && (!t.a0 || !t.a1)) return NF_EFAULT;
    }
    return NF_OK;
}

static inline int h2_bwd_grid(int64_t B) { return grid_for(B, 256, H2_BWD_MAX_BLOCKS); }

}  // namespace nf

extern "C" int nf_hmc2d_grid(int64_t B) { return nf::grid_for(B, 256); }
extern "C" int nf_mh2d_grid(int64_t B) { return nf::grid_for(B, 256); }
extern "C" int nf_hmc2d_bwd_grid(int64_t B) { return nf::h2_bwd_grid(B); }
extern "C" int64_t nf_hmc2d_bwd_scratch_floats(int64_t B) { return B < 0 ? NF_EINVAL : (int64_t)nf::h2_bwd_grid(B) * 4 * nf::H2_NPAR; }

extern "C" int nf_hmc2d(const void *z, const void *eps, const void *u, const void *log_step_size, const void *log_mass, const int *tkind,
                        const float *trec, const void *a00, const void *a01, const void *a10, const void *a11, int nterms, int steps,
                        double max_abs_grad, void *z_out, void *log_det, void *accept, void *side, int64_t B, nf_stream_t stream) {
    using namespace nf;
    H2Target T;
    if (B < 0 || steps < 0 || !(max_abs_grad >= 0.0)) return NF_EINVAL;
    const int rc = h2_target(T, tkind, trec, a00, a01, a10, a11, nterms);
    if (rc != NF_OK) return rc;
    if (B == 0) return NF_OK;
    if (!z || !eps || !u || !log_step_size || !log_mass || !z_out || !log_det || !accept) return NF_EFAULT;
    hipStream_t st = (hipStream_t)stream;
    if (side)
        hipLaunchKernelGGL((hmc2d_kernel<true>), dim3(grid_for(B, 256)), dim3(256), 0, st, (const float *)z, (const float *)eps,
                           (const float *)u, (const float *)log_step_size, (const float *)log_mass, T, steps, (float)max_abs_grad,
                           (float *)z_out, (float *)log_det, (float *)accept, (float *)side, B);
    else
        hipLaunchKernelGGL((hmc2d_kernel<false>), dim3(grid_for(B, 256)), dim3(256), 0, st, (const float *)z, (const float *)eps,
                           (const float *)u, (const float *)log_step_size, (const float *)log_mass, T, steps, (float)max_abs_grad,
                           (float *)z_out, (float *)log_det, (float *)accept, (float *)nullptr, B);
    NF_CHECK_LAUNCH();
    return NF_OK;
}

extern "C" int nf_hmc2d_bwd(const void *gz_out, const void *gld, const void *accept, const void *side, void *gz, void *slabs, void *gpar,
                            int want, int64_t B, nf_stream_t stream) {
    using namespace nf;
    if (B < 0 || want < 0 || want > 3) return NF_EINVAL;
    if (B == 0 || (!gz && !want)) return NF_OK;
    if (!side || !accept || (want && (!slabs || !gpar))) return NF_EFAULT;
    hipStream_t st = (hipStream_t)stream;
    const int grid = h2_bwd_grid(B);
    hipLaunchKernelGGL(hmc2d_bwd_kernel, dim3(grid), dim3(256), 0, st, (const float *)gz_out, (const float *)gld, (const float *)accept,
                       (const float *)side, (float *)gz, (float *)slabs, want, B);
    NF_CHECK_LAUNCH();
    if (want) {
        hipLaunchKernelGGL(hmc2d_reduce_kernel, dim3(1), dim3(256), 0, st, (const float *)slabs, (float *)gpar, grid * 4);
        NF_CHECK_LAUNCH();
    }
    return NF_OK;
}

extern "C" int nf_mh2d(const void *z, const void *eps, const void *u, const void *scale, int nscale, const int *tkind, const float *trec,
                       const void *a00, const void *a01, const void *a10, const void *a11, int nterms, int steps, void *z_out,
                       void *log_det, void *gside, int64_t B, nf_stream_t stream) {
    using namespace nf;
    H2Target T;
    if (B < 0 || steps < 0 || nscale < 1 || nscale > 2) return NF_EINVAL;
    const int rc = h2_target(T, tkind, trec, a00, a01, a10, a11, nterms);
    if (rc != NF_OK) return rc;
    if (B == 0) return NF_OK;
    if (!z || !scale || !z_out || !log_det || (steps > 0 && (!eps || !u))) return NF_EFAULT;
    hipStream_t st = (hipStream_t)stream;
    if (gside)
        hipLaunchKernelGGL((mh2d_kernel<true>), dim3(grid_for(B, 256)), dim3(256), 0, st, (const float *)z, (const float *)eps,
                           (const float *)u, (const float *)scale, nscale, T, steps, (float *)z_out, (float *)log_det, (float *)gside, B);
    else
        hipLaunchKernelGGL((mh2d_kernel<false>), dim3(grid_for(B, 256)), dim3(256), 0, st, (const float *)z, (const float *)eps,
                           (const float *)u, (const float *)scale, nscale, T, steps, (float *)z_out, (float *)log_det, (float *)nullptr,
                           B);
    NF_CHECK_LAUNCH();
    return NF_OK;
}
