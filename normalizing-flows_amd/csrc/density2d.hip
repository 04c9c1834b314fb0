// density2d.hip -- the closed-form two-dimensional target and prior densities for gfx950: log p(z) of a (B, 2) batch, and in the SAME
// launch d log p / d z when the caller wants it, where the formula route spends a dozen (TwoMoons) to seventy
// (CircularGaussianMixture(8): a Python loop with one torch.cat per mode) element-wise launches forward and about twice that in
// autograd -- on every sample of every reverse-KL step.
//
// Reference semantics: normflows/distributions/target.py:109-129 (TwoMoons), :149-160 (CircularGaussianMixture), :188-195
// (RingMixture); normflows/distributions/prior.py:126-149 (TwoModes), :169-194 (Sinusoidal), :218-245 (Sinusoidal_gap), :269-296
// (Sinusoidal_split), :309-327 (Smiley).  The gradient is what PyTorch autograd derives from those lines, kinks included: abs has
// derivative 0 at 0, the 2-norm and the 4-norm have derivative 0 at the origin, log(1 + exp(x)) is evaluated as written.
//
// lane = row, grid-stride loop over the rows.  The parameter record `p` is filled on the host from the instance's attributes at
// call time and travels as a kernel argument (include/nf_mi355x.h has the table).  Mode sums (kinds 5, 6) are a streaming
// log-sum-exp over the modes in registers; CircularGaussianMixture's centres are computed once per workgroup into LDS and its
// `scale` buffer is read from device memory (no host read-back).  Nothing of size B x modes touches memory.
#include "common.hpp"

namespace nf {

constexpr int D2_NP = 8;                // floats of the parameter record
constexpr int D2_MAX_MODES = 256;       // CircularGaussianMixture: centres in LDS
constexpr int D2_MAX_RINGS = 1 << 16;

struct D2Rec { float p[D2_NP]; };

enum { D2_TWO_MODES = 0, D2_SINUSOIDAL = 1, D2_SIN_GAP = 2, D2_SIN_SPLIT = 3, D2_SMILEY = 4, D2_RINGS = 5, D2_CIRC_GMM = 6 };

__device__ __forceinline__ float d2_sign(float x) { return (float)(x > 0.0f) - (float)(x < 0.0f); }   // torch.abs' backward: 0 at 0

// -0.5 ((|z| - loc) / den)^2 and its gradient (0 at the origin, as vector_norm's backward masks it)
__device__ __forceinline__ float d2_ring(float z0, float z1, float loc, float inv_den, float &g0, float &g1) {
    const float n = M<float>::sqrt(z0 * z0 + z1 * z1);
    const float u = (n - loc) * inv_den;
    const float gn = n > 0.0f ? -u * inv_den / n : 0.0f;
    g0 = gn * z0;
    g1 = gn * z1;
    return -0.5f * u * u;
}

// -0.5 ((a - eps) / s)^2 + log(1 + exp(-c a eps)) with c = 2 / s^2: value, d / d a, d / d eps
__device__ __forceinline__ float d2_two_bumps(float a, float eps, float inv_s, float c, float &da, float &deps) {
    const float v = (a - eps) * inv_s;
    const float e = M<float>::exp(-c * (a * eps));
    const float sg = e / (1.0f + e);
    da = -v * inv_s - sg * c * eps;
    deps = v * inv_s - sg * c * a;
    return -0.5f * v * v + M<float>::log(1.0f + e);
}

// -0.5 (|z|_4 / (20 s))^4 = -0.5 (z0^4 + z1^4) k4 with k4 = (20 s)^-4; its gradient -2 z^3 k4 is 0 at the origin as well
__device__ __forceinline__ float d2_envelope(float z0, float z1, float k4, float &g0, float &g1) {
    const float a = z0 * z0, b = z1 * z1;
    g0 = -2.0f * a * z0 * k4;
    g1 = -2.0f * b * z1 * k4;
    return -0.5f * (a * a + b * b) * k4;
}

template <int KIND>
__global__ void __launch_bounds__(256)
density2d_kernel(const float *__restrict__ z, float *__restrict__ lp, float *__restrict__ gz, D2Rec rec, int n,
                 const float *__restrict__ dscale, int64_t B) {
    __shared__ float cx[KIND == D2_CIRC_GMM ? D2_MAX_MODES : 1], cy[KIND == D2_CIRC_GMM ? D2_MAX_MODES : 1];
    const float *p = rec.p;
    float inv2s2 = 0.0f, lognorm = 0.0f;
    if (KIND == D2_CIRC_GMM) {
        for (int i = threadIdx.x; i < n; i += blockDim.x) {
            const float phi = p[0] * (float)i;         // 2 pi / n_modes * i
            cx[i] = 2.0f * ::sinf(phi);
            cy[i] = 2.0f * ::cosf(phi);
        }
        __syncthreads();
        const float s = dscale[0];
        inv2s2 = 1.0f / (2.0f * s * s);
        lognorm = -M<float>::log(p[1] * s * s * (float)n);       // p[1] = 2 pi
    }
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < B; r += (int64_t)gridDim.x * blockDim.x) {
        const float z0 = z[2 * r], z1 = z[2 * r + 1];
        float v, g0, g1;
        if (KIND == D2_TWO_MODES) {
            // p: loc, 1 / (2 scale), |loc|, 1 / (3 scale), 2 / (3 scale)^2
            v = d2_ring(z0, z1, p[0], p[1], g0, g1);
            float da, deps;
            v += d2_two_bumps(fabsf(z0), p[2], p[3], p[4], da, deps);
            g0 += da * d2_sign(z0);
        } else if (KIND == D2_SMILEY) {
            // p: loc, 1 / (2 scale), 0.8, 1.2
            v = d2_ring(z0, z1, p[0], p[1], g0, g1);
            const float y = z1 + p[2];
            const float u = (fabsf(y) - p[3]) * p[1];
            v -= 0.5f * u * u;
            g1 -= u * p[1] * d2_sign(y);
        } else if (KIND == D2_SINUSOIDAL || KIND == D2_SIN_GAP || KIND == D2_SIN_SPLIT) {
            // p: 2 pi / period, 1 / scale, (20 scale)^-4, 2 / scale^2, w amplitude, w centre, w scale
            v = d2_envelope(z0, z1, p[2], g0, g1);
            float sn, cs;
            ::sincosf(p[0] * z0, &sn, &cs);
            const float dw1 = p[0] * cs;
            if (KIND == D2_SINUSOIDAL) {
                const float u = (z1 - sn) * p[1];
                v -= 0.5f * u * u;
                g1 -= u * p[1];
                g0 += u * p[1] * dw1;
            } else {
                const float t = (z0 - p[5]) / p[6];
                float h, dh;                            // h = w / 2 and its derivative in z0
                if (KIND == D2_SIN_GAP) {
                    h = p[4] * M<float>::exp(-0.5f * t * t) * 0.5f;
                    dh = -h * t / p[6];
                } else {
                    const float sg = 1.0f / (1.0f + M<float>::exp(-t));
                    h = p[4] * sg * 0.5f;
                    dh = h * (1.0f - sg) / p[6];
                }
                const float y = z1 - sn + h;
                float da, deps;
                v += d2_two_bumps(fabsf(y), fabsf(h), p[1], p[3], da, deps);
                const float dy = da * d2_sign(y);
                g1 += dy;
                g0 += dy * (dh - dw1) + deps * d2_sign(h) * dh;
            }
        } else {
            // streaming log-sum-exp over the modes: running maximum mx, S = sum exp(t_i - mx), T0 / T1 = sum exp(t_i - mx) d t_i / d z
            float mx = 0.0f, S = 0.0f, T0 = 0.0f, T1 = 0.0f, nrm = 0.0f;
            if (KIND == D2_RINGS) nrm = M<float>::sqrt(z0 * z0 + z1 * z1);
            for (int i = 0; i < n; ++i) {
                float t, d0, d1;
                if (KIND == D2_RINGS) {                 // p: 2 / n_rings, 1 / (2 scale^2)
                    const float u = nrm - p[0] * (float)(i + 1);
                    t = -(u * u) * p[1];
                    d0 = -2.0f * u * p[1];              // d t / d |z|
                    d1 = 0.0f;
                } else {
                    const float u0 = z0 - cx[i], u1 = z1 - cy[i];
                    t = -(u0 * u0 + u1 * u1) * inv2s2;
                    d0 = -2.0f * u0 * inv2s2;
                    d1 = -2.0f * u1 * inv2s2;
                }
                if (i == 0 || t > mx) {
                    const float f = i == 0 ? 0.0f : M<float>::exp(mx - t);
                    S = S * f + 1.0f; T0 = T0 * f + d0; T1 = T1 * f + d1;
                    mx = t;
                } else {
                    const float e = M<float>::exp(t - mx);
                    S += e; T0 = fmaf(e, d0, T0); T1 = fmaf(e, d1, T1);
                }
            }
            v = mx + M<float>::log(S) + lognorm;
            if (KIND == D2_RINGS) {
                const float gn = nrm > 0.0f ? T0 / S / nrm : 0.0f;
                g0 = gn * z0;
                g1 = gn * z1;
            } else {
                g0 = T0 / S;
                g1 = T1 / S;
            }
        }
        lp[r] = v;
        if (gz) {
            gz[2 * r] = g0;
            gz[2 * r + 1] = g1;
        }
    }
}

template <int KIND>
static int d2_launch(const void *z, void *lp, void *gz, const D2Rec &rec, int n, const void *dscale, int64_t B, hipStream_t st) {
    hipLaunchKernelGGL((density2d_kernel<KIND>), dim3(grid_for(B, 256)), dim3(256), 0, st, (const float *)z, (float *)lp, (float *)gz,
                       rec, n, (const float *)dscale, B);
    NF_CHECK_LAUNCH();
    return NF_OK;
}

}  // namespace nf

extern "C" int nf_density2d_grid(int64_t B) { return nf::grid_for(B, 256); }

extern "C" int nf_density2d(const void *z, void *lp, void *gz, int kind, int n, const float *rec_host, int nrec, const void *dscale,
                            int64_t B, nf_stream_t stream) {
    using namespace nf;
    if (kind < D2_TWO_MODES || kind > D2_CIRC_GMM) return NF_ENOTSUP;
    if (B < 0 || nrec < 0 || nrec > D2_NP || (nrec > 0 && !rec_host)) return NF_EINVAL;
    if (kind == D2_RINGS && (n < 1 || n > D2_MAX_RINGS)) return NF_ERANGE;
    if (kind == D2_CIRC_GMM && (n < 1 || n > D2_MAX_MODES)) return NF_ERANGE;
    if (B == 0) return NF_OK;
    if (!z || !lp || (kind == D2_CIRC_GMM && !dscale)) return NF_EFAULT;
    D2Rec rec;
    for (int i = 0; i < D2_NP; ++i) rec.p[i] = i < nrec ? rec_host[i] : 0.0f;
    hipStream_t st = (hipStream_t)stream;
    switch (kind) {
        case D2_TWO_MODES: return d2_launch<D2_TWO_MODES>(z, lp, gz, rec, n, dscale, B, st);
        case D2_SINUSOIDAL: return d2_launch<D2_SINUSOIDAL>(z, lp, gz, rec, n, dscale, B, st);
        case D2_SIN_GAP: return d2_launch<D2_SIN_GAP>(z, lp, gz, rec, n, dscale, B, st);
        case D2_SIN_SPLIT: return d2_launch<D2_SIN_SPLIT>(z, lp, gz, rec, n, dscale, B, st);
        case D2_SMILEY: return d2_launch<D2_SMILEY>(z, lp, gz, rec, n, dscale, B, st);
        case D2_RINGS: return d2_launch<D2_RINGS>(z, lp, gz, rec, n, dscale, B, st);
        default: return d2_launch<D2_CIRC_GMM>(z, lp, gz, rec, n, dscale, B, st);
    }
}
