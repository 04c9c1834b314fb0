// density2d_row.hpp -- the per-row evaluation of the closed-form two-dimensional densities: value and input gradient of one row for
// a kind, in registers.  Shared by density2d.hip (one density per launch, KIND a template argument; it includes the statements of
// density2d_row_body.hpp in place) and hmc2d.hip (whole MCMC transitions per launch, the kind a wave-uniform run-time switch over
// d2_row<KIND>, the same statements as a function).  Shared: the helpers and the row statements.  Not shared: d2_circ_setup below.
#pragma once
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

// CircularGaussianMixture's per-launch constants as nf_density2d holds them: the centres (computed once per workgroup into LDS, in
// float32 from a float32 phase), 1 / (2 s^2) and the log normaliser from the `scale` buffer in device memory.  Every thread of the
// workgroup calls it (it holds a barrier).  density2d.hip ONLY: hmc2d.hip does not use it -- its own h2_circ_setup evaluates the
// centres in double and rounds once, so the two evaluate kind 6 from centres that differ by a few float32 roundings (reason there).
__device__ __forceinline__ void d2_circ_setup(const float *p, int n, const float *__restrict__ dscale, float *cx, float *cy,
                                              float &inv2s2, float &lognorm) {
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

// log p(z0, z1) of kind KIND with record p (include/nf_mi355x.h has the table) and d log p / d z in o0, o1.  cx / cy / inv2s2 /
// lognorm: d2_circ_setup's (kind 6 only).  The statements are density2d_row_body.hpp's, shared with density2d_kernel.
template <int KIND>
__device__ __forceinline__ float d2_row(float z0, float z1, const float *p, int n, const float *cx, const float *cy, float inv2s2,
                                        float lognorm, float &o0, float &o1) {
#include "density2d_row_body.hpp"
    o0 = g0;
    o1 = g1;
    return v;
}

}  // namespace nf
