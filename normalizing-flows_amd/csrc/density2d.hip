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
#include "density2d_row.hpp"

namespace nf {

template <int KIND>
__global__ void __launch_bounds__(256)
density2d_kernel(const float *__restrict__ z, float *__restrict__ lp, float *__restrict__ gz, D2Rec rec, int n,
                 const float *__restrict__ dscale, int64_t B) {
    __shared__ float cx[KIND == D2_CIRC_GMM ? D2_MAX_MODES : 1], cy[KIND == D2_CIRC_GMM ? D2_MAX_MODES : 1];
    const float *p = rec.p;
    float inv2s2 = 0.0f, lognorm = 0.0f;
    if (KIND == D2_CIRC_GMM) d2_circ_setup(p, n, dscale, cx, cy, inv2s2, lognorm);
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < B; r += (int64_t)gridDim.x * blockDim.x) {
        const float z0 = z[2 * r], z1 = z[2 * r + 1];
#include "density2d_row_body.hpp"
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
