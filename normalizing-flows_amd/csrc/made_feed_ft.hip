// made_feed_ft.hip -- the backward of the gathered, fed x tile of nf_made_forward_train_ft (made_fwd.hip FT): what torch autograd does
// with the periodic preprocessing in front of MADE (nets/made.py:250-252 -> utils/nn.py:64-129: index, sin / cos, cat, index) and with
// the column permutation of a permuted mask, under core.py:87-102 + loss.backward(), as ONE element-wise pass + a fixed-order reduction.
//
//   g_pre  (B, D)  the input-gradient chain's result on the degree-order pack (nf_made_backward's g_x): the gradient at the FED values
//   g_xpos (B, D)  the spline's gradient at the raw values in position order (NULL: none)
//   g_x[:, col[f]] = g_pre[:, f] d + g_xpos[:, f],   d = s (w_sin cos(s x) - w_cos sin(s x)) for a periodic position, else 1
//   g_weights[i] = (sum_rows g_pre sin(s x), sum_rows g_pre cos(s x)),  g_bias[i] = sum_rows g_pre   for periodic feature i
//
// Table: made_fwd.hip's tt = [col | scale bits | periodic index or -1]; feed = [w_sin | w_cos | bias] per position, as gathered for the
// forward (the tail of its blob).  A workgroup owns a contiguous chunk of rows; thread (sub,
// f) walks rows sub, sub + nsub, ... of position f (g_pre / g_xpos coalesced, x and g_x within one row), sums its three partials in
// registers, the subs are added in order through LDS and the workgroup's sums go to part[wg][3][n_circ]; a second launch adds the
// workgroups' partials in order: deterministic, no atomics.  With no periodic position only the scatter-add runs.
#include "common.hpp"

namespace nf {

constexpr int FB_NT = 256;          // threads per workgroup
constexpr int FB_MAX_WG = 512;      // row chunks at the most (include/nf_mi355x.h: the caller sizes `part` by it)

__global__ void __launch_bounds__(FB_NT)
made_feed_ft_bwd_kernel(const float *__restrict__ g_pre, const float *__restrict__ g_xpos, const float *__restrict__ x,
                        const int *__restrict__ tt, const float *__restrict__ feed, float *__restrict__ g_x, float *__restrict__ part,
                        int64_t B, int D, int n_circ, int fp, int64_t rows_per) {
    __shared__ float sm[3][FB_NT];
    const int tid = threadIdx.x;
    const int f = tid & (fp - 1), sub = tid / fp, nsub = FB_NT / fp;
    const int64_t r0 = (int64_t)blockIdx.x * rows_per;
    const int64_t r1 = r0 + rows_per < B ? r0 + rows_per : B;
    float ss = 0.0f, sc = 0.0f, sb = 0.0f;
    int pi = -1;
    if (f < D) {
        const int c = tt[f];
        const float s = __int_as_float(tt[D + f]);
        pi = tt[2 * D + f];
        float ws = 0.0f, wc = 0.0f;
        if (pi >= 0) {
            ws = feed[f];
            wc = feed[D + f];
        }
        for (int64_t r = r0 + sub; r < r1; r += nsub) {
            const float g = g_pre[r * D + f];
            const float gs = g_xpos ? g_xpos[r * D + f] : 0.0f;
            float d = 1.0f;
            if (pi >= 0) {
                const float a = s * x[r * D + c];
                float sn, cs;
                sincosf(a, &sn, &cs);          // (as the forward)
                d = s * (ws * cs - wc * sn);
                ss += g * sn;
                sc += g * cs;
                sb += g;
            }
            g_x[r * D + c] = g * d + gs;
        }
    }
    if (n_circ == 0) return;          // (uniform: no periodic position, no partials)
    sm[0][tid] = ss;
    sm[1][tid] = sc;
    sm[2][tid] = sb;
    __syncthreads();
    if (sub == 0 && pi >= 0 && pi < n_circ) {
        float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
        for (int j = 0; j < nsub; ++j) {          // fixed order
            a0 += sm[0][f + fp * j];
            a1 += sm[1][f + fp * j];
            a2 += sm[2][f + fp * j];
        }
        float *pp = part + (size_t)blockIdx.x * 3 * n_circ;
        pp[pi] = a0;
        pp[n_circ + pi] = a1;
        pp[2 * n_circ + pi] = a2;
    }
}

// g_weights (n_circ, 2), g_bias (n_circ) or NULL: the workgroups' partials added in order
__global__ void __launch_bounds__(64)
made_feed_ft_reduce_kernel(const float *__restrict__ part, float *__restrict__ g_w, float *__restrict__ g_b, int n_circ, int nwg) {
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= 3 * n_circ) return;
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
    int k = 0;
    for (; k + 3 < nwg; k += 4) {
        s0 += part[(size_t)k * 3 * n_circ + e];
        s1 += part[(size_t)(k + 1) * 3 * n_circ + e];
        s2 += part[(size_t)(k + 2) * 3 * n_circ + e];
        s3 += part[(size_t)(k + 3) * 3 * n_circ + e];
    }
    for (; k < nwg; ++k) s0 += part[(size_t)k * 3 * n_circ + e];
    const float s = (s0 + s1) + (s2 + s3);
    const int which = e / n_circ, i = e - which * n_circ;
    if (which < 2) g_w[2 * i + which] = s;
    else if (g_b) g_b[i] = s;
}

}  // namespace nf

// The backward of nf_made_forward_train_ft's gather + periodic feed (include/nf_mi355x.h).  part: 512 x 3 x n_circ floats of scratch
// (unused, may be NULL, at n_circ = 0).
extern "C" int nf_made_feed_ft_bwd(const void *g_pre, const void *g_xpos, const void *x, const int32_t *ttable, const void *feed,
                                   void *g_x, void *g_weights, void *g_bias, void *part, int64_t B, int D, int n_circ,
                                   nf_stream_t stream) {
    if (B < 0 || D < 2 || D > 128 || n_circ < 0 || n_circ > D) return NF_EINVAL;
    if (B == 0) return NF_OK;
    if (!g_pre || !x || !ttable || !g_x) return NF_EFAULT;                          // (g_xpos may be NULL: no spline-side gradient)
    if (n_circ > 0 && (!feed || !g_weights || !part)) return NF_EFAULT;         // (g_bias may be NULL: no bias parameter)
    hipStream_t st = (hipStream_t)stream;
    int fp = 2;
    while (fp < D) fp *= 2;
    const int64_t chunks64 = (B + 63) / 64;
    const int nwg = (int)(chunks64 < nf::FB_MAX_WG ? chunks64 : nf::FB_MAX_WG);
    const int64_t rows_per = (B + nwg - 1) / nwg;
    const int used = (int)((B + rows_per - 1) / rows_per);      // (every launched workgroup owns at least one row)
    hipLaunchKernelGGL(nf::made_feed_ft_bwd_kernel, dim3((unsigned)used), dim3(nf::FB_NT), 0, st, (const float *)g_pre,
                       (const float *)g_xpos, (const float *)x, (const int *)ttable, (const float *)feed, (float *)g_x, (float *)part,
                       B, D, n_circ, fp, rows_per);
    NF_CHECK_LAUNCH();
    if (n_circ > 0) {
        hipLaunchKernelGGL(nf::made_feed_ft_reduce_kernel, dim3((unsigned)((3 * n_circ + 63) / 64)), dim3(64), 0, st, (const float *)part,
                           (float *)g_weights, (float *)g_bias, n_circ, used);
        NF_CHECK_LAUNCH();
    }
    return NF_OK;
}
