// lipmlp.hip -- residual flows x + g(x), g a LipschitzMLP on 2-D rows, for gfx950: the density direction of a run of
// [Residual | ActNorm | AffineConstFlow] layers as ONE launch (value, exact 2 x 2 Jacobian and log|det| per Residual record), and one
// launch per call for a single network (x + g(x), or the fixed-point step y - g(x) with a device-side count of the elements that
// have not converged).  The formula route spends 40-60 small launches per layer and direction on the same work: three Swish
// activations of about five element-wise launches each, three weight rescalings in front of three library GEMMs, and three autograd
// passes that build the Jacobian column by column.
//
// Reference semantics: normflows/flows/residual.py:118-161 (iResBlock.forward / _inverse_fixed_point's step / the brute-force
// branch of _logdetgrad), normflows/nets/lipschitz.py:66-67, :272-274, :647-648 (LipschitzMLP / InducedNormLinear / Swish forward),
// normflows/flows/affine/coupling.py:38-54 (AffineConstFlow).
//
// The Jacobian comes from forward-mode tangents: next to the value stream h two tangent streams t_0, t_1 (d/dx_0, d/dx_1) go through
// the same weights.  At a Swish with pre-activation p the value becomes f(p) = p sigmoid(c p) / 1.1 and each tangent is multiplied
// by f'(p) of the VALUE stream; tangents take no bias.  After the last linear layer the value stream is g(x) and the tangent streams
// are the columns of J.
//
// Blob (flows/lipmlp_pack.py; the table is in include/nf_mi355x.h): K headers of 16 floats, then one weight block of
// 2 HP^2 + 7 HP + 4 floats per Residual record, widths zero-padded to HP in {32, 64, 128}.  A padded hidden unit has
// pre-activation 0, so its value f(0) and its tangents (0 times f'(0)) are 0, and its outgoing weights are 0 as well.
//
// Mapping (template <HP, NS>; NS = 3 streams with the Jacobian, 1 without): 256 lanes own a tile of R = 4096 / HP rows; the
// NS x R x HP activations live in LDS.  In a hidden product lane (rg, cg) = (tid / (HP / 4), tid % (HP / 4)) owns rows 4 rg .. 4 rg + 3
// and columns 4 cg .. 4 cg + 3 of all NS streams -- 16 NS accumulators -- reads its activations from LDS as float4 along k (every
// lane of a row group reads the same address: a broadcast) and its weight columns from the blob as float4 (coalesced over cg; the 64 KB
// of a layer stay in L2 / L1).  The three streams of a sample sit in the same lane and register position, so the activation
// epilogue is lane-local.  Plain fp32 FMAs in a fixed order: bit-identical from run to run (the count of the fixed-point step is an
// integer sum, order-free).  A persistent grid of <= NF_PERSISTENT_WORKGROUPS workgroups walks the row tiles.
#include "lipmlp_net.hpp"

namespace nf {

// The density direction of K records on z (B, 2): y (B, 2), logdet (B) combined by acc.
template <int HP, bool VEC>
__global__ void __launch_bounds__(LM_THREADS)
lipmlp_chain_kernel(const float *__restrict__ z, float *__restrict__ y, float *__restrict__ logdet, const float *__restrict__ blob,
                    int64_t B, int K, int nres, int acc) {
    constexpr int R = 4096 / HP, LDH = HP + 4;
    extern __shared__ __attribute__((aligned(16))) float lm_lds[];
    float *H = lm_lds, *xs = H + 3 * R * LDH, *rowA = xs + 2 * R, *res = rowA + 4 * R, *lda = res + 6 * R;
    const int tid = threadIdx.x;
    const int64_t rstride = (int64_t)2 * HP * HP + 7 * HP + 4;
    const int64_t ntiles = (B + R - 1) / R;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t row = tile * R + tid;
        const bool valid = tid < R && row < B;         // a row past the batch runs on zeros
        if (tid < R) {
            xs[2 * tid] = valid ? z[2 * row] : 0.0f;
            xs[2 * tid + 1] = valid ? z[2 * row + 1] : 0.0f;
            lda[tid] = 0.0f;
        }
        __syncthreads();
        for (int q = 0; q < K; ++q) {
            const float *hdr = blob + q * LM_HDR;
            const int kind = (int)hdr[0];
            if (kind == 0) {                           // Residual: x + g(x), log|(1 + J00)(1 + J11) - J01 J10|
                int ri = (int)hdr[11];
                ri = ri < 0 ? 0 : (ri >= nres ? nres - 1 : ri);
                lm_net<HP, 3, VEC>(H, rowA, res, xs, hdr, blob + (int64_t)K * LM_HDR + ri * rstride);
                if (tid < R) {
                    const float *r6 = res + 6 * tid;
                    xs[2 * tid] += r6[0];
                    xs[2 * tid + 1] += r6[1];
                    const float det = (r6[2] + 1.0f) * (r6[5] + 1.0f) - r6[4] * r6[3];
                    lda[tid] += M<float>::log(fabsf(det));
                }
            } else if (tid < R) {                      // ActNorm / AffineConstFlow: e = exp(+-s) and the log-det come packed
                const float e0 = hdr[6], e1 = hdr[7], t0 = hdr[8], t1 = hdr[9];
                if (kind == 1) {
                    xs[2 * tid] = fmaf(xs[2 * tid], e0, t0);
                    xs[2 * tid + 1] = fmaf(xs[2 * tid + 1], e1, t1);
                } else {
                    xs[2 * tid] = (xs[2 * tid] - t0) * e0;
                    xs[2 * tid + 1] = (xs[2 * tid + 1] - t1) * e1;
                }
                lda[tid] += hdr[10];
            }
            __syncthreads();
        }
        if (valid) {
            y[2 * row] = xs[2 * tid];
            y[2 * row + 1] = xs[2 * tid + 1];
            const float l = lda[tid];
            logdet[row] = acc == NF_LD_WRITE ? l : (acc == NF_LD_ADD ? logdet[row] + l : logdet[row] - l);
        }
        __syncthreads();
    }
}

// One network: mode 0: out = x + g(x).  mode 1: out = yin - g(x), and *count += the number of elements of this call with
// !((out - x)^2 / (atol + |yin| rtol) < 1) (residual.py:136-137; a NaN counts).
template <int HP, bool VEC>
__global__ void __launch_bounds__(LM_THREADS)
lipmlp_apply_kernel(const float *__restrict__ x, const float *__restrict__ yin, float *__restrict__ out, int *__restrict__ count,
                    const float *__restrict__ blob, int64_t B, int mode, float atol, float rtol) {
    constexpr int R = 4096 / HP, LDH = HP + 4;
    extern __shared__ __attribute__((aligned(16))) float lm_lds[];
    float *H = lm_lds, *xs = H + R * LDH, *rowA = xs + 2 * R, *res = rowA + 4 * R;
    const int tid = threadIdx.x;
    const int64_t ntiles = (B + R - 1) / R;
    int bad = 0;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t row = tile * R + tid;
        const bool valid = tid < R && row < B;
        if (tid < R) {
            xs[2 * tid] = valid ? x[2 * row] : 0.0f;
            xs[2 * tid + 1] = valid ? x[2 * row + 1] : 0.0f;
        }
        __syncthreads();
        lm_net<HP, 1, VEC>(H, rowA, res, xs, blob, blob + LM_HDR);
        if (valid) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const float g = res[6 * tid + j], xv = xs[2 * tid + j];
                if (mode == 0) {
                    out[2 * row + j] = xv + g;
                } else {
                    const float yv = yin[2 * row + j], o = yv - g, d = o - xv;
                    out[2 * row + j] = o;
                    bad += !(d * d / (atol + fabsf(yv) * rtol) < 1.0f);
                }
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

static int lm_check(int64_t B, int hp, int K, int nres, int64_t nblob) {
    if (hp != 32 && hp != 64 && hp != 128) return NF_ENOTSUP;
    if (K > LM_KMAX) return NF_ERANGE;
    if (K < 1 || B < 0 || nres < 1 || nres > K) return NF_EINVAL;
    if (nblob != (int64_t)K * LM_HDR + nres * lm_rstride(hp)) return NF_EINVAL;
    return NF_OK;
}

}  // namespace nf

extern "C" int nf_lipmlp_width(int hmax) { return hmax < 1 || hmax > 128 ? NF_ENOTSUP : (hmax <= 32 ? 32 : (hmax <= 64 ? 64 : 128)); }

extern "C" int nf_lipmlp_rows(int hp) { return hp != 32 && hp != 64 && hp != 128 ? NF_ENOTSUP : nf::lm_rows(hp); }

extern "C" int64_t nf_lipmlp_blob_floats(int K, int nres, int hp) {
    if (hp != 32 && hp != 64 && hp != 128) return NF_ENOTSUP;
    if (K > nf::LM_KMAX) return NF_ERANGE;
    if (K < 1 || nres < 1 || nres > K) return NF_EINVAL;
    return (int64_t)K * nf::LM_HDR + nres * nf::lm_rstride(hp);
}

extern "C" int nf_lipmlp_chain(const void *z, void *y, void *logdet, const void *blob, int64_t nblob, int64_t B, int hp, int K,
                               int nres, int acc, nf_stream_t stream) {
    const int rc = nf::lm_check(B, hp, K, nres, nblob);
    if (rc != NF_OK) return rc;
    if (acc < NF_LD_SUB || acc > NF_LD_ADD) return NF_EINVAL;
    if (B == 0) return NF_OK;
    if (!z || !y || !logdet || !blob) return NF_EFAULT;
    hipStream_t st = (hipStream_t)stream;
    const int grid = nf::persistent_grid((B + nf::lm_rows(hp) - 1) / nf::lm_rows(hp));
    const size_t lds = nf::lm_lds_bytes(hp, 3);
    const bool vec = !nf_misaligned16(blob);
#define NF_LM_CHAIN(HP, VEC)                                                                                                     \
    hipLaunchKernelGGL((nf::lipmlp_chain_kernel<HP, VEC>), dim3(grid), dim3(nf::LM_THREADS), lds, st, (const float *)z,          \
                       (float *)y, (float *)logdet, (const float *)blob, B, K, nres, acc)
    if (hp == 32) { if (vec) NF_LM_CHAIN(32, true); else NF_LM_CHAIN(32, false); }
    else if (hp == 64) { if (vec) NF_LM_CHAIN(64, true); else NF_LM_CHAIN(64, false); }
    else { if (vec) NF_LM_CHAIN(128, true); else NF_LM_CHAIN(128, false); }
#undef NF_LM_CHAIN
    NF_CHECK_LAUNCH();
    return NF_OK;
}

extern "C" int nf_lipmlp_apply(const void *x, const void *yin, void *out, void *count, const void *blob, int64_t nblob, int64_t B,
                               int hp, int mode, double atol, double rtol, nf_stream_t stream) {
    const int rc = nf::lm_check(B, hp, 1, 1, nblob);
    if (rc != NF_OK) return rc;
    if (mode != 0 && mode != 1) return NF_EINVAL;
    if (mode == 1 && !(atol >= 0.0 && rtol >= 0.0 && atol + rtol > 0.0)) return NF_EINVAL;
    if (B == 0) return NF_OK;
    if (!x || !out || !blob || (mode == 1 && (!yin || !count))) return NF_EFAULT;
    hipStream_t st = (hipStream_t)stream;
    const int grid = nf::persistent_grid((B + nf::lm_rows(hp) - 1) / nf::lm_rows(hp));
    const size_t lds = nf::lm_lds_bytes(hp, 1);
    const bool vec = !nf_misaligned16(blob);
#define NF_LM_APPLY(HP, VEC)                                                                                                     \
    hipLaunchKernelGGL((nf::lipmlp_apply_kernel<HP, VEC>), dim3(grid), dim3(nf::LM_THREADS), lds, st, (const float *)x,          \
                       (const float *)yin, (float *)out, (int *)count, (const float *)blob, B, mode, (float)atol, (float)rtol)
    if (hp == 32) { if (vec) NF_LM_APPLY(32, true); else NF_LM_APPLY(32, false); }
    else if (hp == 64) { if (vec) NF_LM_APPLY(64, true); else NF_LM_APPLY(64, false); }
    else { if (vec) NF_LM_APPLY(128, true); else NF_LM_APPLY(128, false); }
#undef NF_LM_APPLY
    NF_CHECK_LAUNCH();
    return NF_OK;
}
