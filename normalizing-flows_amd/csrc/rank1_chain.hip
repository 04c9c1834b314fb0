// rank1_chain.hip -- runs of Planar / Radial flows for gfx950: a whole run as ONE launch at inference, and as one forward launch,
// one backward launch and one fixed-order slab reduction under autograd, where the formula route spends about a dozen element-wise
// and reduction launches per layer and direction, each of them a pass over the whole batch.
//
// Reference semantics: normflows/flows/planar.py:51-81 (Planar.forward / .inverse), normflows/flows/radial.py:37-46
// (Radial.forward); the gradients are what PyTorch autograd derives from those lines.
//
// Records: P is (K, 2 d + 4) float32, one record per layer, [kind, s0, s1, s2, vecA[d], vecB[d]] (flows/rank1_pack.py builds it on
// the host side of the launch with the reference's own constraint formulas; include/nf_mi355x.h has the table):
//   kind 0 / 1  Planar tanh / leaky:  s0 = b, s1 = w.u_hat, s2 = slope, vecA = w, vecB = u_hat
//   kind 2      Radial:               s0 = |alpha|, s1 = beta', s2 = d - 1, vecA = z_0, vecB unused
// The whole of P sits in LDS (K <= 64: at most 64 x 260 floats = 65 KB, above 64 KB through opt_in_lds).
//
// Row layouts (template <G, NE>: G lanes per row, NE elements per lane):
//   d <= 16        <1, 16>  lane = row: the row lives in registers, 256 rows per workgroup, every parameter read is wave-uniform;
//   16 < d <= 128  <16, 8>  16 lanes per row, 4 rows per wave, 16 rows per workgroup: lane j of the group holds elements j, j + 16,
//                           ... so that loads and stores coalesce; dot products and norms are summed over the group with four
//                           xor-shuffle steps, after which every lane of the group holds the same bits.
// A persistent grid of <= NF_PERSISTENT_WORKGROUPS workgroups walks the row tiles.
//
// Training: the forward saves ONE scalar per executed record and row (Planar: lin, Radial: r).  The backward starts from the
// output y and rebuilds every record's input from its output and that scalar (Planar: z = z' - u_hat h(lin); Radial:
// z - z_0 = (z' - z_0) / (1 + h(r)); Planar inverse: z = z' + a u_hat lin / (1 + a s1)) -- saving the (K, B, d) inputs would be
// 1 GiB per 65 536 rows at d = 128, K = 32.
//
// Parameter gradients: every wave sums its rows' contributions with shuffles (a fixed tree) and keeps them in a slab that ONLY this
// wave writes -- and, per address, only one lane of it: the first tile writes, later tiles add -- so the tile loop has no barrier;
// one reduction launch sums the waves' slabs in a fixed order (train_reduce.hpp).  No atomics: bit-identical from run to run.
#include "common.hpp"
#include "train_reduce.hpp"

namespace nf {

constexpr int R1_DMAX = 128;
constexpr int R1_KMAX = 64;
constexpr int R1_WAVES = 4;                                        // waves of a 256-lane workgroup: slabs per workgroup
constexpr int64_t R1_SCRATCH_MAX_FLOATS = (int64_t)1 << 24;        // 64 MiB of slabs

template <int G> __device__ __forceinline__ float r1_group_sum(float x) {
    if (G == 16) {
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    }
    return x;
}

// Sum over the rows of a wave of a value that lane (lane % G) of every row holds.
template <int G> __device__ __forceinline__ float r1_rows_sum(float x) {
#pragma unroll
    for (int o = 32; o >= G; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

// h, h', h'' of a Planar record at lin.  tanh: sech^2 = 4 e^2 / (1 + e^2)^2 with e = exp(-|lin|): no 1 - tanh^2 cancellation, and
// it goes to 0 for large |lin| without an overflow (planar.py:58 is 1 / cosh^2, which overflows to 1 / inf = 0 as well).  Leaky:
// planar.py:60's (x < 0) rule, so lin == 0 takes slope 1.  hg = the derivative the cotangent of z' meets on its way through h:
// the same as hp except at lin == 0 exactly, where LeakyReLU's own backward (x > 0 ? 1 : slope) gives the slope while the
// log-det's h' (planar.py:60) is 1 -- the reference's autograd has both, and so has this backward.
__device__ __forceinline__ void r1_act(int kind, float lin, float slope, float &h, float &hp, float &hpp, float &hg) {
    if (kind == 0) {
        const float e = M<float>::exp(-fabsf(lin));
        const float e2 = e * e, q = 1.0f + e2;
        h = ::tanhf(lin);
        hp = 4.0f * e2 / (q * q);
        hpp = -2.0f * h * hp;
        hg = hp;
    } else {
        const bool neg = lin < 0.0f;
        h = neg ? slope * lin : lin;
        hp = neg ? slope : 1.0f;
        hpp = 0.0f;
        hg = lin > 0.0f ? 1.0f : slope;
    }
}

template <int G, int NE> __device__ __forceinline__ int r1_idx(int j, int e) { return G == 1 ? e : j + G * e; }

__device__ __forceinline__ void r1_load_P(float *sP, const float *__restrict__ P, int n) {
    for (int i = threadIdx.x; i < n; i += blockDim.x) sP[i] = P[i];
    __syncthreads();
}

// Inference (save == nullptr, logdet combined by acc) and the training forward (save (K, B), logdet written).
template <int G, int NE>
__global__ void __launch_bounds__(256)
rank1_fwd_kernel(const float *__restrict__ z, float *__restrict__ y, float *__restrict__ logdet, float *__restrict__ save,
                 const float *__restrict__ P, int64_t B, int d, int K, int direction, int acc) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float *sP = reinterpret_cast<float *>(smem_raw);
    const int stride = 2 * d + 4;
    r1_load_P(sP, P, K * stride);
    constexpr int rows = 256 / G;
    const int j = threadIdx.x % G, sub = threadIdx.x / G;
    const int64_t ntiles = (B + rows - 1) / rows;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t r = tile * rows + sub;
        const bool valid = r < B;          // a row past the batch runs on zeros (every lane takes part in the shuffles)
        float v[NE];
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const int i = r1_idx<G, NE>(j, e);
            v[e] = (valid && i < d) ? z[r * d + i] : 0.0f;
        }
        float ld = 0.0f;
        for (int q = 0; q < K; ++q) {
            const float *rec = sP + (direction == 0 ? q : K - 1 - q) * stride;
            const int kind = (int)rec[0];
            const float *A = rec + 4, *Bv = A + d;
            float s;
            if (kind == 2) {               // radial.py:38-44
                const float a = rec[1], bp = rec[2], s2 = rec[3];
                float dz[NE], rr = 0.0f;
#pragma unroll
                for (int e = 0; e < NE; ++e) {
                    const int i = r1_idx<G, NE>(j, e);
                    dz[e] = i < d ? v[e] - A[i] : 0.0f;
                    rr = fmaf(dz[e], dz[e], rr);
                }
                rr = M<float>::sqrt(r1_group_sum<G>(rr));
                const float c = a + rr, h = bp / c, h_ = -bp * rr / (c * c);
#pragma unroll
                for (int e = 0; e < NE; ++e) v[e] = fmaf(h, dz[e], v[e]);
                ld += s2 * M<float>::log(1.0f + h) + M<float>::log(1.0f + h + h_);
                s = rr;
            } else {
                const float b = rec[1], s1 = rec[2], slope = rec[3];
                float lin = 0.0f;
#pragma unroll
                for (int e = 0; e < NE; ++e) {
                    const int i = r1_idx<G, NE>(j, e);
                    if (i < d) lin = fmaf(A[i], v[e], lin);
                }
                lin = r1_group_sum<G>(lin) + b;
                s = lin;
                if (direction == 0) {      // planar.py:52-64
                    float h, hp, hpp, hg;
                    r1_act(kind, lin, slope, h, hp, hpp, hg);
#pragma unroll
                    for (int e = 0; e < NE; ++e) {
                        const int i = r1_idx<G, NE>(j, e);
                        if (i < d) v[e] = fmaf(Bv[i], h, v[e]);
                    }
                    ld += M<float>::log(fabsf(1.0f + s1 * hp));
                } else {                   // planar.py:69-81 (leaky records; the callers admit no other kind in this direction)
                    const float a_ = lin < 0.0f ? slope : 1.0f;
                    const float inner = a_ * s1;
                    const float c = kind == 1 ? a_ * lin / (1.0f + inner) : M<float>::nan();
#pragma unroll
                    for (int e = 0; e < NE; ++e) {
                        const int i = r1_idx<G, NE>(j, e);
                        if (i < d) v[e] = fmaf(-Bv[i], c, v[e]);
                    }
                    ld -= M<float>::log(fabsf(1.0f + inner));
                }
            }
            if (save && valid && j == 0) save[(int64_t)q * B + r] = s;
        }
        if (valid) {
#pragma unroll
            for (int e = 0; e < NE; ++e) {
                const int i = r1_idx<G, NE>(j, e);
                if (i < d) y[r * d + i] = v[e];
            }
            if (j == 0) {
                if (save) logdet[r] = ld;
                else ld_store(logdet + r, ld, acc);
            }
        }
    }
}

template <int G, int NE>
__global__ void __launch_bounds__(256)
rank1_bwd_kernel(const float *__restrict__ y, const float *__restrict__ save, const float *__restrict__ gy,
                 const float *__restrict__ gld, float *__restrict__ gz, const float *__restrict__ P, float *__restrict__ slabs,
                 int64_t B, int d, int K, int direction, int need_gP) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float *sP = reinterpret_cast<float *>(smem_raw);
    const int stride = 2 * d + 4;
    r1_load_P(sP, P, K * stride);
    constexpr int rows = 256 / G;
    const int j = threadIdx.x % G, sub = threadIdx.x / G, lane = threadIdx.x & 63;
    float *slab = need_gP ? slabs + ((size_t)blockIdx.x * R1_WAVES + (threadIdx.x >> 6)) * ((size_t)K * stride) : nullptr;
    bool first = true;
    const int64_t ntiles = (B + rows - 1) / rows;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t r = tile * rows + sub;
        const bool valid = r < B;
        float v[NE], g[NE];
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const int i = r1_idx<G, NE>(j, e);
            const bool in = valid && i < d;
            v[e] = in ? y[r * d + i] : 0.0f;
            g[e] = (in && gy) ? gy[r * d + i] : 0.0f;
        }
        const float gl = (valid && gld) ? gld[r] : 0.0f;
        for (int q = K - 1; q >= 0; --q) {
            const int ri = direction == 0 ? q : K - 1 - q;
            const float *rec = sP + ri * stride;
            const int kind = (int)rec[0];
            const float *A = rec + 4, *Bv = A + d;
            const float s = valid ? save[(int64_t)q * B + r] : 0.0f;
            float gA[NE], gB[NE], gs0, gs1;
            if (kind == 2) {
                const float a = rec[1], bp = rec[2], s2 = rec[3];
                const float c = a + s, h = bp / c, inv = 1.0f / (1.0f + h);
                const float c2 = c * c, h_ = -bp * s / c2, D2 = 1.0f + h + h_;
                float dz[NE], gdot = 0.0f;
#pragma unroll
                for (int e = 0; e < NE; ++e) {
                    const int i = r1_idx<G, NE>(j, e);
                    dz[e] = i < d ? (v[e] - A[i]) * inv : 0.0f;
                    if (i < d) v[e] = A[i] + dz[e];
                    gdot = fmaf(g[e], dz[e], gdot);
                }
                gdot = r1_group_sum<G>(gdot);
                const float gh = gdot + gl * (s2 / (1.0f + h) + 1.0f / D2), gh_ = gl / D2;
                const float dh = -bp / c2, t3 = 2.0f * bp * s / (c2 * c);
                const float g_r = gh * dh + gh_ * (dh + t3);
                gs0 = gh * dh + gh_ * t3;
                gs1 = gh / c - gh_ * s / c2;
                const float gr_over_r = s > 0.0f ? g_r / s : 0.0f;       // d r / d dz = dz / r, 0 at r == 0 (vector_norm's backward)
#pragma unroll
                for (int e = 0; e < NE; ++e) {
                    const float gdz = fmaf(g[e], h, gr_over_r * dz[e]);
                    g[e] += gdz;
                    gA[e] = -gdz;
                    gB[e] = 0.0f;
                }
            } else {
                const float s1 = rec[2], slope = rec[3];
                float ug = 0.0f;
#pragma unroll
                for (int e = 0; e < NE; ++e) {
                    const int i = r1_idx<G, NE>(j, e);
                    if (i < d) ug = fmaf(Bv[i], g[e], ug);
                }
                ug = r1_group_sum<G>(ug);
                float zc, g_lin;           // the input is z' - u_hat zc
                if (direction == 0) {
                    float h, hp, hpp, hg;
                    r1_act(kind, s, slope, h, hp, hpp, hg);
                    const float D = 1.0f + s1 * hp;
                    g_lin = ug * hg + gl * s1 * hpp / D;
                    gs1 = gl * hp / D;
                    zc = h;
                } else {
                    const float a_ = s < 0.0f ? slope : 1.0f;
                    const float den = 1.0f / (1.0f + a_ * s1);
                    zc = -(a_ * s * den);
                    g_lin = -ug * a_ * den;
                    gs1 = ug * a_ * a_ * s * den * den - gl * a_ * den;
                }
                gs0 = g_lin;
#pragma unroll
                for (int e = 0; e < NE; ++e) {
                    const int i = r1_idx<G, NE>(j, e);
                    gA[e] = 0.0f; gB[e] = 0.0f;
                    if (i < d) {
                        v[e] = fmaf(-Bv[i], zc, v[e]);
                        gB[e] = g[e] * zc;
                        gA[e] = g_lin * v[e];
                        g[e] = fmaf(A[i], g_lin, g[e]);
                    }
                }
            }
            if (need_gP) {
                if (!valid) {              // (a zero row can divide by zero: its contributions are dropped, not multiplied by 0)
                    gs0 = 0.0f; gs1 = 0.0f;
#pragma unroll
                    for (int e = 0; e < NE; ++e) { gA[e] = 0.0f; gB[e] = 0.0f; }
                }
                float *row = slab + (size_t)ri * stride;
                gs0 = r1_rows_sum<G>(gs0);
                gs1 = r1_rows_sum<G>(gs1);
                if (lane == 0) {
                    if (first) { row[0] = 0.0f; row[1] = gs0; row[2] = gs1; row[3] = 0.0f; }
                    else { row[1] += gs0; row[2] += gs1; }
                }
#pragma unroll
                for (int e = 0; e < NE; ++e) {
                    if (G * e < d) {       // wave-uniform
                        const float sa = r1_rows_sum<G>(gA[e]), sb = r1_rows_sum<G>(gB[e]);
                        const int i = r1_idx<G, NE>(j, e);
                        if (lane < G && i < d) {
                            if (first) { row[4 + i] = sa; row[4 + d + i] = sb; }
                            else { row[4 + i] += sa; row[4 + d + i] += sb; }
                        }
                    }
                }
            }
        }
        first = false;
        if (gz && valid) {
#pragma unroll
            for (int e = 0; e < NE; ++e) {
                const int i = r1_idx<G, NE>(j, e);
                if (i < d) gz[r * d + i] = g[e];
            }
        }
    }
}

// gP[e] = sum over the waves' slabs in a fixed order (train_reduce.hpp: chunk lanes, then lane order).
__global__ void __launch_bounds__(64 * RL)
rank1_reduce_kernel(const float *__restrict__ slabs, float *__restrict__ gP, int64_t n, int chunks) {
    __shared__ float sm[RL][64];
    for (int64_t e0 = (int64_t)blockIdx.x * 64; e0 < n; e0 += (int64_t)gridDim.x * 64)
        wgrad_reduce_group(slabs, gP, nullptr, n, n, n, chunks, 0, 1, 0, nullptr, 0, e0, sm);
}

static inline int r1_rows(int d) { return d <= 16 ? 256 : 16; }
static inline size_t r1_lds(int d, int K) { return (size_t)K * (2 * d + 4) * sizeof(float); }

static inline int r1_grid(int64_t B, int d, int K, bool slabs) {
    int grid = persistent_grid((B + r1_rows(d) - 1) / r1_rows(d));
    const int64_t per = (int64_t)R1_WAVES * K * (2 * d + 4);
    if (slabs && grid * per > R1_SCRATCH_MAX_FLOATS) grid = (int)(R1_SCRATCH_MAX_FLOATS / per);
    return grid < 1 ? 1 : grid;
}

static inline int r1_check(int64_t B, int d, int K, int direction) {
    if (d < 1 || d > R1_DMAX) return NF_ENOTSUP;
    if (K > R1_KMAX) return NF_ERANGE;
    if (B < 0 || K < 1 || (direction != 0 && direction != 1)) return NF_EINVAL;
    return NF_OK;
}

static int r1_launch_fwd(const void *z, void *y, void *logdet, void *save, const void *P, int64_t B, int d, int K, int direction,
                         int acc, hipStream_t st) {
    const size_t lds = r1_lds(d, K);
    const int grid = r1_grid(B, d, K, false);
    if (d <= 16) {
        static LdsOptIn opted;
        if (opt_in_lds(reinterpret_cast<const void *>(&rank1_fwd_kernel<1, 16>), lds, opted) != NF_OK) return NF_ENOTSUP;
        hipLaunchKernelGGL((rank1_fwd_kernel<1, 16>), dim3(grid), dim3(256), lds, st, (const float *)z, (float *)y, (float *)logdet,
                           (float *)save, (const float *)P, B, d, K, direction, acc);
    } else {
        static LdsOptIn opted;
        if (opt_in_lds(reinterpret_cast<const void *>(&rank1_fwd_kernel<16, 8>), lds, opted) != NF_OK) return NF_ENOTSUP;
        hipLaunchKernelGGL((rank1_fwd_kernel<16, 8>), dim3(grid), dim3(256), lds, st, (const float *)z, (float *)y, (float *)logdet,
                           (float *)save, (const float *)P, B, d, K, direction, acc);
    }
    NF_CHECK_LAUNCH();
    return NF_OK;
}

}  // namespace nf

extern "C" int nf_rank1_rows(int d) { return d < 1 || d > nf::R1_DMAX ? NF_ENOTSUP : nf::r1_rows(d); }

extern "C" int64_t nf_rank1_train_scratch_floats(int64_t B, int d, int K) {
    const int rc = nf::r1_check(B, d, K, 0);
    if (rc != NF_OK) return rc;
    return (int64_t)nf::r1_grid(B, d, K, true) * nf::R1_WAVES * K * (2 * d + 4);
}

extern "C" int nf_rank1_chain(const void *z, void *y, void *logdet, const void *P, int64_t B, int d, int K, int direction, int acc,
                              nf_stream_t stream) {
    const int rc = nf::r1_check(B, d, K, direction);
    if (rc != NF_OK) return rc;
    if (acc < NF_LD_SUB || acc > NF_LD_ADD) return NF_EINVAL;
    if (B == 0) return NF_OK;
    if (!z || !y || !logdet || !P) return NF_EFAULT;
    return nf::r1_launch_fwd(z, y, logdet, nullptr, P, B, d, K, direction, acc, (hipStream_t)stream);
}

extern "C" int nf_rank1_chain_train_fwd(const void *z, void *y, void *logdet, void *save, const void *P, int64_t B, int d, int K,
                                        int direction, nf_stream_t stream) {
    const int rc = nf::r1_check(B, d, K, direction);
    if (rc != NF_OK) return rc;
    if (B == 0) return NF_OK;
    if (!z || !y || !logdet || !save || !P) return NF_EFAULT;
    return nf::r1_launch_fwd(z, y, logdet, save, P, B, d, K, direction, NF_LD_WRITE, (hipStream_t)stream);
}

extern "C" int nf_rank1_chain_bwd(const void *y, const void *save, const void *gy, const void *gld, void *gz, const void *P,
                                  void *slabs, void *gP, int64_t B, int d, int K, int direction, int need_gP, nf_stream_t stream) {
    const int rc = nf::r1_check(B, d, K, direction);
    if (rc != NF_OK) return rc;
    if (B == 0) return NF_OK;
    if (!y || !save || !P || (need_gP && (!slabs || !gP))) return NF_EFAULT;
    if (!gz && !need_gP) return NF_OK;
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = nf::r1_lds(d, K);
    const int grid = nf::r1_grid(B, d, K, need_gP != 0);
    if (d <= 16) {
        static nf::LdsOptIn opted;
        if (nf::opt_in_lds(reinterpret_cast<const void *>(&nf::rank1_bwd_kernel<1, 16>), lds, opted) != NF_OK) return NF_ENOTSUP;
        hipLaunchKernelGGL((nf::rank1_bwd_kernel<1, 16>), dim3(grid), dim3(256), lds, st, (const float *)y, (const float *)save,
                           (const float *)gy, (const float *)gld, (float *)gz, (const float *)P, (float *)slabs, B, d, K, direction,
                           need_gP);
    } else {
        static nf::LdsOptIn opted;
        if (nf::opt_in_lds(reinterpret_cast<const void *>(&nf::rank1_bwd_kernel<16, 8>), lds, opted) != NF_OK) return NF_ENOTSUP;
        hipLaunchKernelGGL((nf::rank1_bwd_kernel<16, 8>), dim3(grid), dim3(256), lds, st, (const float *)y, (const float *)save,
                           (const float *)gy, (const float *)gld, (float *)gz, (const float *)P, (float *)slabs, B, d, K, direction,
                           need_gP);
    }
    NF_CHECK_LAUNCH();
    if (need_gP) {
        const int64_t n = (int64_t)K * (2 * d + 4);
        hipLaunchKernelGGL(nf::rank1_reduce_kernel, dim3(nf::grid_for(n, 64)), dim3(64 * nf::RL), 0, st, (const float *)slabs,
                           (float *)gP, n, grid * nf::R1_WAVES);
        NF_CHECK_LAUNCH();
    }
    return NF_OK;
}
