// lipmlp_net.hpp -- the LipschitzMLP of a residual flow on a tile of 2-D rows: value stream and two forward-mode tangent streams
// through one network (lm_net), its Swish, and the blob's sizes.  Shared by the inference kernels (lipmlp.hip) and the training
// kernels (lipmlp_train.hip); the mapping is described at the head of lipmlp.hip.
#pragma once
#include "common.hpp"

namespace nf {

constexpr int LM_KMAX = 32;        // records per launch
constexpr int LM_HDR = 16;         // floats per record header
constexpr int LM_THREADS = 256;

static inline int64_t lm_rstride(int hp) { return (int64_t)2 * hp * hp + 7 * hp + 4; }
static inline int lm_rows(int hp) { return 4096 / hp; }
static inline size_t lm_lds_bytes(int hp, int ns) { return sizeof(float) * ((size_t)ns * lm_rows(hp) * (hp + 4) + 13 * lm_rows(hp)); }

// f(p) = p sigmoid(c p) / 1.1 and f'(p) = (s + c p s (1 - s)) / 1.1, s = sigmoid(c p).
__device__ __forceinline__ void lm_swish(float p, float c, float &h, float &dh) {
    const float s = 1.0f / (1.0f + M<float>::exp(-c * p));
    h = p * s / 1.1f;
    dh = (s + c * p * s * (1.0f - s)) / 1.1f;
}

// Four consecutive weights: one 16-byte load where the blob sits on a 16-byte boundary (what the packer allocates), four 4-byte loads
// for a blob that is a view into a larger buffer.
template <bool VEC> __device__ __forceinline__ float4 lm_ld4(const float *__restrict__ p) {
    if (VEC) return *reinterpret_cast<const float4 *>(p);
    return make_float4(p[0], p[1], p[2], p[3]);
}

// One network on the tile's rows xs (R, 2): res (R, 6) = [g_0, g_1, dg_0/dx_0, dg_1/dx_0, dg_0/dx_1, dg_1/dx_1] (NS == 1: the first
// two only).  hdr: the record's header; W: its weight block.  Ends with a barrier: res is complete for every lane.
template <int HP, int NS, bool VEC>
__device__ __forceinline__ void lm_net(float *__restrict__ H, float *__restrict__ rowA, float *__restrict__ res,
                                       const float *__restrict__ xs, const float *__restrict__ hdr, const float *__restrict__ W) {
    constexpr int CT = HP / 4, R = 4096 / HP, LDH = HP + 4, PL = R * LDH;
    const int tid = threadIdx.x;
    int nmid = (int)hdr[1];
    nmid = nmid < 0 ? 0 : (nmid > 2 ? 2 : nmid);
    if (tid < R) {                         // the input Swish: values and their derivatives, once per row
        float a0, a1, d0, d1;
        lm_swish(xs[2 * tid], hdr[2], a0, d0);
        lm_swish(xs[2 * tid + 1], hdr[2], a1, d1);
        rowA[4 * tid] = a0, rowA[4 * tid + 1] = a1, rowA[4 * tid + 2] = d0, rowA[4 * tid + 3] = d1;
    }
    __syncthreads();
    {                                      // first linear layer (2 -> HP) and its Swish
        const float *W0 = W, *b0 = W + 2 * HP;
        const float c = hdr[3];
        for (int idx = tid; idx < R * HP; idx += LM_THREADS) {
            const int r = idx / HP, o = idx % HP;
            const float w0 = W0[o], w1 = W0[HP + o];
            const float pre = fmaf(w1, rowA[4 * r + 1], fmaf(w0, rowA[4 * r], b0[o]));
            float h, dh;
            lm_swish(pre, c, h, dh);
            H[r * LDH + o] = h;
            if (NS == 3) {
                H[PL + r * LDH + o] = w0 * rowA[4 * r + 2] * dh;
                H[2 * PL + r * LDH + o] = w1 * rowA[4 * r + 3] * dh;
            }
        }
    }
    __syncthreads();
    const int cg = tid % CT, rg = tid / CT;
    for (int m = 0; m < nmid; ++m) {       // hidden products (HP x HP) with their Swish
        const float *Wm = W + 3 * HP + (size_t)m * (HP * HP + HP), *bm = Wm + HP * HP;
        float acc[NS][4][4];
#pragma unroll
        for (int s = 0; s < NS; ++s)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[s][i][j] = 0.0f;
        for (int k = 0; k < HP; k += 4) {
            float4 w[4];
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) w[kk] = lm_ld4<VEC>(Wm + (k + kk) * HP + 4 * cg);
#pragma unroll
            for (int s = 0; s < NS; ++s)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float4 a = *reinterpret_cast<const float4 *>(H + s * PL + (4 * rg + i) * LDH + k);
                    const float av[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
                    for (int kk = 0; kk < 4; ++kk) {
                        acc[s][i][0] = fmaf(av[kk], w[kk].x, acc[s][i][0]);
                        acc[s][i][1] = fmaf(av[kk], w[kk].y, acc[s][i][1]);
                        acc[s][i][2] = fmaf(av[kk], w[kk].z, acc[s][i][2]);
                        acc[s][i][3] = fmaf(av[kk], w[kk].w, acc[s][i][3]);
                    }
                }
        }
        __syncthreads();                   // every lane has read the layer's input: H is free to take its output
        const float4 b4 = lm_ld4<VEC>(bm + 4 * cg);
        const float bv[4] = {b4.x, b4.y, b4.z, b4.w};
        const float c = hdr[4 + m];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float hv[4], dv[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) lm_swish(acc[0][i][j] + bv[j], c, hv[j], dv[j]);
            float *dst = H + (4 * rg + i) * LDH + 4 * cg;
            *reinterpret_cast<float4 *>(dst) = make_float4(hv[0], hv[1], hv[2], hv[3]);
            if (NS == 3) {
#pragma unroll
                for (int s = 1; s < NS; ++s)
                    *reinterpret_cast<float4 *>(dst + s * PL) =
                        make_float4(acc[s][i][0] * dv[0], acc[s][i][1] * dv[1], acc[s][i][2] * dv[2], acc[s][i][3] * dv[3]);
            }
        }
        __syncthreads();
    }
    {                                      // last linear layer (HP -> 2): one lane per (stream, row)
        const float *Wl = W + 3 * HP + 2 * (HP * HP + HP), *bl = Wl + 2 * HP;
        for (int it = tid; it < NS * R; it += LM_THREADS) {
            const int s = it / R, r = it % R;
            const float *h = H + s * PL + r * LDH;
            float o0 = 0.0f, o1 = 0.0f;
            for (int k = 0; k < HP; k += 4) {
                const float4 a = *reinterpret_cast<const float4 *>(h + k);
                const float4 u = lm_ld4<VEC>(Wl + k);
                const float4 v = lm_ld4<VEC>(Wl + HP + k);
                o0 = fmaf(a.w, u.w, fmaf(a.z, u.z, fmaf(a.y, u.y, fmaf(a.x, u.x, o0))));
                o1 = fmaf(a.w, v.w, fmaf(a.z, v.z, fmaf(a.y, v.y, fmaf(a.x, v.x, o1))));
            }
            if (s == 0) o0 += bl[0], o1 += bl[1];
            res[6 * r + 2 * s] = o0, res[6 * r + 2 * s + 1] = o1;
        }
    }
    __syncthreads();
}

}  // namespace nf
